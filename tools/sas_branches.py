#!/usr/bin/env python
"""Which branch directions of oracle/sas_oracle.c do the inputs of the transport tests take?  CPU only, not a test.

    python tools/sas_branches.py BUILD_DIR [--out profiles/sas_branches.txt]

The oracle mirrors the kernels' selects one for one, so a direction that the oracle never takes on the inputs of the device tests is a
direction the kernels' tests never take.  This tool builds the oracle with `-O0 --coverage` (no OpenMP) into BUILD_DIR/existing and
BUILD_DIR/tiefree, runs in a fresh child process each

  existing   the random problems of tests/test_hip_sas.py (random columns of both solver kinds, gamma and reversed exponential, closed-form
             exponents, fifth-root fallback; the shapes of the parametrised tests are read from their marks, the other problems come from
             the builders the tests themselves call) and every day of every SAS golden case from the reference's state
  tiefree    the same plus the tie-free problems (tests/sas_tiefree_columns.py, every configuration, three days, with the margin)

then `gcov -b -c`, and writes every branch direction of the routines of the step (FUNCTIONS) that no input took, with line number and
source text: both lists, and for every direction of the second list the reason it stays untaken (REASONS, by source text and ordinals;
a line without one is marked and the tool exits with status 1).  CANNOT: no input the reference can be given takes the direction.
TIE: the direction is a clip or snap that a tie-free column must not take by definition; the tie-tolerant tests of the first list are
the ones that could hold it.  GAP: a column could take it and no input set holds it."""
import argparse
import ctypes
import glob
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")
SOURCE = "sas_oracle.c"
FUNCTIONS = ("conc_to_delta", "calc_SA", "sas_omega", "calc_tt", "outflux", "outflux_anion", "ageing_anion", "step_anion", "storages_anion",
             "inflow", "conc_storage", "ageing", "storages_iso", "euler_mix", "euler_tt", "conc_iso_flux", "euler_inflow", "euler_inflow_anion",
             "anion_mtt", "explicit_update_anion", "explicit_concentrations_anion", "euler_distributions", "euler_update",
             "euler_concentrations", "euler_substep", "rk4_substep")

CANNOT, TIE, GAP = "CANNOT", "TIE", "GAP"
# (how the line's source text begins, CANNOT / TIE / GAP, the reason); the first entry whose text matches holds for all untaken ordinals of the line
_SWITCH = "inside the diagnostic switch OC_SAS_DEVICE_ORDER, which restates the kernel's summation order and is unset here: no select of the reference"
_NAN_MTT = ("mtt = where(tt > 0, msa, 0) would be NaN where a piston (threshold ages - 1, tt = 1 over no water) reads the NaN marker that ageing leaves in an empty oldest "
            "class -- but the inflow that opens every sub-step (euler_inflow) mixes every class's signal with weight sa / (dsa + sa), gives 0 where that sum is 0, and "
            "zeroes msa where sa <= 0: the marker is gone before any flux reads it, and nothing in a sub-step makes a NaN from finite signals (a NaN C_in is guarded).  "
            "The NaN-marker column of tests/sas_tiefree_columns.py holds exactly this state, its mtt is finite (test_sas_tiefree_reference.py), and this arm stays untaken "
            "with it.  Only a start state with NaN in a class that HOLDS water would take it, which neither solver leaves without a residue tie")
REASONS = (
    ("if ((oc_device_order() & 1) && ages <= 63)", CANNOT, _SWITCH),
    ("for (int i = 0; i < 64; ++i) w[i] =", CANNOT, _SWITCH),
    ("for (int64_t k = 0; k < ages; ++k) SA[k + 1] = (k == 0 ? 0.0 : w[k - 1])", CANNOT, _SWITCH),
    ("if (oc_device_order()", CANNOT, _SWITCH),
    ("if (A > 4096) abort();", CANNOT, _SWITCH),
    ("for (int64_t k = 0; k < A; ++k) ttn_direct[k] = 0;", CANNOT, _SWITCH),
    ("for (int64_t k = 0; k < A; ++k) {", CANNOT, _SWITCH + " (calc_tt's loop under bit 1)"),
    ("double q = (flux * t > sa[k] ? sa[k] : flux * t);", CANNOT, _SWITCH),
    ("tt[k] = (flux > 0 ? q / flux : 0);", CANNOT, _SWITCH),
    ("const double o = (S >= 0 ?", CANNOT, "S < 0: S is the maximum of a cumulative sum of non-negative classes that starts at 0"),
    ("} else if (code == 4) {", CANNOT, "a code of none of the reference's families is no input of the reference: the device reports it as an error "
     "(test_hip_sas.test_unknown_family_is_reported), and the oracle has no error flag and nothing to compare"),
    ("v = ((v > -1e-5) && (v < 0)) ? 0 : v;", TIE, "v <= -1e-5: a class debited by more than it holds plus 1e-5 mm; calc_tt clips every debit to the class, so only a residue of 1e-16 is ever negative"),
    ("m = (m > msa[k] ? msa[k] : m);", TIE, "the solute taken exceeds the class's solute: needs alpha * tt * flux > sa, which calc_tt's clip to the class rules out for alpha <= 1; a partition "
     "coefficient above 1 is no input of the reference's models"),
    ("const int crop = (P->lu_id[i] > 500)", CANNOT, "lu_id >= 599 behind lu_id > 500: the land-use table has no such id (crops are 501 .. 598)"),
    ("if ((P->lu_id[i] > 500)", CANNOT, "lu_id >= 599 behind lu_id > 500: the land-use table has no such id (crops are 501 .. 598)"),
    ("tt[k] = (d >= 0) ? d : 0;", CANNOT, "the differences of a cumulative sum of non-negative normalised increments are not negative (a rounding step down would need a negative term)"),
    ("double dmsa_rz = NZ(mtt_cpr[k])", CANNOT, "anion_mtt yields no NaN from finite state (its division is guarded by sa > 0)"),
    ("double dmsa_ss = NZ(mtt_qrz[k])", CANNOT, "anion_mtt yields no NaN from finite state (its division is guarded by sa > 0)"),
    ("dmsa_rz = (msa_rz[k] + dmsa_rz < 0) ? 0 : dmsa_rz;", TIE, "more solute leaves a class than it holds: each of up to three fluxes may take up to msa (anion_mtt's clamp), so it needs fluxes that "
     "together all but empty the class -- a clip, which a tie-free column must not take; no tie-tolerant anion problem under Euler / RK4 empties one either"),
    ("dmsa_ss = (msa_ss[k] + dmsa_ss < 0) ? 0 : dmsa_ss;", TIE, "as for the root zone on the line before"),
    ("const double dmsa_rz1 = (isnan(mtt_cpr[k])", CANNOT, _NAN_MTT),
    ("const double dmsa_ss1 = (isnan(mtt_qrz[k])", CANNOT, _NAN_MTT),
    ("for (int stage = 0; stage < 4; ++stage) {", CANNOT, "the loop leaves through `if (stage == 3) break`, never through its condition"),
)


def reason_for(src):
    for text, kind, why in REASONS:
        if src.startswith(text):
            return f"{kind}: {why}"
    return None


def build(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for f in glob.glob(os.path.join(out_dir, "*.gc*")):
        os.remove(f)
    so = os.path.join(out_dir, "libsas_oracle_cov.so")
    subprocess.run(["gcc", "-O0", "--coverage", "-fPIC", "-std=c11", "-ffp-contract=off", "-shared", "-o", so,
                    os.path.join(REPO, "oracle", SOURCE), "-lm"], check=True, cwd=out_dir)
    return so


def child(which):
    sys.path.insert(0, TESTS)
    sys.path.insert(0, REPO)
    import sas_binding as B

    B._lib = ctypes.CDLL(os.environ["SAS_ORACLE_COV_SO"])
    import test_hip_sas as H

    def days(st, n=3):
        for _ in range(n):
            st.step_oracle()

    def params_of(test, names):
        """The parameter list of a parametrised test, from its own mark: the tool follows the test."""
        (mark,) = [m for m in test.pytestmark if m.name == "parametrize" and m.args[0] == names]
        return mark.args[1]

    shapes = params_of(H.test_random_columns_against_oracle, "n,ages,substeps,stats")
    assert shapes == params_of(H.test_explicit_solver_random_columns_against_oracle, "n,ages,substeps,stats")
    for n, ages, substeps, stats in shapes:
        days(H.random_problem(n, ages, substeps, seed=ages + n, stats=stats))
        for solver in ("Euler", "RK4"):
            days(H.random_problem(n, ages, substeps, seed=7 * ages + n, stats=stats, solver=solver))
        print("random", n, ages, substeps, flush=True)
    for builder in (H.gamma_problems, H.closed_form_problems, H.fifth_root_problems):   # the problems those tests build, from the tests
        for _, _, st, *_ in builder():
            days(st, 1)
    for case in B.SAS_CASES + B.SOLVER_CASES + B.ANION_SOLVER_CASES + tuple(
            os.path.basename(p)[:-4] for p in sorted(glob.glob(os.path.join(B.GOLDEN, "sas_*.npz")))):
        if not os.path.exists(os.path.join(B.GOLDEN, f"{case}.npz")):
            continue
        g = B.SasGolden(case)
        st = g.new_state()
        for d in range(1, g.ndays + 1):
            g.load_state(st, d - 1)
            g.load_inputs(st, d)
            st.step_oracle()
        print("golden", case, flush=True)
    if which == "tiefree":
        import sas_tiefree_columns as T

        for c in T.CONFIGS + T.STAGED:
            T.reference_days(c)
        print("tie-free", len(T.CONFIGS + T.STAGED), "configurations", flush=True)


def function_ranges():
    """{function: (first line, last line)} of oracle/sas_oracle.c, from the column-0 definitions."""
    with open(os.path.join(REPO, "oracle", SOURCE)) as f:
        src = f.read().split("\n")
    starts = []
    for i, line in enumerate(src, 1):
        m = re.match(r"^(?:static )?(?:inline )?(?:void|double|int)\s+(\w+)\(", line)
        if m:
            starts.append((i, m.group(1)))
    out = {}
    for (a, name), (b, _) in zip(starts, starts[1:] + [(len(src) + 1, None)]):
        out[name] = (a, b - 1)
    return out


def untaken(out_dir):
    gcda = glob.glob(os.path.join(out_dir, "*.gcda"))
    if not gcda:
        raise RuntimeError(f"no .gcda in {out_dir}: the child did not exit normally")
    subprocess.run(["gcov", "-b", "-c", os.path.basename(gcda[0])], check=True, cwd=out_dir, stdout=subprocess.DEVNULL)
    counts, text = {}, {}
    line_re, branch_re = re.compile(r"^\s*([^:]+):\s*(\d+):(.*)$"), re.compile(r"^branch\s+(\d+)\s+(never executed|taken (\d+))")
    cur = None
    with open(os.path.join(out_dir, SOURCE + ".gcov")) as f:
        for raw in f:
            m = branch_re.match(raw)
            if m and cur is not None:
                k = (cur, int(m.group(1)))
                counts[k] = counts.get(k, 0) + (int(m.group(3)) if m.group(3) else 0)
                continue
            m = line_re.match(raw.rstrip("\n"))
            if m and int(m.group(2)) > 0:
                cur = int(m.group(2))
                text[cur] = m.group(3).strip()
    ranges = function_ranges()
    owner = {}
    for name in FUNCTIONS:
        a, b = ranges[name]
        for ln in range(a, b + 1):
            owner[ln] = name
    counts = {k: v for k, v in counts.items() if k[0] in owner and not ("mg_" in text[k[0]] or text[k[0]].startswith(("if (margin", "if (clip_only")))}
    rows = []
    for line in sorted({k[0] for k in counts}):
        on = sorted(b for (ln, b) in counts if ln == line)
        miss = [b for b in on if counts[(line, b)] == 0]
        if miss:
            rows.append((line, owner[line], text[line], miss, len(on)))
    return rows, (sum(1 for v in counts.values() if v > 0), len(counts))


def run(which, build_dir):
    out_dir = os.path.join(os.path.abspath(build_dir), which)
    so = build(out_dir)
    env = dict(os.environ, SAS_ORACLE_COV_SO=so, OMP_NUM_THREADS="1")
    env.pop("OC_SAS_DEVICE_ORDER", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], check=True, env=env, cwd=REPO)
    return untaken(out_dir)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("build_dir", nargs="?")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sas_branches.txt"))
    ap.add_argument("--child", choices=("existing", "tiefree"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.build_dir:
        ap.error("BUILD_DIR is required")
    lines = ["Branch directions of the step routines of oracle/sas_oracle.c that no input of the transport tests takes (tools/sas_branches.py:",
             "gcov -b -c on the oracle built with -O0 --coverage; the margin's own bookkeeping is left out).  `k of n`: the ordinals gcov gives",
             "the line's branch directions.  In the second list every line carries its reason.  CANNOT: no input takes the direction.",
             "TIE: a clip or snap that a tie-free column must not take; only the tie-tolerant inputs of the first list could.  GAP: a column",
             "could take it and no input set holds it.", ""]
    missing = 0
    for which, title in (("existing", "EXISTING: the random problems of tests/test_hip_sas.py and every SAS golden case"),
                         ("tiefree", "WITH THE TIE-FREE PROBLEMS: the same and tests/sas_tiefree_columns.py")):
        rows, (taken, total) = run(which, a.build_dir)
        lines += [title, f"{taken} of {total} branch directions taken ({100.0 * taken / total:.2f} %), {total - taken} not:", ""]
        for line, fn, src, miss, n in rows:
            lines.append(f"  {line:5d}  {fn}  [{','.join(map(str, miss))} of {n}]  {src}")
            if which == "tiefree":
                reason = reason_for(src)
                missing += reason is None
                lines.append(f"         -> {reason or 'NO REASON RECORDED'}")
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {a.out}" + (f"; {missing} lines of the second list carry no reason" if missing else ""))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
