#!/usr/bin/env python
"""Which branch directions of roger_amd/csrc/rh_physics.h do the host-side walks take?  CPU only, not a test.

    python tools/physics_branches.py BUILD_DIR [--out profiles/physics_branches.txt]

The physics is written as selects: every line runs, but one arm of a select may never be chosen, and line coverage does not see
that.  This tool builds tests/host_physics.cpp (the device's column code compiled for the host) with `-O0 --coverage` into
BUILD_DIR/before and BUILD_DIR/after, runs in a fresh child process each

  before   the walks of tests/test_physics_host_vs_oracle.py and tests/test_physics_host_vs_oracle_crops.py (every parametrisation,
           and the setup kernels on their columns) and a walk from the start state of every SVAT and oneD golden case through its
           own forcing (the weighted and the station-mapped cases with their per-cell forcing)
  after    the same plus the walks and the setup kernels of tests/test_physics_host_vs_oracle_edges.py (tests/edge_columns.py)

then `gcov -b -c`, and writes every branch direction of rh_physics.h that no walk took, with line number and source text, to the
output file: both lists, and for every direction of the "after" list the reason it stays untaken (REASONS below, by line number,
source text and ordinals -- a line without one is marked, and the tool exits with status 1; so it does when a walk from a golden case
disagrees with the oracle).  A reason is either CANNOT (no reachable finite state takes the direction) or GAP (a state could, and no
column set holds it: an open gap in the coverage).  The .gcda files are written when the child exits,
which is why BUILD_DIR is a directory of the caller's and not a temporary one."""
import argparse
import glob
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")
HEADER = "rh_physics.h"

CANNOT, GAP = "CANNOT", "GAP"
# line of rh_physics.h: (how the line's source text begins, the ordinals that may stay untaken, CANNOT or GAP, the reason).
# CANNOT: no finite state the model can reach takes the direction; GAP: a state could, and no column set holds it -- an open gap in the
# coverage, not a claim about the code.  A line whose text no longer begins as recorded, or with another ordinal untaken, counts as
# having no reason: edits to rh_physics.h cannot move a reason to another select unnoticed.
REASONS = {
    58: ('const double cap_top = (c.S_int_top_tot < wtmx ?', (0,), CANNOT,
           'rt_snow leaves swe_top at exactly 0 (h_melt: swe += -swe), so wtmx = 0 here and S_int_top_tot is not negative'),
    70: ('c.int_rain_ground = ((room < want) && liquid && ', (3,), CANNOT,
           '`liquid` false behind room < want: with frost rain = 0, so want = 0, and room >= 0 is never below it'),
    93: ('c.int_snow_ground = ((room < want) && frozen && ', (3,), CANNOT,
           '`frozen` false behind room < want: without frost snow = 0, so want = 0, and room >= 0 is never below it'),
    151: ('c.pet_res = (c.pet_res < 0 ? 0.0 : c.pet_res) * ', (0,), CANNOT,
           'pet_res is debited by at most its own value (the selects ahead take min(pet_res, store)): never negative'),
    154: ('c.pet_res = (c.pet_res < 0 ? 0.0 : c.pet_res) * ', (0,), CANNOT,
           'pet_res is debited by at most its own value (the selects ahead take min(pet_res, store)): never negative'),
    170: ('c.transp_coeff = ((r >= 0) && (r <= 1) ? 1 - rh_', (1,), CANNOT,
           'r < 0 needs a negative S_lp_rz or S_ac_rz'),
    191: ('m = (c.S_fp_rz > 0) && (c.ptransp_res > c.S_fp_r', (5,), GAP,
           "S_lp_rz > 0 behind ptransp_res > S_fp_rz > 0: the large pores are debited only on line 195, so it is taken where they hold less than the demand and the rest exceeds the fine pores' water, or in a wet step with ptransp > S_fp_rz: fine pores all but empty under water in the large pores, which no column set holds"),
    212: ('melt = ((pot > 0) && (pot <= swe) && (swe > 0) ?', (5,), CANNOT,
           '`swe > 0` false behind 0 < pot <= swe: swe >= pot > 0'),
    214: ('const bool part = (melt > 0) && (melt <= swe), f', (3,6,), CANNOT,
           'h_melt: melt is `pot` where pot <= swe and `swe` where pot > swe, never above swe, so `full` is false'),
    219: ('swe += (full ? 0.0 : -swe) * mk;', (0,), CANNOT,
           'h_melt: melt is `pot` where pot <= swe and `swe` where pot > swe, never above swe, so `full` is false'),
    221: ('swe = (full ? 0.0 : swe) * mk;', (0,), CANNOT,
           'h_melt: melt is `pot` where pot <= swe and `swe` where pot > swe, never above swe, so `full` is false'),
    236: ('c.pet_res = (c.pet_res < 0 ? 0.0 : c.pet_res) * ', (0,), CANNOT,
           'pet_res is debited by at most its own value (the selects ahead take min(pet_res, store)): never negative'),
    241: ('c.snow_melt_drip = (q_ret > wtmx ? q_ret - wtmx ', (3,4,), CANNOT,
           'h_melt has left swe_top at exactly 0 (swe += -swe), so wtmx = 0 and q_ret = S_int_top; with `over`, S_int_top > S_int_top_tot >= 0 and `q_ret > wtmx` has the column: `wtmx <= 0` is never false and never met with `over` true'),
    264: ('v = (z_soil <= 0 ? 0.01 : v) * mk;', (0,), CANNOT,
           'z_soil <= 0 gives z_root = 0 and the initial conditions compute 0 / 0 (line 1416): the reference starts such a column as NaN; taken out of the column set'),
    277: ('const double v = (c.z_soil > 0 ? (c.theta_fc - c', (1,), CANNOT,
           'z_soil <= 0 gives z_root = 0 and the initial conditions compute 0 / 0 (line 1416): the reference starts such a column as NaN; taken out of the column set'),
    408: ('c.z0 = (c.z0 < 0 ? 0.0 : c.z0) * mk;', (0,), CANNOT,
           'z0 is a sum of non-negative terms, and what is subtracted here was clamped to at most z0 just before'),
    413: ('w0 += (isfinite(d0) ? d0 : 0.0) * mk;', (2,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    415: ('w0 = (w0 > c.z_soil ? c.z_soil : w0) * mk;', (0,), CANNOT,
           'the front is at most z_wf_fc <= z_soil (h_pause_start clamps z_wf_fc) or was clamped to z_soil on the line before'),
    417: ('w1 += (isfinite(d1) ? d1 : 0.0) * mk;', (2,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    419: ('w1 = (w1 > c.z_soil ? c.z_soil : w1) * mk;', (0,), CANNOT,
           'the front is at most z_wf_fc <= z_soil (h_pause_start clamps z_wf_fc) or was clamped to z_soil on the line before'),
    433: ('c.z_wf = (c.z_wf > c.z_soil ? c.z_soil : c.z_wf)', (0,), CANNOT,
           'the front is at most z_wf_fc <= z_soil (h_pause_start clamps z_wf_fc) or was clamped to z_soil on the line before'),
    434: ('c.theta_d = (c.theta_d_t1 <= 0 ? c.theta_d_t0 : ', (1,), CANNOT,
           'theta_d_t1 is written nowhere in the file: it holds the 0 it was allocated with'),
    468: ('return (y < r ? r : y) * mk;', (0,), CANNOT,
           'y = r + sqrt(..) * mk with a non-negative root: not below r'),
    526: ('for (int it = 0; it < (dry ? 0 : substeps); ++it', (0,), GAP,
           '`dry` is set by the DryPath<true> instantiation alone, which only the fused step uses: tools/substep_dry_check.cpp and the device tests run it, the host routines do not'),
    534: ('b2 = (isnan(b2) ? 0.0 : b2) * mk;', (1,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    540: ('y = (y < r ? r : y) * mk;', (0,), CANNOT,
           'y = y1 + y2 + ym1 with y1, y2 >= 0 and ym1 >= r after the first sub-step; in the first, y1 + y2 >= r is the inequality of the two means'),
    541: ('y = (y < ym1 ? ym1 : y) * mk;', (0,), CANNOT,
           'y = y1 + y2 + ym1 with y1 = cb / theta_d / 2 >= 0 and y2 = a / cb / 2 >= 0 (cb, a >= 0, theta_d > 0), then raised to r: never below ym1'),
    549: ('inf = (inf < 0 ? 0.0 : inf) * mk;', (0,), CANNOT,
           'inf is a sum of non-negative di'),
    563: ('share = (share > 1 ? 1.0 : share) * mk;', (0,), CANNOT,
           'share = 1 - (lmpv - z_root) / lmpv_non_sat with lmpv > z_root on this path (line 560 has the rest): below 1'),
    583: ('c.z0 = (c.z0 < 0 ? 0.0 : c.z0) * mk;', (0,), CANNOT,
           'z0 is a sum of non-negative terms, and what is subtracted here was clamped to at most z0 just before'),
    628: ('for (int it = 0; it < (dry ? 0 : substeps); ++it', (0,), GAP,
           '`dry` is set by the DryPath<true> instantiation alone, which only the fused step uses: tools/substep_dry_check.cpp and the device tests run it, the host routines do not'),
    641: ('if (h_same(t, t_in) && h_same(ym1, ym1_in) && h_', (8,), CANNOT,
           'ecs changes only by di > 0, and then ym1 = ecs / l_sc / 2 changes with it (short of two neighbouring doubles that the division rounds together): with t and ym1 unchanged ecs is unchanged'),
    647: ('c.z0 = (c.z0 < 0 ? 0.0 : c.z0) * mk;', (0,), CANNOT,
           'z0 is a sum of non-negative terms, and what is subtracted here was clamped to at most z0 just before'),
    672: ('c.q_hof = (c.q_hof < 0 ? 0.0 : c.q_hof) * mk;', (0,), CANNOT,
           'z0 is a sum of non-negative terms, and what is subtracted here was clamped to at most z0 just before'),
    673: ('const bool full = ((c.S_lp_rz + c.S_fp_rz) > (c.', (0,2,3,), CANNOT,
           'lines 657-665 leave S_fp_rz <= S_ufc_rz and S_lp_rz <= S_ac_rz and rounding is monotonic: the sum is never above S_ac_rz + S_ufc_rz, q_sof stays 0'),
    674: ('c.q_sof = (full ? (c.S_lp_rz + c.S_fp_rz) - (c.S', (0,), CANNOT,
           'lines 657-665 leave S_fp_rz <= S_ufc_rz and S_lp_rz <= S_ac_rz and rounding is monotonic: the sum is never above S_ac_rz + S_ufc_rz, q_sof stays 0'),
    676: ('c.S_fp_rz = (m ? c.S_ufc_rz : c.S_fp_rz) * mk;', (0,), CANNOT,
           'lines 657-665 leave S_fp_rz <= S_ufc_rz and S_lp_rz <= S_ac_rz and rounding is monotonic: the sum is never above S_ac_rz + S_ufc_rz, q_sof stays 0'),
    677: ('c.S_lp_rz = (m ? c.S_ac_rz : c.S_lp_rz) * mk;', (0,), CANNOT,
           'lines 657-665 leave S_fp_rz <= S_ufc_rz and S_lp_rz <= S_ac_rz and rounding is monotonic: the sum is never above S_ac_rz + S_ufc_rz, q_sof stays 0'),
    682: ('c.z0 = (c.z0 < 0 ? 0.0 : c.z0) * mk;', (0,), CANNOT,
           'z0 is a sum of non-negative terms, and what is subtracted here was clamped to at most z0 just before'),
    786: ('double q = ((perc > 0) && (avail >= perc) && abo', (5,), CANNOT,
           '`above` (z_root_m1 < z_soil - z_sat) false behind perc > 0: perc > 0 needs z_sat <= 0 or m3 (z_root < z_soil - z_sat), and z_root_m1 == z_root (lines 1307-1308)'),
    787: ('q = ((perc > 0) && (avail < perc) && above ? c.S', (5,), CANNOT,
           '`above` (z_root_m1 < z_soil - z_sat) false behind perc > 0: perc > 0 needs z_sat <= 0 or m3 (z_root < z_soil - z_sat), and z_root_m1 == z_root (lines 1307-1308)'),
    789: ('q = ((q > 0) && (room > 0) && (q > room) && abov', (3,6,), CANNOT,
           '`room > 0` false behind q > 0: room <= 0 means both subsoil stores are at capacity, then z_sat = S_ac_ss / theta_ac is dz_ss (to an ulp), neither z_sat <= 0 nor m3 holds and perc = 0; `above` false behind q > 0: q > 0 was formed under `above` on lines 786-787'),
    790: ('q = ((c.S_lp_ss >= c.S_ac_ss - 1e-6) && (c.S_fp_', (2,), CANNOT,
           "the fine pores short of S_ufc_ss under large pores at S_ac_ss: every routine fills the subsoil's large pores only above full fine pores and empties them first (h_split_theta, lines 573-575, 803-805, 845-848, 971-980); S_ac_ss <= 1e-6 would do it too and is not drawn"),
    796: ('const bool m1 = (c.S_lp_rz < c.q_pot_rz) && abov', (3,), CANNOT,
           'z_sat >= dz_ss behind S_lp_rz < q_pot_rz: q_pot_rz > 0 survives line 791 only where z_root_m1 < z_soil - z_sat, which is z_sat < dz_ss'),
    889: ('mp = (mp < 0 ? 0.0 : mp) * mk;', (0,), CANNOT,
           'mp is a sum of products of layer thicknesses clamped at 0 (h_layer), table velocities, dmph and positive constants: not negative'),
    907: ('share = (isnan(share) ? 0.0 : share) * mk;', (1,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    970: ('const bool up = (q > 0) && geo;', (3,), GAP,
           "`geo` false behind q > 0: the wetting front below the root zone over a subsoil saturated to the top (z_sat >= z_soil - z_root) while the root zone's large pores are empty and it is drier than the subsoil; no column set holds that state"),
    1040: ('RH_DEV double h_nan0(double x) { return isnan(x)', (1,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    1047: ('bool close = (isfinite(lhs) && isfinite(rhs)) ? ', (2,5,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    1050: ('const bool lower = (a > -K.atol) && (b > -K.atol', (1,3,5,7,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1051: ('const bool upper = (a - K.atol <= h_nan0(c.S_ufc', (5,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1052: ('(d - K.atol <= h_nan0(c.S_ufc_ss)) && (e - K.ato', (1,5,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1053: ('return !(close && lower && upper);', (3,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1060: ('bool close = (isfinite(lhs) && isfinite(rhs)) ? ', (2,5,), CANNOT,
           'no walk feeds this guard a NaN or an infinity; a column that is NaN from the start (z_soil = 0) would, and is not drawn'),
    1063: ('const bool lower = (a > -K.atol) && (b > -K.atol', (1,3,5,7,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1064: ('const bool upper = (a - K.atol <= h_nan0(c.S_ufc', (5,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1065: ('(d - K.atol <= h_nan0(c.S_ufc_ss)) && (e - K.ato', (1,5,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1066: ('return !(close && lower && upper);', (3,), CANNOT,
           "the sanity check's failing arms: a store outside its bounds or a balance that does not close, which no sound step leaves"),
    1168: ('RH_DEV double h_snap0(double x) { return ((x > -', (0,1,2,3,), GAP,
           "h_snap0 is called by rt_after_timestep_oned alone, which no host-side walk runs (the walks end a step with the oracle's after_timestep); the device tests of the oneD model run it"),
    1192: ('c.maskCatch = (c.lu_id != 14) && (c.lu_id != 20)', (7,), GAP,
           'maskCatch = 0 on the way in: every column set starts from maskCatch = 1 (extended_columns.load_primaries)'),
    1203: ('const bool low_veg = (lu == 0) || (lu >= 5 && lu', (1,), CANNOT,
           "an artefact of the compiled form: all evaluations pass on to the second test although lu_id 0 columns are among them (their planes match the oracle's): the front end folds this chain's comparisons into range tests, the ordinal is no arm of the source"),
    1204: ('(lu == 40) || (lu == 41) || (lu == 50) || (lu ==', (6,), GAP,
           "lu_id 60 is listed here and has no row in the goldens' look-up tables (h_lut_row falls back to row 0); no column set draws it"),
    1298: ('(lu == 40) || (lu == 41) || (lu == 50) || (lu ==', (6,), GAP,
           "lu_id 60 is listed here and has no row in the goldens' look-up tables (h_lut_row falls back to row 0); no column set draws it"),
    1287: ('s = (s < 0 ? 0.0 : s) * mk;', (0,), CANNOT,
           'sand below 0 needs a negative theta_ac, which is no porosity'),
    1297: ('const bool listed = (lu == 0) || (lu >= 5 && lu ', (1,), CANNOT,
           "an artefact of the compiled form: all evaluations pass on to the second test although lu_id 0 columns are among them (their planes match the oracle's): the front end folds this chain's comparisons into range tests, the ordinal is no arm of the source"),
}


def reason_for(line, src, miss):
    """The recorded reason, if the line still begins as recorded and no other ordinal is untaken; else None."""
    entry = REASONS.get(line)
    if entry is None:
        return None
    text, ordinals, kind, why = entry
    if not src.startswith(text) or not set(miss) <= set(ordinals):
        return None
    return f"{kind}: {why}"


def build(out_dir):
    sys.path.insert(0, TESTS)
    import host_physics as HP

    os.makedirs(out_dir, exist_ok=True)
    for f in glob.glob(os.path.join(out_dir, "*.gc*")):
        os.remove(f)
    so = os.path.join(out_dir, "libhost_physics.so")
    subprocess.run(HP.compile_command(so, extra=("-O0", "--coverage", "-shared", "-fPIC")), check=True, cwd=out_dir)
    return so


def host_setup(ob, HP, p, luts, lateral, extra=None):
    """The four setup routines of the host-compiled code on the primaries p."""
    import extended_columns as E

    a = ob.OracleState(int(p["lu_id"].size))
    E.load_primaries(a, p, luts, lateral)
    host = HP.HostColumns(a)
    X = HP.StepCtx(month_tau=int(a.scal.month[1]), sel_p=-1, sel_w=-1)
    for name in ("rt_topo", "rt_params_surface", "rt_params_soil"):
        host.call(name, X)
    if lateral:
        a.params_lateral(luts[4])
    E.load_initial_state(a, p)
    if extra is not None:
        extra(a, p)
    host.call("rt_initial_conditions", X)


def golden_walks(ob, T):
    import golden_util as G

    for case in G.CASES + G.WEIGHTED_CASES + G.STATION_CASES:
        g, names, F = G.load_case(case)
        if "state0" not in g.files:
            continue
        lateral = G.is_lateral(g)
        nx, ny = (int(v) for v in g["nx_ny"])
        st = ob.OracleState(nx * ny)
        st.load_snapshot(g["state0"], names)
        st.load_scalars(g["scal0"])
        st.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
        G.configure_settings(st.settings, g)
        driver = ob.ForcingDriver(F, weights=G.load_weights(g), stations=G.load_stations(g))
        bad, census = T.walk_from(ob, st, F, lateral, driver=driver)
        print(f"golden {case}: {census['steps']} steps, {nx * ny} columns, mismatching routines: {sorted(bad)}", flush=True)
        if bad:     # the walk compares every routine with the oracle: a disagreement is a finding, not a measurement
            raise SystemExit(f"golden {case}: the host-compiled routines part from the oracle\n" + "\n".join(m for v in bad.values() for m in v))


def child(which):
    """Runs the walks against the library HOST_PHYSICS_SO names."""
    sys.path.insert(0, TESTS)
    sys.path.insert(0, REPO)
    import crop_columns as CC
    import extended_columns as E
    import host_physics as HP
    import oracle_binding as ob
    import test_physics_host_vs_oracle as T
    import test_physics_host_vs_oracle_crops as TC

    ob.build()
    HP.lib()
    for w in T.WALKS:
        T.walk(*w)
        print("walk", T._id(w), flush=True)
    for lateral in (False, True):
        for gw in ("mixed", "above_soil_base"):
            host_setup(ob, HP, E.extended_params(T.NX, T.NY, T.SEED, gw, "interleaved"), T._luts(lateral), lateral)
        for layout in ("interleaved", "blocks"):
            host_setup(ob, HP, CC.crop_params(T.NX, T.NY, TC.SEED, layout), T._luts(lateral), lateral)
    for w in TC.WALKS:
        TC.crop_walk(*w)
        print("crop walk", TC._id(w), flush=True)
    golden_walks(ob, T)
    if which == "after":
        import edge_columns as EC
        import test_physics_host_vs_oracle_edges as TE

        for w in TE.WALKS:
            TE.edge_walk(*w)
            print("edge walk", TE._id(w), flush=True)
        for lateral in (False, True):
            for layout in TE.LAYOUTS:
                host_setup(ob, HP, EC.edge_params(T.NX, T.NY, EC.SEED, layout), T._luts(lateral), lateral, extra=EC.load_pack)


def untaken(out_dir):
    """[(line number, source text, [untaken branch ordinals], branches on the line)], and (taken, total) over the header."""
    gcda = glob.glob(os.path.join(out_dir, "*.gcda"))
    if not gcda:
        raise RuntimeError(f"no .gcda in {out_dir}: the child did not exit normally")
    subprocess.run(["gcov", "-b", "-c", os.path.basename(gcda[0])], check=True, cwd=out_dir, stdout=subprocess.DEVNULL)
    counts, text = {}, {}
    line_re, branch_re = re.compile(r"^\s*([^:]+):\s*(\d+):(.*)$"), re.compile(r"^branch\s+(\d+)\s+(never executed|taken (\d+))")
    cur = None
    with open(os.path.join(out_dir, HEADER + ".gcov")) as f:
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
    rows = []
    for line in sorted({k[0] for k in counts}):
        on = sorted(b for (ln, b) in counts if ln == line)
        miss = [b for b in on if counts[(line, b)] == 0]
        if miss:
            rows.append((line, text[line], miss, len(on)))
    return rows, (sum(1 for v in counts.values() if v > 0), len(counts))


def run(which, build_dir):
    out_dir = os.path.join(os.path.abspath(build_dir), which)
    so = build(out_dir)
    env = dict(os.environ, HOST_PHYSICS_SO=so)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], check=True, env=env, cwd=REPO)
    return untaken(out_dir)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("build_dir", nargs="?")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "physics_branches.txt"))
    ap.add_argument("--child", choices=("before", "after"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.build_dir:
        ap.error("BUILD_DIR is required")
    lines = ["Branch directions of roger_amd/csrc/rh_physics.h that no host-side walk takes (tools/physics_branches.py: gcov -b -c on",
             "tests/host_physics.cpp built with -O0 --coverage).  `k of n`: the ordinals gcov gives the line's branch directions.",
             "In the AFTER list every line carries its reason.  CANNOT: no finite state the model can reach takes the direction.  GAP: a state",
             "could take it and no column set holds that state -- an open gap in the coverage, not a property of the code.", ""]
    missing = 0
    for which, title in (("before", "BEFORE: the extended and the crop columns, and a walk from every SVAT / oneD golden case"),
                         ("after", "AFTER: the same and the edge columns (tests/edge_columns.py)")):
        rows, (taken, total) = run(which, a.build_dir)
        lines += [title, f"{taken} of {total} branch directions taken ({100.0 * taken / total:.2f} %), {total - taken} not:", ""]
        for line, src, miss, n in rows:
            lines.append(f"  {line:5d}  [{','.join(map(str, miss))} of {n}]  {src}")
            if which == "after":
                reason = reason_for(line, src, miss)
                missing += reason is None
                lines.append(f"         -> {reason or 'NO REASON RECORDED'}")
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {a.out}" + (f"; {missing} lines of the after list carry no reason" if missing else ""))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
