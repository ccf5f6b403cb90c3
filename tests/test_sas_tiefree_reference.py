"""The conditions that the reference alone must meet on the tie-free problems (tests/sas_tiefree_columns.py), on the CPU:

* every unmasked column of every configuration that tests/test_hip_sas_tiefree.py runs keeps a clip and snap margin of 1e-6 on each
  of the three days (oc_sas_step_margin);
* every SAS variant (code, and exact exponent) appears for every flux in at least three unmasked columns of every configuration
  group, every dirac threshold in every group, and the special columns are present and tie-free;
* the criterion holds what it promises on the stand-in the project has for the device's summation order: the oracle under
  OC_SAS_DEVICE_ORDER=7 (the wave scan's association, directly accumulated sub-step distributions and the kernel's treatment of the
  reversed exponential; it applies to ages <= 63 and to the deterministic solver, isotopes and anions) agrees
  with the oracle under 0 on every tie-free column in every output, rtol 1e-10 / atol 1e-12, NaN patterns included.  The switch is read
  once per process, so the other order runs in a child process.

Inputs that miss a condition are wrong inputs: the generator's ranges change, not the bar."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sas_tiefree_columns as T
from sas_binding import FLUXES

ALL = T.CONFIGS + T.STAGED
# The stand-in restates the deterministic solver's kernel.  Under Euler and RK4 it is no stand-in: its cumulative StorAge steps by an ulp
# of either sign over an exactly empty class, the explicit limiter `diff(SA) + ttq < 0` reads that step directly and founds a whole
# distribution on it, while the kernels' block scan keeps the upper edge of an empty class equal to its lower one (blk_cumsum).
SMALL = [c for c in ALL if c[1] <= 63 and c[5] == "deterministic"]


@pytest.mark.parametrize("c", ALL, ids=T.cfg_id)
def test_every_unmasked_column_is_tiefree(c):
    st = T.problem_of(c)
    keep = st.maskCatch != 0
    assert 0 < np.count_nonzero(~keep) < st.n
    for day, (_, margin) in enumerate(T.reference_days(c)):
        print(f"MARGIN {T.cfg_id(c)} day {day}: min {margin[keep].min():.3g}")
        assert (margin[keep] >= T.TIEFREE_MARGIN).all(), \
            f"day {day}: columns {np.flatnonzero(keep & (margin < T.TIEFREE_MARGIN))} are not tie-free, margins {margin[keep & (margin < T.TIEFREE_MARGIN)]}"
        assert (margin[~keep] == 1.0).all()      # a masked column decides nothing


@pytest.mark.parametrize("group", list(T.GROUPS))
def test_every_variant_appears_for_every_flux(group):
    """Per group and flux: every variant (each code, and for code 6 the free exponent and each of the exact 0.5, 1.5, 1.0, 0.2) in at
    least three unmasked columns, with the code and exponent the variant names; per group every dirac threshold."""
    cfgs = T.GROUPS[group]
    variants = T.variants_for(cfgs[0][5])
    assert {c for c, _ in variants} | {4} == set(T.CODES)
    thr = set()
    for j, f in enumerate(FLUXES):
        count = np.zeros(len(variants), int)
        for c in cfgs:
            st = T.problem_of(c)
            keep = T.rotated_columns(c, st)
            v = T.rotated_variants(c, st)[f]
            p = st.sas[f][keep]
            count += np.bincount(v, minlength=len(variants))
            for vi, (code, expo) in enumerate(variants):
                assert (p[v == vi, 0] == code).all()
                assert expo is None or (p[v == vi, 1] == expo).all()
            thr |= {T.dirac_thresholds(c[1]).index(float(x)) for x in p[p[:, 0] == 2, 1]}
        print(f"VARIANTS {group} {f}: {dict(zip([f'{c}' if e is None else f'{c}^{e}' for c, e in variants], count.tolist()))}")
        assert count.min() >= 3, (group, f, count)
    assert thr == set(range(7)), (group, thr)


@pytest.mark.parametrize("c", ALL, ids=T.cfg_id)
def test_special_columns_are_present_and_tiefree(c):
    """The columns that hold a branch direction no other input takes: unmasked, as described, tie-free on every day, and the reference
    takes the direction on them (the unlabelled column's flux signals are NaN, the NaN inflow leaves finite stores)."""
    st = T.problem_of(c)
    u, nn = T.SPECIAL["unlabelled"], T.SPECIAL["nan_in"]
    assert st.maskCatch[u] == 1 and st.maskCatch[nn] == 1
    days = T.reference_days(c)
    if not st.anion:
        assert st.inp["C_in"][u] == 0 and not st.state["msa_rz"][u].any() and not st.state["msa_ss"][u].any()
        taken = [f for f in FLUXES if st.inp[f][u] > 0 and days[0][0][f"tt_{f}"][u].sum() > 0]
        assert taken, "the unlabelled column has no flux that takes water"
        for snap, margin in days:
            assert margin[u] >= T.TIEFREE_MARGIN
            assert all(np.isnan(snap[f"C_{f}"][u]) for f in taken)
    if c[5] != "deterministic":
        assert np.isnan(st.inp["C_in"][nn]) and min(st.inp[k][nn] for k in ("inf_mat_rz", "inf_pf_rz", "inf_pf_ss")) > 0
        for snap, margin in days:
            assert margin[nn] >= T.TIEFREE_MARGIN
            assert np.isfinite(snap["msa_rz"][nn]).all() and np.isfinite(snap["msa_ss"][nn]).all()
    else:
        assert np.isfinite(st.inp["C_in"]).all()
    if T.has_nan_mtt(c[4], c[5]):
        # the NaN-marker column: at the start of every day the root zone's oldest class is empty and carries the marker (on the first day
        # the subsoil's too), both pistons select that class (tt = 1 over no water) -- and no NaN reaches a distribution, a flux signal
        # or a store: the inflow that opens every sub-step mixes the marker with weight 0 / 0 -> 0 before any flux reads it
        m = T.SPECIAL["nan_mtt"]
        assert st.maskCatch[m] == 1
        start = {k: st.state[k][m] for k in st.state}
        assert start["sa_ss"][-1] == 0 and np.isnan(start["msa_ss"][-1])
        for snap, margin in days:
            assert margin[m] >= T.TIEFREE_MARGIN
            assert start["sa_rz"][-1] == 0 and np.isnan(start["msa_rz"][-1])
            assert snap["tt_q_rz"][m, -1] == 1 and snap["tt_cpr_rz"][m, -1] == 1 and snap["sa_ss"][m, -1] > 0
            assert np.isfinite(snap["mtt_q_rz"][m]).all() and np.isfinite(snap["mtt_cpr_rz"][m]).all()
            assert np.isfinite(snap["msa_ss"][m]).all() and np.isfinite(snap["C_ss"][m]) and np.isfinite(snap["msa_rz"][m, :-1]).all()
            start = {k: snap[k][m] for k in st.state}


def test_problem_holds_what_its_docstring_says():
    """Both clamps of S_rel for both stores, every dirac threshold, the exact exponents, empty classes, zero cases."""
    for c in (T.GROUPS["deterministic"][1], T.GROUPS["RK4"][4], T.GROUPS["bromide"][2]):
        st = T.problem_of(c)
        keep = st.maskCatch != 0
        assert st.state["sa_rz"][:, 0].max() == 0 and st.state["sa_ss"][:, 0].max() == 0
        share = (st.state["sa_rz"] == 0).mean()
        assert 0.1 < share < 0.2, share
        assert np.array_equal(st.state["sa_rz"] == 0, st.state["sa_ss"] == 0)
        for f in FLUXES:
            p = st.sas[f][keep]
            S = st.state[f"sa_{T.SOURCE[f]}"].sum(axis=1)[keep]
            assert (S < p[:, 5]).any() and ((S > p[:, 5]) & (S < p[:, 6])).any() and (S > p[:, 6]).any(), f
            assert (st.inp[f][keep] == 0).any() and (st.inp[f][keep] > 0).any(), f
        for k in ("inf_mat_rz", "inf_pf_rz", "inf_pf_ss"):
            assert (st.inp[k][keep] == 0).any() and (st.inp[k][keep] > 0).any(), k


def _outputs(c):
    return [snap for snap, _ in T.reference_days(c)]


def child(path):
    """Every small configuration under the environment's OC_SAS_DEVICE_ORDER into one .npz."""
    out = {}
    for j, c in enumerate(SMALL):
        for day, snap in enumerate(_outputs(c)):
            for k, a in snap.items():
                out[f"c{j}_d{day}_{k}"] = a
    np.savez(path, **out)


def test_device_order_agrees_on_tiefree_columns(tmp_path):
    path = str(tmp_path / "other_order.npz")
    env = dict(os.environ, OC_SAS_DEVICE_ORDER="7")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=os.path.dirname(os.path.abspath(__file__)))
    other = np.load(path)
    assert os.environ.get("OC_SAS_DEVICE_ORDER", "0") == "0"
    differs = 0
    for j, c in enumerate(SMALL):
        st = T.problem_of(c)
        keep = st.maskCatch != 0
        for day, snap in enumerate(_outputs(c)):
            pre = f"c{j}_d{day}_"
            differs += any(not np.array_equal(other[pre + k], a, equal_nan=True) for k, a in snap.items())
            T.assert_columns_agree(lambda k: other[pre + k], lambda k: snap[k], list(snap), keep, f"{T.cfg_id(c)} day {day}", stat_rtol=1e-10)
    assert differs > 0, "the other summation order changed no bit: the switch did not reach the child"


if __name__ == "__main__":
    child(sys.argv[1])
