"""The transport kernels on tie-free columns (tests/sas_tiefree_columns.py) at every shape boundary of both launchers: three days in a
row from the device's own state against the oracle's same days, EVERY unmasked column in EVERY output and state array at the project's
tolerances -- rtol 1e-10 / atol 1e-12, age statistics rtol 1e-9, NaN patterns identical, msa where sa > 0, mtt through mtt * tt.  No
allowed count, no share of tight columns, no loose bound; C_s, C_iso_s and msa_s included (sas_binding.TIE_WIPED is about ties).  Masked
columns give the oracle's values.  That the inputs are tie-free is a property of the reference alone, which
tests/test_sas_tiefree_reference.py asserts on the CPU for every configuration used here.

Both launchers compare nages = ages + 1 (rh_sas_kernels.h: 64, 128, 256, 512, 1024, 2048, 4096; rh_sas_solvers_impl.h: 64, 256, 512,
1024, 2048): each boundary is stepped with the last axis of a shape, the one before it (the last thread holds one class less) and the
first of the next shape (the last thread holds a single class)."""
import pytest

import sas_tiefree_columns as T
from test_hip_sas import make_ctx, pull, push, step_fused_and_staged

pytestmark = pytest.mark.gpu


def run_days(c):
    st = T.problem_of(c)
    keep = st.maskCatch != 0
    ctx = make_ctx(st)
    push(ctx, st)                      # later days continue from the device's own state with the same inputs
    for day, (want, margin) in enumerate(T.reference_days(c)):
        ctx.step(0)
        pull(ctx, st)
        names = list(st.out) + list(st.state)
        got_of = lambda k: st.out[k] if k in st.out else st.state[k]  # noqa: E731
        T.assert_columns_agree(got_of, lambda k: want[k], names, keep, f"{T.cfg_id(c)} day {day}")
        # a masked column: the oracle's values (zeros, and its untouched state)
        T.assert_columns_agree(got_of, lambda k: want[k], names, ~keep, f"{T.cfg_id(c)} day {day} masked")
    ctx.close()


@pytest.mark.parametrize("c", T.GROUPS["deterministic"], ids=T.cfg_id)
def test_deterministic_solver_at_every_shape_boundary(c):
    run_days(c)


@pytest.mark.parametrize("c", T.GROUPS["Euler"] + T.GROUPS["RK4"], ids=T.cfg_id)
def test_explicit_solvers_at_every_shape_boundary(c):
    run_days(c)


@pytest.mark.parametrize("c", T.GROUPS["bromide"] + T.GROUPS["chloride"] + T.GROUPS["virtualtracer"] + T.GROUPS["bromide-Euler"]
                         + T.GROUPS["bromide-RK4"], ids=T.cfg_id)
def test_anion_kernels_at_the_last_axis_of_every_shape(c):
    run_days(c)


@pytest.mark.parametrize("c", T.STAGED, ids=T.cfg_id)
def test_stage_by_stage_equals_fused_at_shape_boundaries(c):
    """test_hip_sas.test_stage_by_stage_equals_fused at 64 / 65, 512 / 513 and 1024 / 1025 age points: the reference's kernels one launch
    at a time give the fused step bit for bit (age statistics of a launch of their own: 1e-12, as there)."""
    st = T.problem_of(c)
    fused, split = make_ctx(st), make_ctx(st)
    push(fused, st)
    push(split, st)
    for day in range(2):
        assert step_fused_and_staged(fused, split) > 20, day
    fused.close()
    split.close()
