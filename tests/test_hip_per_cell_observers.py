"""GPU: the five device observers -- accumulators (k_diag), points (k_points), catchment totals (k_totals_*), zonal totals (k_zonal_*) and
scores (k_scores) -- behind steps with PER-CELL forcing (rh_set_forcing_weights, rh_set_forcing_stations), tolerance zero.

With per-cell forcing the step takes other code than the observer tests of test_hip_points / _totals / _zonal / _scores / _diag_kernel pin
(roger_amd/csrc/rh_stepping.h: step_fused_launches): the one-launch front k_cell_front (or its split pair) forms the control part and
runs the set_forcing hook, the fused kernel follows with RH_TAIL_SKIP; or the predicate-kernel front k_pred1 ... k_select ... k_scalars
with the selection of prec / ta deferred into the fused kernel.  Who writes D->S and when, whether prec / ta in the arena are this step's
when an observer reads them, and whether the sparse KEEP kernel keeps an observer's planes behind these fronts is what this module pins.

Columns, steps, reference and restatements: tests/per_cell_observers.py.  Comparison rule as in the observers' own tests: headers
exactly, sums, moments and gathered values as bits, minimum and maximum with ==."""
import numpy as np
import pytest

import per_cell_observers as P
from per_cell_observers import CASES, DAY, GRIDS, M1, OTHER, PURE, SMALL_GRIDS, VARS, make_ctx, prefix_steps, reference, same_bits

pytestmark = pytest.mark.gpu

ALL = ("diag", "points", "totals", "zonal", "scores")
CASE_GRIDS = [(case, nx, ny) for case in CASES for nx, ny in GRIDS]
CASE_SMALL = [(case, nx, ny) for case in CASES for nx, ny in SMALL_GRIDS]
# the environment of every front and of the selection and store variants (read by rh_create); sparse: the sparse kernel runs under it
FRONTS = {
    "old_front": (dict(RH_PER_CELL_OLD_FRONT="1"), True),
    "old_front_stored_select": (dict(RH_PER_CELL_OLD_FRONT="1", RH_NO_DEFERRED_SELECT="1"), False),   # k_select stores: no lazy rotation
    "split_front": (dict(RH_CELL_AGG_SPLIT_MIN="1"), True),
    "front_max_0": (dict(RH_CELL_FRONT_MAX="0"), True),
    "no_sparse_stores": (dict(RH_NO_SPARSE_STORES="1"), False),
}
SWITCHES = sorted({k for env, _ in FRONTS.values() for k in env})


def default_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def assert_final_state(ctx, ref, what):
    import hip_util as H

    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), ref.final_scalars, err_msg=f"{what}: final scalars")
    for nm, want in ref.final.items():
        got = ctx.download(nm)
        assert got.dtype == want.dtype and (same_bits(got, want) if got.dtype.kind == "f" else (got == want).all()), (what, "final plane", nm)


@pytest.mark.parametrize("case", CASES)
def test_the_prefix_of_the_golden_run(case):
    """The steps every test of this module takes, chosen from the golden file: every step class the golden run has (600, 3600 and 86400 s
    in the station run; the Eberbaechle run takes no ten-minute step in its 40 days), two midnights and more, the month change of the
    Eberbaechle run (2019-12-01), and a stored step with snow on part of the twelve columns."""
    from golden_util import load_case

    g, names, _ = load_case(case)
    n = prefix_steps(case)
    dt, t = g["scal"][:n, 2].astype(np.int64), g["scal"][:n, 1].astype(np.int64)
    assert set(dt) == set(g["scal"][:, 2].astype(np.int64)) == P.CLASSES[case], set(dt)
    assert set().union(*P.CLASSES.values()) == {600, 3600, 86400}
    assert int((t % DAY == 0).sum()) >= 2
    assert n <= 400, n
    if case == "svat_eberbaechle_weights":
        assert set(g["scal"][:n, 12:14].astype(int).ravel()) == {11, 12}, "the month does not change inside the prefix"


@pytest.mark.parametrize("observer", ALL)
@pytest.mark.parametrize("case,nx,ny", CASE_SMALL)
def test_one_call_each_observer_alone(case, nx, ny, observer, monkeypatch):
    """1. One rh_run_steps call, one observer: every row, slot or moment equals the restatement; the sparse KEEP kernel ran behind the front."""
    default_env(monkeypatch)
    ref, n = reference(case, nx, ny), prefix_steps(case)
    ctx = make_ctx(case, nx, ny)
    assert set(PURE) <= set(ctx.pure_output_planes())
    obs = P.configure(ctx, ref, (observer,))
    ctx.run_steps(n)
    assert ctx.sparse_steps() > 0
    assert ctx.step_mode()[0], "the lazy rotation is off"
    P.assert_observers(ctx, ref, (observer,), VARS, obs, P.reference_totals(case, nx, ny), P.reference_zonal(case, nx, ny),
                       what=f"{case} {nx} x {ny} {observer} alone")
    assert_final_state(ctx, ref, f"{case} {nx} x {ny} {observer} alone")
    ctx.close()


@pytest.mark.parametrize("observer", ["points", "scores"])
@pytest.mark.parametrize("case,nx,ny", CASE_SMALL)
def test_an_observed_m1_plane_switches_the_lazy_rotation_off(case, nx, ny, observer, monkeypatch):
    """1b. S_rz_m1 among the observed planes (obs_reads_m1): the eager fused kernel behind the front; rows or moments equal the
    restatement and the run ends in the reference's state."""
    default_env(monkeypatch)
    ref, n = reference(case, nx, ny), prefix_steps(case)
    names = ("q_ss", M1, "S_rz", "aet", "prec")
    ctx = make_ctx(case, nx, ny)
    obs = P.configure(ctx, ref, (observer,), names)
    ctx.run_steps(n)
    assert not ctx.step_mode()[0], "the lazy rotation stayed on"
    assert np.any(ref.planes[M1] != 0)
    P.assert_observers(ctx, ref, (observer,), names, obs, what=f"{case} {nx} x {ny} {observer} with an X_m1 plane")
    assert_final_state(ctx, ref, f"{case} {nx} x {ny} {observer} with an X_m1 plane")
    ctx.close()


def run_all_five(case, nx, ny):
    """A context with all five observers on VARS after one rh_run_steps call of the prefix; (ctx, observations)."""
    ref = reference(case, nx, ny)
    ctx = make_ctx(case, nx, ny)
    obs = P.configure(ctx, ref, ALL)
    ctx.run_steps(prefix_steps(case))
    return ctx, obs


def assert_all_five(ctx, obs, case, nx, ny, what):
    ref = reference(case, nx, ny)
    P.assert_observers(ctx, ref, ALL, VARS, obs, P.reference_totals(case, nx, ny), P.reference_zonal(case, nx, ny), what=what)
    assert_final_state(ctx, ref, what)


@pytest.mark.parametrize("case,nx,ny", CASE_GRIDS)
def test_one_call_all_five_observers(case, nx, ny, monkeypatch):
    """2. One rh_run_steps call, all five observers together, every case and grid.  Guards against a vacuous pass, from the reference's
    downloads: every observed variable is non-zero in some row, prec differs between two columns of one step (the weights act), and in
    some step part of the grid lies under snow and part does not (per-cell predicates decided)."""
    default_env(monkeypatch)
    ref = reference(case, nx, ny)
    for v in VARS:
        assert np.any(ref.planes[v] != 0), f"{v} is zero in every reference row"
    assert np.any(ref.planes["prec"].max(axis=1) != ref.planes["prec"].min(axis=1)), "prec is the same in every column of every step"
    snow = (ref.planes["swe"] > 0).sum(axis=1)
    assert np.any((snow > 0) & (snow < nx * ny)), "no step with snow on part of the grid only"
    assert len(ref.hdr) == prefix_steps(case) and set(ref.hdr[:, 2]) == P.CLASSES[case]
    ctx, obs = run_all_five(case, nx, ny)
    assert ctx.sparse_steps() > 0
    assert_all_five(ctx, obs, case, nx, ny, f"{case} {nx} x {ny} all five")
    ctx.close()


@pytest.mark.parametrize("front", sorted(FRONTS))
@pytest.mark.parametrize("case,nx,ny", CASE_SMALL)
def test_every_front(case, nx, ny, front, monkeypatch):
    """3. Test 2 under every switch of the per-cell step: the predicate-kernel front with the deferred and with the stored selection, the
    split one-launch front, the front switched off by size, and no sparse stores.  The observers' outputs, the final planes and the final
    scalars are the default run's and the restatement's, bit for bit."""
    import hip_util as H

    default_env(monkeypatch)
    ref = reference(case, nx, ny)
    ctx, obs = run_all_five(case, nx, ny)
    default = P.read_observers(ctx, ref)
    default_final = ({nm: ctx.download(nm) for nm in ref.final}, H.scalars_to_row(ctx.get_scalars()))
    ctx.close()
    env, sparse = FRONTS[front]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx, obs2 = run_all_five(case, nx, ny)
    assert (ctx.sparse_steps() > 0) == sparse, (front, ctx.sparse_steps())
    assert ctx.step_mode()[0] == (front != "old_front_stored_select")
    what = f"{case} {nx} x {ny} {front}"
    assert_all_five(ctx, obs2, case, nx, ny, what)
    P.assert_same_outputs(P.read_observers(ctx, ref), default, f"{what} against the default run")
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), default_final[1], err_msg=what)
    for nm, want in default_final[0].items():
        got = ctx.download(nm)
        assert same_bits(got, want) if got.dtype.kind == "f" else (got == want).all(), (what, "final plane against the default run", nm)
    ctx.close()


@pytest.mark.parametrize("case,nx,ny", CASE_SMALL)
def test_calls_in_pieces_with_observers_configured_in_between(case, nx, ny, monkeypatch):
    """4. Calls of 1 and 7 steps, then all five observers configured in the middle of a day on other planes, 30 steps, configured once more
    on the first planes, and the rest.  The rows recorded since each configuration equal the restatement from that step on: a ring
    starts from row 0, the scores from the next day's boundary, an accumulator slot first touched inside its interval counts the
    steps it saw and never learns its start (-1, include/roger_hip.h)."""
    default_env(monkeypatch)
    ref, n = reference(case, nx, ny), prefix_steps(case)
    what = f"{case} {nx} x {ny} in pieces"
    ctx = make_ctx(case, nx, ny)
    obs = P.configure(ctx, ref, ALL)
    ctx.run_steps(1)
    ctx.run_steps(7)
    P.assert_observers(ctx, ref, ALL, VARS, obs, stop=8, what=f"{what}, steps 1 ... 8")
    done = 8
    for names, more in ((OTHER, 30), (VARS, n - 38)):
        now = int(ref.hdr[done - 1, 1])
        assert now % DAY != 0 and int(ctx.get_scalars().time) == now, "not in the middle of a day"
        t_first = -(-now // DAY) * DAY
        obs = P.configure(ctx, ref, ALL, names, t_first=t_first, seed=done)
        ctx.run_steps(more)
        rows = slice(done, done + more)
        totals, zonal = (P.reference_totals(case, nx, ny)[rows], P.reference_zonal(case, nx, ny)[rows]) if names is VARS else (None, None)
        P.assert_observers(ctx, ref, ALL, names, obs, totals, zonal, first=done, stop=done + more, t_first=t_first,
                           what=f"{what}, steps {done + 1} ... {done + more}")
        acc = P.assert_diag(ctx, ref, names, done, done + more, what)
        slot = (now // DAY) % acc.n_slots
        assert acc.t0[slot] == -1 and acc.steps[slot] > 0 and ctx.diag_slot_times(slot)[0] == -1, "the slot of the day of the configuration"
        done += more
    assert done == n
    assert_final_state(ctx, ref, what)
    ctx.close()


@pytest.mark.parametrize("path", ["svat_step", "phases", "routines"])
@pytest.mark.parametrize("case", CASES)
def test_host_driven_steps_record_one_row_per_step(case, path, monkeypatch):
    """5. The hooks on the host (the per-cell day handed over every midnight), the step as rh_svat_step, as rh_step_phase1 / 2 / 3 and
    routine by routine (rh_adaptive_dt, rh_step_core, rh_after_timestep): every observer records one row per step with the reference's
    header, and holds what its restatement makes of the context's own planes after every step (observed are planes
    rh_after_timestep does not assign)."""
    default_env(monkeypatch)
    nx, ny = 257, 1
    ref = reference(case, nx, ny)
    nsteps = {"svat_stations": 60, "svat_eberbaechle_weights": 200}[case]
    ctx = make_ctx(case, nx, ny, resident=False)
    rec = P.Record(VARS)
    # (the observations and the accumulators' slots are sized by the record: the reference's clock, which the headers must equal)
    obs = P.configure(ctx, ref, ALL)
    hooks = P.HostHooks(ctx, case)
    for _ in range(nsteps):
        monthly = hooks.before_step()
        if path == "routines":
            ctx.call("rh_adaptive_dt")
            if monthly:
                ctx.call("rh_params_surface")
            ctx.call("rh_step_core")
            ctx.call("rh_after_timestep")
        elif path == "phases":
            ctx.call("rh_step_phase1")
            ctx.call("rh_step_phase2")
            ctx.step_phase3(monthly)
        else:
            ctx.step(monthly)
        rec.take(ctx)
    rec.freeze()
    np.testing.assert_array_equal(rec.hdr, ref.hdr[:nsteps], err_msg=f"{case} {path}: the clock of the host-driven steps")
    assert len(set(rec.hdr[:, 2])) >= 2 and int((rec.hdr[:, 1] % DAY == 0).sum()) >= 2
    assert np.any(rec.planes["prec"].max(axis=1) != rec.planes["prec"].min(axis=1))
    P.assert_points(ctx, rec, VARS, what=f"{case} {path}")
    P.assert_totals(ctx, rec, VARS, P.want_totals(rec, VARS, P.mask_of(ctx.n)), what=f"{case} {path}")
    P.assert_zonal(ctx, rec, VARS, P.want_zonal(rec, VARS, *P.zones_of(ctx.n)), what=f"{case} {path}")
    P.assert_scores(ctx, P.want_scores(rec, VARS, obs, ctx.n), what=f"{case} {path}")
    P.assert_diag(ctx, rec, VARS, what=f"{case} {path}", n_slots=P.n_days(ref))
    ctx.close()


@pytest.mark.parametrize("case", CASES)
def test_one_rank_communicator_refuses_per_cell_forcing(case, monkeypatch):
    """6. rh_run_steps_dist takes the one-exchange step, which needs forcing shared by all columns: with per-cell forcing it is refused
    with RH_ERR_STATE and its reason, the observers record nothing, and rh_run_steps on the same context records as without a
    communicator."""
    from roger_amd import _native as native

    default_env(monkeypatch)
    nx, ny = 4, 3
    ref, n = reference(case, nx, ny), prefix_steps(case)
    ctx = make_ctx(case, nx, ny)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    obs = P.configure(ctx, ref, ALL)
    with pytest.raises(native.NativeError, match=r"rh_run_steps_dist failed \(-3\).*needs forcing shared by all columns \(rh_step_phase1/2/3 otherwise\)"):
        ctx.run_steps_dist(n)
    assert ctx.points_count() == 0 and ctx.totals_count()[0] == 0 and ctx.zonal_count()[0] == 0 and not ctx.scores_read()[1].any()
    assert ctx.get_scalars().itt == 0
    ctx.run_steps(n)
    assert_all_five(ctx, obs, case, nx, ny, f"{case} rh_run_steps with a one-rank communicator")
    ctx.close()
