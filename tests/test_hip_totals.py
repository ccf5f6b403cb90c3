"""GPU: catchment totals (rh_totals_*, k_totals_tiles / k_totals_finish in roger_amd/csrc/rh_control.h) against their host restatement
(tests/totals_reference.py: tree_totals).

The reference is tests/test_hip_points.py's: a context WITHOUT totals that steps one step at a time and downloads the observed planes
after every step; tree_totals of those planes is what the device must have recorded.  Comparison rule: sums as bits (the order of the
sum is fixed and restated), minimum and maximum by value with == (fmin(-0.0, 0.0) may return either zero), headers exactly.

Grids as for the points: 3 x 2 (one partial wavefront), 257 x 1 (a second tile of one column) and 40 x 25 (four tiles, last wavefront
of 40 lanes), each for SVAT and oneD, over 8 days = 150 steps of all three step classes."""
import functools
import itertools

import numpy as np
import pytest

from diag_reference import HostAccumulator
from test_hip_points import CASES, M1, NSTEPS, VARS, make_ctx, reference, same_bits
from totals_reference import tree_totals

pytestmark = pytest.mark.gpu

GRIDS = ((3, 2), (257, 1), (40, 25))


def mask_of(nx, ny, kind):
    """None (every column) or a bool mask over the n columns."""
    n = nx * ny
    if kind == "all":
        return None
    if kind == "half":
        m = np.random.default_rng(100 + n).random(n) < 0.5
        assert 0 < m.sum() < n
        return m
    if kind == "holes":     # one whole tile and one whole wavefront hold no column
        assert n == 1000
        m = np.ones(n, dtype=bool)
        m[256:512] = False
        m[64:128] = False
        return m
    assert kind == "single"
    m = np.zeros(n, dtype=bool)
    m[n - 1 if n < 300 else 700] = True      # 3 x 2: the last lane in use; 257 x 1: the second tile's only column
    return m


MASKS = {g: ("all", "half", "single") + (("holes",) if g == (40, 25) else ()) for g in GRIDS}
MASK_CASES = [(nx, ny, lateral, kind) for (nx, ny, lateral) in CASES for kind in MASKS[(nx, ny)]]


@functools.lru_cache(maxsize=None)
def want_rows(nx, ny, lateral, kind, names):
    """(steps, V, 3): tree_totals of the reference's planes after every step."""
    ref, mask = reference(nx, ny, lateral), mask_of(nx, ny, kind)
    out = np.array([[tree_totals(ref.planes[v][k], mask) for v in names] for k in range(len(ref.hdr))])
    out.setflags(write=False)
    return out


def assert_totals(got_hdr, got, want_hdr, want, names, what):
    np.testing.assert_array_equal(got_hdr, want_hdr, err_msg=f"{what}: headers")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for j, v in enumerate(names):
        ok = got[:, j, 0].view(np.uint64) == want[:, j, 0].view(np.uint64)
        assert ok.all(), (what, v, "sum, rows", np.flatnonzero(~ok)[:5], got[:, j, 0][~ok][:3], want[:, j, 0][~ok][:3])
        for k, stat in ((1, "min"), (2, "max")):
            ok = got[:, j, k] == want[:, j, k]
            assert ok.all(), (what, v, stat, "rows", np.flatnonzero(~ok)[:5], got[:, j, k][~ok][:3], want[:, j, k][~ok][:3])


def assert_rows(ctx, nx, ny, lateral, kind, names, first, n, what):
    hdr, vals = ctx.totals_read(first, n)
    ref = reference(nx, ny, lateral)
    assert_totals(hdr, vals, ref.hdr[first:first + n], want_rows(nx, ny, lateral, kind, tuple(names))[first:first + n], names, what)


def configured(nx, ny, lateral, kind, names=VARS, **kw):
    ctx, _ = make_ctx(nx, ny, lateral)
    mask = mask_of(nx, ny, kind)
    ctx.totals_configure(names, mask, **kw)
    assert ctx.totals_count() == (0, ctx.n if mask is None else int(mask.sum()))
    return ctx


@pytest.mark.parametrize("nx,ny,lateral,kind", MASK_CASES)
def test_one_call_records_every_step(nx, ny, lateral, kind):
    """1. One rh_run_steps call of 150 steps, every mask; the sparse KEEP kernel ran.  On 40 x 25 with every column: the guard against a
    test that pins nothing -- every variable has a non-zero sum somewhere, and somewhere the tree's sum is not the left-to-right sum."""
    ctx = configured(nx, ny, lateral, kind)
    assert {"aet", "q_ss", "theta"} <= set(ctx.pure_output_planes())
    ctx.run_steps(NSTEPS)
    assert ctx.totals_count()[0] == NSTEPS
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, nx, ny, lateral, kind, VARS, 0, NSTEPS, f"{nx} x {ny} lateral={lateral} mask={kind}")
    ctx.close()
    if (nx, ny, kind) == (40, 25, "all"):
        ref, want = reference(nx, ny, lateral), want_rows(nx, ny, lateral, kind, VARS)
        for j, v in enumerate(VARS):
            assert np.any(want[:, j, 0] != 0), f"{v}: the sum is zero in every row"
        serial = np.array([[np.add.accumulate(ref.planes[v][k])[-1] for v in VARS] for k in range(NSTEPS)])
        differ = serial.view(np.uint64) != np.ascontiguousarray(want[:, :, 0]).view(np.uint64)
        print(f"tree sum != left-to-right sum in {int(differ.sum())} of {differ.size} (row, variable) pairs")
        assert differ.any(), "the order of the sum is not what this test compares"


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces_record_the_same_rows(nx, ny, lateral):
    """2. Pieces of 1, 2, 37 steps and the rest."""
    ctx = configured(nx, ny, lateral, "half")
    done = 0
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
        done += n
        assert ctx.totals_count()[0] == done
    assert_rows(ctx, nx, ny, lateral, "half", VARS, 0, NSTEPS, f"{nx} x {ny} lateral={lateral} in pieces")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_launches_behind_the_time_limit_record_nothing(nx, ny, lateral):
    """3. 500 steps enqueued under a limit of three days: as many rows as the reference needs steps, none beyond the limit."""
    ref = reference(nx, ny, lateral)
    limit = 3 * 86400
    want = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    assert ref.hdr[want - 1, 1] == limit and 3 < want < NSTEPS
    ctx = configured(nx, ny, lateral, "half")
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    assert ctx.totals_count()[0] == want
    hdr, _ = ctx.totals_read(0, want)
    assert hdr[:, 1].max() == limit
    assert_rows(ctx, nx, ny, lateral, "half", VARS, 0, want, f"{nx} x {ny} lateral={lateral} under the limit")
    ctx.run_steps(5)
    assert ctx.totals_count()[0] == want
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_ring_keeps_the_last_rows_and_refuses_the_overwritten_ones(nx, ny, lateral):
    """4. capacity 16 over 150 steps."""
    from roger_amd._native import NativeError

    ctx = configured(nx, ny, lateral, "all", capacity=16)
    ctx.run_steps(NSTEPS)
    assert ctx.totals_count()[0] == NSTEPS
    assert_rows(ctx, nx, ny, lateral, "all", VARS, NSTEPS - 16, 16, "the resident rows")     # straddles the wrap: 134 = 8 * 16 + 6
    assert_rows(ctx, nx, ny, lateral, "all", VARS, NSTEPS - 5, 5, "the last rows")
    for first, n in ((NSTEPS - 17, 1), (NSTEPS - 17, 17), (0, 1)):
        with pytest.raises(NativeError, match=r"rh_totals_read failed \(-1\).*overwritten"):
            ctx.totals_read(first, n)
    with pytest.raises(NativeError, match=r"rh_totals_read failed \(-1\).*not been recorded"):
        ctx.totals_read(NSTEPS - 1, 2)
    ctx.close()


@pytest.mark.parametrize("order", list(itertools.permutations(("totals", "points", "diag"))), ids="-".join)
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_three_observers_keep_each_others_planes(nx, ny, lateral, order):
    """5. Totals, points and accumulators, configured in each order, on disjoint pure outputs: all three equal their references.  Fails
    if one configure call drops another's keep bits (the sparse kernel then leaves that observer's planes unwritten)."""
    from test_hip_points import POINTS, assert_rows as assert_point_rows

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    rate, collect = ("q_ss", "aet"), ("S_rz",)
    p_names, t_names = ("transp", "theta", "swe"), ("q_rz", "evap_soil", "S_fp_rz", "inf_mat_rz")
    ctx, _ = make_ctx(nx, ny, lateral)
    pure = set(ctx.pure_output_planes())
    assert set(rate) <= pure and {"transp", "theta"} <= pure and {"q_rz", "evap_soil"} <= pure
    mask = mask_of(nx, ny, "half")
    for what in order:
        if what == "totals":
            ctx.totals_configure(t_names, mask)
        elif what == "points":
            ctx.points_configure(cells, p_names)
        else:
            ctx.diag_configure(rate=rate, collect=collect, n_slots=3)
    acc = HostAccumulator(rate, collect, 3, ctx.n)
    for k in range(NSTEPS):
        acc.add(ref.hdr[k, 1], ref.hdr[k, 2], {v: ref.planes[v][k] for v in rate + collect})
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, nx, ny, lateral, "half", t_names, 0, NSTEPS, f"totals, order {order}")
    assert np.any(want_rows(nx, ny, lateral, "half", t_names)[:, :2, 0] != 0, axis=0).all()
    assert_point_rows(ctx, ref, p_names, cells, 0, NSTEPS, f"points, order {order}")
    for slot in range(3):
        for v in rate + collect:
            assert same_bits(ctx.diag_download(v, slot), acc.data[v][slot]), (v, slot, order)
        assert ctx.diag_steps(slot) == acc.reported_steps(slot)
    # releasing the totals leaves the others' planes kept
    ctx.totals_configure((), None)
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_an_observed_m1_plane_switches_the_lazy_rotation_off(nx, ny, lateral):
    """6. S_rz_m1 among the variables: the rows equal the reference and the run ends in the reference's state, bit for bit."""
    import hip_util as H

    ref = reference(nx, ny, lateral)
    names = ("q_ss", M1, "S_rz", "aet")
    ctx = configured(nx, ny, lateral, "half", names)
    ctx.run_steps(NSTEPS)
    assert not ctx.step_mode()[0], "the lazy rotation stayed on"
    assert_rows(ctx, nx, ny, lateral, "half", names, 0, NSTEPS, "with an X_m1 plane")
    assert np.any(want_rows(nx, ny, lateral, "half", names)[:, 1, 0] != 0)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), ref.final_scalars)
    for nm, want in ref.final.items():
        got = ctx.download(nm)
        assert got.dtype == want.dtype and (same_bits(got, want) if got.dtype.kind == "f" else (got == want).all()), nm
    ctx.close()


def assert_last_row_is_the_state(ctx, names, mask, k, what):
    """Row k - 1 (the k-th step's) against tree_totals of the context's own planes, and its scalars, after that step."""
    assert ctx.totals_count()[0] == k, what
    hdr, vals = ctx.totals_read(k - 1, 1)
    s = ctx.get_scalars()
    want = np.array([[tree_totals(ctx.download(v), mask) for v in names]])
    assert_totals(hdr, vals, np.array([[s.itt, s.time, s.dt_secs]]), want, names, f"{what} step {k}")


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_paths_record_one_row_per_step(path, lateral):
    """7. rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step: one row per step, equal to tree_totals of the downloads
    after that step (observed are planes rh_after_timestep does not assign)."""
    from test_hip_points import host_hooks

    nx, ny = 257, 1
    names = ("prec", "aet", "q_ss", "inf_mat_rz", "S_rz", "theta", "swe")
    mask = mask_of(nx, ny, "half")
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.totals_configure(names, mask)
    classes = set()
    for k in range(1, 61):
        monthly = host_hooks(ctx, forcing)
        if path == "routines":
            ctx.call("rh_adaptive_dt")
            if monthly:
                ctx.call("rh_params_surface")
            ctx.call("rh_step_core")
            ctx.call("rh_after_timestep")
        else:
            ctx.step(monthly)
        assert_last_row_is_the_state(ctx, names, mask, k, f"{path} lateral={lateral}")
        classes.add(ctx.get_scalars().dt_secs)
    assert len(classes) >= 2, classes
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES[2:])
def test_one_rank_communicator_records_like_run_steps(nx, ny, lateral):
    """8. rh_run_steps_dist with a one-rank RCCL communicator."""
    from roger_amd import _native as native

    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.totals_configure(VARS, mask_of(nx, ny, "half"))
    ctx.run_steps_dist(NSTEPS)
    assert ctx.totals_count()[0] == NSTEPS
    assert_rows(ctx, nx, ny, lateral, "half", VARS, 0, NSTEPS, "rh_run_steps_dist, one rank")
    ctx.close()


def test_routed_steps_record_one_row_per_step(monkeypatch):
    """9. The routed step on the smallest routing golden: rh_step_routed step by step against the downloads after each step, then the
    device-driven routed steps of rh_run_steps (and RH_ROUTED_BY_ROUTINE=1) against those rows."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    names = ("q_sur_out", "q_sub_in", "aet", "prec", "S", "z0", "q_ss")
    nsteps = 40
    ctx = routed_ctx(native, g, names_all)
    mask = np.arange(ctx.n) % 3 != 1
    ctx.totals_configure(names, mask)
    drv = H.HipForcingDriver(ctx, forcing)
    for k in range(1, nsteps + 1):
        ctx.step_routed(drv.before_step())
        assert_last_row_is_the_state(ctx, names, mask, k, "rh_step_routed")
    want_hdr, want = ctx.totals_read(0, nsteps)
    assert all(np.any(want[:, j, 0] != 0) for j in range(len(names)) if names[j] != "q_sub_in"), "a routed variable never held a value"
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.totals_configure(names, mask)
        ctx.run_steps(nsteps)
        assert ctx.totals_count() == (nsteps, int(mask.sum()))
        hdr, vals = ctx.totals_read(0, nsteps)
        assert_totals(hdr, vals, want_hdr, want, names, f"rh_run_steps on a routing context, by_routine={by_routine}")
        ctx.close()


def test_the_strided_pass_over_more_than_256_tiles():
    """10. 65 537 x 1, SVAT, 20 steps, every column: 257 tiles, so thread 0 of the finish kernel adds partial 256 to partial 0.  The
    reference rows differ from the sum of the first 256 tiles and from the tiles added in tile order, so either mistake fails."""
    nx, ny, nsteps = 65537, 1, 20
    import hip_util as H

    names = ("S_rz", "theta", "aet", "swe")
    # the reference as tests/test_hip_points.py's Reference forms it, without its assertion on the water-balance flag: among 65 537
    # random columns of hetero_params one exceeds that check's tolerance, which is reported in the scalars and changes no step
    ctx, forcing = make_ctx(nx, ny, False)
    drv = H.HipForcingDriver(ctx, forcing)
    hdr, planes = [], {v: [] for v in names}
    for _ in range(nsteps):
        ctx.step(drv.before_step())
        s = ctx.get_scalars()
        hdr.append((s.itt, s.time, s.dt_secs))
        for v in names:
            planes[v].append(ctx.download(v))
    ctx.close()
    ref_hdr = np.array(hdr, dtype=np.int64)
    want = np.array([[tree_totals(planes[v][k]) for v in names] for k in range(nsteps)])
    first256 = np.array([[tree_totals(planes[v][k][:65536])[0] for v in names] for k in range(nsteps)])
    in_order = np.array([[np.add.accumulate([tree_totals(planes[v][k][t:t + 256])[0] for t in range(0, nx, 256)])[-1] for v in names[:2]]
                         for k in range(3)])
    assert (first256 != want[:, :, 0])[:, :2].all(), "the last tile's column does not show in the sum"
    assert (in_order != want[:3, :2, 0]).any(), "the order of the tiles does not show in the sum"
    ctx, _ = make_ctx(nx, ny, False)
    ctx.totals_configure(names)
    ctx.run_steps(nsteps)
    assert ctx.totals_count() == (nsteps, nx)
    hdr, vals = ctx.totals_read(0, nsteps)
    assert_totals(hdr, vals, ref_hdr, want, names, "257 tiles")
    ctx.close()


def test_refusals_and_release():
    """11. RH_ERR_ARG with the offending value in the text, RH_ERR_STATE before the configuration and after the release; a new series
    starts from row 0."""
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    for call in (ctx.totals_count, lambda: ctx.totals_read(0, 0)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    ctx.totals_configure(("theta", "swe"), mask, capacity=4)
    ctx.run_steps(3)
    bad = ((dict(names=(ints[0],)), f"plane {ints[0]} is int32"), (dict(names=(not_held[0],)), f"plane id {ctx.index[not_held[0]]} "),
           (dict(names=floats[:33]), "n_planes = 33"), (dict(names=("theta",), capacity=0), "capacity = 0"),
           (dict(names=("theta",), capacity=-3), "capacity = -3"), (dict(names=("theta",), mask=np.zeros(6, dtype=bool)), "0 of 6 "))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_totals_configure failed \(-1\)") as e:
            ctx.totals_configure(**kw)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="the mask has 5 values"):
        ctx.totals_configure(("theta",), np.ones(5, dtype=bool))
    # every refusal left the configuration working
    ctx.run_steps(2)
    assert ctx.totals_count() == (5, 4)
    hdr, vals = ctx.totals_read(1, 4)
    assert list(hdr[:, 0]) == [2, 3, 4, 5] and vals.shape == (4, 2, 3)
    assert same_bits(vals[-1, 0, 0], tree_totals(ctx.download("theta"), mask)[0])
    # 32 planes are accepted, and the release
    ctx.totals_configure(floats[:32], capacity=2)
    ctx.run_steps(3)
    hdr, vals = ctx.totals_read(1, 2)
    assert vals.shape == (2, 32, 3) and same_bits(vals[-1, 5, 0], tree_totals(ctx.download(floats[5]))[0])
    ctx.totals_configure(())
    ctx.run_steps(2)
    for call in (ctx.totals_count, lambda: ctx.totals_read(0, 1)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.totals_configure(("theta",), capacity=1)   # a new series starts at row 0
    assert ctx.totals_count() == (0, 6)
    ctx.run_steps(2)
    hdr, vals = ctx.totals_read(1, 1)
    assert hdr[0, 0] == 12 and vals[0, 0, 1] == ctx.download("theta").min() and vals[0, 0, 2] == ctx.download("theta").max()
    ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """12. End to end: a RogerSetup script with the reference's hook bodies (the device performs them: run() advances in rounds of
    rh_run_steps) and totals with capacity 8 writes the same `.totals.nc` values as the same script stepped routine by routine."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    variables, ndays = ["theta_rz", "q_ss", "swe", "S_rz", "aet", "prec"], 6
    nx, ny = (int(v) for v in g["nx_ny"])
    mask = np.random.default_rng(4).random((nx, ny)) < 0.6
    keys = ["Time", "dt", "itt", "ncells"] + [f"{v}_{s}" for v in variables for s in ("sum", "min", "max", "mean")]
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path):
            state.totals.mask = mask
            state.totals.output_variables = list(variables)
            state.totals.base_output_path = str(path)
            state.totals.capacity = 8

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        rounds = []
        inner = model.run_device
        model.run_device = lambda n, final=True, inner=inner, rounds=rounds: (rounds.append(n), inner(n, final=final))[1]
        model.run()
        assert (mode == "device") == bool(rounds) and all(n <= 8 for n in rounds), rounds
        f = netcdf_file(str(path / "GoldenSVAT.totals.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in keys}
        model.state.backend_context.close()
    nsteps = int(np.sum(g["scal"][:, 1] <= ndays * 86400))
    d = out["device"]
    for k, a in d.items():
        b = out["routine"][k]
        if a.dtype.kind == "f" and not k.endswith(("_min", "_max")):
            assert same_bits(a, b), k
        else:
            assert a.shape == b.shape and np.array_equal(a, b), k
    assert int(d["ncells"].reshape(-1)[0]) == int(mask.sum())
    assert len(d["Time"]) == nsteps + 1 and d["Time"][-1] == ndays and d["dt"][0] == 0 and list(d["itt"]) == list(range(nsteps + 1))
    np.testing.assert_array_equal(d["Time"][1:], g["scal"][:nsteps, 1].astype(np.float64) / 86400.0)
    for v in variables:
        assert np.any(d[f"{v}_sum"][1:] != 0), v
        assert same_bits(d[f"{v}_mean"], d[f"{v}_sum"] / mask.sum())
