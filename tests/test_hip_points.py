"""GPU: time series at observation columns (rh_points_*, k_points in roger_amd/csrc/rh_control.h), tolerance zero.

k_points is a pure gather: after every step one workgroup copies planes x cells into the next row of a ring on the device and writes the
row's header (itt, time at the end of the step, dt_secs).  The reference is a second context WITHOUT points that steps one step at a
time and downloads the observed planes after every step (a call's last step stores every plane), so every value must be the same bits.

Grids: 3 x 2 (one partial wavefront, every cell a point), 257 x 1 (the 256-column tile boundary: cells 0, 63, 64, 255, 256) and 40 x 25
(three tiles and a ragged fourth, last wavefront of 40 lanes: cells 0, 255, 256, 767, 959, 999), each for SVAT and oneD, over the same
8 days of the combo forcing as tests/test_hip_diag_kernel.py: 150 steps of all three step classes."""
import functools

import numpy as np
import pytest

from diag_reference import HostAccumulator

pytestmark = pytest.mark.gpu

VARS = ("prec", "aet", "q_ss", "inf_mat_rz", "S_fp_rz", "S_rz", "theta", "swe")   # pure outputs among them: the KEEP variant runs
M1 = "S_rz_m1"
OTHER = ("transp", "q_rz", "evap_soil")     # further pure outputs, for the points when the accumulators hold q_ss and aet
NDAYS = 8
NSTEPS = 150
POINTS = {(3, 2): (0, 1, 2, 3, 4, 5), (257, 1): (0, 63, 64, 255, 256), (40, 25): (0, 255, 256, 767, 959, 999)}
CASES = [(nx, ny, lateral) for (nx, ny) in POINTS for lateral in (False, True)]
ALL_STEPS = 40    # the every-plane test


def make_ctx(nx, ny, lateral):
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    p = hetero_params(nx * ny, seed=5)
    if lateral:
        p.update(slope=0.05, slope_per=5, dmph=50.0)
        p["z_soil"] = np.maximum(p["z_soil"], 800.0)
    forcing = combo_forcing(ndays=NDAYS + 4)
    ctx = create_svat(nx, ny, params=p, lateral=lateral)
    ctx.set_forcing_series(forcing)
    return ctx, forcing


def float_planes(ctx):
    """The float64 planes the context holds, the X_m1 planes last (one of them switches the lazy rotation off for its whole group)."""
    names = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if not is_int]
    return [nm for nm in names if not nm.endswith("_m1")] + [nm for nm in names if nm.endswith("_m1")]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


class Reference:
    """hdr (steps, 3) int64; planes[name] (steps, n) float64: what a context without points holds after every single step."""

    def __init__(self, nx, ny, lateral, names, until=None, nsteps=None, final=False):
        import hip_util as H

        ctx, forcing = make_ctx(nx, ny, lateral)
        drv = H.HipForcingDriver(ctx, forcing)
        self.names = list(names)
        hdr, rows = [], {v: [] for v in self.names}
        while True:
            ctx.step(drv.before_step())
            s = ctx.get_scalars()
            assert s.sanity_ok == 1
            hdr.append((s.itt, s.time, s.dt_secs))
            for v in self.names:
                rows[v].append(ctx.download(v))
            if (until is not None and s.time >= until) or (nsteps is not None and len(hdr) >= nsteps):
                break
        self.hdr = np.array(hdr, dtype=np.int64)
        self.planes = {v: np.stack(rows[v]) for v in self.names}
        if final:
            self.final = {nm: ctx.download(nm) for nm, _ in ctx.planes[: ctx.planes_held]}
            self.final_scalars = H.scalars_to_row(ctx.get_scalars())
        ctx.close()

    def rows(self, names, cells, first=0, n=None):
        stop = len(self.hdr) if n is None else first + n
        return np.stack([self.planes[v][first:stop][:, list(cells)] for v in names], axis=1)   # (rows, V, K)


@functools.lru_cache(maxsize=None)
def reference(nx, ny, lateral):
    ref = Reference(nx, ny, lateral, VARS + (M1,) + OTHER, until=NDAYS * 86400, final=True)
    assert len(ref.hdr) == NSTEPS and set(ref.hdr[:, 2]) == {600, 3600, 86400}, (len(ref.hdr), set(ref.hdr[:, 2]))
    assert (ref.hdr[:, 0] == np.arange(1, NSTEPS + 1)).all() and (np.diff(ref.hdr[:, 1]) == ref.hdr[1:, 2]).all()
    return ref


def assert_rows(ctx, ref, names, cells, first, n, what):
    hdr, vals = ctx.points_read(first, n)
    np.testing.assert_array_equal(hdr, ref.hdr[first:first + n], err_msg=f"{what}: headers of rows {first} ... {first + n - 1}")
    want = ref.rows(names, cells, first, n)
    assert vals.shape == want.shape, (vals.shape, want.shape)
    for j, v in enumerate(names):
        ok = vals[:, j].view(np.uint64) == want[:, j].view(np.uint64)
        assert ok.all(), (what, v, "rows", first + np.flatnonzero(~ok.all(axis=1))[:5], vals[:, j][~ok][:4], want[:, j][~ok][:4])


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_call_records_every_step(nx, ny, lateral):
    """1. One rh_run_steps call of 150 steps: every header and value equals the reference, the sparse KEEP kernel ran."""
    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    for j, v in enumerate(VARS):
        assert np.any(ref.rows(VARS, cells)[:, j] != 0), f"{v} is zero in every reference row"
    ctx, _ = make_ctx(nx, ny, lateral)
    assert {"aet", "q_ss", "theta"} <= set(ctx.pure_output_planes())
    ctx.points_configure(cells, VARS)
    assert ctx.points_count() == 0
    ctx.run_steps(NSTEPS)
    assert ctx.points_count() == NSTEPS
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, ref, VARS, cells, 0, NSTEPS, f"{nx} x {ny} lateral={lateral}")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces_record_the_same_rows(nx, ny, lateral):
    """2. Pieces of 1, 2, 37 steps and the rest."""
    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.points_configure(cells, VARS)
    done = 0
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
        done += n
        assert ctx.points_count() == done
    assert_rows(ctx, ref, VARS, cells, 0, NSTEPS, f"{nx} x {ny} lateral={lateral} in pieces")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_launches_behind_the_time_limit_record_nothing(nx, ny, lateral):
    """3. 500 steps enqueued under a limit of three days: as many rows as the reference needs steps, none beyond the limit."""
    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    limit = 3 * 86400
    want = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    assert ref.hdr[want - 1, 1] == limit and 3 < want < NSTEPS
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.points_configure(cells, VARS)
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    assert ctx.points_count() == want
    hdr, _ = ctx.points_read(0, want)
    assert hdr[:, 1].max() == limit
    assert_rows(ctx, ref, VARS, cells, 0, want, f"{nx} x {ny} lateral={lateral} under the limit")
    ctx.run_steps(5)
    assert ctx.points_count() == want
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_ring_keeps_the_last_rows_and_refuses_the_overwritten_ones(nx, ny, lateral):
    """4. capacity 16 over 150 steps."""
    from roger_amd._native import NativeError

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.points_configure(cells, VARS, capacity=16)
    ctx.run_steps(NSTEPS)
    assert ctx.points_count() == NSTEPS
    assert_rows(ctx, ref, VARS, cells, NSTEPS - 16, 16, "the resident rows")     # straddles the wrap: 134 = 8 * 16 + 6
    assert_rows(ctx, ref, VARS, cells, NSTEPS - 5, 5, "the last rows")
    for first, n in ((NSTEPS - 17, 1), (NSTEPS - 17, 17), (0, 1)):
        with pytest.raises(NativeError, match=r"rh_points_read failed \(-1\).*overwritten"):
            ctx.points_read(first, n)
    with pytest.raises(NativeError, match=r"rh_points_read failed \(-1\).*not been recorded"):
        ctx.points_read(NSTEPS - 1, 2)
    ctx.close()


@pytest.mark.parametrize("points_first", [False, True])
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_accumulators_and_points_keep_each_others_planes(nx, ny, lateral, points_first):
    """5. Both observers, configured in either order, with disjoint pure outputs: slots and rows equal their references.  Fails if one
    configure call drops the other's keep bits (the sparse kernel then leaves that observer's planes unwritten)."""
    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    rate, collect, names = ("q_ss", "aet"), ("S_rz",), OTHER + ("theta", "swe", "S_fp_rz")
    ctx, _ = make_ctx(nx, ny, lateral)
    pure = set(ctx.pure_output_planes())
    assert set(rate) <= pure and set(OTHER) | {"theta"} <= pure and not pure & {"swe", "S_fp_rz", "S_rz"}
    if points_first:
        ctx.points_configure(cells, names)
    ctx.diag_configure(rate=rate, collect=collect, n_slots=3)
    if not points_first:
        ctx.points_configure(cells, names)
    acc = HostAccumulator(rate, collect, 3, ctx.n)
    for k in range(NSTEPS):
        acc.add(ref.hdr[k, 1], ref.hdr[k, 2], {v: ref.planes[v][k] for v in rate + collect})
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, ref, names, cells, 0, NSTEPS, f"points_first={points_first}")
    for slot in range(3):
        for v in rate + collect:
            assert same_bits(ctx.diag_download(v, slot), acc.data[v][slot]), (v, slot)
        assert ctx.diag_steps(slot) == acc.reported_steps(slot)
        assert ctx.diag_slot_times(slot) == (int(acc.t0[slot]), int(acc.t1[slot]))
    assert np.any(acc.data["q_ss"] != 0) and np.any(acc.data["aet"] != 0)
    # releasing the points leaves the accumulators' planes kept
    ctx.points_configure((), ())
    ctx.diag_configure(rate=rate, collect=collect, n_slots=3)
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_an_observed_m1_plane_switches_the_lazy_rotation_off(nx, ny, lateral):
    """6. S_rz_m1 among the observed planes: the rows equal the reference and the run ends in the reference's state."""
    import hip_util as H

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    names = ("q_ss", M1, "S_rz", "aet")
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.points_configure(cells, names)
    ctx.run_steps(NSTEPS)
    assert not ctx.step_mode()[0], "the lazy rotation stayed on"
    assert_rows(ctx, ref, names, cells, 0, NSTEPS, "with an X_m1 plane")
    assert np.any(ref.rows((M1,), cells) != 0)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), ref.final_scalars)
    for nm, want in ref.final.items():
        got = ctx.download(nm)
        assert got.dtype == want.dtype and (same_bits(got, want) if got.dtype.kind == "f" else (got == want).all()), nm
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True])
def test_every_float_plane_is_recorded_or_refused_by_name(lateral):
    """7. 3 x 2: every float64 plane the model holds, in groups of 32, over 40 steps of one call -- recorded equal to the reference or
    refused by rh_points_configure with its name; only the five lazily derived planes may be refused."""
    from roger_amd._native import NativeError

    nx, ny = 3, 2
    cells = POINTS[(nx, ny)]
    probe, _ = make_ctx(nx, ny, lateral)
    floats = float_planes(probe)
    probe.close()
    assert len(floats) > 150
    ref = Reference(nx, ny, lateral, floats, nsteps=ALL_STEPS)
    refused, recorded = set(), 0
    for g0 in range(0, len(floats), 32):
        group = floats[g0:g0 + 32]
        ctx, _ = make_ctx(nx, ny, lateral)
        while group:
            try:
                ctx.points_configure(cells, group)
                break
            except NativeError as e:
                named = [nm for nm in group if f"plane {nm} " in str(e)]
                assert "(-1)" in str(e) and len(named) == 1, str(e)
                refused.add(named[0])
                group = [nm for nm in group if nm != named[0]]
        if group:
            ctx.run_steps(ALL_STEPS)
            assert ctx.points_count() == ALL_STEPS
            if not any(nm.endswith("_m1") for nm in group):
                assert ctx.sparse_steps() > 0, group
            assert_rows(ctx, ref, group, cells, 0, ALL_STEPS, f"planes {group[0]} ... {group[-1]}")
            recorded += len(group)
        ctx.close()
    print(f"every-plane test, lateral={lateral}: {recorded} planes recorded, refused: {sorted(refused)}")
    assert refused <= {"k_rz", "k_ss", "h_rz", "h_ss", "ks_ss"}, refused
    assert recorded + len(refused) == len(floats)


def host_hooks(ctx, forcing):
    """set_forcing / set_parameters on the host, for the routine-by-routine step; returns the month-change decision."""
    import hip_util as H

    return H.HipForcingDriver(ctx, forcing).before_step()


def assert_last_row_is_the_state(ctx, names, cells, k, what):
    """Row k - 1 (the k-th step's) against the context's own planes and scalars after that step."""
    assert ctx.points_count() == k, what
    hdr, vals = ctx.points_read(k - 1, 1)
    s = ctx.get_scalars()
    assert tuple(hdr[0]) == (s.itt, s.time, s.dt_secs), (what, hdr, (s.itt, s.time, s.dt_secs))
    for j, v in enumerate(names):
        assert same_bits(vals[0, j], ctx.download(v)[list(cells)]), (what, v, k)


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_paths_record_one_row_per_step(path, lateral):
    """8a. rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step: one row per step, equal to the downloads after that
    step.  (Behind rh_step_core the row is written in front of rh_after_timestep, which leaves the tau planes alone but for snapping
    S_fp_* / S_lp_* in (-1e-6, 0) to zero: observed here are planes it does not assign.)"""
    nx, ny = 257, 1
    cells = POINTS[(nx, ny)]
    names = ("prec", "aet", "q_ss", "inf_mat_rz", "S_rz", "theta", "swe")
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.points_configure(cells, names)
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
        assert_last_row_is_the_state(ctx, names, cells, k, f"{path} lateral={lateral} step {k}")
        classes.add(ctx.get_scalars().dt_secs)
    assert len(classes) >= 2, classes
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES[2:4])
def test_one_rank_communicator_records_like_run_steps(nx, ny, lateral):
    """8b. rh_run_steps_dist with a one-rank RCCL communicator."""
    from roger_amd import _native as native

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.points_configure(cells, VARS)
    ctx.run_steps_dist(NSTEPS)
    assert ctx.points_count() == NSTEPS
    assert_rows(ctx, ref, VARS, cells, 0, NSTEPS, "rh_run_steps_dist, one rank")
    ctx.close()


def test_routed_steps_record_one_row_per_step(monkeypatch):
    """8c. The routed step on the smallest routing golden (4 x 6): rh_step_routed step by step against the downloads after each step,
    then the device-driven routed steps of rh_run_steps (and RH_ROUTED_BY_ROUTINE=1) against those rows."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    names = ("q_sur_out", "q_sub_in", "aet", "prec", "S", "z0", "q_ss")
    nsteps = 40
    ctx = routed_ctx(native, g, names_all)
    cells = tuple(range(ctx.n))
    ctx.points_configure(cells, names)
    drv = H.HipForcingDriver(ctx, forcing)
    for k in range(1, nsteps + 1):
        ctx.step_routed(drv.before_step())
        assert_last_row_is_the_state(ctx, names, cells, k, f"rh_step_routed step {k}")
    want_hdr, want = ctx.points_read(0, nsteps)
    assert all(np.any(want[:, j] != 0) for j in range(len(names)) if names[j] != "q_sub_in"), "a routed variable never held a value"
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.points_configure(cells, names)
        ctx.run_steps(nsteps)
        assert ctx.points_count() == nsteps
        hdr, vals = ctx.points_read(0, nsteps)
        np.testing.assert_array_equal(hdr, want_hdr)
        assert same_bits(vals, want), f"rh_run_steps on a routing context, by_routine={by_routine}"
        ctx.close()


def test_refusals_and_release():
    """9. RH_ERR_ARG with the offending value in the text, RH_ERR_STATE before the configuration and after the release."""
    from roger_amd._native import NativeError

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    for call in (ctx.points_count, lambda: ctx.points_read(0, 0)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.points_configure((0, 5), ("theta", "swe"), capacity=4)
    ctx.run_steps(3)
    bad = ((dict(cells=(0, 6), names=("theta",)), "cell 6 "), (dict(cells=(-1,), names=("theta",)), "cell -1 "),
           (dict(cells=(2, 4, 2), names=("theta",)), "cell 2 is given twice"), (dict(cells=(0,), names=(ints[0],)), f"plane {ints[0]} is int32"),
           (dict(cells=(0,), names=(not_held[0],)), f"plane id {ctx.index[not_held[0]]} "), (dict(cells=(0,), names=floats[:33]), "n_planes = 33"),
           (dict(cells=(0,), names=("theta",), capacity=0), "capacity = 0"), (dict(cells=(0,), names=("theta",), capacity=-3), "capacity = -3"))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_points_configure failed \(-1\)") as e:
            ctx.points_configure(**kw)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(NativeError, match=r"rh_points_configure failed \(-1\).*n_cells = 257"):
        ctx.points_configure(tuple(range(257)), ("theta",))
    # every refusal left the configuration working
    ctx.run_steps(2)
    assert ctx.points_count() == 5
    hdr, vals = ctx.points_read(1, 4)
    assert list(hdr[:, 0]) == [2, 3, 4, 5] and vals.shape == (4, 2, 2)
    assert same_bits(vals[-1, 0], ctx.download("theta")[[0, 5]])
    # 256 cells x 32 planes are accepted (a 257-column grid), and the release
    ctx.close()
    ctx, _ = make_ctx(257, 1, False)
    ctx.points_configure(tuple(range(256)), floats[:32], capacity=2)
    ctx.run_steps(3)
    hdr, vals = ctx.points_read(1, 2)
    assert vals.shape == (2, 32, 256) and same_bits(vals[-1, 5], ctx.download(floats[5])[:256])
    ctx.points_configure((), ("theta",))
    ctx.run_steps(2)
    for call in (ctx.points_count, lambda: ctx.points_read(0, 1)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.points_configure((3,), ("theta",), capacity=1)   # a new series starts at row 0
    assert ctx.points_count() == 0
    ctx.run_steps(2)
    hdr, vals = ctx.points_read(1, 1)
    assert hdr[0, 0] == 7 and same_bits(vals[0, 0], ctx.download("theta")[[3]])
    ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """End to end: a RogerSetup script with the reference's hook bodies (the device performs them: run() advances in rounds of
    rh_run_steps) and points with capacity 8 writes the same `.points.nc` values as the same script stepped routine by routine."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    cells, variables, ndays = [(0, 0), (2, 1), (1, 3)], ["theta_rz", "q_ss", "swe", "S_rz", "aet", "prec"], 6
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path):
            state.points.cells = list(cells)
            state.points.output_variables = list(variables)
            state.points.base_output_path = str(path)
            state.points.capacity = 8

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        rounds = []
        inner = model.run_device
        model.run_device = lambda n, final=True, inner=inner, rounds=rounds: (rounds.append(n), inner(n, final=final))[1]
        model.run()
        assert (mode == "device") == bool(rounds) and all(n <= 8 for n in rounds), rounds
        f = netcdf_file(str(path / "GoldenSVAT.points.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in ["Time", "dt", "itt", "ix", "iy", "x", "y"] + variables}
        model.state.backend_context.close()
    nsteps = int(np.sum(g["scal"][:, 1] <= ndays * 86400))
    for k, a in out["device"].items():
        b = out["routine"][k]
        assert a.shape == b.shape and same_bits(a, b) if a.dtype.kind == "f" else np.array_equal(a, b), k
    d = out["device"]
    assert len(d["Time"]) == nsteps + 1 and d["Time"][-1] == ndays and d["dt"][0] == 0 and list(d["itt"]) == list(range(nsteps + 1))
    # the file holds days: the golden's whole seconds divided by 86400 in float64, which multiplying back would not give exactly
    np.testing.assert_array_equal(d["Time"][1:], g["scal"][:nsteps, 1].astype(np.float64) / 86400.0)
    np.testing.assert_array_equal(np.rint(d["Time"][1:] * 86400), g["scal"][:nsteps, 1])
    assert all(np.any(d[v][1:] != 0) for v in variables)
