"""GPU: scores against observed series (rh_scores_*, k_scores in roger_amd/csrc/rh_scores.h) against the host restatement
(tests/scores_reference.py), moments as bits, closed flags exactly.

The reference is tests/test_hip_points.py's: a context WITHOUT observers that steps one step at a time and downloads the planes and the
clock after every step; the restatement forms the moments from them.  Grids: 3 x 2 (one partial wavefront), 257 x 1 (one column in the
second tile), 40 x 25, each for SVAT and oneD, over 8 days of the combo forcing: 150 steps of all three step classes, so that a daily
interval closes eight times and the hours under a daily step stay open."""
import functools

import numpy as np
import pytest

from diag_reference import HostAccumulator
from scores_reference import LAST, SUM, HostScores
from test_hip_points import CASES, M1, NDAYS, NSTEPS, make_ctx, reference, same_bits

pytestmark = pytest.mark.gpu

ITEMS = (("q_ss", SUM), ("S_rz", LAST), ("aet", SUM), ("theta", LAST))      # pure outputs (q_ss, aet, theta) and a stored plane
NAMES, KINDS = tuple(v for v, _ in ITEMS), tuple(k for _, k in ITEMS)
DAY = 86400


def series_of(n, kind):
    """The series map: None (every column series 0), or three series with holes."""
    if kind == "none":
        return None, 1
    s = (np.arange(n) % 3).astype(np.int32)
    if n == 6:
        s[4] = -1                                     # a single hole
    else:
        s[70] = -1                                    # a single hole,
        s[128:192] = -1                               # a whole empty wavefront
        if n == 257:
            s[256] = 2
        else:
            s[256:512] = -1                           # and a whole empty tile
    return s, 3


def observations(n_items, n_series, n_intervals, seed=0):
    rng = np.random.default_rng(100 + seed)
    o = rng.uniform(0.0, 5.0, size=(n_items, n_series, n_intervals))
    o[rng.random(o.shape) < 0.15] = np.nan           # missing observations
    o[:, :, 1] = np.where(np.arange(n_series)[None, :] == 0, np.nan, o[:, :, 1])
    return o


def expected(ref, names, kinds, obs, series, iv, t_first=0, nsteps=NSTEPS):
    h = HostScores(kinds, obs, ref.planes[names[0]].shape[1], series, iv, t_first)
    for k in range(nsteps):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in names])
    return h


def assert_scores(ctx, want, what):
    moments, closed = ctx.scores_read()
    np.testing.assert_array_equal(closed, want.closed, err_msg=f"{what}: closed")
    assert moments.shape == want.moments.shape, (what, moments.shape)
    ok = moments.view(np.uint64) == want.moments.view(np.uint64)
    assert ok.all(), (what, "(item, moment, column)", np.argwhere(~ok)[:5], moments[~ok][:3], want.moments[~ok][:3])


def configured(nx, ny, lateral, kind, iv, names=NAMES, kinds=KINDS):
    ref = reference(nx, ny, lateral)
    series, ns = series_of(nx * ny, kind)
    nk = NDAYS * DAY // iv + 2                        # two intervals beyond the run stay open
    obs = observations(len(names), ns, nk, seed=ns)
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.scores_configure(names, kinds, obs, series, iv, 0)
    return ctx, forcing, expected(ref, names, kinds, obs, series, iv)


@pytest.mark.parametrize("iv", [DAY, 3600])
@pytest.mark.parametrize("kind", ["none", "holes"])
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_call_against_the_restatement(nx, ny, lateral, kind, iv):
    """1. One rh_run_steps call; n_series 1 and 3, a hole, an empty wavefront, an empty tile, NaN observations, a day and an hour."""
    ctx, _, want = configured(nx, ny, lateral, kind, iv)
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_scores(ctx, want, f"{nx} x {ny} lateral={lateral} series={kind} iv={iv}")
    ctx.close()
    if iv == DAY:
        assert list(want.closed) == [1] * NDAYS + [0, 0]
    else:
        assert 0 < want.closed.sum() < NDAYS * 24 and not want.closed[-2:].any(), "the hours under a daily step stay open"
    assert all(np.any(want.moments[j, 1:] != 0) for j in range(len(NAMES)))


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces(nx, ny, lateral):
    """2. Pieces of 1, 2, 37 steps and the rest."""
    ctx, _, want = configured(nx, ny, lateral, "holes", DAY)
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
    assert_scores(ctx, want, f"{nx} x {ny} lateral={lateral} in pieces")
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_entry_points(path, lateral):
    """3. rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step: the moments of the context's own planes after every step
    (items are planes rh_after_timestep does not assign)."""
    from test_hip_points import host_hooks

    nx, ny, iv = 257, 1, 3600
    names, kinds = ("q_ss", "S_rz", "aet"), (SUM, LAST, SUM)
    series, ns = series_of(nx * ny, "holes")
    obs = observations(3, ns, 200, seed=5)
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.scores_configure(names, kinds, obs, series, iv, 0)
    h = HostScores(kinds, obs, ctx.n, series, iv, 0)
    classes = set()
    for _ in range(60):
        monthly = host_hooks(ctx, forcing)
        if path == "routines":
            ctx.call("rh_adaptive_dt")
            if monthly:
                ctx.call("rh_params_surface")
            ctx.call("rh_step_core")
            ctx.call("rh_after_timestep")
        else:
            ctx.step(monthly)
        s = ctx.get_scalars()
        h.add(s.time - s.dt_secs, s.time, [ctx.download(v) for v in names])
        classes.add(s.dt_secs)
    assert len(classes) >= 2 and h.closed.any()
    assert_scores(ctx, h, f"{path} lateral={lateral}")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_launches_behind_the_time_limit_change_nothing(nx, ny, lateral):
    """4. 500 steps enqueued under a limit of three days: the moments of the steps up to the limit, and nothing from the skipped launches."""
    ref = reference(nx, ny, lateral)
    limit = 3 * DAY
    nsteps = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    series, ns = series_of(nx * ny, "holes")
    obs = observations(len(NAMES), ns, 10, seed=1)
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.scores_configure(NAMES, KINDS, obs, series, DAY, 0)
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    want = expected(ref, NAMES, KINDS, obs, series, DAY, nsteps=nsteps)
    assert list(want.closed) == [1, 1, 1] + [0] * 7
    assert_scores(ctx, want, "under the limit")
    ctx.run_steps(5)
    assert_scores(ctx, want, "five more skipped launches")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES[2:])
def test_one_rank_communicator(nx, ny, lateral):
    """5. rh_run_steps_dist with a one-rank RCCL communicator."""
    from roger_amd import _native as native

    ctx, _, want = configured(nx, ny, lateral, "holes", DAY)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.run_steps_dist(NSTEPS)
    assert_scores(ctx, want, "rh_run_steps_dist, one rank")
    ctx.close()


def test_routed_steps(monkeypatch):
    """6. The routed step on the smallest routing golden: rh_step_routed step by step against the downloads after each step, then the
    device-driven routed steps of rh_run_steps (and RH_ROUTED_BY_ROUTINE=1) against those moments."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    names, kinds, nsteps, iv = ("q_sur_out", "aet", "S", "q_ss"), (SUM, SUM, LAST, SUM), 40, 3600
    ctx = routed_ctx(native, g, names_all)
    series = (np.arange(ctx.n) % 4 - 1).astype(np.int32)      # every fourth column not scored
    obs = observations(4, 3, 100, seed=9)
    ctx.scores_configure(names, kinds, obs, series, iv, 0)
    h = HostScores(kinds, obs, ctx.n, series, iv, 0)
    drv = H.HipForcingDriver(ctx, forcing)
    for _ in range(nsteps):
        ctx.step_routed(drv.before_step())
        s = ctx.get_scalars()
        h.add(s.time - s.dt_secs, s.time, [ctx.download(v) for v in names])
    assert h.closed.any() and np.any(h.moments[:, 1:] != 0)
    assert_scores(ctx, h, "rh_step_routed")
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.scores_configure(names, kinds, obs, series, iv, 0)
        ctx.run_steps(nsteps)
        assert_scores(ctx, h, f"rh_run_steps on a routing context, by_routine={by_routine}")
        ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_an_m1_item_switches_the_lazy_rotation_off(nx, ny, lateral):
    """7. S_rz_m1 among the items, next to a pure output and a stored plane."""
    names, kinds = ("q_ss", M1, "S_rz"), (SUM, LAST, LAST)
    ctx, _, want = configured(nx, ny, lateral, "holes", DAY, names, kinds)
    ctx.run_steps(NSTEPS)
    assert not ctx.step_mode()[0], "the lazy rotation stayed on"
    assert_scores(ctx, want, "with an X_m1 plane")
    assert np.any(want.moments[1, 1] != 0)
    ctx.close()


@pytest.mark.parametrize("order", ["first", "last", "again"])
@pytest.mark.parametrize("nx,ny,lateral", CASES[2:])
def test_with_the_other_observers(nx, ny, lateral, order):
    """8. Scores configured first, last, and a second time while accumulators, points, totals and zonal totals are active, on disjoint
    pure outputs: all five equal their references."""
    from test_hip_points import POINTS, assert_rows as assert_point_rows
    from test_hip_totals import assert_rows as assert_total_rows, mask_of
    from test_hip_zonal import assert_rows as assert_zonal_rows, zones_of

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    rate, collect = ("q_ss",), ("S_rz",)
    p_names, t_names, z_names = ("transp", "theta"), ("q_rz", "evap_soil"), ("inf_mat_rz", "swe")
    names, kinds = ("aet", "S_fp_rz"), (SUM, LAST)
    series, ns = series_of(nx * ny, "holes")
    obs = observations(2, ns, 10, seed=3)
    ctx, _ = make_ctx(nx, ny, lateral)
    zone, nz = zones_of(nx, ny, "mixed")

    def scores():
        ctx.scores_configure(names, kinds, obs, series, DAY, 0)

    def others():
        ctx.zonal_configure(z_names, zone, nz)
        ctx.totals_configure(t_names, mask_of(nx, ny, "half"))
        ctx.points_configure(cells, p_names)
        ctx.diag_configure(rate=rate, collect=collect, n_slots=3)

    if order == "first":
        scores(), others()
    elif order == "last":
        others(), scores()
    else:
        ctx.scores_configure(("theta", "q_rz"), (LAST, SUM), np.zeros((2, 1, 3)), None, 3600, 0)
        others(), scores()
    acc = HostAccumulator(rate, collect, 3, ctx.n)
    for k in range(NSTEPS):
        acc.add(ref.hdr[k, 1], ref.hdr[k, 2], {v: ref.planes[v][k] for v in rate + collect})
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_scores(ctx, expected(ref, names, kinds, obs, series, DAY), f"scores, configured {order}")
    assert_zonal_rows(ctx, nx, ny, lateral, "mixed", z_names, 0, NSTEPS, f"zonal, scores configured {order}")
    assert_total_rows(ctx, nx, ny, lateral, "half", t_names, 0, NSTEPS, f"totals, scores configured {order}")
    assert_point_rows(ctx, ref, p_names, cells, 0, NSTEPS, f"points, scores configured {order}")
    for slot in range(3):
        for v in rate + collect:
            assert same_bits(ctx.diag_download(v, slot), acc.data[v][slot]), (v, slot, order)
    ctx.scores_configure(())   # releasing the scores leaves the others' planes kept
    ctx.close()


@functools.lru_cache(maxsize=None)
def daily_sums(nx, ny, lateral):
    """(NDAYS, n): q_ss of every day by the output accumulators, eight slots resident -- an independent path on the device."""
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.diag_configure(rate=("q_ss",), n_slots=NDAYS)
    ctx.run_steps(NSTEPS)
    out = np.stack([ctx.diag_download("q_ss", d) for d in range(NDAYS)])
    assert all(ctx.diag_slot_times(d) == (d * DAY, (d + 1) * DAY) for d in range(NDAYS))
    ctx.close()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_cross_check_with_the_accumulators(nx, ny, lateral):
    """9. obs = 0 and a SUM item: m1 is the sequential sum over the days of what rh_diag_download gives for the same plane as a rate
    accumulator, bit for bit; m4 == m2; m3 == 0."""
    days = daily_sums(nx, ny, lateral)
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.scores_configure(("q_ss",), (SUM,), np.zeros((1, 1, NDAYS)), None, DAY, 0)
    ctx.run_steps(NSTEPS)
    m, closed = ctx.scores_read()
    ctx.close()
    assert closed.all()
    m1, m2 = np.zeros(ctx.n), np.zeros(ctx.n)
    for d in range(NDAYS):
        m1 = m1 + days[d]
        m2 = m2 + days[d] * days[d]
    assert np.any(m1 != 0)
    assert same_bits(m[0, 1], m1) and same_bits(m[0, 2], m2) and same_bits(m[0, 4], m[0, 2]) and (m[0, 3] == 0).all()
    assert same_bits(m[0, 0], days[-1])


@pytest.mark.parametrize("lateral", [False, True])
def test_twin_on_the_device(lateral):
    """10. Run one records a column's daily q_ss through the accumulators; run two scores every column of the heterogeneous grid against
    it: that column has sse == 0 exactly, every column that differs from it in any daily value has sse > 0."""
    nx, ny = 40, 25
    days = daily_sums(nx, ny, lateral)
    twin = int(np.argmax(days.sum(axis=0)))
    assert days[:, twin].any()
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.scores_configure(("q_ss",), (SUM,), np.ascontiguousarray(days[:, twin]).reshape(1, 1, NDAYS), None, DAY, 0)
    ctx.run_steps(NSTEPS)
    m, closed = ctx.scores_read()
    ctx.close()
    assert closed.all() and m[0, 4, twin] == 0.0
    differs = (days != days[:, twin:twin + 1]).any(axis=0)
    assert differs.sum() > ctx.n // 2 and (m[0, 4, differs] > 0).all() and (m[0, 4, ~differs] == 0).all()


def test_refusals_reconfiguration_and_release():
    """11. RH_ERR_ARG with the offending value in the text, RH_ERR_STATE before the configuration and after the release; a new
    configuration clears the moments."""
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    with pytest.raises(NativeError, match=r"rh_scores_read failed \(-3\)"):
        ctx.scores_read()
    ok = dict(names=("q_ss",), kinds=(SUM,), obs=np.zeros((1, 2, 4)), series=np.array([0, 1, -1, 0, 1, 1]), interval=3600, t_first=0)
    ctx.scores_configure(**ok)
    ctx.run_steps(8)
    now = int(ctx.get_scalars().time)
    assert now > 3600
    bad = ((dict(names=(ints[0],)), f"plane {ints[0]} is int32"), (dict(names=(not_held[0],)), f"plane id {ctx.index[not_held[0]]} "),
           (dict(names=floats[:17], kinds=(SUM,) * 17, obs=np.zeros((17, 2, 4))), "n_items = 17"),
           (dict(kinds=(2,)), "kind 2 of item 0"), (dict(obs=np.zeros((1, 1025, 2))), "n_series = 1025"),
           (dict(interval=7200, t_first=7200), "interval_seconds = 7200"), (dict(t_first=3600 * 24 * 30 + 600), "is not a multiple of the interval"),
           (dict(t_first=0), "lies behind the context's clock"), (dict(series=np.array([0, 1, 2, 0, 0, 0])), "series 2 of column 2"))
    for kw, text in bad:
        args = dict(ok, t_first=-(-now // 3600) * 3600)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_scores_configure failed \(-1\)") as e:
            ctx.scores_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="the series map has 5 values"):
        ctx.scores_configure(**dict(ok, series=np.zeros(5), t_first=-(-now // 3600) * 3600))
    # every refusal left the configuration working
    ctx.run_steps(2)
    m, closed = ctx.scores_read()
    assert m.shape == (1, 5, 6) and closed.shape == (4,) and (m[0, :, 2] == 0).all()
    # sixteen items and 1024 series are accepted; a new configuration starts from cleared moments at the next boundary
    t_first = -(-int(ctx.get_scalars().time) // 600) * 600
    ctx.scores_configure(floats[:16], (LAST,) * 16, np.ones((16, 1024, 3)), None, 600, t_first)
    m, closed = ctx.scores_read()
    assert m.shape == (16, 5, 6) and not m.any() and not closed.any()
    ctx.run_steps(3)
    ctx.scores_configure(())
    ctx.run_steps(2)
    with pytest.raises(NativeError, match=r"rh_scores_read failed \(-3\)"):
        ctx.scores_read()
    ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """12. End to end: a RogerSetup script with the reference's hook bodies and scores writes the same `.scores.nc` as the same script
    stepped routine by routine."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    nx, ny = (int(v) for v in g["nx_ny"])
    ndays = 6
    rng = np.random.default_rng(4)
    series = rng.integers(-1, 3, size=(nx, ny))
    obs = {"q_ss": rng.uniform(0.0, 3.0, size=(3, ndays + 1)), "theta_rz": rng.uniform(0.2, 0.4, size=(3, ndays + 1))}
    obs["q_ss"][0, 2] = np.nan
    keys = ["closed", "interval", "series"] + [f"{v}_{k}" for v in obs for k in ("sum_sim", "sum_sim2", "sum_simobs", "sse", "n", "bias", "rmse", "r", "nse", "kge")]
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path):
            state.scores.observations = obs
            state.scores.series = series
            state.scores.base_output_path = str(path)

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        model.run()
        f = netcdf_file(str(path / "GoldenSVAT.scores.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in keys}
        model.state.backend_context.close()
    d = out["device"]
    for k, a in d.items():
        b = out["routine"][k]
        assert (same_bits(a, b) if a.dtype.kind == "f" else (a.shape == b.shape and np.array_equal(a, b))), k
    assert list(d["closed"]) == [1] * ndays + [0] and (d["q_ss_n"][series.T == 0] == ndays - 1).all() and (d["q_ss_n"][series.T < 0] == 0).all()
    assert np.any(d["q_ss_sum_sim"][series.T >= 0] != 0) and np.any(d["theta_rz_sum_sim"][series.T >= 0] != 0)
