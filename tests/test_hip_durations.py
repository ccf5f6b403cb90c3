"""GPU: duration curves (rh_durations_*, k_durations in roger_amd/csrc/rh_durations.h) against the host restatement
(tests/durations_reference.py): counters and spell planes exactly, the float planes {acc, min, max} as bits.

The reference is tests/test_hip_points.py's: a context WITHOUT observers that steps one step at a time and downloads the planes and the
clock after every step; the restatement forms the histograms from them.  Grids: 3 x 2 (one partial wavefront), 257 x 1 (one column in the
second tile), 40 x 25 (several tiles), each for SVAT and oneD, over 8 days of the combo forcing: 150 steps of all three step classes.

Items: q_ss and aet summed (two pure outputs: the KEEP variant of the sparse kernel runs), S_rz at the interval's end with a `below`
spell, theta at the interval's end with an `at_or_above` spell.  Edges and thresholds come from the reference run itself (`config_of`):
the edges are quantiles of the reference's interval values, 0.0 and two values that occur exactly as interval values of some column;
the thresholds are the medians.  Before anything is compared the restatement alone must show at least three populated finite bins per
item, a value exactly on an edge, and -- at the hourly interval -- a column with longest >= 2 and n_spells >= 2."""
import functools

import numpy as np
import pytest

from durations_reference import AT_OR_ABOVE, BELOW, LAST, LONGEST, NSPELLS, SUM, HostDurations, interval_series
from test_hip_points import CASES, NDAYS, NSTEPS, make_ctx, reference

pytestmark = pytest.mark.gpu

ITEMS = (("q_ss", SUM, None), ("aet", SUM, None), ("S_rz", LAST, BELOW), ("theta", LAST, AT_OR_ABOVE))
NAMES, KINDS = tuple(v for v, _, _ in ITEMS), tuple(k for _, k, _ in ITEMS)
DAY = 86400
PROBS = (0.02, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.98)


def mask_of(n):
    """tests/test_hip_scores.py::series_of's holes as a mask: a single hole, a whole empty wavefront and, on 40 x 25, a whole empty tile."""
    from test_hip_scores import series_of

    return (series_of(n, "holes")[0] >= 0).astype(np.uint8)


def config_of(hdr, planes, iv, items=ITEMS):
    """(edges per item, spells per item) from a record's own interval values, and the checks on them."""
    edges, spells = [], []
    on_edge = 0
    for v, kind, side in items:
        steps = [(int(t1) - int(dt), int(t1), planes[v][k]) for k, (_, t1, dt) in enumerate(hdr)]
        s = interval_series(steps, kind, iv, 0)
        assert s.shape[0] >= 8 and np.isfinite(s).all(), (v, s.shape)
        flat = np.sort(s.reshape(-1))
        picked = (s[s.shape[0] // 2, s.shape[1] // 2], s[-1, 0])                  # two values that occur exactly as interval values
        e = np.unique(np.concatenate([np.quantile(flat, PROBS), [0.0], picked]))
        assert e.size <= 63
        bins = (e[None, :] <= flat[:, None]).sum(axis=1)
        assert np.count_nonzero(np.bincount(bins, minlength=e.size + 1)) >= 3, (v, "fewer than three finite bins are populated")
        on_edge += int(np.isin(flat, e).sum())
        edges.append(e)
        spells.append(None if side is None else (side, float(np.median(flat))))
    assert on_edge >= 1
    return edges, spells


@functools.lru_cache(maxsize=None)
def config(nx, ny, lateral, iv):
    ref = reference(nx, ny, lateral)
    return config_of(ref.hdr, ref.planes, iv)


def expected(ref, cfg, iv, mask=None, t_first=0, first=0, nsteps=NSTEPS, names=NAMES, kinds=KINDS):
    edges, spells = cfg
    h = HostDurations(kinds, edges, ref.planes[names[0]].shape[1], spells, mask, iv, t_first)
    for k in range(first, nsteps):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in names])
    return h


def assert_durations(ctx, want, what):
    counts, vals, spells = ctx.durations_read()
    assert len(counts) == len(want.counts)
    for j, c in enumerate(counts):
        np.testing.assert_array_equal(c, want.counts[j], err_msg=f"{what}: counts of item {j}")
    np.testing.assert_array_equal(spells, want.spells, err_msg=f"{what}: spell planes (item, {{run, longest, n_spells}}, column)")
    assert vals.shape == want.vals.shape, (what, vals.shape)
    ok = vals.view(np.uint64) == want.vals.view(np.uint64)
    assert ok.all(), (what, "(item, {acc, min, max}, column)", np.argwhere(~ok)[:5], vals[~ok][:3], want.vals[~ok][:3])


def configured(nx, ny, lateral, iv, masked, t_first=0):
    ref = reference(nx, ny, lateral)
    cfg = config(nx, ny, lateral, iv)
    mask = mask_of(nx * ny) if masked else None
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], mask, iv, t_first)
    return ctx, forcing, ref, cfg, mask


@functools.lru_cache(maxsize=None)
def one_call(nx, ny, lateral, iv, masked):
    """What the restatement holds after the whole run (shared by the cases that must equal (a))."""
    ref, cfg = reference(nx, ny, lateral), config(nx, ny, lateral, iv)
    return expected(ref, cfg, iv, mask_of(nx * ny) if masked else None)


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_the_restatement_alone_exercises_the_rule(nx, ny, lateral):
    """At the hourly interval some column has a longest run of at least two and at least two spells; the hours under a daily step are
    not counted; at the daily interval every day is."""
    want = one_call(nx, ny, lateral, 3600, False)
    both = (want.spells[:, LONGEST] >= 2) & (want.spells[:, NSPELLS] >= 2)
    assert (both[2] | both[3]).any(), "no column with longest >= 2 and n_spells >= 2"
    n = want.counts[0].sum(axis=0)
    assert (n == n[0]).all() and 0 < n[0] < NDAYS * 24
    assert (one_call(nx, ny, lateral, DAY, False).counts[0].sum(axis=0) == NDAYS).all()


@pytest.mark.parametrize("iv", [DAY, 3600])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_call_against_the_restatement(nx, ny, lateral, masked, iv):
    """(a) One rh_run_steps call; a day and an hour; without and with a mask."""
    ctx, _, _, _, mask = configured(nx, ny, lateral, iv, masked)
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    want = one_call(nx, ny, lateral, iv, masked)
    assert_durations(ctx, want, f"{nx} x {ny} lateral={lateral} masked={masked} iv={iv}")
    ctx.close()
    if masked:
        off = mask == 0
        assert off.any() and not any(c[:, off].any() for c in want.counts) and (want.vals[:, 1, off] == np.inf).all()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces(nx, ny, lateral):
    """(b) Pieces of 1, 2, 37 steps and the rest."""
    ctx, _, _, _, _ = configured(nx, ny, lateral, 3600, True)
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
    assert_durations(ctx, one_call(nx, ny, lateral, 3600, True), f"{nx} x {ny} lateral={lateral} in pieces")
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_entry_points(path, lateral):
    """(c) rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step at 257 x 1: the histograms of the context's own planes
    after every step (items are planes rh_after_timestep does not assign)."""
    from test_hip_points import host_hooks

    nx, ny, iv = 257, 1, 3600
    cfg, mask = config(nx, ny, lateral, iv), mask_of(nx * ny)
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], mask, iv, 0)
    h = HostDurations(KINDS, cfg[0], ctx.n, cfg[1], mask, iv, 0)
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
        h.add(s.time - s.dt_secs, s.time, [ctx.download(v) for v in NAMES])
        classes.add(s.dt_secs)
    assert len(classes) >= 2 and h.counts[0].any() and h.spells.any()
    assert_durations(ctx, h, f"{path} lateral={lateral}")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_without_sparse_stores(nx, ny, lateral, monkeypatch):
    """(d) RH_NO_SPARSE_STORES: equal to (a)."""
    monkeypatch.setenv("RH_NO_SPARSE_STORES", "1")
    ctx, _, _, _, _ = configured(nx, ny, lateral, 3600, True)
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() == 0
    assert_durations(ctx, one_call(nx, ny, lateral, 3600, True), f"{nx} x {ny} lateral={lateral} without sparse stores")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_reconfiguration_in_the_middle_of_a_day(nx, ny, lateral):
    """(e) A new configuration in the middle of a day: the counters restart, and `acc` of the interval under way holds only what was
    seen from then on -- the rule of an accumulator slot first touched inside its interval -- so that day is counted with that part;
    a refused configuration leaves the previous one counting."""
    from roger_amd._native import NativeError

    ref = reference(nx, ny, lateral)
    inside = [k for k in range(20, NSTEPS - 20) if ref.hdr[k - 1, 1] % DAY and ref.hdr[k, 1] % DAY]
    n1 = inside[len(inside) // 2]
    cfg = config(nx, ny, lateral, DAY)
    ctx, _, _, _, mask = configured(nx, ny, lateral, 3600, True)
    ctx.run_steps(n1)
    assert any(c.any() for c in ctx.durations_read()[0])
    ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], None, DAY, 0)
    counts, vals, spells = ctx.durations_read()
    assert not any(c.any() for c in counts) and not spells.any() and not vals[:, 0].any()
    assert (vals[:, 1] == np.inf).all() and (vals[:, 2] == -np.inf).all()
    for kw, text in ((dict(edges=[np.arange(64.0)] + list(cfg[0][1:])), "64 edges of item 0"),
                     (dict(edges=list(cfg[0][:3]) + [np.array([0.0, 1.0, 1.0])]), "edges of item 3 are not strictly ascending"),
                     (dict(interval=7200), "interval_seconds = 7200")):
        args = dict(names=NAMES, kinds=KINDS, edges=cfg[0], spells=cfg[1], mask=None, interval=DAY, t_first=0)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_durations_configure failed \(-1\)") as e:
            ctx.durations_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    ctx.run_steps(NSTEPS - n1)
    want = expected(ref, cfg, DAY, None, first=n1)
    day = int(ref.hdr[n1, 1]) // DAY
    assert (want.counts[0].sum(axis=0) == NDAYS - day).all(), "the day under way is counted with the part that was seen"
    assert_durations(ctx, want, f"{nx} x {ny} lateral={lateral} reconfigured after {n1} steps")
    ctx.close()


def read_six(ctx, slots):
    out = {"points": ctx.points_read(0, NSTEPS), "totals": ctx.totals_read(0, NSTEPS), "zonal": ctx.zonal_read(0, NSTEPS), "scores": ctx.scores_read()}
    hdr, values, lost = ctx.events_read()
    out["events"] = (hdr, np.stack([values[s] for s in sorted(values)]), np.array(sorted(values) + [int(lost)]))
    out["diag"] = (np.array([(ctx.diag_steps(s),) + ctx.diag_slot_times(s) for s in range(slots)]),
                   np.stack([ctx.diag_download(v, s) for v in NAMES for s in range(slots)]))
    return out


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_with_all_six_other_observers_on_the_same_planes(nx, ny, lateral):
    """(f) Accumulators, points, totals, zonal totals, scores and event outputs on the durations' planes: their results are what they
    are without state.durations, and the durations equal (a)."""
    from test_hip_points import POINTS
    from test_hip_scores import observations, series_of
    from test_hip_totals import mask_of as area_of
    from test_hip_zonal import zones_of

    cfg = config(nx, ny, lateral, 3600)
    series, ns = series_of(nx * ny, "holes")
    obs = observations(len(NAMES), ns, NDAYS + 2, seed=2)
    zone, nz = zones_of(nx, ny, "mixed")
    got = {}
    for with_durations in (False, True):
        ctx, _ = make_ctx(nx, ny, lateral)
        if with_durations:
            ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], mask_of(nx * ny), 3600, 0)
        ctx.diag_configure(rate=NAMES[:2], collect=NAMES[2:], n_slots=NDAYS)
        ctx.points_configure(POINTS[(nx, ny)], NAMES)
        ctx.totals_configure(NAMES, area_of(nx, ny, "half"))
        ctx.zonal_configure(NAMES, zone, nz)
        ctx.scores_configure(NAMES, KINDS, obs, series, DAY, 0)
        ctx.events_configure(NAMES, (0, 1, 2, 3), 16)
        ctx.run_steps(NSTEPS)
        assert ctx.sparse_steps() > 0
        got[with_durations] = read_six(ctx, NDAYS)
        if with_durations:
            assert_durations(ctx, one_call(nx, ny, lateral, 3600, True), f"{nx} x {ny} lateral={lateral} with the six other observers")
        ctx.close()
    for key, parts in got[False].items():
        for a, b in zip(parts, got[True][key]):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, key
            same = a.view(np.uint64) == b.view(np.uint64) if a.dtype == np.float64 else a == b
            assert same.all(), (key, "changed by the durations", np.argwhere(~same)[:5])
    assert np.any(got[True]["points"][1] != 0) and np.any(got[True]["scores"][0] != 0)


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_launches_behind_the_time_limit_count_nothing(nx, ny, lateral):
    """(g) 500 steps enqueued under a limit of three days: the histograms of the steps up to the limit, nothing from the skipped launches."""
    ref = reference(nx, ny, lateral)
    limit = 3 * DAY
    nsteps = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    ctx, _, _, cfg, mask = configured(nx, ny, lateral, 3600, True)
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    want = expected(ref, cfg, 3600, mask, nsteps=nsteps)
    assert ref.hdr[nsteps - 1, 1] == limit and want.counts[0].any()
    assert_durations(ctx, want, "under the limit")
    ctx.run_steps(5)
    assert_durations(ctx, want, "five more skipped launches")
    ctx.close()


@pytest.mark.parametrize("front", ["one_launch", "predicate_kernels"])
def test_per_cell_forcing(front, monkeypatch):
    """(h) Per-cell forcing (stations and weights) on 257 x 1, behind the one-launch front and behind the predicate-kernel front."""
    import per_cell_observers as P

    case, nx, ny, iv = "svat_stations", 257, 1, 3600
    rec = P.reference(case, nx, ny)
    nsteps = len(rec.hdr)
    assert set(rec.hdr[:, 2]) == {600, 3600, 86400}
    cfg = config_of(rec.hdr, rec.planes, iv)
    mask = mask_of(nx * ny)
    want = expected(rec, cfg, iv, mask, nsteps=nsteps)
    assert want.counts[0].any() and want.spells[2:, LONGEST].any()
    if front == "predicate_kernels":
        monkeypatch.setenv("RH_PER_CELL_OLD_FRONT", "1")
    ctx = P.make_ctx(case, nx, ny)
    ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], mask, iv, 0)
    for n in (1, 2, nsteps - 3):
        ctx.run_steps(n)
    assert ctx.sparse_steps() > 0
    assert_durations(ctx, want, f"{case} {nx} x {ny}, {front}")
    ctx.close()


def test_refusals_and_release():
    """RH_ERR_ARG naming the item, RH_ERR_STATE before the configuration and after the release; sixteen items of 63 edges are accepted."""
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    with pytest.raises(NativeError, match=r"rh_durations_read failed \(-3\)"):
        ctx.durations_read()
    e = np.array([0.0, 1.0])
    ok = dict(names=("q_ss", "theta"), kinds=(SUM, LAST), edges=[e, []], spells=[None, (BELOW, 0.3)], mask=None, interval=3600, t_first=0)
    ctx.durations_configure(**ok)
    ctx.run_steps(8)
    bad = ((dict(names=(ints[0], "theta")), f"item 0: plane {ints[0]} is int32"), (dict(names=("q_ss", not_held[0])), f"item 1: plane id {ctx.index[not_held[0]]} "),
           (dict(names=floats[:17], kinds=(SUM,) * 17, edges=[e] * 17, spells=[None] * 17), "n_items = 17"),
           (dict(kinds=(SUM, 2)), "kind 2 of item 1"), (dict(edges=[e, np.arange(64.0)]), "64 edges of item 1"),
           (dict(edges=[np.array([0.0, np.inf]), []]), "edge 1 of item 0 is not finite"), (dict(edges=[np.array([np.nan]), []]), "edge 0 of item 0 is not finite"),
           (dict(edges=[e, np.array([1.0, 1.0])]), "the edges of item 1 are not strictly ascending"),
           (dict(spells=[None, (2, 0.3)]), "side 2 of item 1"),
           (dict(interval=7200, t_first=7200), "interval_seconds = 7200"), (dict(t_first=600), "is not a multiple of the interval"))
    for kw, text in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_durations_configure failed \(-1\)") as err:
            ctx.durations_configure(**args)
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(ValueError, match="the mask has 5 values"):
        ctx.durations_configure(**dict(ok, mask=np.ones(5)))
    # every refusal left the configuration counting
    ctx.run_steps(2)
    counts, vals, spells = ctx.durations_read()
    assert [c.shape for c in counts] == [(4, 6), (2, 6)] and vals.shape == (2, 3, 6) and spells.shape == (2, 3, 6) and counts[0].any()
    # sixteen items of 63 edges are accepted, from cleared counters
    ctx.durations_configure(floats[:16], (LAST,) * 16, [np.arange(63.0)] * 16, [(AT_OR_ABOVE, 0.0)] * 16, None, 600, 0)
    counts, vals, spells = ctx.durations_read()
    assert len(counts) == 16 and all(c.shape == (65, 6) and not c.any() for c in counts) and not spells.any()
    ctx.run_steps(3)
    ctx.durations_configure(())
    ctx.run_steps(2)
    with pytest.raises(NativeError, match=r"rh_durations_read failed \(-3\)"):
        ctx.durations_read()
    ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """End to end: a RogerSetup script with the reference's hook bodies and durations writes the same `.durations.nc` as the same script
    stepped routine by routine."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine
    from roger_amd.durations import log_edges

    g, names, forcing = load_case("svat_hetero_combo")
    nx, ny = (int(v) for v in g["nx_ny"])
    ndays = 6
    mask = np.ones((nx, ny), dtype=int)
    mask[1, 2] = 0
    variables = {"q_ss": np.concatenate([[0.0], log_edges(1e-3, 10.0, 12)]), "theta_rz": np.linspace(0.1, 0.5, 9)}
    keys = [f"{v}_{k}" for v in variables for k in ("count", "n", "nan", "min", "max", "exceed", "q")] + ["theta_rz_longest", "theta_rz_spells", "theta_rz_run"]
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path):
            state.durations.variables = variables
            state.durations.spells = {"theta_rz": ("below", 0.3)}
            state.durations.mask = mask
            state.durations.base_output_path = str(path)

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        model.run()
        f = netcdf_file(str(path / "GoldenSVAT.durations.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in keys}
        model.state.backend_context.close()
    d = out["device"]
    for k, a in d.items():
        b = out["routine"][k]
        assert a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all() if a.dtype == np.float64 else np.array_equal(a, b), k
    assert (d["q_ss_n"][mask.T != 0] == ndays).all() and (d["q_ss_n"][mask.T == 0] == 0).all()
    assert np.count_nonzero(d["q_ss_count"].sum(axis=(1, 2))) >= 2 and d["theta_rz_longest"].max() >= 1
