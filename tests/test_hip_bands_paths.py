"""GPU: the three quantile selections of the ensemble bands -- plain (k_bands_select), per zone (k_bands_zonal) and likelihood-weighted
(k_bands_select_w), roger_amd/csrc/rh_bands.h -- behind every way the project takes a step, as the clock-driven observers before them
(scores, events, durations) were pinned: lateral flow, the single-step entry points and the routed steps (launch_observers with
after_fused == 0: rh_step_core, routed_core, routed_passes), per-cell forcing on every front, no sparse stores, the seven other
observers on the same planes, and launches skipped behind the time limit.

The rule of tests/test_hip_bands.py holds throughout: the reference is never taken from the bands under test.  Planes and scalars come
from a context WITHOUT bands that is read after every single step (or, at the single-step entry points, from the stepping context's own
planes after every step, as tests/test_hip_durations.py (c) has it) and go through the host restatements bands_reference.HostBands,
bands_zonal_reference.HostZonalBands and bands_weighted_reference.HostWeightedBands.  Headers, m, n_nan, W and the zone counts are
compared exactly, values as uint64 bit patterns.

The three selections: plain under test_hip_bands.mask_of(n), per zone under test_hip_bands_zonal.three_zones(n), weighted under
test_hip_bands_weighted.weights_of(n).  mask_of and weights_of need 257 columns or more; on the 24 columns of the routing golden the
plain mask and the weights' zeros are `small_mask`: every fifth column off."""
import functools

import numpy as np
import pytest

from bands_reference import LAST, SUM, HostBands
from bands_weighted_reference import HostWeightedBands
from bands_zonal_reference import HostZonalBands
from durations_reference import AT_OR_ABOVE, BELOW, HostDurations
from test_hip_bands import DAY, GRIDS, KINDS, NAMES, PROBS, assert_rows, assert_state, expected, mask_of
from test_hip_bands import reference as svat_reference
from test_hip_bands_weighted import assert_weighted_rows, read_weighted, weights_of
from test_hip_bands_weighted import expected as weighted_expected
from test_hip_bands_zonal import assert_zonal_rows, three_zones, zonal_expected
from test_hip_durations import assert_durations, config_of
from test_hip_points import NDAYS, NSTEPS, POINTS, Reference, host_hooks, make_ctx

pytestmark = pytest.mark.gpu

SELECTIONS = ("plain", "zonal", "weighted")


def small_mask(n):
    return (np.arange(n) % 5 != 2).astype(np.uint8)


class Selection:
    """One of the three selections on n columns: its configuration, its host restatement, its reader and its comparison."""

    def __init__(self, kind, n):
        self.kind, self.n = kind, int(n)
        mask = mask_of(n) if n >= 257 else small_mask(n)
        self.mask = mask if kind == "plain" else None
        self.zone = three_zones(n) if kind == "zonal" else None
        if kind == "weighted":
            self.w = weights_of(n) if n >= 257 else (np.random.default_rng(17).integers(1, 65536, n) * mask).astype(np.uint16)
            assert (self.w == 0).any() and (self.w > 0).sum() > n // 2

    def configure(self, ctx, names, kinds, iv, capacity, probs=PROBS):
        if self.kind == "plain":
            ctx.bands_configure(names, kinds, probs, iv, 0, self.mask, capacity)
        elif self.kind == "zonal":
            ctx.bands_configure(names, kinds, probs, iv, 0, None, capacity, zones=self.zone, n_zones=3)
        else:
            ctx.bands_configure(names, kinds, probs, iv, 0, None, capacity, weights=self.w)
        assert ctx.bands_count() == 0

    def host(self, kinds, iv, probs=PROBS):
        if self.kind == "plain":
            return HostBands(kinds, probs, self.n, self.mask, iv, 0)
        if self.kind == "zonal":
            return HostZonalBands(kinds, probs, self.n, self.zone, 3, iv, 0)
        return HostWeightedBands(kinds, probs, self.n, self.w, iv, 0)

    def expected(self, ref, iv, nsteps=NSTEPS):
        """The rows of NAMES / KINDS over the first nsteps steps of a tests/test_hip_points.py Reference."""
        if self.kind == "plain":
            return expected(ref, iv, self.mask, nsteps=nsteps)
        if self.kind == "zonal":
            return zonal_expected(ref, iv, self.zone, 3, nsteps=nsteps)
        return weighted_expected(ref, iv, self.w, nsteps=nsteps)

    def read(self, ctx):
        n = ctx.bands_count()
        if self.kind == "plain":
            return ctx.bands_read(0, n)
        return ctx.bands_zonal_read(0, n) if self.kind == "zonal" else read_weighted(ctx)

    def assert_rows(self, got, want, what):
        check = {"plain": assert_rows, "zonal": assert_zonal_rows, "weighted": assert_weighted_rows}[self.kind]
        check(got, want, f"{self.kind}: {what}")

    @staticmethod
    def values(rows):
        """The float64 values of a result, whichever selection: (rows, item, ...)."""
        return rows[2] if len(rows) == 3 and rows[2].dtype == np.float64 else rows[1]


def restated(host, hdr, planes, names, nsteps=None):
    """The rows a restatement forms from a record: hdr (steps, 3) {itt, t1, dt_secs}, planes[name] (steps, n)."""
    for k in range(len(hdr) if nsteps is None else nsteps):
        t1, dt = int(hdr[k, 1]), int(hdr[k, 2])
        host.add(t1 - dt, t1, [planes[v][k] for v in names])
    return host.rows()


@functools.lru_cache(maxsize=None)
def reference(nx, ny, lateral):
    """tests/test_hip_bands.py's reference (a context without observers, read after every step), with lateral flow too: built the way
    tests/test_hip_durations.py builds its reference(nx, ny, lateral)."""
    if not lateral:
        return svat_reference(nx, ny)
    ref = Reference(nx, ny, True, NAMES, until=NDAYS * DAY, final=True)
    assert len(ref.hdr) == NSTEPS and set(ref.hdr[:, 2]) == {600, 3600, DAY}
    assert np.any(ref.planes["q_ss"] != 0) and np.ptp(ref.planes["theta_rz"][-1]) > 0
    return ref


# ---- 1. lateral flow ----
@pytest.mark.parametrize("pieces", [(NSTEPS,), (1, 2, 37, NSTEPS - 40)], ids=["one_call", "pieces"])
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_lateral_flow(sel, nx, ny, pieces):
    ref = reference(nx, ny, True)
    s = Selection(sel, nx * ny)
    want = s.expected(ref, 3600)
    assert NDAYS < len(want[0]) < NDAYS * 24
    ctx, _ = make_ctx(nx, ny, True)
    s.configure(ctx, NAMES, KINDS, 3600, NSTEPS)
    for n in pieces:
        ctx.run_steps(n)
    assert ctx.sparse_steps() > 0
    what = f"{nx} x {ny} lateral, calls of {pieces}"
    s.assert_rows(s.read(ctx), want, what)
    assert_state(ctx, ref, what)
    ctx.close()


# ---- 2. single-step entry points (after_fused == 0 behind rh_step_core) ----
@pytest.mark.parametrize("iv", [3600, 600])
@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
@pytest.mark.parametrize("sel", SELECTIONS)
def test_single_step_entry_points(sel, path, lateral, iv):
    """rh_adaptive_dt / rh_step_core / rh_after_timestep (launch_observers(ctx, 0) behind k_advance) and rh_svat_step at 257 x 1: the
    rows of the context's own planes and scalars after every step.  The items are planes rh_after_timestep does not assign."""
    nx, ny = 257, 1
    ctx, forcing = make_ctx(nx, ny, lateral)
    s = Selection(sel, ctx.n)
    s.configure(ctx, NAMES, KINDS, iv, 64)
    h = s.host(KINDS, iv)
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
        sc = ctx.get_scalars()
        h.add(sc.time - sc.dt_secs, sc.time, [ctx.download(v) for v in NAMES])
        classes.add(int(sc.dt_secs))
    want = h.rows()
    assert len(classes) >= 2 and iv in classes and len(want[0]) >= 3, (classes, len(want[0]))
    s.assert_rows(s.read(ctx), want, f"{path} lateral={lateral} iv={iv}")
    ctx.close()


# ---- 3. routed steps (after_fused == 0 in routed_core and in routed_passes) ----
ROUTED_STEPS = 140
# planes the routing writes, and S_m1: on a routing context the observers run between the numerics and the rotation (rh_stepping.h,
# routed_core and routed_passes), so an X_m1 plane still holds the PREVIOUS step's X when they read it
ROUTED_ITEMS = (("q_sur_out", SUM), ("q_ss", SUM), ("S", LAST), ("z0", LAST), ("S_m1", LAST))
ROUTED_NAMES, ROUTED_KINDS = tuple(v for v, _ in ROUTED_ITEMS), tuple(k for _, k in ROUTED_ITEMS)
ROUTED_DURATIONS = (("q_sur_out", SUM, None), ("q_ss", SUM, None), ("S", LAST, BELOW), ("theta", LAST, AT_OR_ABOVE))
ROUTED_WAYS = ("step_routed", "run_steps", "run_steps_by_routine")


def routed_case():
    from golden_util import ROUTING_CASES, load_case

    return load_case(ROUTING_CASES[0])


class RoutedRecord:
    pass


@functools.lru_cache(maxsize=None)
def routed_record():
    """What a routing context WITHOUT observers (the smallest routing golden, 4 x 6) holds after each of 140 calls of rh_step_routed:
    the scalars and the planes as the observers of that step see them -- an X_m1 plane as it was BEFORE the step's rotation, which is
    the download after the previous step (no routine of the routed step assigns one; the rotation does)."""
    import hip_util as H
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = routed_case()
    names = sorted(set(ROUTED_NAMES) | {v for v, _, _ in ROUTED_DURATIONS})
    ctx = routed_ctx(native, g, names_all)
    drv = H.HipForcingDriver(ctx, forcing)
    hdr, rows = [], {v: [] for v in names}
    before = {v: ctx.download(v) for v in names if v.endswith("_m1")}
    for _ in range(ROUTED_STEPS):
        ctx.step_routed(drv.before_step())
        s = ctx.get_scalars()
        hdr.append((s.itt, s.time, s.dt_secs))
        for v in names:
            now = ctx.download(v)
            rows[v].append(before[v] if v in before else now)
            if v in before:
                before[v] = now
    ctx.close()
    rec = RoutedRecord()
    rec.hdr = np.array(hdr, dtype=np.int64)
    rec.planes = {v: np.stack(rows[v]) for v in names}
    assert set(rec.hdr[:, 2]) == {600, 3600, DAY}, "the 140 steps do not hold the three step classes"
    assert (rec.planes["S_m1"][1:] == rec.planes["S"][:-1]).all() and (rec.planes["S_m1"] != rec.planes["S"]).any()
    return rec


def routed_run(way, configure, monkeypatch):
    """A fresh routing context, configured by `configure(ctx)`, after 140 routed steps taken in one of the three ways."""
    import hip_util as H
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = routed_case()
    if way == "run_steps_by_routine":
        monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
    else:
        monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
    ctx = routed_ctx(native, g, names_all)
    if way == "step_routed":
        configure(ctx)
        drv = H.HipForcingDriver(ctx, forcing)
        for _ in range(ROUTED_STEPS):
            ctx.step_routed(drv.before_step())
    else:
        ctx.set_forcing_series(forcing)
        configure(ctx)
        ctx.run_steps(ROUTED_STEPS)
    return ctx


@pytest.mark.parametrize("iv", [600, 3600])
@pytest.mark.parametrize("way", ROUTED_WAYS)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_routed_steps(sel, way, iv, monkeypatch):
    """rh_step_routed step by step (routed_core behind k_advance), then rh_run_steps on a routing context: the device-driven routed step
    (routed_passes, where the control kernel has advanced the time and rotated the scalars before the bands read the clock) and, with
    RH_ROUTED_BY_ROUTINE=1, the routine-by-routine step.  All three against the restatement of the observer-free record."""
    rec = routed_record()
    s = Selection(sel, rec.planes["S"].shape[1])
    want = restated(s.host(ROUTED_KINDS, iv), rec.hdr, rec.planes, ROUTED_NAMES)
    closing = rec.hdr[(rec.hdr[:, 1] % iv == 0) & (rec.hdr[:, 2] <= iv)]
    assert len(want[0]) == len(closing) >= 8 and (want[0][:, 1] == closing[:, 1]).all()
    if iv == 600:       # a step longer than the interval never closes one: the hourly and daily steps close no row
        assert set(closing[:, 2]) == {600} and (rec.hdr[:, 2] > 600).sum() >= 5
    values = s.values(want)
    assert all(np.any(np.nan_to_num(values[:, j]) != 0) for j in range(len(ROUTED_NAMES))), "a routed item never held a value"
    ctx = routed_run(way, lambda c: s.configure(c, ROUTED_NAMES, ROUTED_KINDS, iv, 256), monkeypatch)
    s.assert_rows(s.read(ctx), want, f"routing context, {way}, iv={iv}")
    ctx.close()


@pytest.mark.parametrize("iv", [600, 3600])
@pytest.mark.parametrize("way", ROUTED_WAYS)
def test_routed_steps_durations(way, iv, monkeypatch):
    """The clock's other user, k_durations, in the same three ways on the routing context: counters, spells and {acc, min, max} against
    HostDurations over the observer-free record, edges and thresholds from the record's own interval values (config_of)."""
    rec = routed_record()
    n = rec.planes["S"].shape[1]
    names, kinds = tuple(v for v, _, _ in ROUTED_DURATIONS), tuple(k for _, k, _ in ROUTED_DURATIONS)
    edges, spells = config_of(rec.hdr, rec.planes, iv, ROUTED_DURATIONS)
    mask = small_mask(n)
    h = HostDurations(kinds, edges, n, spells, mask, iv, 0)
    for k in range(len(rec.hdr)):
        t1, dt = int(rec.hdr[k, 1]), int(rec.hdr[k, 2])
        h.add(t1 - dt, t1, [rec.planes[v][k] for v in names])
    assert all(c.any() for c in h.counts) and h.spells.any()
    ctx = routed_run(way, lambda c: c.durations_configure(names, kinds, edges, spells, mask, iv, 0), monkeypatch)
    assert_durations(ctx, h, f"durations on a routing context, {way}, iv={iv}")
    ctx.close()


# ---- 4. per-cell forcing ----
PER_CELL_ITEMS = (("q_ss", SUM), ("prec", LAST), ("ta", LAST))   # a pure output; two planes the deferred selection applies inside the fused kernel
PER_CELL_CASES = [("svat_stations", 257, 1), ("svat_eberbaechle_weights", 40, 25)]


@pytest.mark.parametrize("front", ["one_launch", "old_front", "split_front", "front_max_0"])
@pytest.mark.parametrize("case,nx,ny", PER_CELL_CASES)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_per_cell_forcing(sel, case, nx, ny, front, monkeypatch):
    """Stations (all three step classes) on 257 x 1 and weights on 40 x 25, behind the default one-launch front k_cell_front and behind
    the predicate-kernel front, the split front and the front switched off by size; calls of 1, 2 steps and the rest."""
    import per_cell_observers as P
    from test_hip_per_cell_observers import FRONTS, assert_final_state, default_env

    default_env(monkeypatch)
    rec = P.reference(case, nx, ny)
    nsteps = len(rec.hdr)
    assert set(rec.hdr[:, 2]) == P.CLASSES[case]
    names, kinds = tuple(v for v, _ in PER_CELL_ITEMS), tuple(k for _, k in PER_CELL_ITEMS)
    s = Selection(sel, nx * ny)
    want = restated(s.host(kinds, 3600), rec.hdr, rec.planes, names)
    values = s.values(want)
    assert len(want[0]) >= 8 and all(np.any(values[:, j] != 0) for j in range(len(names)))
    assert np.any(rec.planes["prec"].max(axis=1) != rec.planes["prec"].min(axis=1)), "prec is the same in every column of every step"
    sparse = True
    if front != "one_launch":
        env, sparse = FRONTS[front]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    ctx = P.make_ctx(case, nx, ny)
    s.configure(ctx, names, kinds, 3600, nsteps)
    for n in (1, 2, nsteps - 3):
        ctx.run_steps(n)
    assert (ctx.sparse_steps() > 0) == sparse
    what = f"{case} {nx} x {ny}, {front}"
    s.assert_rows(s.read(ctx), want, what)
    assert_final_state(ctx, rec, what)
    ctx.close()


# ---- 5. RH_NO_SPARSE_STORES ----
@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_without_sparse_stores(sel, nx, ny, lateral, monkeypatch):
    """No sparse step runs, and the rows are those of the one-call run with sparse stores (and the restatement's)."""
    ref = reference(nx, ny, lateral)
    s = Selection(sel, nx * ny)
    rows = {}
    for sparse in (True, False):
        if not sparse:
            monkeypatch.setenv("RH_NO_SPARSE_STORES", "1")
        ctx, _ = make_ctx(nx, ny, lateral)
        s.configure(ctx, NAMES, KINDS, 3600, NSTEPS)
        ctx.run_steps(NSTEPS)
        assert (ctx.sparse_steps() > 0) == sparse and (sparse or ctx.sparse_steps() == 0)
        rows[sparse] = s.read(ctx)
        ctx.close()
    what = f"{nx} x {ny} lateral={lateral}"
    s.assert_rows(rows[False], rows[True], f"{what}: without sparse stores against the one-call run")
    s.assert_rows(rows[False], s.expected(ref, 3600), f"{what}: without sparse stores against the restatement")


# ---- 6. with the seven other observers on the same planes ----
OTHERS_DURATIONS = (("q_ss", SUM, None), ("theta_rz", LAST, BELOW))


def read_seven(ctx):
    """tests/test_hip_durations.py::read_six for the bands' planes, and the durations."""
    out = {"points": ctx.points_read(0, NSTEPS), "totals": ctx.totals_read(0, NSTEPS), "zonal": ctx.zonal_read(0, NSTEPS), "scores": ctx.scores_read()}
    hdr, values, lost = ctx.events_read()
    out["events"] = (hdr, np.stack([values[k] for k in sorted(values)]), np.array(sorted(values) + [int(lost)]))
    out["diag"] = (np.array([(ctx.diag_steps(k),) + ctx.diag_slot_times(k) for k in range(NDAYS)]),
                   np.stack([ctx.diag_download(v, k) for v in NAMES for k in range(NDAYS)]))
    counts, vals, spells = ctx.durations_read()
    out["durations"] = tuple(counts) + (vals, spells)
    return out


def with_the_seven(nx, ny, lateral, bands=None):
    """One call of 150 steps with diag, points, totals, zonal totals, scores, events and durations on NAMES [and the bands: a
    Selection]; (what the seven hold, the bands' rows or None)."""
    from test_hip_scores import observations, series_of
    from test_hip_totals import mask_of as area_of
    from test_hip_zonal import zones_of

    ref = reference(nx, ny, lateral)
    edges, spells = config_of(ref.hdr, ref.planes, 3600, OTHERS_DURATIONS)
    series, ns = series_of(nx * ny, "holes")
    zone, nz = zones_of(nx, ny, "mixed")
    ctx, _ = make_ctx(nx, ny, lateral)
    if bands is not None:
        bands.configure(ctx, NAMES, KINDS, 3600, NSTEPS)
    ctx.diag_configure(rate=NAMES[:1], collect=NAMES[1:], n_slots=NDAYS)
    ctx.points_configure(POINTS[(nx, ny)], NAMES)
    ctx.totals_configure(NAMES, area_of(nx, ny, "half"))
    ctx.zonal_configure(NAMES, zone, nz)
    ctx.scores_configure(NAMES, KINDS, observations(len(NAMES), ns, NDAYS + 2, seed=2), series, DAY, 0)
    ctx.events_configure(NAMES, (0, 3), 16)
    ctx.durations_configure(NAMES, KINDS, edges, spells, mask_of(nx * ny), 3600, 0)
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    out = read_seven(ctx), (None if bands is None else bands.read(ctx))
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def the_seven_alone(nx, ny, lateral):
    return with_the_seven(nx, ny, lateral)[0]


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("sel", SELECTIONS)
def test_with_the_seven_other_observers_on_the_same_planes(sel, lateral):
    """Accumulators, points, totals, zonal totals, scores, event outputs and duration curves on the bands' planes: what they hold is
    bit for bit what they hold without the bands, and the bands' rows are the restatement's."""
    nx, ny = 40, 25
    s = Selection(sel, nx * ny)
    alone = the_seven_alone(nx, ny, lateral)
    beside, rows = with_the_seven(nx, ny, lateral, s)
    assert alone.keys() == beside.keys()
    for key, parts in alone.items():
        assert len(parts) == len(beside[key]), key
        for a, b in zip(parts, beside[key]):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, key
            same = a.view(np.uint64) == b.view(np.uint64) if a.dtype == np.float64 else a == b
            assert same.all(), (key, "changed by the bands", np.argwhere(~same)[:5])
    assert np.any(alone["points"][1] != 0) and np.any(alone["scores"][0] != 0) and any(c.any() for c in alone["durations"][:2])
    s.assert_rows(rows, s.expected(reference(nx, ny, lateral), 3600), f"{nx} x {ny} lateral={lateral} beside the seven other observers")


# ---- 7. the time limit ----
@pytest.mark.parametrize("iv", [3600, DAY])
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_launches_behind_the_time_limit_record_nothing_and_leave_the_selection_clean(sel, nx, ny, iv):
    """500 steps enqueued under a limit of three days: the rows of the steps up to the limit, none from the skipped launches (each of
    the bands' seven to nine launches per step returns on D->skipped), none from five more.  rh_set_time_limit takes the limit away
    again (-1), so the run goes on to the end of the reference: the rows that follow are the restatement's, which they are only if the
    skipped launches left bands_done, the histograms, the prefixes and the counters as a finished selection leaves them."""
    ref = reference(nx, ny, False)
    limit = 3 * DAY
    nsteps = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    assert ref.hdr[nsteps - 1, 1] == limit and 3 < nsteps < NSTEPS
    s = Selection(sel, nx * ny)
    want = s.expected(ref, iv, nsteps=nsteps)
    assert len(want[0]) >= 3 and (iv != DAY or want[0][-1, 1] == limit)
    ctx, _ = make_ctx(nx, ny, False)
    s.configure(ctx, NAMES, KINDS, iv, NSTEPS)
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    what = f"{nx} x {ny} iv={iv}"
    assert ctx.bands_count() == len(want[0])
    s.assert_rows(s.read(ctx), want, f"{what}: under the limit")
    ctx.run_steps(5)
    assert ctx.bands_count() == len(want[0])
    s.assert_rows(s.read(ctx), want, f"{what}: five more skipped steps")
    ctx.set_time_limit(None)
    ctx.run_steps(NSTEPS - nsteps)
    full = s.expected(ref, iv)
    assert len(full[0]) > len(want[0])
    s.assert_rows(s.read(ctx), full, f"{what}: on to the end with the limit taken away")
    assert_state(ctx, ref, what)
    ctx.close()
