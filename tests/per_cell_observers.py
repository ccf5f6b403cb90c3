"""Helpers of tests/test_hip_per_cell_observers.py: contexts with per-cell forcing (rh_set_forcing_weights, rh_set_forcing_stations) from
the two goldens of the reference that carry it, a reference without observers, and the observers' numpy restatements applied to it.

Columns: the golden's twelve (4 x 3), tiled over the grid with their weights and station indices (`rep`, as
tests/test_hip_parity.py::test_eberbaechle_full_series_80x53), so the global predicates and with them every step length stay the golden
run's.  Steps: a prefix of the golden run, chosen from the golden file alone (`prefix_steps`).

The reference (`Reference`) never contains an observer: a context with the same forcing steps with rh_run_steps(1) -- a call's last step
stores every plane -- and the observed planes and the scalars are downloaded after every call.  It is anchored to the reference
implementation at every stored step of the golden inside the prefix.  What an observer must hold is its existing restatement
(diag_reference.HostAccumulator, the plain gather, totals_reference.tree_totals with a mask / per zone, scores_reference.HostScores)
applied to those downloads."""
import functools

import numpy as np

from diag_reference import HostAccumulator
from golden_util import compare, load_case, load_stations, load_weights
from scores_reference import LAST, SUM, HostScores
from totals_reference import tree_totals

CASES = ("svat_eberbaechle_weights", "svat_stations")
GRIDS = ((4, 3), (257, 1), (40, 25))     # the golden's own twelve columns: one partial wavefront; a second tile of one column; four tiles
SMALL_GRIDS = ((4, 3), (40, 25))
# forcing planes (the deferred selection applies prec / ta inside the fused kernel), pure outputs (aet, q_ss, theta among them), state
VARS = ("prec", "ta", "pet", "aet", "q_ss", "inf_mat_rz", "S_rz", "theta", "swe")
PURE = ("aet", "q_ss", "theta")
M1 = "S_rz_m1"
OTHER = ("transp", "q_rz", "evap_soil", "S_fp_rz", "prec", "swe")     # the second configuration of the test in pieces
RATE, COLLECT = ("prec", "pet", "aet", "q_ss", "inf_mat_rz"), ("ta", "S_rz", "theta", "swe")
KIND_OF = dict({v: SUM for v in RATE}, **{v: LAST for v in COLLECT}, **{M1: LAST, "transp": SUM, "q_rz": SUM, "evap_soil": SUM, "S_fp_rz": LAST})
POINTS = {(4, 3): tuple(range(12)), (257, 1): (0, 63, 64, 255, 256), (40, 25): (0, 255, 256, 767, 959, 999)}
DAY = 86400
# The step classes of the whole golden run: the Eberbaechle run takes no ten-minute step in any of its 40 days (528 hourly and 18 daily
# steps), the station run takes all three.
CLASSES = {"svat_eberbaechle_weights": {3600, 86400}, "svat_stations": {600, 3600, 86400}}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def stored_steps(g):
    return sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit())


@functools.lru_cache(maxsize=None)
def prefix_steps(case):
    """The shortest prefix of the golden run that ends at a stored step and (a) shows every step class the run has, (b) holds two
    midnights, (c) holds a stored step at which part of the twelve columns lie under snow and part do not.  From the golden file alone."""
    g, names, _ = load_case(case)
    dt, t = g["scal"][:, 2].astype(np.int64), g["scal"][:, 1].astype(np.int64)
    swe = names.index("swe")
    partial = [s for s in stored_steps(g) if 0 < int((g[f"s{s:05d}"][swe] > 0).sum()) < g[f"s{s:05d}"].shape[1]]
    for n in stored_steps(g):
        if set(dt[:n]) == set(dt) and int((t[:n] % DAY == 0).sum()) >= 2 and partial and partial[0] <= n:
            return n
    raise AssertionError(f"{case}: no prefix of the golden run qualifies")


def rep_of(nx, ny):
    return np.arange(nx * ny) % 12


def day_of(case, nx, ny, i):
    """The per-cell day (n, 144) x 3 beginning at record i of the series, as the setups' set_forcing hook forms it on the host."""
    g, _, forcing = load_case(case)
    rep = rep_of(nx, ny)
    w, st = load_weights(g), load_stations(g)
    if st is not None:
        idx = st["station_index"][rep]
        rows = [np.where(idx[:, None] >= 0, st[k][np.maximum(idx, 0), i:i + 144], 0.0) for k in ("PREC", "TA", "PET")]
    else:
        rows = [np.broadcast_to(forcing[k][i:i + 144], (nx * ny, 144)) for k in ("PREC", "TA", "PET")]
    return (rows[0] * w["prec_weight"][rep][:, None], rows[1] + w["ta_offset"][rep][:, None], rows[2] * w["pet_weight"][rep][:, None])


def make_ctx(case, nx, ny, resident=True):
    """A context of nx x ny columns in the golden's initial state; resident: the series (or the stations') and the weights on the device."""
    import hip_util as H
    from roger_amd import _native as native

    g, names, forcing = load_case(case)
    assert tuple(int(v) for v in g["nx_ny"]) == (4, 3)
    rep = rep_of(nx, ny)
    ctx = native.Context(nx, ny)
    for row, nm in zip(g["state0"], names):
        if nm in ctx.index and ctx.index[nm] < ctx.planes_held:
            ctx.upload(nm, row[rep])
    ctx.set_scalars(H.scalars_from_row(g["scal0"]))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    if resident:
        st, w = load_stations(g), load_weights(g)
        if st is not None:
            ctx.set_forcing_stations(dict(PREC=st["PREC"], TA=st["TA"], PET=st["PET"], YEAR=forcing["YEAR"], MONTH=forcing["MONTH"],
                                          DOY=forcing["DOY"]), st["station_index"][rep])
        else:
            ctx.set_forcing_series(forcing)
        ctx.set_forcing_weights(w["prec_weight"][rep], w["ta_offset"][rep], w["pet_weight"][rep])
    return ctx


class HostHooks:
    """set_forcing / set_parameters on the host with the per-cell day handed over every midnight (hip_util.HipForcingDriver with the
    setups' weights and stations)."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.F = load_case(case)[2]

    def before_step(self):
        s = self.ctx.get_scalars()
        if s.time % DAY == 0:
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(self.F["YEAR"][i]), int(self.F["MONTH"][i]), int(self.F["DOY"][i])
            s.itt_forc = i + 144
            self.ctx.set_scalars(s)
            self.ctx.set_forcing_day(*day_of(self.case, self.ctx.nx, self.ctx.ny, i))
        return (s.month[1] != s.month[0]) and (s.itt > 1)


class Record:
    """hdr (steps, 3) int64: itt, time at the end of the step, dt_secs; planes[name] (steps, n) float64: what a context holds after
    every single step."""

    def __init__(self, names):
        self.names = tuple(names)
        self._hdr, self._rows = [], {v: [] for v in self.names}

    def take(self, ctx):
        s = ctx.get_scalars()
        self._hdr.append((s.itt, s.time, s.dt_secs))
        for v in self.names:
            self._rows[v].append(ctx.download(v))
        return s

    def freeze(self):
        self.hdr = np.array(self._hdr, dtype=np.int64)
        self.planes = {v: np.stack(self._rows[v]) for v in self.names}
        self.hdr.setflags(write=False)
        for a in self.planes.values():
            a.setflags(write=False)
        return self


@functools.lru_cache(maxsize=None)
def reference(case, nx, ny):
    """The Record of a context WITHOUT observers over prefix_steps(case) calls of rh_run_steps(1), anchored to the golden; with the
    final planes and scalars."""
    import hip_util as H

    g, names, _ = load_case(case)
    nsteps, rep = prefix_steps(case), rep_of(nx, ny)
    ctx = make_ctx(case, nx, ny)
    rec = Record(VARS + (M1,) + OTHER[:4])
    anchored = 0
    for step in range(1, nsteps + 1):
        ctx.run_steps(1)
        s = rec.take(ctx)
        assert s.sanity_ok == 1
        if f"s{step:05d}" in g.files:
            np.testing.assert_array_equal(H.scalars_to_row(s), g["scal"][step - 1], err_msg=f"{case} {nx} x {ny}: scalars of step {step}")
            compare(H.download_snapshot(ctx, names), g[f"s{step:05d}"][:, rep], names, what=f"{case} {nx} x {ny}: reference context, step {step}")
            anchored += 1
    rec.freeze()
    assert anchored >= 4 and (rec.hdr == g["scal"][:nsteps, :3].astype(np.int64)).all()
    rec.final = {nm: ctx.download(nm) for nm, _ in ctx.planes[: ctx.planes_held]}
    rec.final_scalars = H.scalars_to_row(ctx.get_scalars())
    ctx.close()
    return rec


# ---- the observers' configurations (per grid) and what they must hold ----------------------------------------------------------------
def mask_of(n):
    m = np.random.default_rng(100 + n).random(n) < 0.5
    assert 0 < m.sum() < n
    return m


def zones_of(n):
    """Two zones and columns outside every zone; on the larger grids an empty wavefront, on 40 x 25 an empty tile."""
    z = np.random.default_rng(7 + n).integers(-1, 2, size=n).astype(np.int32)
    if n > 128:
        z[64:128] = -1
    if n > 512:
        z[256:512] = -1
    assert (z == 0).any() and (z == 1).any() and (z < 0).any()
    return z, 2


def series_of(n):
    """Three observed series and columns that are not scored."""
    s = (np.arange(n) % 3).astype(np.int32)
    s[4] = -1
    if n > 192:
        s[128:192] = -1
    return s, 3


def observations(n_items, n_series, n_intervals, seed=0):
    """tests/test_hip_scores.py's: uniform values with missing ones."""
    rng = np.random.default_rng(100 + seed)
    o = rng.uniform(0.0, 5.0, size=(n_items, n_series, n_intervals))
    o[rng.random(o.shape) < 0.15] = np.nan
    o[:, :, 1] = np.where(np.arange(n_series)[None, :] == 0, np.nan, o[:, :, 1])
    return o


def n_days(rec):
    return int(-(-int(rec.hdr[-1, 1]) // DAY))


def obs_of(rec, names, t_first=0, seed=0):
    return observations(len(names), 3, n_days(rec) - t_first // DAY + 2, seed=seed)


def split(names):
    """(rate, collect) of a list of planes, in its order."""
    return tuple(v for v in names if KIND_OF[v] == SUM), tuple(v for v in names if KIND_OF[v] == LAST)


def configure(ctx, rec, which, names=VARS, t_first=0, seed=0, cells=None, mask=None, zones=None, series=None):
    """Configure the observers named in `which` on `names`; returns the scores' observations (None without scores).  cells, mask,
    zones = (map, number of zones), series: the context's own instead of the grid's (a rank's block of a global domain)."""
    n = ctx.n
    obs = None
    if "diag" in which:
        rate, collect = split(names)
        ctx.diag_configure(rate=rate, collect=collect, n_slots=n_days(rec))
    if "points" in which:
        ctx.points_configure(POINTS[(ctx.nx, ctx.ny)] if cells is None else cells, names)
    if "totals" in which:
        ctx.totals_configure(names, mask_of(n) if mask is None else mask)
    if "zonal" in which:
        ctx.zonal_configure(names, *(zones_of(n) if zones is None else zones))
    if "scores" in which:
        obs = obs_of(rec, names, t_first, seed)
        ctx.scores_configure(names, [KIND_OF[v] for v in names], obs, series_of(n)[0] if series is None else series, DAY, t_first)
    return obs


def want_totals(rec, names, mask, first=0, stop=None):
    return np.array([[tree_totals(rec.planes[v][k], mask) for v in names] for k in range(first, len(rec.hdr) if stop is None else stop)])


def want_zonal(rec, names, zone, nz, first=0, stop=None):
    return np.array([[[tree_totals(rec.planes[v][k], zone == z) for v in names] for z in range(nz)]
                     for k in range(first, len(rec.hdr) if stop is None else stop)])


@functools.lru_cache(maxsize=None)
def reference_totals(case, nx, ny):
    out = want_totals(reference(case, nx, ny), VARS, mask_of(nx * ny))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_zonal(case, nx, ny):
    out = want_zonal(reference(case, nx, ny), VARS, *zones_of(nx * ny))
    out.setflags(write=False)
    return out


def assert_diag(ctx, rec, names, first=0, stop=None, what="", n_slots=None):
    """The accumulators against HostAccumulator fed rows first ... stop - 1: every slot's values as bits, its steps and its times.
    n_slots: the slots the accumulators were configured with, if that was not this record's number of days."""
    rate, collect = split(names)
    acc = HostAccumulator(rate, collect, n_slots or n_days(rec), ctx.n)
    for k in range(first, len(rec.hdr) if stop is None else stop):
        acc.add(rec.hdr[k, 1], rec.hdr[k, 2], {v: rec.planes[v][k] for v in rate + collect})
    for slot in range(acc.n_slots):
        for v in rate + collect:
            got = ctx.diag_download(v, slot)
            ok = got.view(np.uint64) == acc.data[v][slot].view(np.uint64)
            assert ok.all(), (what, "accumulator", v, "slot", slot, "columns", np.flatnonzero(~ok)[:5], got[~ok][:3], acc.data[v][slot][~ok][:3])
        assert ctx.diag_steps(slot) == acc.reported_steps(slot), (what, "steps of slot", slot, ctx.diag_steps(slot), acc.reported_steps(slot))
        assert ctx.diag_slot_times(slot) == (int(acc.t0[slot]), int(acc.t1[slot])), (what, "times of slot", slot, ctx.diag_slot_times(slot),
                                                                                   (int(acc.t0[slot]), int(acc.t1[slot])))
    return acc


def assert_points(ctx, rec, names, first=0, stop=None, what="", cells=None):
    stop = len(rec.hdr) if stop is None else stop
    cells = list(POINTS[(ctx.nx, ctx.ny)] if cells is None else cells)
    assert ctx.points_count() == stop - first, (what, ctx.points_count(), stop - first)
    hdr, vals = ctx.points_read(0, stop - first)
    np.testing.assert_array_equal(hdr, rec.hdr[first:stop], err_msg=f"{what}: headers of the points' rows")
    want = np.stack([rec.planes[v][first:stop][:, cells] for v in names], axis=1)
    assert vals.shape == want.shape, (what, vals.shape, want.shape)
    for j, v in enumerate(names):
        ok = vals[:, j].view(np.uint64) == np.ascontiguousarray(want[:, j]).view(np.uint64)
        assert ok.all(), (what, "points", v, "rows", first + np.flatnonzero(~ok.all(axis=1))[:5], vals[:, j][~ok][:4], want[:, j][~ok][:4])


def _assert_sum_min_max(got, want, names, axis_v, what):
    """Sums as bits, minimum and maximum with == (fmin(-0.0, 0.0) may return either zero)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for j, v in enumerate(names):
        g, w = np.take(got, j, axis=axis_v), np.take(want, j, axis=axis_v)
        ok = np.ascontiguousarray(g[..., 0]).view(np.uint64) == np.ascontiguousarray(w[..., 0]).view(np.uint64)
        assert ok.all(), (what, v, "sum, at", np.argwhere(~ok)[:5], g[..., 0][~ok][:3], w[..., 0][~ok][:3])
        for k, stat in ((1, "min"), (2, "max")):
            ok = g[..., k] == w[..., k]
            assert ok.all(), (what, v, stat, "at", np.argwhere(~ok)[:5], g[..., k][~ok][:3], w[..., k][~ok][:3])


def assert_totals(ctx, rec, names, want, first=0, stop=None, what="", mask=None):
    stop = len(rec.hdr) if stop is None else stop
    assert ctx.totals_count() == (stop - first, int((mask_of(ctx.n) if mask is None else np.asarray(mask)).sum())), (what, ctx.totals_count())
    hdr, vals = ctx.totals_read(0, stop - first)
    np.testing.assert_array_equal(hdr, rec.hdr[first:stop], err_msg=f"{what}: headers of the totals' rows")
    _assert_sum_min_max(vals, want, names, 1, f"{what}: totals")


def assert_zonal(ctx, rec, names, want, first=0, stop=None, what="", zones=None):
    stop = len(rec.hdr) if stop is None else stop
    zone, nz = zones_of(ctx.n) if zones is None else zones
    rows, cells = ctx.zonal_count()
    assert rows == stop - first and list(cells) == list(np.bincount(zone[zone >= 0], minlength=nz)), (what, rows, cells)
    hdr, vals = ctx.zonal_read(0, stop - first)
    np.testing.assert_array_equal(hdr, rec.hdr[first:stop], err_msg=f"{what}: headers of the zonal rows")
    _assert_sum_min_max(vals, want, names, 2, f"{what}: zonal totals")


def want_scores(rec, names, obs, n, t_first=0, first=0, stop=None, series=None):
    h = HostScores([KIND_OF[v] for v in names], obs, n, series_of(n)[0] if series is None else series, DAY, t_first)
    for k in range(first, len(rec.hdr) if stop is None else stop):
        t1, dt = int(rec.hdr[k, 1]), int(rec.hdr[k, 2])
        h.add(t1 - dt, t1, [rec.planes[v][k] for v in names])
    return h


def assert_scores(ctx, want, what=""):
    moments, closed = ctx.scores_read()
    np.testing.assert_array_equal(closed, want.closed, err_msg=f"{what}: closed intervals of the scores")
    assert moments.shape == want.moments.shape, (what, moments.shape)
    ok = moments.view(np.uint64) == want.moments.view(np.uint64)
    assert ok.all(), (what, "scores (item, moment, column)", np.argwhere(~ok)[:5], moments[~ok][:3], want.moments[~ok][:3])


def assert_observers(ctx, rec, which, names, obs, totals=None, zonal=None, first=0, stop=None, t_first=0, what="", cells=None, mask=None,
                     zones=None, series=None):
    """Every observer of `which` against its restatement over rows first ... stop - 1 of the record.  totals / zonal: the expected rows
    if they are at hand (reference_totals / reference_zonal), formed here otherwise.  cells, mask, zones, series: as `configure`."""
    n = ctx.n
    if "diag" in which:
        assert_diag(ctx, rec, names, first, stop, what)
    if "points" in which:
        assert_points(ctx, rec, names, first, stop, what, cells)
    if "totals" in which:
        m = mask_of(n) if mask is None else mask
        assert_totals(ctx, rec, names, want_totals(rec, names, m, first, stop) if totals is None else totals, first, stop, what, mask)
    if "zonal" in which:
        z = zones_of(n) if zones is None else zones
        assert_zonal(ctx, rec, names, want_zonal(rec, names, *z, first, stop) if zonal is None else zonal, first, stop, what, zones)
    if "scores" in which:
        assert_scores(ctx, want_scores(rec, names, obs, n, t_first, first, stop, series), what)


def read_observers(ctx, rec, names=VARS):
    """Everything the five observers hold after the record's steps, for a comparison between two runs."""
    nrows, slots = len(rec.hdr), range(n_days(rec))
    out = {"points": ctx.points_read(0, nrows), "totals": ctx.totals_read(0, nrows), "zonal": ctx.zonal_read(0, nrows), "scores": ctx.scores_read()}
    out["diag"] = ({(v, s): ctx.diag_download(v, s) for v in names for s in slots}, [(ctx.diag_steps(s),) + ctx.diag_slot_times(s) for s in slots])
    return out


def assert_same_outputs(a, b, what):
    """Two read_observers results: headers, counts and closed flags exactly, values as bits (minimum and maximum with ==)."""
    np.testing.assert_array_equal(a["points"][0], b["points"][0], err_msg=what)
    assert same_bits(a["points"][1], b["points"][1]), (what, "points")
    for k in ("totals", "zonal"):
        np.testing.assert_array_equal(a[k][0], b[k][0], err_msg=what)
        assert same_bits(a[k][1][..., 0], b[k][1][..., 0]) and (a[k][1][..., 1:] == b[k][1][..., 1:]).all(), (what, k)
    assert same_bits(a["scores"][0], b["scores"][0]) and (a["scores"][1] == b["scores"][1]).all(), (what, "scores")
    assert a["diag"][1] == b["diag"][1] and a["diag"][0].keys() == b["diag"][0].keys(), (what, "accumulator slots")
    for key, v in a["diag"][0].items():
        assert same_bits(v, b["diag"][0][key]), (what, "accumulator", key)
