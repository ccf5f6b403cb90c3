"""Helpers and child process of tests/test_hip_ranks_observers.py: the six device observers (accumulators, points, catchment totals, zonal
totals, scores, event outputs) behind the stepping of MORE THAN ONE RANK -- rh_run_steps_dist on SVAT blocks, the device-driven routed
steps with a communicator, and rh_step_routed's phase-1 / all-reduce / phase-2 path.  Ranks are threads of this process, one context
each, joined by the loopback communicator (tests/loopback_nccl.cpp through RH_RCCL_LIB), as in tests/loopback_ranks_child.py.

    python tests/ranks_observers.py svat_golden | svat_golden_alone | svat_tiles | routed | routed_by_routine

The reference is never the code under test: a single-domain context with NO observer and NO communicator steps with rh_run_steps(1)
-- a call's last step stores every plane -- and the observed planes and the scalars (itt, time, dt_secs, dt, event_id[1]) are downloaded
after every step (`reference`), anchored to the golden file where the case is one.  What rank r must hold is the observers' existing
numpy restatements (tests/per_cell_observers.py's assert_* / want_*, events_reference.HostEvents) applied to THE BLOCK'S COLUMNS of that
record (`Block`).  Masks, zone maps, series maps and point cells are defined on the global domain and cut to the block -- with
totals.local_mask / points.local_cells where the blocks are equal (the host package's own cut), by the block's column indices where they
are not (275 + 725, 256 + 1), and both ways where both apply.  An observer whose cut holds no column on a rank is not configured there,
as the host package leaves it off.  Tolerance zero: values as bits, headers, counts, closed flags and the lost flag exactly (minimum and
maximum with ==, tests/per_cell_observers.py::_assert_sum_min_max).

A rank thread only steps, reads and returns arrays (`Held`: what was read, behind the context's own read methods); every comparison
happens in the main thread after run_ranks has returned, so a failing assertion never leaves a peer waiting in a collective."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hip_util as H  # noqa: E402
import per_cell_observers as P  # noqa: E402
from events_reference import FIRST, LAST, PEAK, SUM, HostEvents  # noqa: E402
from golden_util import ROUTING_CASES, compare, load_case  # noqa: E402
from grid_ranks_child import block, neighbour_count, stitch  # noqa: E402
from grid_ranks_child import routed_ctx as routed_block_ctx  # noqa: E402
from loopback_ranks_child import loopback_counts, routed_ctx, run_ranks, svat_ctx  # noqa: E402
from roger_amd import _native as native  # noqa: E402
from roger_amd.points import local_cells  # noqa: E402
from roger_amd.totals import local_mask  # noqa: E402

ALL = ("diag", "points", "totals", "zonal", "scores", "events")
# the event outputs' items: all four kinds on pure outputs (q_ss, aet, theta), a stored plane (S_rz) and prec
EVENT_ITEMS = (("prec", SUM), ("prec", PEAK), ("q_ss", SUM), ("aet", PEAK), ("theta", FIRST), ("theta", LAST), ("S_rz", FIRST), ("S_rz", LAST))
EVENT_NAMES, EVENT_KINDS = tuple(v for v, _ in EVENT_ITEMS), tuple(k for _, k in EVENT_ITEMS)
EVENT_SLOTS = 16     # no event is lost: at most ten events in any run here
DAY = P.DAY


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
class Record(P.Record):
    """tests/per_cell_observers.py's Record with the two scalars the event outputs read: e (steps,) int64 = event_id[1], dt (steps,)."""

    def __init__(self, names):
        super().__init__(names)
        self._ev = []

    def take(self, ctx):
        s = super().take(ctx)
        self._ev.append((int(s.event_id[1]), float(s.dt)))
        return s

    def freeze(self):
        super().freeze()
        self.e = np.array([x[0] for x in self._ev], dtype=np.int64)
        self.dt = np.array([x[1] for x in self._ev], dtype=np.float64)
        return self


class Block:
    """The columns `cols` (global flat indices, in the block's own C order) of a Record: what the restatements of one rank are fed."""

    def __init__(self, rec, cols):
        self.hdr, self.e, self.dt = rec.hdr, rec.e, rec.dt
        self.planes = {v: np.ascontiguousarray(a[:, cols]) for v, a in rec.planes.items()}


def reference(ctx, nsteps, names, g=None, golden_names=None, snapshots=True, sane=True, what=""):
    """The Record of `ctx` (no observer, no communicator) over nsteps calls of rh_run_steps(1), with the final planes and scalars.  g: the
    golden file the run is anchored to -- the scalar row of EVERY step, and (snapshots) every stored snapshot inside the run.  sane:
    sanity_ok is asserted (not on routed runs: the reference's own water balance check fails there, as bench.py notes)."""
    rec = Record(names)
    anchored = 0
    for step in range(1, nsteps + 1):
        ctx.run_steps(1)
        s = rec.take(ctx)
        assert s.sanity_ok == 1 or not sane, (what, step)
        if g is not None:
            np.testing.assert_array_equal(H.scalars_to_row(s), g["scal"][step - 1], err_msg=f"{what}: scalars of the reference, step {step}")
            if snapshots and f"s{step:05d}" in g.files:
                compare(H.download_snapshot(ctx, golden_names), g[f"s{step:05d}"], golden_names, what=f"{what}: reference context, step {step}")
                anchored += 1
    rec.freeze()
    assert g is None or not snapshots or anchored >= 1, (what, "no stored snapshot inside the run")
    rec.final = {nm: ctx.download(nm) for nm, _ in ctx.planes[: ctx.planes_held]}
    rec.final_scalars = H.scalars_to_row(ctx.get_scalars())
    ctx.close()
    for v in ("prec", "aet", "q_ss", "S_rz", "theta"):
        assert v not in names or np.any(rec.planes[v] != 0), (what, v, "is zero at every step of the reference")
    rec.all_zero = [v for v in names if not np.any(rec.planes[v] != 0)]
    return rec


def classes_of(rec):
    """{step length: steps} inside events and outside them."""
    dts = rec.hdr[:, 2]
    return ({int(c): int(((dts == c) & (rec.e > 0)).sum()) for c in sorted(set(dts[rec.e > 0]))},
            {int(c): int(((dts == c) & (rec.e == 0)).sum()) for c in sorted(set(dts[rec.e == 0]))})


# ---- the global configuration and its cut to a block ----------------------------------------------------------------------------------
def point_cells(nx, ny):
    """Global flat cells: the tile and wavefront edges of tests/per_cell_observers.py on its grids, every second cell and the last one
    on the small domains."""
    if (nx, ny) in P.POINTS and nx * ny > 64:
        return tuple(P.POINTS[(nx, ny)])
    return tuple(range(0, nx * ny, 2)) + (nx * ny - 1,)


class Setup:
    """Mask, zone map, series map and point cells over the global nx x ny domain, and their cut to a block of columns."""

    def __init__(self, nx, ny):
        self.nx, self.ny, n = nx, ny, nx * ny
        self.mask = P.mask_of(n)
        self.zone, self.nz = P.zones_of(n)
        self.series = P.series_of(n)[0]
        self.cells = point_cells(nx, ny)

    def cut(self, cols, grid=None, rank=None):
        """dict(cells, mask, zones, series, rows) of a block; rows: the positions of the block's points in the global list.  With a
        process grid the host package's own cut must give the same."""
        cols = np.asarray(cols)
        where = {int(c): k for k, c in enumerate(cols)}
        rows = [k for k, c in enumerate(self.cells) if c in where]
        out = dict(cells=tuple(where[self.cells[k]] for k in rows), rows=rows, mask=self.mask[cols], zones=(np.ascontiguousarray(self.zone[cols]), self.nz),
                   series=np.ascontiguousarray(self.series[cols]))
        if grid is not None:
            nx, ny = self.nx, self.ny
            lc = local_cells([divmod(c, ny) for c in self.cells], nx, ny, grid, rank)
            assert [k for k, _ in lc] == rows and tuple(c for _, c in lc) == out["cells"], (grid, rank, lc, out["cells"])
            assert (local_mask(self.mask.reshape(nx, ny), nx, ny, grid, rank) == out["mask"]).all(), (grid, rank)
            assert (local_mask(self.zone.reshape(nx, ny), nx, ny, grid, rank) == out["zones"][0]).all(), (grid, rank)
            assert (local_mask(self.series.reshape(nx, ny), nx, ny, grid, rank) == out["series"]).all(), (grid, rank)
        return out


def on_this_rank(which, cut):
    """The observers of `which` the rank configures: one whose cut holds no column stays off (roger_amd/totals.py, zonal_totals.py,
    points.py: `_on`)."""
    off = set()
    if not cut["cells"]:
        off.add("points")
    if not cut["mask"].any():
        off.add("totals")
    if not (cut["zones"][0] >= 0).any():
        off.add("zonal")
    return tuple(w for w in which if w not in off)


# ---- a rank: configure, step, read -----------------------------------------------------------------------------------------------------
def configure(ctx, rec, which, names, cut):
    """`which` on `names` (the event outputs on EVENT_ITEMS); returns the scores' observations."""
    obs = P.configure(ctx, rec, [w for w in which if w != "events"], names, cells=cut["cells"], mask=cut["mask"], zones=cut["zones"], series=cut["series"])
    if "events" in which:
        ctx.events_configure(EVENT_NAMES, EVENT_KINDS, EVENT_SLOTS)
    return obs


class Held:
    """What a rank read from its context after the run, behind the context's own read methods: the assert_* helpers take it for a
    context, in the main thread."""

    def __init__(self, ctx, which, names, n_slots, snapshot_names=None):
        self.n, self.nx, self.ny, self.which = ctx.n, ctx.nx, ctx.ny, tuple(which)
        self.row = H.scalars_to_row(ctx.get_scalars())
        if "diag" in which:
            self._diag = {(v, s): ctx.diag_download(v, s) for v in names for s in range(n_slots)}
            self._dsteps = [ctx.diag_steps(s) for s in range(n_slots)]
            self._dtimes = [ctx.diag_slot_times(s) for s in range(n_slots)]
        if "points" in which:
            self._pcount = ctx.points_count()
            self._points = ctx.points_read(0, self._pcount)
        if "totals" in which:
            self._tcount = ctx.totals_count()
            self._totals = ctx.totals_read(0, self._tcount[0])
        if "zonal" in which:
            self._zcount = ctx.zonal_count()
            self._zonal = ctx.zonal_read(0, self._zcount[0])
        if "scores" in which:
            self._scores = ctx.scores_read()
        if "events" in which:
            self._events = ctx.events_read(slots=range(EVENT_SLOTS))
        if snapshot_names is not None:
            self.snap = H.download_snapshot(ctx, snapshot_names)
        else:
            self.final = {nm: ctx.download(nm) for nm, _ in ctx.planes[: ctx.planes_held]}

    def diag_download(self, v, slot):
        return self._diag[(v, slot)]

    def diag_steps(self, slot):
        return self._dsteps[slot]

    def diag_slot_times(self, slot):
        return self._dtimes[slot]

    def points_count(self):
        return self._pcount

    def points_read(self, first, n):
        return self._points[0][first:first + n], self._points[1][first:first + n]

    def totals_count(self):
        return self._tcount

    def totals_read(self, first, n):
        return self._totals[0][first:first + n], self._totals[1][first:first + n]

    def zonal_count(self):
        return self._zcount

    def zonal_read(self, first, n):
        return self._zonal[0][first:first + n], self._zonal[1][first:first + n]

    def scores_read(self):
        return self._scores

    def events_read(self, slots=None):
        return self._events


def step_in_pieces(ctx, pieces, dist, touch=None):
    """The calls of a run; touch: a plane the host writes back unchanged after the third piece (held.exch_valid / held.pre_valid are
    dropped, the next call starts from the arena).  Returns the largest rh_sparse_steps of a call."""
    sparse = 0
    for k, n in enumerate(pieces):
        if dist:
            ctx.run_steps_dist(n)
        else:
            ctx.run_steps(n)
        sparse = max(sparse, ctx.sparse_steps())
        if touch is not None and k == 2 and len(pieces) > 3:
            ctx.upload(touch, ctx.download(touch))
    return sparse


def want_events(blk, n):
    h = HostEvents(EVENT_KINDS, n, EVENT_SLOTS)
    for k in range(len(blk.hdr)):
        t1, dts = int(blk.hdr[k, 1]), int(blk.hdr[k, 2])
        h.add(blk.e[k], t1 - dts, t1, blk.dt[k], [blk.planes[v][k] for v in EVENT_NAMES])
    return h


def assert_events(held, want, what):
    """Headers and the lost flag exactly, every slot's maps as bits (tests/test_hip_events.py::assert_state)."""
    hdr, values, lost = held.events_read()
    np.testing.assert_array_equal(hdr, want.hdr, err_msg=f"{what}: headers of the event outputs")
    assert lost == want.lost and not lost, (what, "lost", lost)
    for s in range(want.ns):
        ok = values[s].view(np.uint64) == want.values[s].view(np.uint64)
        assert ok.all(), (what, "event outputs, slot", s, "(item, column)", np.argwhere(~ok)[:5], values[s][~ok][:3], want.values[s][~ok][:3])


class Expected:
    """The restatements of one rank that do not depend on the run: formed once, shared by the one-call run and the run in pieces."""

    def __init__(self, rec, cols, names, cut):
        self.blk, self.names, self.cut = Block(rec, cols), names, cut
        self.totals = P.want_totals(self.blk, names, cut["mask"]) if cut["mask"].any() else None
        self.zonal = P.want_zonal(self.blk, names, *cut["zones"]) if (cut["zones"][0] >= 0).any() else None
        self.events = want_events(self.blk, len(cols))

    def check(self, held, obs, what):
        cut = self.cut
        P.assert_observers(held, self.blk, [w for w in held.which if w != "events"], self.names, obs, totals=self.totals, zonal=self.zonal, what=what,
                           cells=cut["cells"], mask=cut["mask"], zones=cut["zones"], series=cut["series"])
        if "events" in held.which:
            assert_events(held, self.events, what)


def run_blocks(make, rec, setup, blocks, which, names, pieces, dist, grid=None, set_grid=False, touch=None, snapshot_names=None):
    """One run of len(blocks) ranks.  make(r): the rank's context (no communicator yet); blocks[r]: its global columns.  Returns
    (held per rank, observations, cuts, largest sparse count per rank, sends, all-reduces)."""
    nr = len(blocks)
    cuts = [setup.cut(blocks[r], grid, r if grid is not None else None) for r in range(nr)]
    on = [on_this_rank(which, cuts[r]) for r in range(nr)]
    for w in which:
        assert any(w in o for o in on), (w, "is configured on no rank")
    n_slots = P.n_days(rec)
    uid = native.comm_unique_id()
    s0, _, a0 = loopback_counts()

    def rank(r):
        ctx = make(r)
        ctx.comm_init(uid, nr, r)
        assert ctx.comm_info() == (nr, r)
        if set_grid:
            ctx.comm_set_grid(*grid)
        obs = configure(ctx, rec, on[r], names, cuts[r])
        sparse = step_in_pieces(ctx, pieces, dist, touch)
        held = Held(ctx, on[r], names, n_slots, snapshot_names)
        ctx.close()
        return held, obs, sparse

    res = run_ranks(rank, nr)
    s1, _, a1 = loopback_counts()
    obs = next((x[1] for x in res if x[1] is not None), None)
    return [x[0] for x in res], obs, cuts, [x[2] for x in res], s1 - s0, a1 - a0


def check_run(rec, expected, held, obs, what):
    """Every rank's scalars are the reference's, every configured observer holds its restatement."""
    for r, h in enumerate(held):
        np.testing.assert_array_equal(h.row, rec.final_scalars, err_msg=f"{what}, rank {r}: scalars differ from the single domain")
        expected[r].check(h, obs, f"{what}, rank {r} of {len(held)}")


def final_snapshot(rec, gnames):
    """The reference's final planes in the layout of hip_util.download_snapshot (a plane the context does not hold: zeros)."""
    n = len(next(iter(rec.final.values())))
    return np.stack([rec.final[nm].astype(np.float64) if nm in rec.final else np.zeros(n) for nm in gnames])


def assert_same_snapshot(got, rec, gnames, what):
    want = final_snapshot(rec, gnames)
    assert np.array_equal(got, want, equal_nan=True), (what, "planes differ from the single domain",
                                                       [gnames[p] for p in np.unique(np.argwhere(~((got == want) | ((got != got) & (want != want))))[:, 0])][:8])


def assert_final_planes(rec, held, blocks, what):
    """The blocks' final planes together are the reference's: the observers did not change the run."""
    for nm, want in rec.final.items():
        got = np.empty_like(want)
        for h, cols in zip(held, blocks):
            got[cols] = h.final[nm]
        ok = (got == want) | ((got != got) & (want != want)) if want.dtype.kind == "f" else got == want
        assert ok.all(), (what, "plane", nm, "columns", np.flatnonzero(~ok)[:5])


# ---- scenario 1: the SVAT golden under rh_run_steps_dist --------------------------------------------------------------------------------
def golden_prefix(g):
    """240 steps if that prefix of the golden run holds at least three events, all three step classes and two midnights -- from the
    golden's scalars alone -- and the whole run otherwise."""
    scal = g["scal"]
    for n in (240, int(g["nsteps"])):
        e, dts, t = scal[:n, 9].astype(np.int64), scal[:n, 2].astype(np.int64), scal[:n, 1].astype(np.int64)
        if len(set(e[e > 0])) >= 3 and set(dts) == {600, 3600, 86400} and int((t % DAY == 0).sum()) >= 2:
            return n
    raise AssertionError("the golden run holds fewer than three events, step classes or two midnights")


def svat_golden(alone):
    """svat_hetero_combo, 4 x 4: two halves and four one-column slabs with all six observers (alone = False; the halves once more with
    an X_m1 plane among the items), or every observer on its own on the two halves (alone = True: the plane union, has_observers and the
    KEEP bits differ).  Pieces of 1, 2, 38, 79 steps and the rest, a plane written back unchanged after the third."""
    case = "svat_hetero_combo"
    g, gnames, forcing = load_case(case)
    nx, ny = (int(v) for v in g["nx_ny"])
    nsteps = golden_prefix(g)
    pieces = (1, 2, 38, 79, nsteps - 120)
    rec = reference(svat_ctx(g, gnames, forcing), nsteps, P.VARS + (P.M1,), g, gnames, what=case)
    inside, outside = classes_of(rec)
    assert len(set(rec.e[rec.e > 0])) >= 3 and set(inside) | set(outside) == {600, 3600, 86400} and int((rec.hdr[:, 1] % DAY == 0).sum()) >= 2
    setup = Setup(nx, ny)
    flat = np.arange(nx * ny).reshape(nx, ny)
    halves, slabs = [flat[:nx // 2].ravel(), flat[nx // 2:].ravel()], [flat[x].ravel() for x in range(nx)]
    if alone:
        runs = [(f"{w} alone, two halves", halves, (w,), P.VARS) for w in ALL]
    else:
        runs = [("all six, two halves", halves, ALL, P.VARS), ("all six, four slabs", slabs, ALL, P.VARS),
                ("all six with S_rz_m1, two halves", halves, ALL, P.VARS + (P.M1,))]
    for what, blocks, which, names in runs:
        nr = len(blocks)
        edges = [int(b[0]) // ny for b in blocks] + [nx]
        held, obs, cuts, _, sends, reduces = run_blocks(lambda r: svat_ctx(g, gnames, forcing, columns=(edges[r], edges[r + 1])), rec, setup, blocks,
                                                        which, names, pieces, True, grid=(nr, 1), touch="S_dep", snapshot_names=gnames)
        expected = [Expected(rec, blocks[r], names, cuts[r]) for r in range(nr)]
        check_run(rec, expected, held, obs, f"{case}: {what}")
        got = np.concatenate([h.snap.reshape(len(gnames), -1, ny) for h in held], axis=1).reshape(len(gnames), -1)
        assert_same_snapshot(got, rec, gnames, f"{case}: {what}")
        compare(got, g[f"s{nsteps:05d}"], gnames, what=f"{case}: {what}, step {nsteps}")
        assert reduces >= nsteps and sends == 0, (what, sends, reduces)
        print(f"{case}: {what}: {nr} ranks == restatements of the single domain over {nsteps} steps; {reduces} all-reduces; "
              f"steps inside events {inside}, outside {outside}")


# ---- scenario 2: more than one workgroup per rank under rh_run_steps_dist ----------------------------------------------------------------
def svat_tiles():
    """tests/test_hip_points.py::make_ctx's columns (hetero_params(n, seed=5), combo forcing, 150 steps, four events), the parameters cut
    per block: 40 x 25 at x = 11 (275 + 725 columns: two and three workgroups, each with a ragged last wavefront) and 257 x 1 as
    256 + 1 (a full tile, and a rank of one column); all six observers, in one call and in pieces of 1, 2, 37 and the rest."""
    from test_hip_points import NDAYS, NSTEPS

    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    forcing = combo_forcing(ndays=NDAYS + 4)
    for (nx, ny, cutx) in ((40, 25, 11), (257, 1, 256)):
        for lateral in (False, True):
            what = f"{nx} x {ny} cut at x = {cutx}, lateral={lateral}"
            p = hetero_params(nx * ny, seed=5)
            if lateral:
                p.update(slope=0.05, slope_per=5, dmph=50.0)
                p["z_soil"] = np.maximum(p["z_soil"], 800.0)

            def make(r, p=p, lateral=lateral, nx=nx, ny=ny, cutx=cutx):
                x0, x1 = ((0, nx), (0, cutx), (cutx, nx))[r + 1]
                pr = {k: (v[x0 * ny:x1 * ny] if np.ndim(v) else v) for k, v in p.items()}
                ctx = create_svat(x1 - x0, ny, params=pr, lateral=lateral)
                ctx.set_forcing_series(forcing)
                return ctx

            rec = reference(make(-1), NSTEPS, P.VARS, what=what)
            assert rec.hdr[-1, 1] == NDAYS * DAY
            inside, outside = classes_of(rec)
            assert len(set(rec.e[rec.e > 0])) >= 3 and {600, 3600} <= set(inside) and 86400 in outside, (what, inside, outside)
            setup = Setup(nx, ny)
            blocks = [np.arange(0, cutx * ny), np.arange(cutx * ny, nx * ny)]
            expected = None
            for pieces in ((NSTEPS,), (1, 2, 37, NSTEPS - 40)):
                held, obs, cuts, sparse, sends, reduces = run_blocks(make, rec, setup, blocks, ALL, P.VARS, pieces, True, touch="S_dep")
                expected = expected or [Expected(rec, blocks[r], P.VARS, cuts[r]) for r in range(2)]
                check_run(rec, expected, held, obs, f"{what}, pieces {pieces}")
                assert_final_planes(rec, held, blocks, f"{what}, pieces {pieces}")
                assert all(s > 0 for s in sparse), (what, pieces, "rh_sparse_steps", sparse)
                assert reduces >= NSTEPS and sends == 0, (what, sends, reduces)
            print(f"svat tiles {what}: blocks of {[len(b) for b in blocks]} columns == restatements of the single domain over {NSTEPS} steps, in one "
                  f"call and in pieces; steps inside events {inside}, outside {outside}")


# ---- scenario 3: routed steps with ranks --------------------------------------------------------------------------------------------------
def routed(by_routine):
    """Device-driven rh_run_steps on routing contexts with a communicator: oned_routing (4 x 6, 240 steps) on two halves along x and on
    a (2, 2) grid (corner halos), oned_routing_combo (5 x 4, 202 steps) on (1, 2); all six observers, in one call and in pieces of 1,
    2, 37 and the rest.  by_routine (RH_ROUTED_BY_ROUTINE=1 in the environment): the two halves of oned_routing through rh_step_routed's
    phase-1 / all-reduce / phase-2 path.  The sends are tests/grid_ranks_child.py's per step, and the stitched final planes and the
    scalars the reference's: the observers change neither the exchange nor the run."""
    assert (os.environ.get("RH_ROUTED_BY_ROUTINE") == "1") == by_routine
    plan = [("oned_routing", (2, 1), False)] if by_routine else [("oned_routing", (2, 1), False), ("oned_routing", (2, 2), True),
                                                                 ("oned_routing_combo", (1, 2), True)]
    recs = {}
    for case, grid, set_grid in plan:
        g, gnames, forcing = load_case(case)
        nx, ny = (int(v) for v in g["nx_ny"])
        nsteps = int(g["nsteps"])
        if case not in recs:
            whole = routed_ctx(g, gnames)
            whole.set_forcing_series(forcing)
            recs[case] = reference(whole, nsteps, P.VARS, g, gnames, snapshots=case in ROUTING_CASES, sane=False, what=case)
        rec = recs[case]
        inside, outside = classes_of(rec)
        assert len(set(rec.e[rec.e > 0])) >= 2, (case, set(rec.e))
        if case == "oned_routing_combo":
            assert {600, 3600} <= set(inside) and set(inside) | set(outside) == {600, 3600, 86400}, (inside, outside)
        nr = grid[0] * grid[1]
        blocks = [block(g, "state0", grid, r)[1] for r in range(nr)]
        setup = Setup(nx, ny)

        def make(r, g=g, gnames=gnames, forcing=forcing, grid=grid):
            ctx = routed_block_ctx(g, gnames, grid, r)
            ctx.set_forcing_series(forcing)
            return ctx

        expected = None
        for pieces in ((nsteps,), (1, 2, 37, nsteps - 40)):
            what = f"{case} on {grid}{', by routine' if by_routine else ''}, pieces {pieces}"
            held, obs, cuts, _, sends, reduces = run_blocks(make, rec, setup, blocks, ALL, P.VARS, pieces, False, grid=grid, set_grid=set_grid,
                                                            snapshot_names=gnames)
            expected = expected or [Expected(rec, blocks[r], P.VARS, cuts[r]) for r in range(nr)]
            check_run(rec, expected, held, obs, what)
            got = stitch(g, gnames, grid, [h.snap for h in held])
            assert_same_snapshot(got, rec, gnames, what)
            if case in ROUTING_CASES:
                compare(got, g[f"s{nsteps:05d}"], gnames, what=what)
            n = neighbour_count(grid)
            assert sends == (2 * nsteps + 2) * n and reduces >= nsteps, (what, sends, (2 * nsteps + 2) * n, reduces)
        print(f"routed {case} on {grid}{', by routine' if by_routine else ''}: {nr} ranks == restatements of the single domain over {nsteps} "
              f"steps, in one call and in pieces; {sends} sends = (2 x {nsteps} + 2) x {n} neighbours; steps inside events {inside}, outside {outside}")


SCENARIOS = {"svat_golden": lambda: svat_golden(False), "svat_golden_alone": lambda: svat_golden(True), "svat_tiles": svat_tiles,
             "routed": lambda: routed(False), "routed_by_routine": lambda: routed(True)}

if __name__ == "__main__":
    t0 = time.perf_counter()
    SCENARIOS[sys.argv[1]]()
    print(f"{sys.argv[1]}: {time.perf_counter() - t0:.1f} s")
