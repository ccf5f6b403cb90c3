"""The zonal recorder of the SAS context (rh_sas_zonal_*, roger_amd/csrc/rh_sas_zonal.h) restated on the host in numpy and loops: the
index over a zone map and both walks over its slots (include/roger_hip_sas.h).  Imports nothing from roger_amd.

A (tile of 256 cells, zone) pair that exists is a slot.  Width 1 (`slot_trees`, `finish_width1`): a slot's tile holds the identity
wherever a cell is not counted or belongs to another zone and goes through the wavefront trees and (w0 op w1) op (w2 op w3); accumulator
t of a zone takes the slots of the tiles with tile mod 256 == t in increasing tile order; the 256 accumulators go through the same two
levels.  Width W > 1 (`slot_runs`, `finish_ages`): the slot's cells are added left to right from +0.0; the zone's slots are walked in
increasing run order with nested accumulators -- a2 takes the slot partials, is added into a3 and cleared where run // 256 changes, a3
into a4 where run // 65536 changes, both flushed at the end.

What a block must equal is NOT computed here: the tests compare with sas_totals_reference.item_block(values, weight, zone == z)."""
import numpy as np

import sas_totals_reference as T

TILE = 256
STATS = (("sum", 0.0), ("sum", 0.0), ("sum", 0.0), ("min", np.inf), ("max", -np.inf))     # wsum, count, sum, min, max


class Index:
    """zone (n,) int: -1 outside, else 0 ... n_zones - 1.  slot_tile, slot_zone (S,): the slots, ascending by (tile, zone); cells[s]: the
    slot's cells in increasing order; acc[z][t] and runs[z]: the slots accumulator t of zone z takes, and the slots zone z walks, both
    in increasing tile order."""

    def __init__(self, zone, n_zones):
        zone = np.asarray(zone).reshape(-1).astype(np.int64)
        assert ((zone >= -1) & (zone < n_zones)).all()
        self.n, self.n_zones = zone.size, int(n_zones)
        self.slot_tile, self.slot_zone, self.cells = [], [], []
        for b in range((self.n + TILE - 1) // TILE):
            piece = zone[b * TILE:(b + 1) * TILE]
            for z in sorted(set(piece[piece >= 0].tolist())):
                self.slot_tile.append(b)
                self.slot_zone.append(z)
                self.cells.append(b * TILE + np.flatnonzero(piece == z))
        self.acc = [[[] for _ in range(TILE)] for _ in range(self.n_zones)]
        self.runs = [[] for _ in range(self.n_zones)]
        for s, (b, z) in enumerate(zip(self.slot_tile, self.slot_zone)):
            self.acc[z][b % TILE].append(s)
            self.runs[z].append(s)
        self.ncells = np.bincount(zone[zone >= 0], minlength=self.n_zones).astype(np.int64)


def slot_trees(ix, x, stat, identity):
    """x (n,) already holds the identity where a cell is not counted: the (S,) partials of the slots."""
    S = len(ix.cells)
    tiles = np.full((S, TILE), identity, dtype=np.float64)
    for s, c in enumerate(ix.cells):
        tiles[s, c - ix.slot_tile[s] * TILE] = x[c]
    return T._tile(tiles.reshape(S, 4, 64), T.OP[stat]) if S else np.zeros(0)


def finish_width1(ix, partials, stat, identity):
    op = T.OP[stat]
    out = np.empty(ix.n_zones)
    for z in range(ix.n_zones):
        acc = np.full(TILE, identity, dtype=np.float64)
        for t in range(TILE):
            for s in ix.acc[z][t]:            # in increasing tile order
                acc[t] = op(acc[t], partials[s])
        out[z] = T._tile(acc.reshape(1, 4, 64), op)[0]
    return out


def slot_runs(ix, t):
    """t (n, W) already holds +0.0 for skipped cells and NaN elements: (S, W), every slot's cells added left to right from +0.0."""
    out = np.zeros((len(ix.cells), t.shape[1]), dtype=np.float64)
    for s, c in enumerate(ix.cells):
        acc = np.zeros(t.shape[1], dtype=np.float64)
        for k in c:
            acc = acc + t[k]
        out[s] = acc
    return out


def finish_ages(ix, partials):
    out = np.empty((ix.n_zones, partials.shape[1]))
    for z in range(ix.n_zones):
        a2, a3, a4 = (np.zeros(partials.shape[1]) for _ in range(3))
        prev = None
        for s in ix.runs[z]:                  # in increasing run order
            run = ix.slot_tile[s]
            if prev is not None and run // 256 != prev // 256:
                a3, a2 = a3 + a2, np.zeros_like(a2)
                if run // 65536 != prev // 65536:
                    a4, a3 = a4 + a3, np.zeros_like(a3)
            a2 = a2 + partials[s]
            prev = run
        a3 = a3 + a2
        out[z] = a4 + a3
    return out


def zone_blocks(ix, values, weight=None, live=True):
    """(n_zones, 5) for values (n,), (n_zones, 2 + W) for values (n, W): every zone's row block of one item."""
    v = np.asarray(values, dtype=np.float64)
    n = v.shape[0]
    assert n == ix.n
    e = T.eligible(n, weight, None, live)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        if v.ndim == 1:
            c = e & ~np.isnan(v)
            t = v if weight is None else v * w                                    # rounded before it is added
            cols = (np.where(c, w, 0.0), np.where(c, 1.0, 0.0), np.where(c, t, 0.0), np.where(c, v, np.inf), np.where(c, v, -np.inf))
        else:
            t = v if weight is None else v * w[:, None]
            t = np.where(e[:, None] & ~np.isnan(v), t, 0.0)
            cols = (np.where(e, w, 0.0), np.where(e, 1.0, 0.0))
        head = [finish_width1(ix, slot_trees(ix, x, stat, ident), stat, ident) for x, (stat, ident) in zip(cols, STATS)]
        if v.ndim == 1:
            return np.stack(head, axis=1)
        return np.concatenate([np.stack(head, axis=1), finish_ages(ix, slot_runs(ix, t))], axis=1)


def want_rows(ix, d, items, day):
    """{item: (n_zones, block)} for a record with `day` on the inputs of sas_totals_reference.make_inputs (a negative day: no daily row)."""
    out = {}
    r = day % 3 if day >= 0 else 0
    for it in items:
        v, w = (it, None) if isinstance(it, str) else it
        live = day >= 0 or (w is None and v not in T.DAILY)
        out[v if w is None else f"{v}_by_{w}"] = zone_blocks(ix, d[v][r] if v in T.DAILY else d[v], None if w is None else d[w][r], live)
    return out


def as_blocks(stats, k):
    """Row k of the dict of SasContext.zonal_read for one item as (n_zones, block)."""
    head = [stats["wsum"][k][:, None], stats["count"][k][:, None]]
    total = stats["sum"][k]
    tail = [stats["min"][k][:, None], stats["max"][k][:, None]] if "min" in stats else []
    return np.concatenate(head + [total[:, None] if total.ndim == 1 else total] + tail, axis=1)


def _with_an_empty_id(zone, used):
    """`zone` over the ids 0 ... used - 1 -> the ids 0 ... used with id used // 2 left without a cell."""
    hole = used // 2
    return np.where(zone >= hole, zone + 1, zone).astype(np.int32), used + 1


def zone_maps(n, Z=7):
    """{name: (zone (n,) int32, n_zones)}; every map has one zone id without a cell.
    blocks  contiguous zones whose borders fall inside tiles, with -1 sprinkled in
    mix     random ids, -1 included
    many    300 zones over n = 1000 (at that n only)
    sparse  a zone living only in the cells >= 65 536 (where n is smaller: in the last cells), a zone with a single cell, the rest
            in two interleaved zones with gaps"""
    rng = np.random.default_rng(77 * n + Z)
    c = np.arange(n)
    used = Z - 1
    out = {}
    blocks = np.minimum(c * used // max(n, 1), used - 1) if n >= used else c % used
    if n > 300:
        blocks = np.minimum((c + 37) * used // (n + 37), used - 1)        # (borders off the multiples of 256)
    blocks = blocks.copy()
    if n >= 5:
        blocks[rng.permutation(n)[:max(1, n // 9)]] = -1
    out["blocks"] = _with_an_empty_id(blocks, used)
    mix = rng.integers(-1, used, size=n)
    if not (mix >= 0).any():
        mix[0] = 0
    out["mix"] = _with_an_empty_id(mix, used)
    if n == 1000:
        many = rng.integers(0, 299, size=n)
        many[rng.permutation(n)[:50]] = -1
        out["many"] = _with_an_empty_id(many, 299)
    far = 65536 if n > 65536 else n - 1 - (n - 1) // 4
    sparse = np.where(c % 3 == 2, -1, c % 3)
    sparse[far:] = np.where(c[far:] % 2 == 0, 2, sparse[far:])
    sparse[n // 3] = 3
    if n == 1:
        sparse[0] = 0
    out["sparse"] = _with_an_empty_id(sparse, 4)
    return out


def __getattr__(name):
    """ZonalOracleSasContext: the oracle double with the four zonal_* methods of `_native.SasContext`, for the host-package tests.  Built
    on first use, so that importing this module imports nothing from roger_amd."""
    if name != "ZonalOracleSasContext":
        raise AttributeError(name)
    from test_host_package_sas_totals import TotalsOracleSasContext

    class ZonalOracleSasContext(TotalsOracleSasContext):
        _zon = None

        def zonal_configure(self, items, zones=None, n_zones=0, capacity=4096):
            items = [(it, None) if isinstance(it, str) else tuple(it) for it in items]
            self._zon = None
            if items:
                self._zon = dict(items=items, ix=Index(zones, n_zones), cap=int(capacity), rows=[], tags=[])

        def zonal_record(self, tag=0, day=-1):
            from roger_amd._native import DAILY_INPUTS

            t, held = self._zon, self._arrays()
            row = {}
            for v, w in t["items"]:
                live = day >= 0 or (w is None and v not in DAILY_INPUTS)
                row[v if w is None else f"{v}_by_{w}"] = zone_blocks(t["ix"], held[v], None if w is None else held[w], live)
            t["rows"].append(row)
            t["tags"].append(int(tag))

        def zonal_count(self):
            return len(self._zon["rows"]), self._zon["ix"].ncells.copy()

        def zonal_read(self, first, n):
            t = self._zon
            assert first >= len(t["rows"]) - t["cap"] and first + n <= len(t["rows"]), "rows overwritten or not recorded"
            out = {}
            for key in t["rows"][0] if t["rows"] else ():
                blocks = np.array([r[key] for r in t["rows"][first:first + n]]).reshape(n, t["ix"].n_zones, -1)
                d = {"wsum": blocks[:, :, 0].copy(), "count": blocks[:, :, 1].copy()}
                if blocks.shape[2] == 5:
                    d.update(sum=blocks[:, :, 2].copy(), min=blocks[:, :, 3].copy(), max=blocks[:, :, 4].copy())
                else:
                    d["sum"] = blocks[:, :, 2:].copy()
                out[key] = d
            return np.array(t["tags"][first:first + n], dtype=np.int64), out

        def step(self, day):
            super().step(day)
            if self._zon is not None:
                self.zonal_record(day, day)

    globals()[name] = ZonalOracleSasContext
    return ZonalOracleSasContext
