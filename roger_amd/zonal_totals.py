"""Zonal totals: the sum, minimum, maximum and mean of output variables for EVERY zone of a zone map after every step -- per
sub-catchment (one gauge each), per land use, per soil class -- in one pass over the planes, on top of the device-side recorder
(include/roger_hip.h, rh_zonal_*; k_zonal_tiles, k_zonal_finish in roger_amd/csrc/rh_zonal.h).  `state.totals` (roger_amd/totals.py)
is the same for one masked area.

A setup script fills `state.zonal_totals` in `set_diagnostics`:

    state.zonal_totals.zones = subcatchment          # int (nx, ny) over the GLOBAL interior; values <= 0: outside every zone
    state.zonal_totals.output_variables = ["prec", "aet", "q_ss", "S"]
    state.zonal_totals.base_output_path = ...        # as for the diagnostics
    state.zonal_totals.capacity = 512                # rows resident on the device; None: as many as 64 MiB hold, at most 4096

and gets `<identifier>.zonal_totals.nc`: dimensions Time (unlimited) and zone; `zone` holds the distinct positive values of the map
in ascending order (the ids as the script gave them), `ncells(zone)` the columns of each, `Time`, `dt`, `itt` as in the totals' file,
and per variable `<v>_sum`, `<v>_min`, `<v>_max`, `<v>_mean = <v>_sum / ncells`, each (Time, zone) float64.  Record 0 holds the initial
values with dt = 0.

The sums of zone z are, bit for bit, what `state.totals` records with `mask = (zones == z)`: the order is the totals' (a tree over
each 64 columns, (w0 + w1) + (w2 + w3) over each 256, the 256-column partials strided over 256 accumulators and those through the same
two levels), and leaving out the partials of the tiles without a column of z changes no bit (roger_amd/csrc/rh_zonal.h).
`zone_totals` below is that rule in numpy; record 0 is computed with it, so the file has one rule.

The host drains the ring as it drains the totals'.  With several ranks a rank records its own block and writes one file of its own
(`.0000.nc`) over the GLOBAL zone list -- a zone without a column in the rank's block has ncells 0, sum 0 and `_FillValue` for minimum,
maximum and mean; a rank whose block holds no column of any zone writes none; `combine` merges the ranks' files.
Restart: a restarted run starts a new series."""
import numpy as np

from . import runtime_settings as rs, totals
from .observers import (DAY, MAX_VARIABLES, RingSeries, check_map_shape, check_planes, check_request, claim_output_file, combined_from,
                        interior_plane, local_mask, read_rank_files, svat_only, time_variables)
from .totals import STATS, TILE, _OPS, _tile_reduce

MAX_ZONES = 1024                  # include/roger_hip.h: RH_ZONAL_MAX_ZONES
RING_BYTES = 64 << 20             # what the default capacity keeps the device's ring under
FILL = 9.969209968386869e36       # netCDF's default _FillValue of a double


def zone_ids(zones):
    """(ids, index): the distinct positive values of a zone map in ascending order, and the map as indices into them (-1: outside)."""
    z = np.asarray(zones)
    if z.dtype.kind not in "iub":
        raise ValueError(f"zonal totals: the zone map holds {z.dtype} values (an integer id per column, <= 0: outside)")
    z = z.astype(np.int64)
    ids = np.unique(z[z > 0])
    index = np.where(z > 0, np.searchsorted(ids, z), -1).astype(np.int32)
    return ids, index


def zone_totals(values, zone, n_zones):
    """(n_zones, 3): sum, min, max of `values` over the columns of every zone (`zone`: an index per column, -1 outside), in the order of
    the device kernels -- for every zone z what totals.tree_totals(values, zone == z) gives, from the (tile, zone) pairs that exist."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    zi = np.asarray(zone).reshape(-1).astype(np.int64)
    assert zi.size == v.size
    n_zones = int(n_zones)
    col = np.flatnonzero(zi >= 0)
    pair, slot_of = np.unique((col // TILE) * n_zones + zi[col], return_inverse=True)   # ascending (tile, zone): the slots
    p_tile, p_zone = pair // n_zones, pair % n_zones
    p_acc = p_tile % TILE
    # the k-th partial accumulator (zone, t) takes, in increasing tile order
    order = np.lexsort((p_tile, p_acc, p_zone))
    group = p_zone[order] * TILE + p_acc[order]
    start = np.flatnonzero(np.r_[True, group[1:] != group[:-1]]) if group.size else np.zeros(0, dtype=np.int64)
    rank = np.empty(pair.size, dtype=np.int64)
    rank[order] = np.arange(pair.size) - np.repeat(start, np.diff(np.r_[start, pair.size]))
    out = np.empty((n_zones, 3))
    for k, (op, identity) in enumerate(_OPS):
        x = np.full((pair.size, TILE), identity)
        x[slot_of.reshape(-1), col % TILE] = v[col]
        partials = _tile_reduce(x.reshape(-1), op) if pair.size else np.zeros(0)
        acc = np.full((n_zones, TILE), identity)
        for r in range(int(rank.max()) + 1 if pair.size else 0):
            sel = rank == r
            acc[p_zone[sel], p_acc[sel]] = op(acc[p_zone[sel], p_acc[sel]], partials[sel])
        out[:, k] = _tile_reduce(acc.reshape(-1), op)
    return out


def check_zones(what, zones, settings):
    """(ids, index) of a script's zone map (zone_ids), or the refusal: of the grid's shape, with a zone, and not too many."""
    zones = np.asarray(zones)
    check_map_shape(what, "zone map", zones, settings)
    ids, index = zone_ids(zones)
    if not ids.size:
        raise ValueError(f"{what}: the zone map holds no column in any zone (no value > 0)")
    if ids.size > MAX_ZONES:
        raise ValueError(f"{what}: {ids.size} zones (at most {MAX_ZONES})")
    return ids, index


class ZonalTotals(RingSeries):
    """`state.zonal_totals`: what the script sets (zones, output_variables, base_output_path, capacity) and the rows drained so far:
    headers (n, 3) int64 itt, time, dt_secs and values (n, Z, V, 3) float64."""

    label, attribute = "zonal totals", "zonal_totals"

    def __init__(self):
        super().__init__()
        self.zones = None
        self.output_variables = []
        self.base_output_path = None
        self.capacity = None
        self.output_path = "{identifier}.zonal_totals.nc"
        self._ids = np.zeros(0, dtype=np.int64)      # the zone ids as the script gave them, ascending (the GLOBAL list)
        self._ncells = np.zeros(0, dtype=np.int64)   # columns of every zone on this rank

    @property
    def active(self):
        return bool(self.output_variables) and self.zones is not None

    def _count(self, ctx):
        return ctx.zonal_count()[0]

    def _rows(self, ctx, first, n):
        return ctx.zonal_read(first, n)

    def _write(self, state):
        hdr, values = np.concatenate(self._hdr), np.concatenate(self._values)
        _write_file(self._path, _file_variables(hdr, values, self.output_variables, self._ids, self._ncells, state.settings.time_origin),
                    state.settings.identifier)


def default_capacity(n_zones, n_variables):
    """Rows of (n_zones, n_variables, 3) float64 that RING_BYTES hold, at most 4096 and at least one."""
    return int(max(1, min(4096, RING_BYTES // (int(n_zones) * int(n_variables) * 3 * 8))))


def initialize(state):
    """Validate what the script asked for, configure the recorder and write record 0 (the initial values)."""
    from . import runtime_state

    t = state.zonal_totals
    if not t.active:
        return
    settings = state.settings
    svat_only("zonal totals", settings, " and its output is read after every step (state.diagnostics); the recorder belongs to the SVAT / oneD step "
              "-- the transport model's own totals are state.transport_totals (roger_amd/sas_totals.py), per zone "
              "state.transport_zonal_totals (roger_amd/sas_zonal_totals.py)")
    if len(t.output_variables) > MAX_VARIABLES:
        raise ValueError(f"zonal totals: {len(t.output_variables)} variables (at most {MAX_VARIABLES})")
    ids, index = check_zones("zonal totals", t.zones, settings)
    check_planes("zonal totals", t.output_variables, state)
    if t.capacity is None:
        t.capacity = default_capacity(ids.size, len(t.output_variables))
    check_request("zonal totals", (), len(t.output_variables), t.capacity, settings)   # (no cells to check: the capacity)
    local = local_mask(index, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ids = ids.astype(np.int64)
    t._ncells = np.bincount(local[local >= 0], minlength=ids.size).astype(np.int64)
    if not t._ncells.any():
        return   # (several ranks: no column of any zone in this rank's block)
    vs = state.variables
    vs.flush_to_device()
    state.backend_context.zonal_configure(list(t.output_variables), local, int(ids.size), int(t.capacity))
    t._begin()
    first = np.empty((1, ids.size, len(t.output_variables), 3))
    for j, v in enumerate(t.output_variables):
        first[0, :, j] = zone_totals(interior_plane(vs, v), local, ids.size)
    t._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    t._values = [first]
    t._path = claim_output_file(t, state, "zonal totals")
    t.write(state)


def close(state):
    state.zonal_totals.close(state)


def _file_variables(hdr, values, names, ids, ncells, time_origin, days=None):
    """The variables of a zonal totals file from headers (n, 3), values (n, Z, V, 3), the zone ids and the columns of every zone
    (`days`: the rows' Time where the headers do not hold it)."""
    from .diagnostics import _UNITS

    ncells = np.asarray(ncells, dtype=np.int64)
    empty = ncells == 0
    tv = time_variables(hdr[:, 0], hdr[:, 1] / float(DAY) if days is None else days, time_origin, dt=hdr[:, 2])
    variables = {
        "Time": tv["Time"],
        "zone": (("zone",), np.asarray(ids, dtype=np.int64), {"long_name": "zone id of the zone map", "units": ""}),
        "dt": tv["dt"],
        "itt": tv["itt"],
        "ncells": (("zone",), ncells, {"long_name": "columns of the zone", "units": ""}),
    }
    for j, name in enumerate(names):
        units = _UNITS.get(name, "")
        for k, stat in enumerate(STATS):
            a = np.ascontiguousarray(values[:, :, j, k])
            attrs = {"long_name": f"{stat} of {name} over the columns of the zone", "units": units}
            if k:
                a[:, empty] = FILL
                attrs["_FillValue"] = np.float64(FILL)
            variables[f"{name}_{stat}"] = (("Time", "zone"), a, attrs)
        mean = np.full(values.shape[:2], FILL)
        mean[:, ~empty] = values[:, ~empty, j, 0] / ncells[~empty].astype(np.float64)
        variables[f"{name}_mean"] = (("Time", "zone"), mean, {"long_name": f"mean of {name} over the columns of the zone ({name}_sum / ncells)",
                                                               "units": units, "_FillValue": np.float64(FILL)})
    return variables


def _write_file(path, variables, identifier, extra=None):
    totals._write_file(path, variables, identifier, extra, {"Time": None, "zone": int(len(variables["zone"][1]))})


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: per zone the sums added in rank order, the minimum of the minima, the maximum of
    the maxima (a rank without a column of the zone takes no part), ncells added, means formed again.  Files whose zone list, itt or Time
    differ are refused."""
    paths, recs, names = read_rank_files("zonal_totals", paths, ("zone", "itt", "Time", "dt"))
    first = recs[0]["variables"]
    hdr = totals.rank_headers(first)
    ids = np.asarray(first["zone"][1], dtype=np.int64)
    cells = [np.asarray(rec["variables"]["ncells"][1], dtype=np.int64) for rec in recs]
    values = np.empty((len(hdr), ids.size, len(names), 3))
    for j, name in enumerate(names):
        for k, (stat, (op, identity)) in enumerate(zip(STATS, _OPS)):
            total = np.full((len(hdr), ids.size), identity)
            for rec, c in zip(recs, cells):
                a = np.array(rec["variables"][f"{name}_{stat}"][1], dtype=np.float64)
                a[:, c == 0] = identity
                total = op(total, a)
            values[:, :, j, k] = total
    variables = _file_variables(hdr, values, names, ids, np.sum(cells, axis=0), first["Time"][2].get("time_origin", ""), days=first["Time"][1])
    _write_file(str(out), variables, recs[0]["attributes"].get("setup_identifier", ""), combined_from(paths))
