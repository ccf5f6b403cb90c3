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
import datetime
import os

import numpy as np

from . import runtime_settings as rs
from .points import DAY, MAX_VARIABLES, WRITE_BYTES, check_request, claim_output_file, output_file_name
from .totals import STATS, TILE, _OPS, _tile_reduce, local_mask

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


class ZonalTotals:
    """`state.zonal_totals`: what the script sets (zones, output_variables, base_output_path, capacity) and the rows drained so far."""

    def __init__(self):
        self.zones = None
        self.output_variables = []
        self.base_output_path = None
        self.capacity = None
        self.output_path = "{identifier}.zonal_totals.nc"
        self._on = False         # initialize() configured the device (this rank holds at least one column of a zone)
        self._ids = np.zeros(0, dtype=np.int64)      # the zone ids as the script gave them, ascending (the GLOBAL list)
        self._ncells = np.zeros(0, dtype=np.int64)   # columns of every zone on this rank
        self._hdr = []           # drained headers, arrays (n, 3) int64: itt, time, dt_secs
        self._values = []        # drained rows, arrays (n, Z, V, 3) float64
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # host-loop steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.output_variables) and self.zones is not None

    def get_output_file_name(self, state):
        return output_file_name(self, state)


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
    if settings.enable_offline_transport:
        raise NotImplementedError("zonal totals: the offline transport model steps by the day and its output is read after every step "
                                  "(state.diagnostics); the recorder belongs to the SVAT / oneD step -- the transport model's own totals are "
                                  "state.transport_totals (roger_amd/sas_totals.py), per zone state.transport_zonal_totals "
                                  "(roger_amd/sas_zonal_totals.py)")
    if len(t.output_variables) > MAX_VARIABLES:
        raise ValueError(f"zonal totals: {len(t.output_variables)} variables (at most {MAX_VARIABLES})")
    zones = np.asarray(t.zones)
    if zones.shape != (settings.nx, settings.ny):
        raise ValueError(f"zonal totals: the zone map has shape {zones.shape}, the grid {settings.nx} x {settings.ny} columns")
    ids, index = zone_ids(zones)
    if not ids.size:
        raise ValueError("zonal totals: the zone map holds no column in any zone (no value > 0)")
    if ids.size > MAX_ZONES:
        raise ValueError(f"zonal totals: {ids.size} zones (at most {MAX_ZONES})")
    for v in t.output_variables:
        meta = state.var_meta.get(v)
        if meta is None or meta.plane is None or meta.dtype is not None:
            raise NotImplementedError(f"zonal totals: {v!r} is not a float64 (x, y) variable of the device arena")
    if t.capacity is None:
        t.capacity = default_capacity(ids.size, len(t.output_variables))
    check_request("zonal totals", (), len(t.output_variables), t.capacity, settings)   # (no cells to check: the capacity)
    local = local_mask(index, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ids = ids.astype(np.int64)
    t._ncells = np.bincount(local[local >= 0], minlength=ids.size).astype(np.int64)
    if not t._ncells.any():
        return   # (several ranks: no column of any zone in this rank's block)
    ctx = state.backend_context
    state.variables.flush_to_device()
    ctx.zonal_configure(list(t.output_variables), local, int(ids.size), int(t.capacity))
    t._on, t._read, t._steps, t._unwritten = True, 0, 0, 0
    vs = state.variables
    first = np.empty((1, ids.size, len(t.output_variables), 3))
    for j, v in enumerate(t.output_variables):
        a = np.asarray(getattr(vs, v))[2:-2, 2:-2]
        if a.ndim == 3:
            a = a[:, :, 1]
        first[0, :, j] = zone_totals(a, local, ids.size)
    t._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    t._values = [first]
    t._path = claim_output_file(t, state, "zonal totals")
    _write(state)


def check_call(state, nsteps):
    """Before a call that enqueues nsteps steps: more than the ring holds would overwrite rows nobody has read."""
    t = state.zonal_totals
    if t._on and int(nsteps) > int(t.capacity):
        raise RuntimeError(f"{int(nsteps)} steps in one call but only {int(t.capacity)} rows of the zonal totals are resident on the device: "
                           "call run_device() in shorter pieces, or raise state.zonal_totals.capacity")


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    t = state.zonal_totals
    if not t._on:
        return
    ctx = state.backend_context
    total = int(ctx.zonal_count()[0])
    n = total - t._read
    if n > int(t.capacity):
        raise RuntimeError(f"{n} rows of the zonal totals recorded since the last drain but only {int(t.capacity)} are resident on the device")
    if n > 0:
        hdr, values = ctx.zonal_read(t._read, n)
        t._hdr.append(hdr)
        t._values.append(values)
        t._read = total
        t._unwritten += values.nbytes + hdr.nbytes
    t._steps = 0
    if final or t._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """A host loop made one step call: drain when the calls since the last drain reach the capacity."""
    t = state.zonal_totals
    if not t._on:
        return
    t._steps += 1
    if t._steps >= int(t.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _file_variables(hdr, values, names, ids, ncells, time_origin):
    """The variables of a zonal totals file from headers (n, 3), values (n, Z, V, 3), the zone ids and the columns of every zone."""
    from .diagnostics import _UNITS

    ncells = np.asarray(ncells, dtype=np.int64)
    empty = ncells == 0
    variables = {
        "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time", "units": "days", "time_origin": str(time_origin)}),
        "zone": (("zone",), np.asarray(ids, dtype=np.int64), {"long_name": "zone id of the zone map", "units": ""}),
        "dt": (("Time",), hdr[:, 2].astype(np.float64), {"long_name": "length of the time step", "units": "s"}),
        "itt": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "time step", "units": ""}),
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
    from . import nc4lite

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    attributes = {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "First record (dt = 0) contains initial values. Every further record is one time step, Time at its end.",
        "setup_identifier": str(identifier)}
    attributes.update(extra or {})
    nc4lite.write(path, {"Time": None, "zone": int(len(variables["zone"][1]))}, variables, attributes)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    t = state.zonal_totals
    t._unwritten = 0
    if not t._path:
        return
    hdr, values = np.concatenate(t._hdr), np.concatenate(t._values)
    _write_file(t._path, _file_variables(hdr, values, t.output_variables, t._ids, t._ncells, state.settings.time_origin),
                state.settings.identifier)


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: per zone the sums added in rank order, the minimum of the minima, the maximum of
    the maxima (a rank without a column of the zone takes no part), ncells added, means formed again.  Files whose zone list, itt or Time
    differ are refused."""
    from . import nc4lite

    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("zonal_totals.combine: no files")
    recs = [nc4lite.read(p) for p in paths]
    first = recs[0]["variables"]
    names = [k[:-4] for k in first if k.endswith("_sum")]
    for p, rec in zip(paths[1:], recs[1:]):
        v = rec["variables"]
        if [k[:-4] for k in v if k.endswith("_sum")] != names:
            raise ValueError(f"zonal_totals.combine: {p} holds other variables than {paths[0]}")
        for key in ("zone", "itt", "Time", "dt"):
            if not np.array_equal(np.asarray(v[key][1]), np.asarray(first[key][1])):
                raise ValueError(f"zonal_totals.combine: {key} of {p} differs from {paths[0]}")
    hdr = np.stack([np.asarray(first["itt"][1], dtype=np.int64), np.zeros(len(first["itt"][1]), dtype=np.int64),
                    np.asarray(first["dt"][1]).astype(np.int64)], axis=1)
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
    variables = _file_variables(hdr, values, names, ids, np.sum(cells, axis=0), first["Time"][2].get("time_origin", ""))
    variables["Time"] = (("Time",), np.asarray(first["Time"][1], dtype=np.float64), variables["Time"][2])   # (the files' own days)
    _write_file(str(out), variables, recs[0]["attributes"].get("setup_identifier", ""), {"combined_from": ", ".join(os.path.basename(p) for p in paths)})
