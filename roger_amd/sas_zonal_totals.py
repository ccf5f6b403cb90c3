"""Zonal totals of the offline transport model: what `state.transport_totals` (roger_amd/sas_totals.py) records over one masked area --
the flux-weighted concentration of the percolate, the backward travel time distribution, the storage by age -- for EVERY zone of a
zone map (sub-catchments with a gauge and an isotope series each, land uses, soil classes), a row per model day, in one pass that
loads each row of an age-resolved array once (include/roger_hip_sas.h, rh_sas_zonal_*; kernels in roger_amd/csrc/rh_sas_zonal.h).
The sibling of roger_amd/zonal_totals.py, which belongs to the SVAT / oneD step.

A setup script fills `state.transport_zonal_totals` in `set_diagnostics`:

    state.transport_zonal_totals.zones = subcatchment        # int (nx, ny) over the GLOBAL interior; values <= 0: outside every zone
    state.transport_zonal_totals.output_variables = [("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s"]   # value or (value, weight)
    state.transport_zonal_totals.base_output_path = ...      # as for the diagnostics
    state.transport_zonal_totals.capacity = 512              # rows resident on the device; None: as many as 64 MiB hold, at most 4096

and gets `<identifier>.transport_zonal_totals.nc`: dimensions Time (unlimited), zone and, where used, ages / nages; `zone` holds the
distinct positive values of the map in ascending order (the ids as the script gave them), `ncells(zone)` the columns of each, `Time`
and `itt` as in the totals' file, and per item -- named `<v>` or `<v>_by_<w>` -- `_sum` (Time, zone[, ages | nages]), `_count` (Time,
zone), `_wsum` (Time, zone; weighted items only), `_mean` (`_sum / _wsum` when weighted, `_sum / _count` otherwise) and, for per-cell
variables, `_min` and `_max` (Time, zone).  Where nothing was counted, minimum, maximum and mean hold `_FillValue`.

Block (zone z, item) of a row is, bit for bit, what `state.transport_totals` records with `mask = (zones == z)`; the rules -- which
cells count, NaN, the fixed order of the sums -- are in include/roger_hip_sas.h.

The life cycle is that of roger_amd/sas_totals.py: nothing is recorded during the warm-up runs; record 0 takes the initial values of
the run proper, in which no day's flux exists yet; from then on the day's launch itself is followed by the row's.  The ring is drained
every `capacity` steps, before a restart file is written and at the end of run(); a restarted run starts a new series.  With several
ranks a rank records its own block and writes one file of its own (`.NNNN.nc`) over the GLOBAL zone list; a rank whose block holds no
column of any zone writes none; `combine` merges the ranks' files."""
import numpy as np

from . import runtime_settings as rs
from ._native import totals_item_name
from .observers import RingSeries, claim_output_file, combined_from, local_mask, read_rank_files, time_variables
from .sas_totals import _STATS, _write_file, check_items, held_rows, keep_item_rows
from .zonal_totals import FILL, RING_BYTES, check_zones

WHO = "transport_zonal_totals"


class TransportZonalTotals(RingSeries):
    """`state.transport_zonal_totals`: what the script sets (zones, output_variables, base_output_path, capacity) and the rows drained
    so far: {item: {stat: [arrays (n, Z) or (n, Z, width)]}}."""

    label, attribute = "transport zonal totals", WHO
    context, host_header = "sas_context", True

    def __init__(self):
        super().__init__()
        self.zones = None
        self.output_variables = []
        self.base_output_path = None
        self.capacity = None
        self.output_path = "{identifier}.transport_zonal_totals.nc"
        self._items = []         # [(value, weight or None)] as the script's names
        self._ids = np.zeros(0, dtype=np.int64)      # the zone ids as the script gave them, ascending (the GLOBAL list)
        self._index = None       # the map as indices into them over the GLOBAL interior (-1: outside)
        self._ncells = np.zeros(0, dtype=np.int64)   # columns of every zone on this rank
        self._values = {}

    @property
    def active(self):
        return bool(self.output_variables) and self.zones is not None

    def _count(self, ctx):
        return ctx.zonal_count()[0]

    def _rows(self, ctx, first, n):
        return ctx.zonal_read(first, n)

    def _keep(self, state, tags, rows):
        return keep_item_rows(self, rows)

    def _write(self, state):
        dims, variables = _file_variables(*held_rows(self), self._ids, self._ncells, state.settings.time_origin, state.settings.ages)
        _write_file(self._path, dims, variables, state.settings.identifier)


def default_capacity(n_zones, zone_elems):
    """Rows of n_zones x zone_elems float64 that RING_BYTES hold, at most 4096 and at least one."""
    return int(max(1, min(4096, RING_BYTES // (int(n_zones) * int(zone_elems) * 8))))


def initialize(state):
    """setup(): validate what the script asked for.  The recorder itself starts with the run proper (start)."""
    t = state.transport_zonal_totals
    if not t.active:
        return
    settings = state.settings
    if not settings.enable_offline_transport:
        raise NotImplementedError(f"{WHO}: the zonal totals of the offline transport model; the SVAT / oneD step records through "
                                  "state.zonal_totals")
    items = check_items(state, t.output_variables, 1 if t.capacity is None else t.capacity, WHO)
    ids, index = check_zones(WHO, t.zones, settings)
    if t.capacity is None:
        width = {"ages": settings.ages, "nages": settings.ages + 1}
        elems = sum(next((2 + width[d] for d in state.var_meta[v].dims if d in width), 5) for v, _ in items)
        t.capacity = default_capacity(ids.size, elems)
    t._items, t._ids, t._index = items, ids.astype(np.int64), index


def start(state):
    """The run proper begins (warmup() is through, or a restart file of a warmed-up run was read): configure the recorder, take
    record 0 and write the file's first version.  Called again, it starts a new series."""
    from . import runtime_state

    t = state.transport_zonal_totals
    if not t.active or not state.settings.enable_offline_transport:
        return
    settings, vs = state.settings, state.variables
    local = local_mask(t._index, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ncells = np.bincount(local[local >= 0], minlength=t._ids.size).astype(np.int64)
    if not t._ncells.any():
        return   # (several ranks: no column of any zone in this rank's block)
    sas = state.sas_context
    vs.flush_to_device()
    sas.zonal_configure([(state.var_meta[v].sas, None if w is None else state.var_meta[w].sas) for v, w in t._items],
                        local, int(t._ids.size), int(t.capacity))
    sas.zonal_record(int(vs.itt), day=-1)   # (the initial values: no day's flux yet)
    t._begin()
    t._hdr = [(int(vs.itt), int(vs.time))]
    t._values = {totals_item_name(v, w): {} for v, w in t._items}
    t._path = claim_output_file(t, state, "transport zonal totals")
    t.drain(state, final=True)


def _file_variables(hdr, days, items, ids, ncells, time_origin, ages):
    """(dims, variables) of a zonal file.  hdr (n,) itt; days (n,) float64; items [(name, weighted, {stat: array (n, Z[, width])})]."""
    from .diagnostics import _UNITS

    dims = {"Time": None, "zone": int(len(ids))}
    tv = time_variables(hdr, days, time_origin)
    variables = {
        "Time": tv["Time"],
        "zone": (("zone",), np.asarray(ids, dtype=np.int64), {"long_name": "zone id of the zone map", "units": ""}),
        "itt": tv["itt"],
        "ncells": (("zone",), np.asarray(ncells, dtype=np.int64), {"long_name": "columns of the zone", "units": ""}),
    }
    for name, weighted, stats in items:
        units = _UNITS.get(name.split("_by_")[0], "")
        total = np.asarray(stats["sum"], dtype=np.float64)
        extra = ()
        if total.ndim == 3:   # (Time, zone, ages | nages)
            dim = "ages" if total.shape[2] == ages else "nages"
            dims.setdefault(dim, total.shape[2])
            extra = (dim,)
        over = "the columns of the zone" + (f" whose {name.split('_by_')[1]} is > 0" if weighted else "")
        none = np.asarray(stats["count"], dtype=np.float64) == 0       # (Time, zone): nothing was counted
        for s in _STATS:
            if s not in stats or (s == "wsum" and not weighted):
                continue
            a = np.array(stats[s], dtype=np.float64)
            attrs = {"long_name": f"{s} of {name} over {over}", "units": units if s not in ("count", "wsum") else ""}
            if s in ("min", "max"):
                a[none] = FILL
                attrs["_FillValue"] = np.float64(FILL)
            variables[f"{name}_{s}"] = (("Time", "zone") + (extra if s == "sum" else ()), np.ascontiguousarray(a), attrs)
        den = np.asarray(stats["wsum" if weighted else "count"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = total / (den[:, :, None] if total.ndim == 3 else den)
        mean[none] = FILL
        variables[f"{name}_mean"] = (("Time", "zone") + extra, np.ascontiguousarray(mean),
                                     {"long_name": f"mean of {name} over {over} ({name}_sum / {name}_{'wsum' if weighted else 'count'})",
                                      "units": units, "_FillValue": np.float64(FILL)})
    return dims, variables


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: per zone the sums, wsums and counts added in rank order, the minimum of the
    minima, the maximum of the maxima (a rank that counted nothing in the zone takes no part), ncells added, means formed again.  Files
    whose zone list, itt or Time differ are refused."""
    paths, recs, names = read_rank_files("sas_zonal_totals", paths, ("zone", "itt", "Time"), what="items")
    first = recs[0]["variables"]
    items, ages = [], 0
    for name in names:
        stats = {}
        counts = [np.asarray(rec["variables"][f"{name}_count"][1], dtype=np.float64) for rec in recs]
        for s in _STATS:
            if f"{name}_{s}" not in first:
                continue
            cols = [np.array(rec["variables"][f"{name}_{s}"][1], dtype=np.float64) for rec in recs]
            if s in ("min", "max"):
                for a, c in zip(cols, counts):
                    a[c == 0] = np.inf if s == "min" else -np.inf
                stats[s] = (np.fmin if s == "min" else np.fmax).reduce(cols)
            else:
                total = cols[0].copy()
                for c in cols[1:]:   # in rank order
                    total = total + c
                stats[s] = total
        if "ages" in first[f"{name}_sum"][0]:
            ages = stats["sum"].shape[2]
        items.append((name, "wsum" in stats, stats))
    ncells = np.sum([np.asarray(rec["variables"]["ncells"][1], dtype=np.int64) for rec in recs], axis=0)
    dims, variables = _file_variables(first["itt"][1], first["Time"][1], items, first["zone"][1], ncells,
                                      first["Time"][2].get("time_origin", ""), ages)
    _write_file(str(out), dims, variables, recs[0]["attributes"].get("setup_identifier", ""), combined_from(paths))
