"""Catchment totals of the offline transport model: the flux-weighted concentration of the percolate, sum(q_ss C_q_ss) / sum(q_ss), the
catchment's backward travel time distribution, sum(q_ss tt_q_ss(T)) / sum(q_ss), its storage by age, sum(sa_s(T)) -- a row per model
day over a masked area, on top of the SAS context's recorder (include/roger_hip_sas.h, rh_sas_totals_*; kernels in
roger_amd/csrc/rh_sas_totals.h).  The sibling of roger_amd/totals.py, which belongs to the SVAT / oneD step; it stands where the
reference has its `tracer_monitor` diagnostic.

A setup script fills `state.transport_totals` in `set_diagnostics`:

    state.transport_totals.mask = catchment                  # bool (nx, ny) over the GLOBAL interior; None: every column
    state.transport_totals.output_variables = [("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s"]   # value or (value, weight)
    state.transport_totals.base_output_path = ...            # as for the diagnostics
    state.transport_totals.capacity = 4096                   # rows resident on the device

and gets `<identifier>.transport_totals.nc`: dimensions Time (unlimited) and, where used, ages / nages; `Time` in days with
`time_origin`, `itt`, the scalar `ncells` (columns inside the mask) and per item -- named `<v>` or `<v>_by_<w>` -- `_sum`, `_count`,
`_wsum` (weighted items only) and `_mean` (`_sum / _wsum` when weighted, `_sum / _count` otherwise); per-cell variables add `_min` and
`_max`.  Per-cell items are (Time,), age-resolved ones (Time, ages | nages) with `_count` and `_wsum` (Time,).  A weight is one of the
daily flux inputs; a cell counts where it lies inside the mask and its weight is > 0 -- the per-cell concentrations are NaN wherever
the day's flux is zero, and NaN values are skipped (include/roger_hip_sas.h has the rules and the fixed order of the sums).

The life cycle is that of roger_amd/sas_points.py: nothing is recorded during the warm-up runs; once `warmup()` has set `warmup_done`
-- or `setup()` has read a restart file of a warmed-up run: a restarted run starts a new series -- the recorder is configured and
record 0 takes the initial values, in which no day's flux exists yet: weighted items and daily inputs count no cell there.  From then
on the day's launch itself is followed by the row's.  The ring is drained every `capacity` steps, before a restart file is written and
at the end of run().  With several ranks a rank records its own block and writes one file of its own (`.NNNN.nc`); a rank whose block
holds no masked column writes none; `combine` merges the ranks' files."""
import numpy as np

from . import runtime_settings as rs
from ._native import DAILY_INPUTS, totals_item_name
from .observers import (DAY, MAX_VARIABLES, RingSeries, check_mask, check_request, claim_output_file, combined_from, global_attributes, local_mask,
                        read_rank_files, time_variables, write_file)

_GRIDS = (("x", "y"), ("x", "y", "timesteps"), ("x", "y", "ages"), ("x", "y", "nages"), ("x", "y", "timesteps", "ages"))
_STATS = ("sum", "count", "wsum", "min", "max")


def keep_item_rows(t, rows):
    """Hold the rows {item: {stat: array}} a totals_read / zonal_read gave in t._values, item by item in the order of t._items; the
    bytes they take."""
    held_bytes = 0
    for (v, w), stats in zip(t._items, rows.values()):
        held = t._values[totals_item_name(v, w)]
        for s, a in stats.items():
            held.setdefault(s, []).append(a)
            held_bytes += a.nbytes
    return held_bytes


def held_rows(t):
    """(itt (n,), days (n,), [(name, weighted, {stat: array})]) of the rows held in t, as `_file_variables` takes them."""
    hdr = np.array(t._hdr[:t._read], dtype=np.int64).reshape(-1, 2)
    items = [(totals_item_name(v, w), w is not None, {s: np.concatenate(a) for s, a in t._values[totals_item_name(v, w)].items()})
             for v, w in t._items]
    return hdr[:, 0], hdr[:, 1] / float(DAY), items


class TransportTotals(RingSeries):
    """`state.transport_totals`: what the script sets (mask, output_variables, base_output_path, capacity) and the rows drained so far:
    {item: {stat: [arrays (n,) or (n, width)]}}."""

    label, attribute = "transport totals", "transport_totals"
    context, host_header = "sas_context", True

    def __init__(self):
        super().__init__()
        self.mask = None
        self.output_variables = []
        self.base_output_path = None
        self.output_path = "{identifier}.transport_totals.nc"
        self._items = []         # [(value, weight or None)] as the script's names
        self._ncells = 0         # masked columns of this rank
        self._values = {}

    @property
    def active(self):
        return bool(self.output_variables)

    def _count(self, ctx):
        return ctx.totals_count()[0]

    def _rows(self, ctx, first, n):
        return ctx.totals_read(first, n)

    def _keep(self, state, tags, rows):
        return keep_item_rows(self, rows)

    def _write(self, state):
        dims, variables = _file_variables(*held_rows(self), self._ncells, state.settings.time_origin, state.settings.ages)
        _write_file(self._path, dims, variables, state.settings.identifier)


def _items(output_variables, who="transport_totals"):
    out = []
    for it in output_variables:
        if isinstance(it, str):
            out.append((it, None))
        elif isinstance(it, (tuple, list)) and len(it) == 2 and all(isinstance(s, str) for s in it):
            out.append((it[0], it[1]))
        else:
            raise ValueError(f"{who}: {it!r} is neither a variable's name nor a pair (value, weight)")
    return out


def check_items(state, output_variables, capacity, who="transport_totals"):
    """[(value, weight or None)] of what a script asked for, or the refusal; `who` opens the messages (roger_amd/sas_zonal_totals.py
    asks with its own name)."""
    from .diagnostics import _AGED

    settings = state.settings
    items = _items(output_variables, who)
    if len(items) > MAX_VARIABLES:
        raise ValueError(f"{who}: {len(items)} items (at most {MAX_VARIABLES})")
    check_request(who, (), len(items), capacity, settings)   # (no cells to check: the capacity)
    if len(set(items)) != len(items):
        raise ValueError(f"{who}: an item is given twice")
    for v, w in items:
        meta = state.var_meta.get(v)
        if v in _AGED:
            raise NotImplementedError(f"{who}: {v!r} would be reduced after the ageing, the reference writes it before "
                                      "(use sa_s / msa_s)")
        if meta is not None and meta.dims is not None and tuple(meta.dims[:2]) == ("x", "y") and meta.sas is None:
            raise NotImplementedError(f"{who}: {v!r} exists on the host only (the setup script's hooks form it): "
                                      "not an array of the SAS context")
        if meta is None or meta.dims is None or tuple(meta.dims) not in _GRIDS or meta.dtype is not None:
            raise NotImplementedError(f"{who}: {v!r} is not a float64 per-cell variable of the transport step")
        if w is not None:
            wmeta = state.var_meta.get(w)
            if wmeta is None or wmeta.sas not in DAILY_INPUTS or wmeta.sas == "C_in":
                raise NotImplementedError(f"{who}: the weight {w!r} of {v!r} is not a daily flux input "
                                          f"({', '.join(d for d in DAILY_INPUTS if d != 'C_in')})")
    return items


def initialize(state):
    """setup(): validate what the script asked for.  The recorder itself starts with the run proper (start)."""
    t = state.transport_totals
    if not t.active:
        return
    settings = state.settings
    if not settings.enable_offline_transport:
        raise NotImplementedError("transport_totals: the totals of the offline transport model; the SVAT / oneD step records through state.totals")
    items = check_items(state, t.output_variables, t.capacity)
    check_mask("transport_totals", t.mask, settings)
    t._items = items


def start(state):
    """The run proper begins (warmup() is through, or a restart file of a warmed-up run was read): configure the recorder, take
    record 0 and write the file's first version.  Called again, it starts a new series."""
    from . import runtime_state

    t = state.transport_totals
    if not t.active or not state.settings.enable_offline_transport:
        return
    settings, vs = state.settings, state.variables
    mask = np.ones((settings.nx, settings.ny), dtype=bool) if t.mask is None else np.asarray(t.mask) != 0
    local = local_mask(mask, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ncells = int(local.sum())
    if not t._ncells:
        return   # (several ranks: no masked column in this rank's block)
    sas = state.sas_context
    vs.flush_to_device()
    sas.totals_configure([(state.var_meta[v].sas, None if w is None else state.var_meta[w].sas) for v, w in t._items],
                         None if local.all() else local, int(t.capacity))
    sas.totals_record(int(vs.itt), day=-1)   # (the initial values: no day's flux yet)
    t._begin()
    t._hdr = [(int(vs.itt), int(vs.time))]
    t._values = {totals_item_name(v, w): {} for v, w in t._items}
    t._path = claim_output_file(t, state, "transport totals")
    t.drain(state, final=True)


def _file_variables(hdr, days, items, ncells, time_origin, ages):
    """(dims, variables) of a totals file.  hdr (n,) itt; days (n,) float64; items [(name, weighted, {stat: array})]."""
    from .diagnostics import _UNITS

    dims = {"Time": None}
    variables = time_variables(hdr, days, time_origin)
    variables["ncells"] = ((), np.array(int(ncells), dtype=np.int64), {"long_name": "columns inside the mask", "units": ""})
    for name, weighted, stats in items:
        units = _UNITS.get(name.split("_by_")[0], "")
        total = np.asarray(stats["sum"], dtype=np.float64)
        extra = ()
        if total.ndim == 2:   # (Time, ages | nages)
            dim = "ages" if total.shape[1] == ages else "nages"
            dims.setdefault(dim, total.shape[1])
            extra = (dim,)
        over = "the masked columns" + (f" whose {name.split('_by_')[1]} is > 0" if weighted else "")
        for s in _STATS:
            if s not in stats or (s == "wsum" and not weighted):
                continue
            d = ("Time",) + (extra if s == "sum" else ())
            variables[f"{name}_{s}"] = (d, np.ascontiguousarray(stats[s], dtype=np.float64),
                                        {"long_name": f"{s} of {name} over {over}", "units": units if s not in ("count", "wsum") else ""})
        den = np.asarray(stats["wsum" if weighted else "count"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = total / (den[:, None] if total.ndim == 2 else den)
        variables[f"{name}_mean"] = (("Time",) + extra, np.ascontiguousarray(mean),
                                     {"long_name": f"mean of {name} over {over} ({name}_sum / {name}_{'wsum' if weighted else 'count'})",
                                      "units": units})
    return dims, variables


def _write_file(path, dims, variables, identifier, extra=None):
    write_file(path, dims, variables, global_attributes(
        identifier, "First record contains the initial values of the run proper, in which no day's flux exists yet. "
                    "Every further record is one day, Time at its end.", extra))


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: sums, wsums and counts added in rank order, minimum of the minima, maximum of
    the maxima, ncells added, means formed again.  Files whose itt or Time differ are refused."""
    paths, recs, names = read_rank_files("sas_totals", paths, ("itt", "Time"), what="items")
    first = recs[0]["variables"]
    items, ages = [], 0
    for name in names:
        stats = {}
        for s in _STATS:
            if f"{name}_{s}" not in first:
                continue
            cols = [np.asarray(rec["variables"][f"{name}_{s}"][1], dtype=np.float64) for rec in recs]
            if s == "min":
                stats[s] = np.fmin.reduce(cols)
            elif s == "max":
                stats[s] = np.fmax.reduce(cols)
            else:
                total = cols[0].copy()
                for c in cols[1:]:   # in rank order
                    total = total + c
                stats[s] = total
        if "ages" in first[f"{name}_sum"][0]:
            ages = stats["sum"].shape[1]
        items.append((name, "wsum" in stats, stats))
    ncells = sum(int(np.asarray(rec["variables"]["ncells"][1]).reshape(-1)[0]) for rec in recs)
    dims, variables = _file_variables(first["itt"][1], first["Time"][1], items, ncells, first["Time"][2].get("time_origin", ""), ages)
    _write_file(str(out), dims, variables, recs[0]["attributes"].get("setup_identifier", ""), combined_from(paths))
