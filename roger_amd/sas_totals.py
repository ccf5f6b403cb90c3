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
import datetime
import os

import numpy as np

from . import runtime_settings as rs
from ._native import DAILY_INPUTS, totals_item_name
from .points import DAY, MAX_VARIABLES, WRITE_BYTES, check_request, claim_output_file, output_file_name
from .totals import local_mask

_GRIDS = (("x", "y"), ("x", "y", "timesteps"), ("x", "y", "ages"), ("x", "y", "nages"), ("x", "y", "timesteps", "ages"))
_STATS = ("sum", "count", "wsum", "min", "max")


class TransportTotals:
    """`state.transport_totals`: what the script sets (mask, output_variables, base_output_path, capacity) and the rows drained so far."""

    def __init__(self):
        self.mask = None
        self.output_variables = []
        self.base_output_path = None
        self.capacity = 4096
        self.output_path = "{identifier}.transport_totals.nc"
        self._on = False         # start() configured the device (this rank holds at least one masked column)
        self._items = []         # [(value, weight or None)] as the script's names
        self._ncells = 0         # masked columns of this rank
        self._hdr = []           # (itt, time) of every row: the drained ones, then the ones still on the device
        self._values = {}        # {item: {stat: [arrays (n,) or (n, width)]}} drained so far
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.output_variables)

    def get_output_file_name(self, state):
        return output_file_name(self, state)


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
    if t.mask is not None:
        mask = np.asarray(t.mask)
        if mask.shape != (settings.nx, settings.ny):
            raise ValueError(f"transport_totals: the mask has shape {mask.shape}, the grid {settings.nx} x {settings.ny} columns")
        if not (mask != 0).any():
            raise ValueError("transport_totals: the mask holds no column")
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
    t._on, t._read, t._steps, t._unwritten = True, 0, 0, 0
    t._hdr = [(int(vs.itt), int(vs.time))]
    t._values = {totals_item_name(v, w): {} for v, w in t._items}
    t._path = claim_output_file(t, state, "transport totals")
    drain(state, final=True)


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    t = state.transport_totals
    if not t._on:
        return
    sas = state.sas_context
    total = int(sas.totals_count()[0])
    n = total - t._read
    if n > int(t.capacity) or total != len(t._hdr):
        raise RuntimeError(f"{n} rows of the transport totals recorded since the last drain ({total} in all, {len(t._hdr)} steps known "
                           f"to the host) but only {int(t.capacity)} are resident on the device")
    if n > 0:
        _, rows = sas.totals_read(t._read, n)
        for (v, w), stats in zip(t._items, rows.values()):
            held = t._values[totals_item_name(v, w)]
            for s, a in stats.items():
                held.setdefault(s, []).append(a)
                t._unwritten += a.nbytes
        t._read = total
    t._steps = 0
    if final or t._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """_step_offline_transport made a step (rh_sas_step recorded its row): note its itt and time, drain when the steps since the last
    drain reach the capacity."""
    t = state.transport_totals
    if not t._on:
        return
    vs = state.variables
    t._hdr.append((int(vs.itt), int(vs.time)))
    t._steps += 1
    if t._steps >= int(t.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _file_variables(hdr, days, items, ncells, time_origin, ages):
    """(dims, variables) of a totals file.  hdr (n,) itt; days (n,) float64; items [(name, weighted, {stat: array})]."""
    from .diagnostics import _UNITS

    dims = {"Time": None}
    variables = {
        "Time": (("Time",), np.asarray(days, dtype=np.float64), {"long_name": "Time", "units": "days", "time_origin": str(time_origin)}),
        "itt": (("Time",), np.asarray(hdr, dtype=np.int64), {"long_name": "time step", "units": ""}),
        "ncells": ((), np.array(int(ncells), dtype=np.int64), {"long_name": "columns inside the mask", "units": ""}),
    }
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
    from . import nc4lite

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    attributes = {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "First record contains the initial values of the run proper, in which no day's flux exists yet. "
                   "Every further record is one day, Time at its end.",
        "setup_identifier": str(identifier)}
    attributes.update(extra or {})
    nc4lite.write(path, dims, variables, attributes)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    t = state.transport_totals
    t._unwritten = 0
    if not t._path:
        return
    settings = state.settings
    hdr = np.array(t._hdr[:t._read], dtype=np.int64).reshape(-1, 2)
    items = [(totals_item_name(v, w), w is not None, {s: np.concatenate(a) for s, a in t._values[totals_item_name(v, w)].items()})
             for v, w in t._items]
    dims, variables = _file_variables(hdr[:, 0], hdr[:, 1] / float(DAY), items, t._ncells, settings.time_origin, settings.ages)
    _write_file(t._path, dims, variables, settings.identifier)


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: sums, wsums and counts added in rank order, minimum of the minima, maximum of
    the maxima, ncells added, means formed again.  Files whose itt or Time differ are refused."""
    from . import nc4lite

    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("sas_totals.combine: no files")
    recs = [nc4lite.read(p) for p in paths]
    first = recs[0]["variables"]
    names = [k[:-4] for k in first if k.endswith("_sum")]
    for p, rec in zip(paths[1:], recs[1:]):
        v = rec["variables"]
        if [k[:-4] for k in v if k.endswith("_sum")] != names:
            raise ValueError(f"sas_totals.combine: {p} holds other items than {paths[0]}")
        for key in ("itt", "Time"):
            if not np.array_equal(np.asarray(v[key][1]), np.asarray(first[key][1])):
                raise ValueError(f"sas_totals.combine: {key} of {p} differs from {paths[0]}")
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
    _write_file(str(out), dims, variables, recs[0]["attributes"].get("setup_identifier", ""),
                {"combined_from": ", ".join(os.path.basename(p) for p in paths)})
