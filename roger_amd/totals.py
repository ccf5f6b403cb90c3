"""Catchment totals: the sum, minimum, maximum and mean of output variables over a masked area after every step -- the areal
precipitation, evapotranspiration, runoff and storage that are compared with a gauge and that close a water balance -- on top of the
device-side recorder (include/roger_hip.h, rh_totals_*; k_totals_tiles, k_totals_finish).  It stands where the reference has its
`water_monitor` diagnostic.

A setup script fills `state.totals` in `set_diagnostics`:

    state.totals.mask = catchment            # bool (nx, ny) over the GLOBAL interior; None: every column
    state.totals.output_variables = ["prec", "aet", "q_ss", "S"]
    state.totals.base_output_path = ...      # as for the diagnostics
    state.totals.capacity = 4096             # rows resident on the device

and gets `<identifier>.totals.nc`: dimension Time (unlimited); `Time` in days at the END of each step with `time_origin`, `dt` in
seconds, `itt`, the scalar `ncells` (columns inside the mask) and per variable `<v>_sum`, `<v>_min`, `<v>_max` and
`<v>_mean = <v>_sum / ncells`, each (Time,) float64.  Record 0 holds the initial values with dt = 0.

The sum has ONE fixed order (include/roger_hip.h): a tree over each 64 columns, (w0 + w1) + (w2 + w3) over each 256, the 256-column
partials strided over 256 accumulators and those through the same two levels.  `tree_totals` below is that order in numpy -- record 0
is computed with it, so the file has one rule.  The order follows the columns of a rank's block: totals of different decompositions
differ in the last bits.

The host drains the ring as it drains the points' (roger_amd/points.py).  With several ranks a rank records its own block and writes
one file of its own (`.0000.nc`); a rank whose block holds no masked column writes none; `combine` merges the ranks' files.
Restart: a restarted run starts a new series."""
import datetime
import os

import numpy as np

from . import runtime_settings as rs
from .points import DAY, MAX_VARIABLES, WRITE_BYTES, check_request, claim_output_file, output_file_name

TILE, WAVE = 256, 64
STATS = ("sum", "min", "max")
_OPS = ((np.add, 0.0), (np.fmin, np.inf), (np.fmax, -np.inf))


def _tile_reduce(x, op):
    """(tiles * 256,) -> (tiles,): the wavefront tree with strides 32 ... 1, then (w0 + w1) + (w2 + w3)."""
    x = x.reshape(-1, TILE // WAVE, WAVE)
    stride = WAVE // 2
    while stride:
        x = op(x[..., :stride], x[..., stride:2 * stride])
        stride //= 2
    w = x[..., 0]
    return op(op(w[:, 0], w[:, 1]), op(w[:, 2], w[:, 3]))


def tree_totals(values, mask=None):
    """(sum, min, max) of `values` over the columns where `mask` is set (None: all), in the order of the device kernels."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    inside = np.ones(v.size, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    ntiles = -(-v.size // TILE)
    out = []
    for op, identity in _OPS:
        x = np.full(ntiles * TILE, identity)
        x[:v.size] = np.where(inside, v, identity)
        partials = _tile_reduce(x, op)
        acc = np.full(TILE, identity)
        for k in range(0, ntiles, TILE):       # accumulator t: partials t, t + 256, ... in increasing order
            piece = partials[k:k + TILE]
            acc[:piece.size] = op(acc[:piece.size], piece)
        out.append(float(_tile_reduce(acc, op)[0]))
    return tuple(out)


def local_mask(mask, nx, ny, num_proc, rank):
    """The block of `rank` of a mask over the global interior, flat in C order over the block's (x, y).  Ranks x-fastest."""
    px, py = int(num_proc[0]), int(num_proc[1])
    nxl, nyl = int(nx) // px, int(ny) // py
    bx, by = rank % px, rank // px
    return np.ascontiguousarray(mask[bx * nxl:(bx + 1) * nxl, by * nyl:(by + 1) * nyl]).reshape(-1)


class AreaTotals:
    """`state.totals`: what the script sets (mask, output_variables, base_output_path, capacity) and the rows drained so far."""

    def __init__(self):
        self.mask = None
        self.output_variables = []
        self.base_output_path = None
        self.capacity = 4096
        self.output_path = "{identifier}.totals.nc"
        self._on = False         # initialize() configured the device (this rank holds at least one masked column)
        self._ncells = 0         # masked columns of this rank
        self._hdr = []           # drained headers, arrays (n, 3) int64: itt, time, dt_secs
        self._values = []        # drained rows, arrays (n, V, 3) float64
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # host-loop steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.output_variables)

    def get_output_file_name(self, state):
        return output_file_name(self, state)


def initialize(state):
    """Validate what the script asked for, configure the recorder and write record 0 (the initial values)."""
    from . import runtime_state

    t = state.totals
    if not t.active:
        return
    settings = state.settings
    if settings.enable_offline_transport:
        raise NotImplementedError("totals: the offline transport model steps by the day and its output is read after every step "
                                  "(state.diagnostics); the recorder belongs to the SVAT / oneD step -- the transport model's own totals are "
                                  "state.transport_totals (roger_amd/sas_totals.py)")
    if len(t.output_variables) > MAX_VARIABLES:
        raise ValueError(f"totals: {len(t.output_variables)} variables (at most {MAX_VARIABLES})")
    check_request("totals", (), len(t.output_variables), t.capacity, settings)   # (no cells to check: the capacity)
    for v in t.output_variables:
        meta = state.var_meta.get(v)
        if meta is None or meta.plane is None or meta.dtype is not None:
            raise NotImplementedError(f"totals: {v!r} is not a float64 (x, y) variable of the device arena")
    if t.mask is None:
        mask = np.ones((settings.nx, settings.ny), dtype=bool)
    else:
        mask = np.asarray(t.mask)
        if mask.shape != (settings.nx, settings.ny):
            raise ValueError(f"totals: the mask has shape {mask.shape}, the grid {settings.nx} x {settings.ny} columns")
        mask = mask != 0
    if not mask.any():
        raise ValueError("totals: the mask holds no column")
    local = local_mask(mask, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ncells = int(local.sum())
    if not t._ncells:
        return   # (several ranks: no masked column in this rank's block)
    ctx = state.backend_context
    state.variables.flush_to_device()
    ctx.totals_configure(list(t.output_variables), None if local.all() else local, int(t.capacity))
    t._on, t._read, t._steps, t._unwritten = True, 0, 0, 0
    vs = state.variables
    first = np.empty((1, len(t.output_variables), 3))
    for j, v in enumerate(t.output_variables):
        a = np.asarray(getattr(vs, v))[2:-2, 2:-2]
        if a.ndim == 3:
            a = a[:, :, 1]
        first[0, j] = tree_totals(a, local)
    t._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    t._values = [first]
    t._path = claim_output_file(t, state, "totals")
    _write(state)


def check_call(state, nsteps):
    """Before a call that enqueues nsteps steps: more than the ring holds would overwrite rows nobody has read."""
    t = state.totals
    if t._on and int(nsteps) > int(t.capacity):
        raise RuntimeError(f"{int(nsteps)} steps in one call but only {int(t.capacity)} rows of the totals are resident on the device: "
                           "call run_device() in shorter pieces, or raise state.totals.capacity")


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    t = state.totals
    if not t._on:
        return
    ctx = state.backend_context
    total = int(ctx.totals_count()[0])
    n = total - t._read
    if n > int(t.capacity):
        raise RuntimeError(f"{n} rows of the totals recorded since the last drain but only {int(t.capacity)} are resident on the device")
    if n > 0:
        hdr, values = ctx.totals_read(t._read, n)
        t._hdr.append(hdr)
        t._values.append(values)
        t._read = total
        t._unwritten += values.nbytes + hdr.nbytes
    t._steps = 0
    if final or t._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """A host loop made one step call: drain when the calls since the last drain reach the capacity."""
    t = state.totals
    if not t._on:
        return
    t._steps += 1
    if t._steps >= int(t.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _file_variables(hdr, values, names, ncells, time_origin):
    """The variables of a totals file from headers (n, 3), values (n, V, 3) and the number of masked columns."""
    from .diagnostics import _UNITS

    variables = {
        "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time", "units": "days", "time_origin": str(time_origin)}),
        "dt": (("Time",), hdr[:, 2].astype(np.float64), {"long_name": "length of the time step", "units": "s"}),
        "itt": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "time step", "units": ""}),
        "ncells": ((), np.array(int(ncells), dtype=np.int64), {"long_name": "columns inside the mask", "units": ""}),
    }
    for j, name in enumerate(names):
        units = _UNITS.get(name, "")
        for k, stat in enumerate(STATS):
            variables[f"{name}_{stat}"] = (("Time",), np.ascontiguousarray(values[:, j, k]),
                                           {"long_name": f"{stat} of {name} over the masked columns", "units": units})
        variables[f"{name}_mean"] = (("Time",), values[:, j, 0] / float(ncells),
                                     {"long_name": f"mean of {name} over the masked columns ({name}_sum / ncells)", "units": units})
    return variables


def _write_file(path, variables, identifier, extra=None):
    from . import nc4lite

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    attributes = {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "First record (dt = 0) contains initial values. Every further record is one time step, Time at its end.",
        "setup_identifier": str(identifier)}
    attributes.update(extra or {})
    nc4lite.write(path, {"Time": None}, variables, attributes)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    t = state.totals
    t._unwritten = 0
    if not t._path:
        return
    hdr, values = np.concatenate(t._hdr), np.concatenate(t._values)
    _write_file(t._path, _file_variables(hdr, values, t.output_variables, t._ncells, state.settings.time_origin), state.settings.identifier)


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: sums added in rank order, minimum of the minima, maximum of the maxima, ncells
    added, means formed again.  Files whose itt or Time differ are refused."""
    from . import nc4lite

    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("totals.combine: no files")
    recs = [nc4lite.read(p) for p in paths]
    first = recs[0]["variables"]
    names = [k[:-4] for k in first if k.endswith("_sum")]
    for p, rec in zip(paths[1:], recs[1:]):
        v = rec["variables"]
        if [k[:-4] for k in v if k.endswith("_sum")] != names:
            raise ValueError(f"totals.combine: {p} holds other variables than {paths[0]}")
        for key in ("itt", "Time", "dt"):
            if not np.array_equal(np.asarray(v[key][1]), np.asarray(first[key][1])):
                raise ValueError(f"totals.combine: {key} of {p} differs from {paths[0]}")
    hdr = np.stack([np.asarray(first["itt"][1], dtype=np.int64), np.zeros(len(first["itt"][1]), dtype=np.int64),
                    np.asarray(first["dt"][1]).astype(np.int64)], axis=1)
    values = np.empty((len(hdr), len(names), 3))
    for j, name in enumerate(names):
        cols = [[np.asarray(rec["variables"][f"{name}_{stat}"][1], dtype=np.float64) for rec in recs] for stat in STATS]
        total = cols[0][0].copy()
        for c in cols[0][1:]:
            total = total + c
        values[:, j, 0] = total
        values[:, j, 1] = np.fmin.reduce(cols[1])
        values[:, j, 2] = np.fmax.reduce(cols[2])
    ncells = sum(int(np.asarray(rec["variables"]["ncells"][1]).reshape(-1)[0]) for rec in recs)
    variables = _file_variables(hdr, values, names, ncells, first["Time"][2].get("time_origin", ""))
    variables["Time"] = (("Time",), np.asarray(first["Time"][1], dtype=np.float64), variables["Time"][2])   # (the files' own days)
    _write_file(str(out), variables, recs[0]["attributes"].get("setup_identifier", ""), {"combined_from": ", ".join(os.path.basename(p) for p in paths)})
