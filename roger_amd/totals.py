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
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, MAX_VARIABLES, RingSeries, check_mask, check_planes, check_request, claim_output_file, combined_from,  # noqa: F401
                        global_attributes, interior_plane, local_mask, read_rank_files, svat_only, time_variables, write_file)

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


class AreaTotals(RingSeries):
    """`state.totals`: what the script sets (mask, output_variables, base_output_path, capacity) and the rows drained so far:
    headers (n, 3) int64 itt, time, dt_secs and values (n, V, 3) float64."""

    label = attribute = "totals"

    def __init__(self):
        super().__init__()
        self.mask = None
        self.output_variables = []
        self.base_output_path = None
        self.output_path = "{identifier}.totals.nc"
        self._ncells = 0         # masked columns of this rank

    @property
    def active(self):
        return bool(self.output_variables)

    def _count(self, ctx):
        return ctx.totals_count()[0]

    def _rows(self, ctx, first, n):
        return ctx.totals_read(first, n)

    def _write(self, state):
        hdr, values = np.concatenate(self._hdr), np.concatenate(self._values)
        _write_file(self._path, _file_variables(hdr, values, self.output_variables, self._ncells, state.settings.time_origin), state.settings.identifier)


def initialize(state):
    """Validate what the script asked for, configure the recorder and write record 0 (the initial values)."""
    from . import runtime_state

    t = state.totals
    if not t.active:
        return
    settings = state.settings
    svat_only("totals", settings, " and its output is read after every step (state.diagnostics); the recorder belongs to the SVAT / oneD step "
              "-- the transport model's own totals are state.transport_totals (roger_amd/sas_totals.py)")
    if len(t.output_variables) > MAX_VARIABLES:
        raise ValueError(f"totals: {len(t.output_variables)} variables (at most {MAX_VARIABLES})")
    check_request("totals", (), len(t.output_variables), t.capacity, settings)   # (no cells to check: the capacity)
    check_planes("totals", t.output_variables, state)
    mask = np.ones((settings.nx, settings.ny), dtype=bool) if t.mask is None else check_mask("totals", t.mask, settings)
    local = local_mask(mask, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    t._ncells = int(local.sum())
    if not t._ncells:
        return   # (several ranks: no masked column in this rank's block)
    vs = state.variables
    vs.flush_to_device()
    state.backend_context.totals_configure(list(t.output_variables), None if local.all() else local, int(t.capacity))
    t._begin()
    first = np.empty((1, len(t.output_variables), 3))
    for j, v in enumerate(t.output_variables):
        first[0, j] = tree_totals(interior_plane(vs, v), local)
    t._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    t._values = [first]
    t._path = claim_output_file(t, state, "totals")
    t.write(state)


def close(state):
    state.totals.close(state)


def _file_variables(hdr, values, names, ncells, time_origin, days=None):
    """The variables of a totals file from headers (n, 3), values (n, V, 3) and the number of masked columns (`days`: the rows' Time
    where the headers do not hold it)."""
    from .diagnostics import _UNITS

    variables = time_variables(hdr[:, 0], hdr[:, 1] / float(DAY) if days is None else days, time_origin, dt=hdr[:, 2])
    variables["ncells"] = ((), np.array(int(ncells), dtype=np.int64), {"long_name": "columns inside the mask", "units": ""})
    for j, name in enumerate(names):
        units = _UNITS.get(name, "")
        for k, stat in enumerate(STATS):
            variables[f"{name}_{stat}"] = (("Time",), np.ascontiguousarray(values[:, j, k]),
                                           {"long_name": f"{stat} of {name} over the masked columns", "units": units})
        variables[f"{name}_mean"] = (("Time",), values[:, j, 0] / float(ncells),
                                     {"long_name": f"mean of {name} over the masked columns ({name}_sum / ncells)", "units": units})
    return variables


def _write_file(path, variables, identifier, extra=None, dims=None):
    write_file(path, dims or {"Time": None}, variables, global_attributes(
        identifier, "First record (dt = 0) contains initial values. Every further record is one time step, Time at its end.", extra))


def rank_headers(first):
    """The headers (n, 3) of the rows of a rank's file (its variables `first`); the time is left to the file's own days."""
    itt = np.asarray(first["itt"][1], dtype=np.int64)
    return np.stack([itt, np.zeros(len(itt), dtype=np.int64), np.asarray(first["dt"][1]).astype(np.int64)], axis=1)


def combine(paths, out):
    """The ranks' files `paths` (in rank order) as one: sums added in rank order, minimum of the minima, maximum of the maxima, ncells
    added, means formed again.  Files whose itt or Time differ are refused."""
    paths, recs, names = read_rank_files("totals", paths, ("itt", "Time", "dt"))
    first = recs[0]["variables"]
    hdr = rank_headers(first)
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
    variables = _file_variables(hdr, values, names, ncells, first["Time"][2].get("time_origin", ""), days=first["Time"][1])
    _write_file(str(out), variables, recs[0]["attributes"].get("setup_identifier", ""), combined_from(paths))
