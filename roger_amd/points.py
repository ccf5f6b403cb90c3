"""Time series at observation columns ("points"): a handful of columns -- a lysimeter, a soil-moisture profile, a snow pillow, the
cell above a gauge -- written at the model's own time resolution, on top of the device-side recorder (include/roger_hip.h,
rh_points_*; k_points).

A setup script fills `state.points` in `set_diagnostics`:

    state.points.cells = [(ix, iy), ...]          # interior indices of the GLOBAL grid, 0-based
    state.points.output_variables = ["theta_rz", "q_ss", "swe"]
    state.points.base_output_path = ...           # as for the diagnostics
    state.points.capacity = 4096                  # rows resident on the device

and gets `<identifier>.points.nc`: dimensions Time (unlimited) and point; `Time` in days at the END of each step with
`time_origin`, `dt` in seconds, `itt`, per point `ix`, `iy` (global) and `x`, `y` in m, every variable (Time, point) float64.  Record
0 holds the initial values with dt = 0, as the diagnostics' files do.  The device records one row after every step into a ring of
`capacity` rows; the host drains the ring before it can wrap (RogerSetup: after every round of device steps, every `capacity`
steps of the host loops, at the end of run() and before a restart file is written), so no row is lost.  With several ranks a rank
records the points inside its block and writes one file of its own, named like the diagnostics' (`.0000.nc`); a rank whose block
holds no point writes none.  Restart: a restarted run starts a new series."""
import datetime
import os

import numpy as np

from . import runtime_settings as rs

DAY = 24 * 60 * 60
MAX_CELLS, MAX_VARIABLES = 256, 32     # include/roger_hip.h: rh_points_configure
WRITE_BYTES = 32 << 20                 # rows drained since the last write beyond which the file is written (as diagnostics.output)


def local_cells(cells, nx, ny, num_proc, rank):
    """[(k, local cell)] for the points k of `cells` (global interior (ix, iy)) that lie in the block of `rank`: the local cell is
    the index rh_upload / rh_download use, C order over the rank's (x, y) interior.  Ranks x-fastest (distributed.proc_rank_to_index)."""
    px, py = int(num_proc[0]), int(num_proc[1])
    nxl, nyl = int(nx) // px, int(ny) // py
    bx, by = rank % px, rank // px
    out = []
    for k, (ix, iy) in enumerate(cells):
        if ix // nxl == bx and iy // nyl == by:
            out.append((k, (ix - bx * nxl) * nyl + (iy - by * nyl)))
    return out


def check_request(what, cells, n_variables, capacity, settings):
    """What `state.points` and `state.transport_points` (roger_amd/sas_points.py) check alike -- the cells lie in the grid, none is
    given twice, the counts are within the recorder's limits, the ring holds a row: the cells as tuples of ints."""
    cells = [(int(c[0]), int(c[1])) for c in cells]
    for ix, iy in cells:
        if not (0 <= ix < settings.nx and 0 <= iy < settings.ny):
            raise ValueError(f"{what}: cell ({ix}, {iy}) is outside the grid of {settings.nx} x {settings.ny} columns")
    if len(set(cells)) != len(cells):
        twice = sorted({c for c in cells if cells.count(c) > 1})
        raise ValueError(f"{what}: cell {twice[0]} is given twice")
    if len(cells) > MAX_CELLS or n_variables > MAX_VARIABLES:
        raise ValueError(f"{what}: {len(cells)} cells x {n_variables} variables (at most {MAX_CELLS} x {MAX_VARIABLES})")
    if int(capacity) < 1:
        raise ValueError(f"{what}: capacity = {capacity} (at least one row resident on the device)")
    return cells


def output_file_name(series, state):
    """The file of a series (`output_path`, `base_output_path`): one per rank, named like the diagnostics', with several ranks."""
    from . import runtime_state

    name = series.output_path.format(identifier=state.settings.identifier)
    if runtime_state.proc_num > 1:
        name = name[:-3] + f".{runtime_state.proc_rank:04d}.nc"
    return os.path.join(series.base_output_path, name) if series.base_output_path else name


def claim_output_file(series, state, what):
    """The path the series writes to (None in diskless mode); a file that is already there is not overwritten unasked."""
    path = None if rs.diskless_mode else output_file_name(series, state)
    if path and os.path.isfile(path) and not getattr(rs, "force_overwrite", False):
        raise IOError(f"output file {path} for the {what} exists (change the output path, enable the force_overwrite runtime "
                      "setting or delete it)")
    return path


def point_coordinates(state, cells, local):
    """ix, iy (global), x, y of the points [(k, local cell)] of this rank, as the variables of the file."""
    vs, settings = state.variables, state.settings
    nyl = settings.ny // rs.num_proc[1]
    x, y = np.asarray(vs.x)[2:-2], np.asarray(vs.y)[2:-2]
    pts = [cells[k] for k, _ in local]
    return {
        "ix": (("point",), np.array([c[0] for c in pts], dtype=np.int64), {"long_name": "global interior x index", "units": ""}),
        "iy": (("point",), np.array([c[1] for c in pts], dtype=np.int64), {"long_name": "global interior y index", "units": ""}),
        "x": (("point",), np.array([x[c // nyl] for _, c in local], dtype=np.float64), {"long_name": "x", "units": "m"}),
        "y": (("point",), np.array([y[c % nyl] for _, c in local], dtype=np.float64), {"long_name": "y", "units": "m"}),
    }


class PointSeries:
    """`state.points`: what the script sets (cells, output_variables, base_output_path, capacity) and the rows drained so far."""

    def __init__(self):
        self.cells = []
        self.output_variables = []
        self.base_output_path = None
        self.capacity = 4096
        self.output_path = "{identifier}.points.nc"
        self._on = False         # initialize() configured the device (this rank holds at least one point)
        self._local = []         # [(k, local cell)] of this rank
        self._hdr = []           # drained headers, arrays (n, 3) int64: itt, time, dt_secs
        self._values = []        # drained rows, arrays (n, V, K) float64
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # host-loop steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.cells) and bool(self.output_variables)

    def get_output_file_name(self, state):
        return output_file_name(self, state)


def initialize(state):
    """Validate what the script asked for, configure the recorder and write record 0 (the initial values)."""
    from . import runtime_state

    p = state.points
    if not p.active:
        return
    settings = state.settings
    if settings.enable_offline_transport:
        raise NotImplementedError("points: the offline transport model steps by the day and its output is read after every step "
                                  "(state.diagnostics); the recorder belongs to the SVAT / oneD step")
    cells = check_request("points", p.cells, len(p.output_variables), p.capacity, settings)
    for v in p.output_variables:
        meta = state.var_meta.get(v)
        if meta is None or meta.plane is None or meta.dtype is not None:
            raise NotImplementedError(f"points: {v!r} is not a float64 (x, y) variable of the device arena")
    p.cells = cells
    p._local = local_cells(cells, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    if not p._local:
        return   # (several ranks: no point in this rank's block)
    ctx = state.backend_context
    state.variables.flush_to_device()
    ctx.points_configure([c for _, c in p._local], list(p.output_variables), int(p.capacity))
    p._on, p._read, p._steps, p._unwritten = True, 0, 0, 0
    vs = state.variables
    nyl = settings.ny // rs.num_proc[1]
    first = np.empty((1, len(p.output_variables), len(p._local)))
    for j, v in enumerate(p.output_variables):
        a = np.asarray(getattr(vs, v))[2:-2, 2:-2]
        if a.ndim == 3:
            a = a[:, :, 1]
        first[0, j] = [a[c // nyl, c % nyl] for _, c in p._local]
    p._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    p._values = [first]
    p._path = claim_output_file(p, state, "points")
    _write(state)


def check_call(state, nsteps):
    """Before a call that enqueues nsteps steps: more than the ring holds would overwrite rows nobody has read."""
    p = state.points
    if p._on and int(nsteps) > int(p.capacity):
        raise RuntimeError(f"{int(nsteps)} steps in one call but only {int(p.capacity)} rows of the points are resident on the device: "
                           "call run_device() in shorter pieces, or raise state.points.capacity")


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    p = state.points
    if not p._on:
        return
    ctx = state.backend_context
    total = int(ctx.points_count())
    n = total - p._read
    if n > int(p.capacity):
        raise RuntimeError(f"{n} rows of the points recorded since the last drain but only {int(p.capacity)} are resident on the device")
    if n > 0:
        hdr, values = ctx.points_read(p._read, n)
        p._hdr.append(hdr)
        p._values.append(values)
        p._read = total
        p._unwritten += values.nbytes + hdr.nbytes
    p._steps = 0
    if final or p._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """A host loop made one step call: drain when the calls since the last drain reach the capacity."""
    p = state.points
    if not p._on:
        return
    p._steps += 1
    if p._steps >= int(p.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    p = state.points
    p._unwritten = 0
    if not p._path:
        return
    from . import nc4lite

    vs, settings = state.variables, state.settings
    os.makedirs(os.path.dirname(os.path.abspath(p._path)), exist_ok=True)
    hdr, values = np.concatenate(p._hdr), np.concatenate(p._values)
    dims = {"Time": None, "point": len(p._local)}
    variables = {
        "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time", "units": "days", "time_origin": str(settings.time_origin)}),
        "dt": (("Time",), hdr[:, 2].astype(np.float64), {"long_name": "length of the time step", "units": "s"}),
        "itt": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "time step", "units": ""}),
    }
    variables.update(point_coordinates(state, p.cells, p._local))
    from .diagnostics import _UNITS

    for j, name in enumerate(p.output_variables):
        variables[name] = (("Time", "point"), np.ascontiguousarray(values[:, j, :]),
                           {"_FillValue": np.float64(-9999.0), "long_name": name, "units": _UNITS.get(name, "")})
    nc4lite.write(p._path, dims, variables, {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "First record (dt = 0) contains initial values. Every further record is one time step, Time at its end.",
        "setup_identifier": str(settings.identifier)})
