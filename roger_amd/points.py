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
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, MAX_CELLS, MAX_VARIABLES, WRITE_BYTES, RingSeries, check_planes, check_request, claim_output_file,  # noqa: F401
                        global_attributes, interior_plane, local_cells, output_file_name, svat_only, time_variables, write_file)


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


class PointSeries(RingSeries):
    """`state.points`: what the script sets (cells, output_variables, base_output_path, capacity) and the rows drained so far:
    headers (n, 3) int64 itt, time, dt_secs and values (n, V, K) float64."""

    label = attribute = "points"

    def __init__(self):
        super().__init__()
        self.cells = []
        self.output_variables = []
        self.base_output_path = None
        self.output_path = "{identifier}.points.nc"
        self._local = []         # [(k, local cell)] of this rank

    @property
    def active(self):
        return bool(self.cells) and bool(self.output_variables)

    def _count(self, ctx):
        return ctx.points_count()

    def _rows(self, ctx, first, n):
        return ctx.points_read(first, n)

    def _write(self, state):
        from .diagnostics import _UNITS

        hdr, values = np.concatenate(self._hdr), np.concatenate(self._values)
        variables = time_variables(hdr[:, 0], hdr[:, 1] / float(DAY), state.settings.time_origin, dt=hdr[:, 2])
        variables.update(point_coordinates(state, self.cells, self._local))
        for j, name in enumerate(self.output_variables):
            variables[name] = (("Time", "point"), np.ascontiguousarray(values[:, j, :]),
                               {"_FillValue": np.float64(-9999.0), "long_name": name, "units": _UNITS.get(name, "")})
        write_file(self._path, {"Time": None, "point": len(self._local)}, variables, global_attributes(
            state.settings.identifier, "First record (dt = 0) contains initial values. Every further record is one time step, Time at its end."))


def initialize(state):
    """Validate what the script asked for, configure the recorder and write record 0 (the initial values)."""
    from . import runtime_state

    p = state.points
    if not p.active:
        return
    settings = state.settings
    svat_only("points", settings, " and its output is read after every step (state.diagnostics); the recorder belongs to the SVAT / oneD step")
    cells = check_request("points", p.cells, len(p.output_variables), p.capacity, settings)
    check_planes("points", p.output_variables, state)
    p.cells = cells
    p._local = local_cells(cells, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    if not p._local:
        return   # (several ranks: no point in this rank's block)
    vs = state.variables
    vs.flush_to_device()
    state.backend_context.points_configure([c for _, c in p._local], list(p.output_variables), int(p.capacity))
    p._begin()
    nyl = settings.ny // rs.num_proc[1]
    first = np.empty((1, len(p.output_variables), len(p._local)))
    for j, v in enumerate(p.output_variables):
        a = interior_plane(vs, v)
        first[0, j] = [a[c // nyl, c % nyl] for _, c in p._local]
    p._hdr = [np.array([[int(vs.itt), int(vs.time), 0]], dtype=np.int64)]
    p._values = [first]
    p._path = claim_output_file(p, state, "points")
    p.write(state)


def close(state):
    state.points.close(state)
