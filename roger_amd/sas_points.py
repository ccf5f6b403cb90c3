"""Time series at observation columns of the offline transport model: the concentration in a lysimeter's percolate, in the root
zone, the travel time distribution of q_ss at that column -- a row per model day, on top of the SAS context's recorder
(include/roger_hip_sas.h, rh_sas_points_*; k_sas_points).  The sibling of roger_amd/points.py, which belongs to the SVAT / oneD step.

A setup script fills `state.transport_points` in `set_diagnostics`:

    state.transport_points.cells = [(ix, iy), ...]          # interior indices of the GLOBAL grid, 0-based
    state.transport_points.output_variables = ["C_iso_q_ss", "C_iso_rz", "tt50_q_ss", "TT_q_ss", "sa_s"]
    state.transport_points.base_output_path = ...           # as for the diagnostics
    state.transport_points.capacity = 4096                  # rows resident on the device

and gets `<identifier>.transport_points.nc`: dimensions Time (unlimited), point and, where used, ages / nages; `Time` in days with
`time_origin`, `itt`, per point `ix`, `iy` (global) and `x`, `y`; per-cell variables (Time, point), age-resolved ones
(Time, point, ages | nages), float64 with `_FillValue`.  Accepted are the float64 (x, y), (x, y, timesteps), (x, y, ages) and
(x, y, nages) variables that the SAS context computes or keeps per cell.

Nothing is recorded during the warm-up runs.  Once `warmup()` has set `warmup_done` -- or `setup()` has read a restart file of a
warmed-up run: a restarted run starts a new series -- the recorder is configured and record 0 takes the initial values
(rh_sas_points_record), where `diagnostics.output_transport` writes its initial record.  From then on the day's launch itself is
followed by the row's (rh_sas_step); nothing is downloaded per step.  The ring is drained every `capacity` steps, before a restart
file is written and at the end of run().  The host makes one step per row and keeps `itt` and `time` of each beside the rows.  With
several ranks a rank records the points of its block and writes a file of its own (`.NNNN.nc`); a rank without a point writes none."""
import numpy as np

from . import runtime_settings as rs
from ._native import DAILY_INPUTS
from .observers import DAY, RingSeries, check_request, claim_output_file, global_attributes, local_cells, time_variables, write_file
from .points import point_coordinates

_GRIDS = (("x", "y"), ("x", "y", "timesteps"), ("x", "y", "ages"), ("x", "y", "nages"), ("x", "y", "timesteps", "ages"))


class TransportPointSeries(RingSeries):
    """`state.transport_points`: what the script sets (cells, output_variables, base_output_path, capacity) and the rows drained so far:
    {variable: [arrays (n, K) or (n, K, width)]}."""

    label, attribute = "transport points", "transport_points"
    context, host_header = "sas_context", True

    def __init__(self):
        super().__init__()
        self.cells = []
        self.output_variables = []
        self.base_output_path = None
        self.output_path = "{identifier}.transport_points.nc"
        self._local = []         # [(k, local cell)] of this rank
        self._values = {}

    @property
    def active(self):
        return bool(self.cells) and bool(self.output_variables)

    def _count(self, ctx):
        return ctx.points_count()

    def _rows(self, ctx, first, n):
        return ctx.points_read(first, n)

    def _keep(self, state, tags, values):
        held = 0
        for v in self.output_variables:
            a = values[state.var_meta[v].sas]
            self._values[v].append(a)
            held += a.nbytes
        return held

    def _write(self, state):
        from .diagnostics import _UNITS

        settings = state.settings
        hdr = np.array(self._hdr[:self._read], dtype=np.int64).reshape(-1, 2)
        dims = {"Time": None, "point": len(self._local)}
        variables = time_variables(hdr[:, 0], hdr[:, 1] / float(DAY), settings.time_origin)
        variables.update(point_coordinates(state, self.cells, self._local))
        for name in self.output_variables:
            data = np.concatenate(self._values[name])
            extra = ()
            if data.ndim == 3:   # (Time, point, ages | nages)
                dim = "ages" if data.shape[2] == settings.ages else "nages"
                dims.setdefault(dim, data.shape[2])
                extra = (dim,)
            variables[name] = (("Time", "point") + extra, np.ascontiguousarray(data, dtype=np.float64),
                               {"_FillValue": np.float64(-9999.0), "long_name": name, "units": _UNITS.get(name, "")})
        write_file(self._path, dims, variables, global_attributes(
            settings.identifier, "First record contains the initial values of the run proper. Every further record is one day, Time at its end."))


def initialize(state):
    """setup(): validate what the script asked for.  The recorder itself starts with the run proper (start)."""
    from .diagnostics import _AGED

    p = state.transport_points
    if not p.active:
        return
    if not state.settings.enable_offline_transport:
        raise NotImplementedError("transport_points: the series of the offline transport model; the SVAT / oneD step records through state.points")
    p.cells = check_request("transport_points", p.cells, len(p.output_variables), p.capacity, state.settings)
    for v in p.output_variables:
        meta = state.var_meta.get(v)
        if v in _AGED:
            raise NotImplementedError(f"transport_points: {v!r} would be recorded after the ageing, the reference writes it before "
                                      "(use sa_s / msa_s, or read vs.<name> from the setup script)")
        if meta is not None and meta.dims is not None and tuple(meta.dims[:2]) == ("x", "y") and meta.sas is None:
            raise NotImplementedError(f"transport_points: {v!r} exists on the host only (the setup script's hooks form it): "
                                      "not an array of the SAS context")
        if meta is None or meta.dims is None or tuple(meta.dims) not in _GRIDS or meta.dtype is not None or meta.sas in DAILY_INPUTS:
            raise NotImplementedError(f"transport_points: {v!r} is not a float64 per-cell result of the transport step")


def start(state):
    """The run proper begins (warmup() is through, or a restart file of a warmed-up run was read): configure the recorder, take
    record 0 and write the file's first version.  Called again, it starts a new series."""
    from . import runtime_state

    p = state.transport_points
    if not p.active or not state.settings.enable_offline_transport:
        return
    settings, vs = state.settings, state.variables
    p._local = local_cells(p.cells, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
    if not p._local:
        return   # (several ranks: no point in this rank's block)
    sas = state.sas_context
    vs.flush_to_device()
    sas.points_configure([c for _, c in p._local], [state.var_meta[v].sas for v in p.output_variables], int(p.capacity))
    sas.points_record(int(vs.itt))
    p._begin()
    p._hdr = [(int(vs.itt), int(vs.time))]
    p._values = {v: [] for v in p.output_variables}
    p._path = claim_output_file(p, state, "transport points")
    p.drain(state, final=True)
