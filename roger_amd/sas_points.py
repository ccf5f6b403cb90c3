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
import datetime
import os

import numpy as np

from . import runtime_settings as rs
from ._native import DAILY_INPUTS
from .points import DAY, WRITE_BYTES, check_request, claim_output_file, local_cells, output_file_name, point_coordinates

_GRIDS = (("x", "y"), ("x", "y", "timesteps"), ("x", "y", "ages"), ("x", "y", "nages"), ("x", "y", "timesteps", "ages"))


class TransportPointSeries:
    """`state.transport_points`: what the script sets (cells, output_variables, base_output_path, capacity) and the rows drained so far."""

    def __init__(self):
        self.cells = []
        self.output_variables = []
        self.base_output_path = None
        self.capacity = 4096
        self.output_path = "{identifier}.transport_points.nc"
        self._on = False         # start() configured the device (this rank holds at least one point)
        self._local = []         # [(k, local cell)] of this rank
        self._hdr = []           # (itt, time) of every row: the drained ones, then the ones still on the device
        self._values = {}        # {variable: [arrays (n, K) or (n, K, width)]} drained so far
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.cells) and bool(self.output_variables)

    def get_output_file_name(self, state):
        return output_file_name(self, state)


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
    p._on, p._read, p._steps, p._unwritten = True, 0, 0, 0
    p._hdr = [(int(vs.itt), int(vs.time))]
    p._values = {v: [] for v in p.output_variables}
    p._path = claim_output_file(p, state, "transport points")
    drain(state, final=True)


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    p = state.transport_points
    if not p._on:
        return
    sas = state.sas_context
    total = int(sas.points_count())
    n = total - p._read
    if n > int(p.capacity) or total != len(p._hdr):
        raise RuntimeError(f"{n} rows of the transport points recorded since the last drain ({total} in all, {len(p._hdr)} steps known "
                           f"to the host) but only {int(p.capacity)} are resident on the device")
    if n > 0:
        _, values = sas.points_read(p._read, n)
        for v in p.output_variables:
            a = values[state.var_meta[v].sas]
            p._values[v].append(a)
            p._unwritten += a.nbytes
        p._read = total
    p._steps = 0
    if final or p._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """_step_offline_transport made a step (rh_sas_step recorded its row): note its itt and time, drain when the steps since the last
    drain reach the capacity."""
    p = state.transport_points
    if not p._on:
        return
    vs = state.variables
    p._hdr.append((int(vs.itt), int(vs.time)))
    p._steps += 1
    if p._steps >= int(p.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    p = state.transport_points
    p._unwritten = 0
    if not p._path:
        return
    from . import nc4lite
    from .diagnostics import _UNITS

    settings = state.settings
    os.makedirs(os.path.dirname(os.path.abspath(p._path)), exist_ok=True)
    hdr = np.array(p._hdr[:p._read], dtype=np.int64).reshape(-1, 2)
    dims = {"Time": None, "point": len(p._local)}
    variables = {
        "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time", "units": "days", "time_origin": str(settings.time_origin)}),
        "itt": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "time step", "units": ""}),
    }
    variables.update(point_coordinates(state, p.cells, p._local))
    for name in p.output_variables:
        data = np.concatenate(p._values[name])
        extra = ()
        if data.ndim == 3:   # (Time, point, ages | nages)
            dim = "ages" if data.shape[2] == settings.ages else "nages"
            dims.setdefault(dim, data.shape[2])
            extra = (dim,)
        variables[name] = (("Time", "point") + extra, np.ascontiguousarray(data, dtype=np.float64),
                           {"_FillValue": np.float64(-9999.0), "long_name": name, "units": _UNITS.get(name, "")})
    nc4lite.write(p._path, dims, variables, {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "First record contains the initial values of the run proper. Every further record is one day, Time at its end.",
        "setup_identifier": str(settings.identifier)})
