"""Ensemble bands: the exact quantiles ACROSS the columns of a variable, per interval -- the 5 % / 50 % / 95 % prediction band of a
parameter study in which every column is one parameter set of the same plot (GLUE and its relatives: select the behavioural columns
from the score maps, rerun with that mask, ask for the band) -- recorded on the device (include/roger_hip.h, rh_bands_*; k_bands and
k_bands_select in roger_amd/csrc/rh_bands.h).  One row per interval instead of whole planes downloaded and sorted on the host.

A setup script fills `state.bands` in `set_diagnostics`:

    state.bands.variables     = ["q_ss", "theta_rz"]                  # at most 8
    state.bands.aggregation   = {"theta_rz": "last"}                  # default: "sum" for the names diagnostics._UNITS gives "mm/dt", else "last"
    state.bands.probabilities = (0.05, 0.5, 0.95)                     # at most 8, each within [0, 1]
    state.bands.frequency     = 24 * 60 * 60                          # or 3600, 600
    state.bands.start         = 0                                     # seconds, a multiple of frequency
    state.bands.mask          = None                                  # or (nx, ny) over the GLOBAL interior, 0: column takes no part
    state.bands.capacity      = 4096                                  # rows resident on the device
    state.bands.base_output_path = ...                                # as for the diagnostics

and gets `<identifier>.bands.nc`: dimensions Time (unlimited) and probability; `Time` in days at the END of each interval, `interval`
(its number k), the coordinate `probability`, and per variable `v(Time, probability)`, `v_n(Time)` (the columns that took part) and
`v_nan(Time)` (the masked-in columns that held a NaN).  `state.bands.read()` synchronises and returns what was recorded so far.

The device rule.  After a step over (t0, t1], with f the frequency: a "sum" variable is accumulated as the output accumulators accumulate
a rate (the first step of an interval overwrites, every other adds, in step order), a "last" variable is taken at the interval's end.  A
step with t1 on a boundary (and no longer than f) closes interval k = (t1 - t_first) / f - 1; if k >= 0 the interval is counted.  The
interval value of a column is s = (sum or value) + 0.0, so a -0.0 is a +0.0.  A NaN is counted in v_nan and takes no further part;
+-inf are ordinary values; m is the number of masked-in columns that are left.  For a probability p the rank is
r = clamp(ceil(p * m) - 1, 0, m - 1) -- one double multiplication, one ceil -- and the result is the r-th smallest s: `np.sort(s)[r]`,
the "inverted CDF" quantile, bit for bit.  p = 0 is the minimum and p = 1 the maximum.  With m == 0 the row holds NaN and the file
`_FillValue`.  An hourly or ten-minute interval under a longer step is never started: it has no row.

Several ranks.  Order statistics of blocks do not merge, so there is no `combine`: a rank computes the bands of ITS OWN block and writes
one file of its own, named as the diagnostics name theirs, with the global attribute columns = "this rank's block".  A parameter study
is a one-rank run.

Start and restart.  `start` is a multiple of `frequency`.  If the model's clock is past `start` when the run begins -- after a restart --
the next interval boundary starts the first counted interval.  The ring and the accumulators are NOT part of restart files: a continued
run starts a new series there.  The host drains the ring as it drains the totals' (roger_amd/totals.py)."""
import datetime
import os

import numpy as np

from . import runtime_settings as rs
from .points import DAY, WRITE_BYTES, claim_output_file, output_file_name
from .scores import FILL, default_kind
from .totals import local_mask

MAX_VARIABLES = 8                 # roger_amd/csrc/rh_bands.h: RH_BANDS_MAX_ITEMS
MAX_PROBABILITIES = 8             # ... RH_BANDS_MAX_PROBS
FREQUENCIES = (DAY, 3600, 600)    # the step classes
KINDS = {"sum": 0, "last": 1}


class Bands:
    """`state.bands`: what the script sets (variables, aggregation, probabilities, frequency, start, mask, capacity, base_output_path)
    and the rows drained so far."""

    def __init__(self):
        self.variables = []
        self.aggregation = {}
        self.probabilities = (0.05, 0.5, 0.95)
        self.frequency = DAY
        self.start = 0
        self.mask = None
        self.capacity = 4096
        self.base_output_path = None
        self.output_path = "{identifier}.bands.nc"
        self._state = None
        self._on = False         # start() configured the device (this rank holds at least one masked-in column)
        self._names = []
        self._kinds = []
        self._probs = ()
        self._local = None       # the mask of this rank's block, or None
        self._t_first = 0        # the start of the first counted interval on the device
        self._hdr = []           # drained headers, arrays (n, 2 + 2 V) int64
        self._values = []        # drained rows, arrays (n, V, P) float64
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # host-loop steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    @property
    def active(self):
        return bool(self.variables)

    def get_output_file_name(self, state):
        return output_file_name(self, state)

    def read(self):
        """Synchronise, drain and return {"interval": (n,) int64, "time": (n,) int64 seconds, "<v>": (n, P) float64 with NaN where no
        column took part, "<v>_n", "<v>_nan": (n,) int64}; None while nothing is configured on this rank."""
        if not self._on:
            return None
        drain(self._state)
        hdr, values = _rows(self)
        out = {"interval": hdr[:, 0].copy(), "time": hdr[:, 1].copy()}
        for j, v in enumerate(self._names):
            out[v] = values[:, j].copy()
            out[f"{v}_n"] = hdr[:, 2 + 2 * j].copy()
            out[f"{v}_nan"] = hdr[:, 3 + 2 * j].copy()
        return out


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`, once the clock is known."""
    b = state.bands
    b._state = state
    if not b.active:
        return
    settings = state.settings
    if settings.enable_offline_transport:
        raise NotImplementedError("bands: the offline transport model steps by the day over its own arrays; the quantiles of state.bands "
                                  "belong to the SVAT / oneD step (a sibling for the transport model is not built)")
    names = list(b.variables)
    if len(names) > MAX_VARIABLES:
        raise ValueError(f"bands: {len(names)} variables (at most {MAX_VARIABLES})")
    if len(set(names)) != len(names):
        raise ValueError(f"bands: a variable is named twice ({names!r})")
    probs = tuple(float(p) for p in b.probabilities)
    if not 1 <= len(probs) <= MAX_PROBABILITIES:
        raise ValueError(f"bands: {len(probs)} probabilities (1 ... {MAX_PROBABILITIES})")
    if any(not 0.0 <= p <= 1.0 for p in probs):
        raise ValueError(f"bands: probabilities = {tuple(b.probabilities)!r} (each within [0, 1])")
    if int(b.frequency) not in FREQUENCIES:
        raise ValueError(f"bands: frequency = {b.frequency} s (the interval is a day, an hour or ten minutes: the step classes)")
    f = int(b.frequency)
    if int(b.start) < 0 or int(b.start) % f:
        raise ValueError(f"bands: start = {b.start} s is not a multiple of the frequency ({f} s)")
    if int(b.capacity) < 1:
        raise ValueError(f"bands: capacity = {b.capacity} (at least one row)")
    for v in b.aggregation:
        if v not in names:
            raise ValueError(f"bands: aggregation names {v!r}, which is not among the variables")
        if b.aggregation[v] not in KINDS:
            raise ValueError(f'bands: aggregation of {v!r} is {b.aggregation[v]!r} ("sum" or "last")')
    for v in names:
        meta = state.var_meta.get(v)
        if meta is None or meta.plane is None or meta.dtype is not None:
            raise NotImplementedError(f"bands: {v!r} is not a float64 (x, y) variable of the device arena")
    if b.mask is not None:
        m = np.asarray(b.mask)
        if m.shape != (settings.nx, settings.ny):
            raise ValueError(f"bands: the mask has shape {m.shape}, the grid {settings.nx} x {settings.ny} columns")
        if not m.any():
            raise ValueError("bands: the mask holds no column")
    b._names = names
    b._kinds = [KINDS[b.aggregation.get(v, default_kind(v))] for v in names]
    b._probs = probs


def start(state):
    """Configure the device (after the restart file was read: the clock is known).  The first counted interval starts at `start`, or
    at the next boundary if the clock is past it."""
    from . import runtime_state

    b = state.bands
    if not b.active or not b._names:
        return
    settings, vs = state.settings, state.variables
    f, now = int(b.frequency), int(vs.time)
    b._t_first = int(b.start) if now <= int(b.start) else -(-now // f) * f
    b._local = None
    if b.mask is not None:
        b._local = local_mask((np.asarray(b.mask) != 0).astype(np.uint8), settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        if not b._local.any():
            return   # (several ranks: no masked-in column in this rank's block)
    vs.flush_to_device()
    state.backend_context.bands_configure(b._names, b._kinds, b._probs, f, b._t_first, b._local, int(b.capacity))
    b._on, b._read, b._steps, b._unwritten = True, 0, 0, 0
    b._hdr, b._values = [], []
    b._path = claim_output_file(b, state, "bands")


def check_call(state, nsteps):
    """Before a call that enqueues nsteps steps: a step closes at most one interval, more than the ring holds could overwrite rows nobody
    has read."""
    b = state.bands
    if b._on and int(nsteps) > int(b.capacity):
        raise RuntimeError(f"{int(nsteps)} steps in one call but only {int(b.capacity)} rows of the bands are resident on the device: "
                           "call run_device() in shorter pieces, or raise state.bands.capacity")


def drain(state, final=False):
    """Read the rows the device recorded since the last drain."""
    b = state.bands
    if not b._on:
        return
    ctx = state.backend_context
    total = int(ctx.bands_count())
    n = total - b._read
    if n > int(b.capacity):
        raise RuntimeError(f"{n} rows of the bands recorded since the last drain but only {int(b.capacity)} are resident on the device")
    if n > 0:
        hdr, values = ctx.bands_read(b._read, n)
        b._hdr.append(hdr)
        b._values.append(values)
        b._read = total
        b._unwritten += values.nbytes + hdr.nbytes
    b._steps = 0
    if final or b._unwritten > WRITE_BYTES:
        _write(state)


def stepped(state):
    """A host loop made one step call: drain when the calls since the last drain reach the capacity."""
    b = state.bands
    if not b._on:
        return
    b._steps += 1
    if b._steps >= int(b.capacity):
        drain(state)


def close(state):
    """End of run(): the rest of the ring, and the file."""
    drain(state, final=True)


def _rows(b):
    nv, npr = len(b._names), len(b._probs)
    if not b._hdr:
        return np.empty((0, 2 + 2 * nv), dtype=np.int64), np.empty((0, nv, npr))
    return np.concatenate(b._hdr), np.concatenate(b._values)


def _write(state):
    """The whole file from the rows held in memory, through roger_amd.nc4lite."""
    from . import nc4lite
    from .diagnostics import _UNITS

    b = state.bands
    b._unwritten = 0
    if not b._path:
        return
    settings = state.settings
    hdr, values = _rows(b)
    variables = {
        "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time at the end of the interval", "units": "days", "time_origin": str(settings.time_origin)}),
        "interval": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "number of the interval, from the first counted one", "units": ""}),
        "probability": (("probability",), np.asarray(b._probs, dtype=np.float64), {"long_name": "non-exceedance probability", "units": ""}),
    }
    for j, v in enumerate(b._names):
        kind = "sum over the interval" if b._kinds[j] == 0 else "value at the end of the interval"
        q = np.ascontiguousarray(values[:, j])
        variables[v] = (("Time", "probability"), np.where(np.isnan(q), FILL, q),
                        {"_FillValue": np.float64(FILL), "long_name": f"{v} ({kind}): quantiles across the columns, sorted[ceil(p n) - 1]", "units": _UNITS.get(v, "")})
        variables[f"{v}_n"] = (("Time",), np.ascontiguousarray(hdr[:, 2 + 2 * j]), {"long_name": f"{v}: columns that took part", "units": ""})
        variables[f"{v}_nan"] = (("Time",), np.ascontiguousarray(hdr[:, 3 + 2 * j]), {"long_name": f"{v}: masked-in columns with a NaN", "units": ""})
    os.makedirs(os.path.dirname(os.path.abspath(b._path)), exist_ok=True)
    nc4lite.write(b._path, {"Time": None, "probability": len(b._probs)}, variables, {
        "date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)",
        "comment": "Exact quantiles across the columns of interval values, one record per counted interval.",
        "columns": "this rank's block", "setup_identifier": str(settings.identifier), "frequency_seconds": int(b.frequency),
        "first_interval_starts_seconds": int(b._t_first)})
