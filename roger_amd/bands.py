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
    state.bands.zones         = None                                  # or int (nx, ny) over the GLOBAL interior, <= 0: outside every zone
    state.bands.weights       = None                                  # or (nx, ny) over the GLOBAL interior: likelihood weights, the GLUE band
    state.bands.capacity      = 4096                                  # rows resident on the device; with zones at most what 64 MiB hold
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

Zones.  With `zones` (the convention of `state.zonal_totals.zones`: the zone list is the distinct positive values in ascending order, at
most 1024) one run records the band of EVERY zone: a column takes part iff its zone is > 0 and, where a mask is given as well, mask != 0;
a zone that the mask empties stays in the list.  The file gains the dimension zone: `zone(zone)` the ids as given, `ncells(zone)` this
rank's participating columns of each, and per variable `v(Time, zone, probability)`, `v_n(Time, zone)`, `v_nan(Time, zone)`, with
`_FillValue` where a zone had no column with a number; `read()` returns the same arrays with the zone axis.  THE PROMISE: block z of a
row is, bit for bit, the row `state.bands` records without zones and with mask = (zones == z) & mask -- np.sort(s)[clamp(ceil(p m) - 1,
0, m - 1)] with the + 0.0 rule and the NaN rule below (roger_amd/csrc/rh_bands.h).  Without `zones` the file and `read()` are what they
were.  A row is V Z P 8 + V Z 16 + 16 bytes (up to 0.6 MiB), so with zones `initialize` lowers `capacity` to the rows that 64 MiB hold
(never below 1), from the GLOBAL zone list: the same number on every rank.  On the device ONE workgroup selects a zone's quantiles in its
own LDS, so the largest zone sets the time of a counted step: a map with one dominant zone belongs to `mask`.

Weights.  A GLUE band is not the plain quantile over the behavioural sets but the likelihood-weighted one: each column carries a weight,
for example max(NSE, 0) from `<identifier>.scores.nc`, and the 5 % / 95 % bounds are the values at which the cumulative weight passes
5 % / 95 % of the total.  `weights` is None (every masked-in column counts the same: everything above) or an (nx, ny) array over the
GLOBAL interior.  An integer dtype is taken as it is; a value outside 0 ... 65535 is a ValueError that names it.  A float dtype must be
finite and >= 0 with a positive maximum, and is turned into np.rint(w / w.max() * 65535.0).astype(np.uint16), the maximum taken over the
global array, so that every rank forms the same integers: A COLUMN WHOSE WEIGHT ROUNDS TO 0 TAKES NO PART.  A `mask` on top is folded in
on the host: a column takes part iff mask != 0 and its integer weight is > 0; no participating column anywhere is a ValueError, none in
this rank's block means the rank configures nothing and writes no file, like a mask.  `weights` with `zones` is refused: it is not
built.  The device rule (roger_amd/csrc/rh_bands.h) -- everything is the rule above except what is named here: clock, aggregation,
s = (sum or value) + 0.0, NaN handling.  Integer weights w_i, one uint16 per column; a column with w_i == 0 takes no part, exactly as a
masked-out column, and is in neither v_n nor v_nan.  m is the number of participating columns whose s is not a NaN, n_nan the number
whose s is a NaN: column counts, as above.  New: W = sum of w_i over the m columns, an int64 (W < 2^47, so float(W) is exact).  For a
probability p the target is T = clamp(ceil(p * W), 1, W) -- one double multiplication, one ceil -- and the result is the smallest s with
sum_{s_i <= s} w_i >= T:
    o = np.argsort(s, kind="stable");  cw = np.cumsum(w[o].astype(np.int64));  value = s[o][np.searchsorted(cw, T, side="left")]
equivalently np.sort(np.repeat(s, w))[T - 1], bit for bit: column i counts as w_i identical members.  p = 0 is the participants'
minimum and p = 1 their maximum; with m == 0 the row holds NaN and W = 0.  With every weight in {0, 1} the row is bit for bit the row
without weights under mask = (w != 0), and W == m.  `read()` gains "<v>_w", an (n,) int64, and the file `v_w(Time)` and the global
attribute weights = "integer 0 ... 65535: rint(w / max(w) * 65535)".  Without weights `read()` and the file are byte for byte what
they were.

Several ranks.  With zones a rank computes the bands of its own block over the GLOBAL zone list: a zone without a column in the block has
v_n = 0 and fill values, and a rank whose block holds no participating column configures nothing and writes no file.  Order statistics
of blocks do not merge, so there is no `combine`: a rank computes the bands of ITS OWN block and writes
one file of its own, named as the diagnostics name theirs, with the global attribute columns = "this rank's block".  A parameter study
is a one-rank run.

Start and restart.  `start` is a multiple of `frequency`.  If the model's clock is past `start` when the run begins -- after a restart --
the next interval boundary starts the first counted interval.  Without `resume` the ring and the accumulators are not part of restart
files: a continued run starts a new series there.  The host drains the ring as it drains the totals' (roger_amd/totals.py).

Resuming.  With `state.bands.resume = True` every restart file that is written holds the group "hip_bands": the SUM accumulators of the
interval under way, the start of the first counted interval, the number of rows recorded so far and the request.  The rows themselves do
not go into the restart file: the ring is drained and `<identifier>.bands.nc` is written at that moment.  A run that reads such a file with
`resume = True` and the same request -- variables and kinds, probabilities, frequency, start, mask, zone map, grid and, where weights are
given, their integer map (a file written with weights resumed without them, or the other way round, is the same error) -- configures the
device with the stored start, uploads the accumulators and goes on numbering rows and intervals where the interrupted run stopped: the
interrupted run's rows followed by the continued run's are the uninterrupted run's, the interval that holds the restart among them, plain
and per zone.  (The ring, the key planes and the selection's scratch are no state: they are rewritten or zero between two steps.)  A
different request is a RuntimeError that names the first difference; a restart file without the group too (set `resume = False` to start a
new series).  One rank only: `initialize` refuses `resume = True` with several ranks."""
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, RingSeries, carried_group, check_map_shape, check_mask, check_planes, check_resume, check_same_request, claim_output_file,
                        global_attributes, local_mask, map_array, names_array, request_group, svat_only, write_file)
from .scores import FILL, default_kind
from .zonal_totals import RING_BYTES, check_zones

MAX_VARIABLES = 8                 # roger_amd/csrc/rh_bands.h: RH_BANDS_MAX_ITEMS
MAX_PROBABILITIES = 8             # ... RH_BANDS_MAX_PROBS
MAX_WEIGHT = 65535                # the weight plane is uint16
WEIGHTS_ATTRIBUTE = "integer 0 ... 65535: rint(w / max(w) * 65535)"
FREQUENCIES = (DAY, 3600, 600)    # the step classes
KINDS = {"sum": 0, "last": 1}


class Bands(RingSeries):
    """`state.bands`: what the script sets (variables, aggregation, probabilities, frequency, start, mask, zones, weights, capacity,
    base_output_path) and the rows drained so far: headers (n, 2 + 2 V) int64 and values (n, V, P) float64 -- with zones headers (n, 2),
    counts (n, V, Z, 2) int64 and values (n, V, Z, P); with weights the weight sums (n, V) int64 beside the headers."""

    label = attribute = "bands"
    group = "hip_bands"

    def __init__(self):
        super().__init__()
        self.variables = []
        self.aggregation = {}
        self.probabilities = (0.05, 0.5, 0.95)
        self.frequency = DAY
        self.start = 0
        self.mask = None
        self.zones = None
        self.weights = None
        self.base_output_path = None
        self.output_path = "{identifier}.bands.nc"
        self._state = None
        self._names = []
        self._kinds = []
        self._probs = ()
        self._local = None       # the mask of this rank's block, or None
        self._t_first = 0        # the start of the first counted interval on the device
        self._ids = None         # zones: the ids as the script gave them, ascending (the GLOBAL list); None without zones
        self._index = None       # ... the global map as indices into them (-1: outside, or masked out)
        self._ncells = None      # ... this rank's participating columns of every zone
        self._counts = []        # ... drained counts
        self._weights = None     # weights: the GLOBAL integer map, uint16 (nx, ny), as quantised by `initialize`; None without weights
        self._wsum = []          # ... drained weight sums

    @property
    def active(self):
        return bool(self.variables)

    def read(self):
        """Synchronise, drain and return {"interval": (n,) int64, "time": (n,) int64 seconds, "<v>": (n, P) float64 with NaN where no
        column took part, "<v>_n", "<v>_nan": (n,) int64 and, with weights, "<v>_w": (n,) int64}; None while nothing is configured on
        this rank."""
        if not self._on:
            return None
        self.drain(self._state)
        if self._ids is not None:
            hdr, counts, values = self._all_zonal_rows()
            out = {"interval": hdr[:, 0].copy(), "time": hdr[:, 1].copy()}
            for j, v in enumerate(self._names):
                out[v] = values[:, j].copy()              # (n, Z, P)
                out[f"{v}_n"] = counts[:, j, :, 0].copy()   # (n, Z)
                out[f"{v}_nan"] = counts[:, j, :, 1].copy()
            return out
        hdr, values = self._all_rows()
        out = {"interval": hdr[:, 0].copy(), "time": hdr[:, 1].copy()}
        for j, v in enumerate(self._names):
            out[v] = values[:, j].copy()
            out[f"{v}_n"] = hdr[:, 2 + 2 * j].copy()
            out[f"{v}_nan"] = hdr[:, 3 + 2 * j].copy()
            if self._weights is not None:
                out[f"{v}_w"] = self._all_wsum()[:, j].copy()
        return out

    def _request(self, state):
        """What a resumed run must ask for again (observers.check_same_request)."""
        request = {"variables": names_array(self._names), "kinds": np.asarray(self._kinds, dtype=np.int64),
                   "probabilities": np.asarray(self._probs, dtype=np.float64), "frequency": np.int64(self.frequency), "start": np.int64(self.start),
                   "mask": map_array(None if self.mask is None else np.asarray(self.mask) != 0, np.uint8), "zones": map_array(self.zones, np.int64),
                   "grid": np.asarray([state.settings.nx, state.settings.ny], dtype=np.int64)}
        if self._weights is not None:   # (only then: the groups of runs without weights stay what they were)
            request["weights"] = map_array(self._weights, np.int64)
        return request

    def restart_state(self, state):
        """The group "hip_bands" of a restart file.  The ring is drained and the file written first; what is carried is the SUM
        accumulators, the start of the first counted interval and the number of rows so far."""
        if not self._on:
            return None
        self.drain(state, final=True)
        ctx = state.backend_context
        return dict(request_group(self._request(state)), acc=np.asarray(ctx.bands_state(), dtype=np.float64),
                    scalars=np.asarray([self._t_first, ctx.bands_count()], dtype=np.int64))

    def _count(self, ctx):
        return ctx.bands_count()

    def _rows(self, ctx, first, n):
        if self._weights is not None:
            return ctx.bands_read(first, n) + (ctx.bands_weight_sums(first, n),)
        return ctx.bands_read(first, n) if self._ids is None else ctx.bands_zonal_read(first, n)

    def _keep(self, state, hdr, *rest):
        if self._weights is not None:
            values, wsum = rest
            self._wsum.append(wsum)
            return super()._keep(state, hdr, values) + wsum.nbytes
        if self._ids is None:
            return super()._keep(state, hdr, *rest)
        counts, values = rest
        self._counts.append(counts)
        return super()._keep(state, hdr, values) + counts.nbytes

    def _all_rows(self):
        nv, npr = len(self._names), len(self._probs)
        if not self._hdr:
            return np.empty((0, 2 + 2 * nv), dtype=np.int64), np.empty((0, nv, npr))
        return np.concatenate(self._hdr), np.concatenate(self._values)

    def _all_wsum(self):
        return np.concatenate(self._wsum) if self._wsum else np.empty((0, len(self._names)), dtype=np.int64)

    def _all_zonal_rows(self):
        nv, nz, npr = len(self._names), len(self._ids), len(self._probs)
        if not self._hdr:
            return np.empty((0, 2), dtype=np.int64), np.empty((0, nv, nz, 2), dtype=np.int64), np.empty((0, nv, nz, npr))
        return np.concatenate(self._hdr), np.concatenate(self._counts), np.concatenate(self._values)

    def _write(self, state):
        from .diagnostics import _UNITS

        if self._ids is not None:
            return self._write_zonal(state)
        settings = state.settings
        hdr, values = self._all_rows()
        variables = {
            "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time at the end of the interval", "units": "days", "time_origin": str(settings.time_origin)}),
            "interval": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "number of the interval, from the first counted one", "units": ""}),
            "probability": (("probability",), np.asarray(self._probs, dtype=np.float64), {"long_name": "non-exceedance probability", "units": ""}),
        }
        for j, v in enumerate(self._names):
            kind = "sum over the interval" if self._kinds[j] == 0 else "value at the end of the interval"
            q = np.ascontiguousarray(values[:, j])
            variables[v] = (("Time", "probability"), np.where(np.isnan(q), FILL, q),
                            {"_FillValue": np.float64(FILL), "long_name": f"{v} ({kind}): quantiles across the columns, sorted[ceil(p n) - 1]", "units": _UNITS.get(v, "")})
            variables[f"{v}_n"] = (("Time",), np.ascontiguousarray(hdr[:, 2 + 2 * j]), {"long_name": f"{v}: columns that took part", "units": ""})
            variables[f"{v}_nan"] = (("Time",), np.ascontiguousarray(hdr[:, 3 + 2 * j]), {"long_name": f"{v}: masked-in columns with a NaN", "units": ""})
            if self._weights is not None:
                variables[f"{v}_w"] = (("Time",), np.ascontiguousarray(self._all_wsum()[:, j]),
                                       {"long_name": f"{v}: sum of the integer weights of the columns that took part", "units": ""})
        extra = {"frequency_seconds": int(self.frequency), "first_interval_starts_seconds": int(self._t_first)}
        if self._weights is not None:
            extra["weights"] = WEIGHTS_ATTRIBUTE
        write_file(self._path, {"Time": None, "probability": len(self._probs)}, variables, global_attributes(
            settings.identifier, "Exact quantiles across the columns of interval values, one record per counted interval.", extra,
            lead={"columns": "this rank's block"}))


    def _write_zonal(self, state):
        from .diagnostics import _UNITS

        settings = state.settings
        hdr, counts, values = self._all_zonal_rows()
        variables = {
            "Time": (("Time",), hdr[:, 1] / float(DAY), {"long_name": "Time at the end of the interval", "units": "days", "time_origin": str(settings.time_origin)}),
            "interval": (("Time",), hdr[:, 0].astype(np.int64), {"long_name": "number of the interval, from the first counted one", "units": ""}),
            "probability": (("probability",), np.asarray(self._probs, dtype=np.float64), {"long_name": "non-exceedance probability", "units": ""}),
            "zone": (("zone",), np.asarray(self._ids, dtype=np.int64), {"long_name": "zone id of the zone map", "units": ""}),
            "ncells": (("zone",), np.asarray(self._ncells, dtype=np.int64), {"long_name": "columns of the zone that take part", "units": ""}),
        }
        for j, v in enumerate(self._names):
            kind = "sum over the interval" if self._kinds[j] == 0 else "value at the end of the interval"
            q = np.ascontiguousarray(values[:, j])
            variables[v] = (("Time", "zone", "probability"), np.where(np.isnan(q), FILL, q),
                            {"_FillValue": np.float64(FILL), "long_name": f"{v} ({kind}): quantiles across the columns of the zone, sorted[ceil(p n) - 1]",
                             "units": _UNITS.get(v, "")})
            variables[f"{v}_n"] = (("Time", "zone"), np.ascontiguousarray(counts[:, j, :, 0]), {"long_name": f"{v}: columns of the zone that took part", "units": ""})
            variables[f"{v}_nan"] = (("Time", "zone"), np.ascontiguousarray(counts[:, j, :, 1]), {"long_name": f"{v}: participating columns of the zone with a NaN", "units": ""})
        write_file(self._path, {"Time": None, "zone": len(self._ids), "probability": len(self._probs)}, variables, global_attributes(
            settings.identifier, "Exact quantiles across the columns of every zone of interval values, one record per counted interval.",
            {"frequency_seconds": int(self.frequency), "first_interval_starts_seconds": int(self._t_first)}, lead={"columns": "this rank's block"}))


def zonal_capacity(capacity, n_variables, n_zones, n_probabilities):
    """The rows of V Z P 8 + V Z 16 + 16 bytes that RING_BYTES (64 MiB) hold, at most `capacity` and at least one."""
    v, z, p = int(n_variables), int(n_zones), int(n_probabilities)
    return int(max(1, min(int(capacity), RING_BYTES // (v * z * p * 8 + v * z * 16 + 16))))


def check_weights(weights, mask, settings):
    """`state.bands.weights` as the GLOBAL integer map, uint16 (nx, ny): an integer array as it is, a float array as
    rint(w / max(w) * 65535) with the maximum over the global array.  `mask`: booleans or None; at least one column takes part."""
    w = np.asarray(weights)
    check_map_shape("bands", "weights map", w, settings)
    if w.dtype.kind in "iub":
        bad = np.argwhere((w < 0) | (w > MAX_WEIGHT))
        if bad.size:
            ix, iy = (int(c) for c in bad[0])
            raise ValueError(f"bands: weight {int(w[ix, iy])} at cell ({ix}, {iy}) (integer weights lie within 0 ... {MAX_WEIGHT})")
        q = w.astype(np.uint16)
    elif w.dtype.kind == "f":
        w = w.astype(np.float64)
        bad = np.argwhere(~(np.isfinite(w) & (w >= 0.0)))
        if bad.size:
            ix, iy = (int(c) for c in bad[0])
            raise ValueError(f"bands: weight {float(w[ix, iy])!r} at cell ({ix}, {iy}) (weights are finite and >= 0)")
        if not w.max() > 0.0:
            raise ValueError("bands: every weight is 0 (the largest weight must be positive)")
        q = np.rint(w / w.max() * float(MAX_WEIGHT)).astype(np.uint16)
    else:
        raise ValueError(f"bands: the weights have dtype {w.dtype} (an integer or a float array)")
    if not ((q != 0) if mask is None else (q != 0) & mask).any():
        raise ValueError("bands: no column takes part (a column takes part iff its integer weight is > 0" + (")" if mask is None else " and mask != 0)"))
    return q


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`, once the clock is known."""
    b = state.bands
    b._state = state
    if not b.active:
        return
    settings = state.settings
    check_resume("bands", b)
    svat_only("bands", settings, " over its own arrays; the quantiles of state.bands belong to the SVAT / oneD step (a sibling for the "
              "transport model is not built)")
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
    check_planes("bands", names, state)
    mask = check_mask("bands", b.mask, settings)
    b._ids = b._index = b._weights = None
    if b.weights is not None:
        if b.zones is not None:
            raise ValueError("bands: weights with zones is not built (the per-zone selection counts in 32-bit histograms, one per zone)")
        b._weights = check_weights(b.weights, mask, settings)
    if b.zones is not None:
        ids, index = check_zones("bands", b.zones, settings)
        b._ids = ids.astype(np.int64)
        b._index = index if mask is None else np.where(mask, index, -1).astype(np.int32)   # (a zone the mask empties stays in the list)
        b.capacity = zonal_capacity(b.capacity, len(names), ids.size, len(probs))
    b._names = names
    b._kinds = [KINDS[b.aggregation.get(v, default_kind(v))] for v in names]
    b._probs = probs


def start(state):
    """Configure the device (after the restart file was read: the clock is known).  The first counted interval starts at `start`, or
    at the next boundary if the clock is past it.  A resumed run (`resume`, and the restart file holds "hip_bands") takes the stored
    start instead, the accumulators with it, and numbers its rows from the stored count on."""
    from . import runtime_state

    b = state.bands
    if not b.active or not b._names:
        return
    settings, vs = state.settings, state.variables
    f, now = int(b.frequency), int(vs.time)
    b._t_first = int(b.start) if now <= int(b.start) else -(-now // f) * f
    held = carried_group("bands", b)
    if held is not None:
        check_same_request("bands", b, held, b._request(state))
        if b._weights is None and held.get("request_weights") is not None:   # (the other direction is check_same_request's: a key the file lacks)
            raise RuntimeError(f"bands: resume = True, but the restart file {b._restart_file} was written with weights = an array of shape "
                               f"{np.asarray(held['request_weights']).shape} and this run asks for weights = None: a resumed observer takes the same request")
        b._t_first = int(held["scalars"][0])
    b._local = None
    if b._ids is not None:
        b._local = local_mask(b._index, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        b._ncells = np.bincount(b._local[b._local >= 0], minlength=b._ids.size).astype(np.int64)
        if not b._ncells.any():
            return   # (several ranks: no participating column in this rank's block)
        vs.flush_to_device()
        state.backend_context.bands_configure(b._names, b._kinds, b._probs, f, b._t_first, None, int(b.capacity), zones=b._local,
                                              n_zones=int(b._ids.size))
    elif b._weights is not None:
        folded = b._weights if b.mask is None else np.where(np.asarray(b.mask) != 0, b._weights, 0).astype(np.uint16)
        b._local = local_mask(folded, settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        if not b._local.any():
            return   # (several ranks: no participating column in this rank's block)
        vs.flush_to_device()
        state.backend_context.bands_configure(b._names, b._kinds, b._probs, f, b._t_first, None, int(b.capacity), weights=b._local)
    else:
        if b.mask is not None:
            b._local = local_mask((np.asarray(b.mask) != 0).astype(np.uint8), settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
            if not b._local.any():
                return   # (several ranks: no masked-in column in this rank's block)
        vs.flush_to_device()
        state.backend_context.bands_configure(b._names, b._kinds, b._probs, f, b._t_first, b._local, int(b.capacity))
    b._begin()
    b._hdr, b._values, b._counts, b._wsum = [], [], [], []
    if held is not None:
        rows = int(held["scalars"][1])
        state.backend_context.bands_restore(held["acc"], rows)
        b._read = rows   # (the rows before it are in the interrupted run's file)
    b._path = claim_output_file(b, state, "bands")


def close(state):
    state.bands.close(state)
