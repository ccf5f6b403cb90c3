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
    state.bands.observations  = {}                                    # or {"q_ss": series}: where the measurement falls in the ensemble
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

Observations.  Does the band contain the measurement?  `observations = {"q_ss": obs}` gives a variable a float series, NaN: missing, of
shape (n_intervals,) -- with zones (n_zones, n_intervals) in the order of the ascending global zone list, or (n_intervals,) for every
zone.  The rule (roger_amd/csrc/rh_bands.h) -- everything is the rule above as it stands, and on top of it: the series is indexed from
`start`, not from the first counted interval: for row interval number k the element is o = obs[k + (t_first - start) / frequency], so a
continued run without `resume` stays aligned; an index beyond the series means missing.  On a counted step, per variable (and zone), an
int64 pair (below, equal): o a NaN (missing, or the variable has no observations) gives below = equal = -1; else o' = o + 0.0 and, over
the participating columns whose s is a number, below = sum c_i [s_i < o'] and equal = sum c_i [s_i == o'], c_i = 1 or, with weights, the
integer weight w_i; with m == 0: (0, 0).  In numpy, x and wx the participants that are numbers:
    below = int(wx[x < o].sum());  equal = int(wx[x == o].sum())
exact integers, like the rest of the row.  With T_tot = m (or W with weights): 0 <= below, 0 <= equal, below + equal <= T_tot, and for a
recorded probability p with T = clamp(ceil(p * T_tot), 1, T_tot) and recorded quantile q: q <= o <=> below + equal >= T, and q < o <=>
below >= T -- so o lies inside [q_lo, q_hi] iff below + equal >= T_lo and below < T_hi: `inside`, whose mean over the observed rows is the
containing ratio.  `read()` gains "<v>_obs" (float64, NaN where missing), "<v>_below" and "<v>_equal" (int64, -1 where missing); the file
gains `v_obs`, `v_below`, `v_equal` and `v_pit = (below + equal / 2) / T_tot` (`_FillValue` where the observation is missing or the
total is 0) over (Time) or (Time, zone) -- `rank_histogram` bins it -- and the global attribute `observations`.  Without observations
nothing new is launched and `read()` and the file are byte for byte what they were.

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
given, their integer map, and likewise the observations (a file written with weights or observations resumed without them, or the other
way round, is the same error) -- configures the
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
OBSERVATIONS_ATTRIBUTE = ("v_below, v_equal: the members (with weights: their integer weights) whose interval value is < and == v_obs, -1 where it is "
                          "missing; v_pit = (below + equal / 2) / total; v_obs lies inside [q(p_lo), q(p_hi)] iff below + equal >= T(p_lo) and "
                          "below < T(p_hi), T(p) = clamp(ceil(p total), 1, total), total = v_n (with weights v_w)")
FREQUENCIES = (DAY, 3600, 600)    # the step classes
KINDS = {"sum": 0, "last": 1}


class Bands(RingSeries):
    """`state.bands`: what the script sets (variables, aggregation, probabilities, frequency, start, mask, zones, weights, capacity,
    base_output_path) and the rows drained so far: headers (n, 2 + 2 V) int64 and values (n, V, P) float64 -- with zones headers (n, 2),
    counts (n, V, Z, 2) int64 and values (n, V, Z, P); with weights the weight sums (n, V) int64 beside the headers; with observations the
    pairs (n, V, 2) or (n, V, Z, 2) int64 {below, equal}."""

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
        self.observations = {}
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
        self._obs = None         # observations: float64 (V, L) or (V, Z, L), NaN: missing, as formed by `initialize`; None without
        self._pairs = []         # ... drained pairs

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
            self._read_observations(out, hdr)
            return out
        hdr, values = self._all_rows()
        out = {"interval": hdr[:, 0].copy(), "time": hdr[:, 1].copy()}
        for j, v in enumerate(self._names):
            out[v] = values[:, j].copy()
            out[f"{v}_n"] = hdr[:, 2 + 2 * j].copy()
            out[f"{v}_nan"] = hdr[:, 3 + 2 * j].copy()
            if self._weights is not None:
                out[f"{v}_w"] = self._all_wsum()[:, j].copy()
        self._read_observations(out, hdr)
        return out

    def _first_index(self):
        """The element of a series the first counted interval reads: the series is indexed from `start`."""
        return (int(self._t_first) - int(self.start)) // int(self.frequency)

    def _obs_rows(self, hdr):
        """The observation of every drained row, (n, V) or (n, V, Z): NaN where missing or beyond the series."""
        at = hdr[:, 0] + self._first_index()
        ok = (at >= 0) & (at < self._obs.shape[-1])
        out = np.full(self._obs.shape[:-1] + (len(at),), np.nan)
        out[..., ok] = self._obs[..., at[ok]]
        return np.moveaxis(out, -1, 0)

    def _all_pairs(self):
        return np.concatenate(self._pairs) if self._pairs else np.empty((0,) + self._obs.shape[:-1] + (2,), dtype=np.int64)

    def _read_observations(self, out, hdr):
        """`read()`: "<v>_obs", "<v>_below", "<v>_equal" of the observed variables; nothing without observations."""
        if self._obs is None:
            return
        obs, pairs = self._obs_rows(hdr), self._all_pairs()
        for j, v in enumerate(self._names):
            if v in self.observations:
                out[f"{v}_obs"] = obs[:, j].copy()
                out[f"{v}_below"] = pairs[:, j, ..., 0].copy()
                out[f"{v}_equal"] = pairs[:, j, ..., 1].copy()

    def _write_observations(self, variables, extra, hdr, totals, dims):
        """The file: v_obs, v_below, v_equal and v_pit over `dims`, and the global attribute; totals (n, V[, Z]): m, or W with weights."""
        if self._obs is None:
            return
        obs, pairs = self._obs_rows(hdr), self._all_pairs()
        for j, v in enumerate(self._names):
            if v not in self.observations:
                continue
            o, below, equal, total = obs[:, j], pairs[:, j, ..., 0], pairs[:, j, ..., 1], np.asarray(totals)[:, j]
            variables[f"{v}_obs"] = (dims, np.where(np.isnan(o), FILL, o), {"_FillValue": np.float64(FILL), "long_name": f"{v}: the observation of the interval", "units": ""})
            variables[f"{v}_below"] = (dims, np.ascontiguousarray(below), {"long_name": f"{v}: members below the observation (-1: no observation)", "units": ""})
            variables[f"{v}_equal"] = (dims, np.ascontiguousarray(equal), {"long_name": f"{v}: members equal to the observation (-1: no observation)", "units": ""})
            variables[f"{v}_pit"] = (dims, pit(below, equal, total, fill=FILL),
                                     {"_FillValue": np.float64(FILL), "long_name": f"{v}: (below + equal / 2) / total, where the observation sits in the ensemble", "units": ""})
        extra["observations"] = OBSERVATIONS_ATTRIBUTE

    def _request(self, state):
        """What a resumed run must ask for again (observers.check_same_request)."""
        request = {"variables": names_array(self._names), "kinds": np.asarray(self._kinds, dtype=np.int64),
                   "probabilities": np.asarray(self._probs, dtype=np.float64), "frequency": np.int64(self.frequency), "start": np.int64(self.start),
                   "mask": map_array(None if self.mask is None else np.asarray(self.mask) != 0, np.uint8), "zones": map_array(self.zones, np.int64),
                   "grid": np.asarray([state.settings.nx, state.settings.ny], dtype=np.int64)}
        if self._weights is not None:   # (only then: the groups of runs without weights stay what they were)
            request["weights"] = map_array(self._weights, np.int64)
        if self._obs is not None:       # (likewise)
            request["observations"] = map_array(self._obs, np.float64)
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
        pairs = () if self._obs is None else (ctx.bands_obs_read(first, n),)
        if self._weights is not None:
            return ctx.bands_read(first, n) + (ctx.bands_weight_sums(first, n),) + pairs
        return (ctx.bands_read(first, n) if self._ids is None else ctx.bands_zonal_read(first, n)) + pairs

    def _keep(self, state, hdr, *rest):
        if self._obs is not None:       # (the pairs beside the rows, last)
            self._pairs.append(rest[-1])
            return self._keep_rows(state, hdr, *rest[:-1]) + rest[-1].nbytes
        return self._keep_rows(state, hdr, *rest)

    def _keep_rows(self, state, hdr, *rest):
        if self._weights is not None:
            values, wsum = rest
            self._wsum.append(wsum)
            return RingSeries._keep(self, state, hdr, values) + wsum.nbytes
        if self._ids is None:
            return RingSeries._keep(self, state, hdr, *rest)
        counts, values = rest
        self._counts.append(counts)
        return RingSeries._keep(self, state, hdr, values) + counts.nbytes

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
        self._write_observations(variables, extra, hdr, self._all_wsum() if self._weights is not None else hdr[:, 2::2], ("Time",))
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
        extra = {"frequency_seconds": int(self.frequency), "first_interval_starts_seconds": int(self._t_first)}
        self._write_observations(variables, extra, hdr, counts[..., 0], ("Time", "zone"))
        write_file(self._path, {"Time": None, "zone": len(self._ids), "probability": len(self._probs)}, variables, global_attributes(
            settings.identifier, "Exact quantiles across the columns of every zone of interval values, one record per counted interval.",
            extra, lead={"columns": "this rank's block"}))


def zonal_capacity(capacity, n_variables, n_zones, n_probabilities):
    """The rows of V Z P 8 + V Z 16 + 16 bytes that RING_BYTES (64 MiB) hold, at most `capacity` and at least one."""
    v, z, p = int(n_variables), int(n_zones), int(n_probabilities)
    return int(max(1, min(int(capacity), RING_BYTES // (v * z * p * 8 + v * z * 16 + 16))))


def targets(p, total):
    """T = clamp(ceil(p * total), 1, total) of a probability under totals (m, or W with weights): one double multiplication, one ceil."""
    total = np.asarray(total, dtype=np.int64)
    return np.clip(np.ceil(float(p) * total.astype(np.float64)).astype(np.int64), 1, np.maximum(total, 1))


def inside(below, equal, total, p_lo, p_hi):
    """Whether the observation lies inside [q(p_lo), q(p_hi)], from the recorded counts alone: below + equal >= T(p_lo) and below <
    T(p_hi) -- the same answer as q_lo <= o <= q_hi on the recorded quantiles.  False where the observation is missing (-1) or nothing
    took part (total == 0).  The containing ratio is its mean over the observed rows."""
    below, equal, total = (np.asarray(a, dtype=np.int64) for a in (below, equal, total))
    return (below >= 0) & (total > 0) & (below + equal >= targets(p_lo, total)) & (below < targets(p_hi, total))


def pit(below, equal, total, fill=np.nan):
    """(below + equal / 2) / total, `fill` where the observation is missing (-1) or nothing took part (total == 0)."""
    below, equal, total = (np.asarray(a, dtype=np.int64) for a in (below, equal, total))
    ok = (below >= 0) & (total > 0)
    return np.where(ok, (below + equal / 2.0) / np.where(ok, total, 1), fill)


def rank_histogram(pit_values, bins=10, fill=None):
    """Counts of the PIT values in `bins` equal bins over [0, 1] (1.0 in the last): int64 (bins,).  NaN and `fill` (default: the files'
    _FillValue) are left out.  A flat histogram: the ensemble spreads as the observations do."""
    x = np.asarray(pit_values, dtype=np.float64).reshape(-1)
    x = x[(x == x) & (x != (FILL if fill is None else fill))]
    if int(bins) < 1:
        raise ValueError(f"bands.rank_histogram: bins = {bins} (at least one)")
    if x.size and (x.min() < 0.0 or x.max() > 1.0):
        raise ValueError(f"bands.rank_histogram: PIT values lie within [0, 1] (got {x.min()} ... {x.max()})")
    return np.histogram(x, bins=int(bins), range=(0.0, 1.0))[0].astype(np.int64)


def check_observations(observations, names, n_zones):
    """`state.bands.observations` as float64 (V, L) -- with zones (V, Z, L) -- NaN: missing, a variable without observations all NaN, a
    shorter series NaN behind its end."""
    series = {}
    for v, a in dict(observations).items():
        if v not in names:
            raise ValueError(f"bands: observations names {v!r}, which is not among the variables")
        a = np.asarray(a)
        if a.dtype.kind != "f":
            raise ValueError(f"bands: the observations of {v!r} have dtype {a.dtype} (a float array, NaN: missing)")
        if a.ndim != 1 and not (n_zones is not None and a.ndim == 2 and a.shape[0] == n_zones):
            want = "(n_intervals,)" if n_zones is None else f"(n_intervals,) or ({n_zones}, n_intervals): a series per zone of the ascending zone list"
            raise ValueError(f"bands: the observations of {v!r} have shape {a.shape} ({want})")
        if a.shape[-1] == 0:
            raise ValueError(f"bands: the observations of {v!r} are empty (at least one interval)")
        series[v] = a.astype(np.float64)
    out = np.full((len(names),) + (() if n_zones is None else (int(n_zones),)) + (max(a.shape[-1] for a in series.values()),), np.nan)
    for j, v in enumerate(names):
        if v in series:
            out[j, ..., :series[v].shape[-1]] = series[v]
    return out


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
    b._obs = check_observations(b.observations, names, None if b._ids is None else b._ids.size) if b.observations else None
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
        if b._obs is None and held.get("request_observations") is not None:   # (likewise)
            raise RuntimeError(f"bands: resume = True, but the restart file {b._restart_file} was written with observations = an array of shape "
                               f"{np.asarray(held['request_observations']).shape} and this run asks for observations = {{}}: a resumed observer takes "
                               "the same request")
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
    if b._obs is not None:
        state.backend_context.bands_observations(b._obs, first_index=b._first_index())
    b._begin()
    b._hdr, b._values, b._counts, b._wsum, b._pairs = [], [], [], [], []
    if held is not None:
        rows = int(held["scalars"][1])
        state.backend_context.bands_restore(held["acc"], rows)
        b._read = rows   # (the rows before it are in the interrupted run's file)
    b._path = claim_output_file(b, state, "bands")


def close(state):
    state.bands.close(state)
