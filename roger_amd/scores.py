"""Scores against observed series: one goodness-of-fit number per column -- bias, RMSE, r, NSE and KGE maps of simulated against
observed interval values -- from four per-column moments that stay on the device (include/roger_hip.h, rh_scores_*; k_scores in
roger_amd/csrc/rh_scores.h).  The workload is the parameter study: every column is one parameter set of the same plot and all of them
are compared with one lysimeter or soil-moisture record (or each with the record of its own series).

A setup script fills `state.scores` in `set_diagnostics`:

    state.scores.observations = {"q_ss": obs, "theta_rz": obs2}   # (n_intervals,) or (n_series, n_intervals); NaN: missing
    state.scores.aggregation  = {"theta_rz": "last"}              # default: "sum" for the names diagnostics._UNITS gives "mm/dt", else "last"
    state.scores.frequency    = 24 * 60 * 60                      # or 3600, 600
    state.scores.start        = 0                                 # seconds: observation k belongs to (start + k f, start + (k + 1) f]
    state.scores.series       = None                              # or int (nx, ny) over the GLOBAL interior, < 0: column not scored
    state.scores.base_output_path = ...                           # as for the diagnostics

and gets `<identifier>.scores.nc` at the end of the run: dimensions x, y and interval; `closed(interval)` is 1 for the intervals a step
closed while they were scored; per variable v, each (y, x): the raw moments `v_sum_sim`, `v_sum_sim2`, `v_sum_simobs`, `v_sse`, the count
`v_n` and the metrics `v_bias`, `v_rmse`, `v_r`, `v_nse`, `v_kge`.  `state.scores.read()` synchronises and returns the same maps at any
time.  With several ranks a rank writes one file of its own for its block, named as the diagnostics name theirs.

The device rule.  After a step over (t0, t1], with f the frequency: a "sum" variable is accumulated as the output accumulators
accumulate a rate (the first step of an interval overwrites, every other adds), a "last" variable is taken at the interval's end.  A
step with t1 on a boundary (and no longer than f) closes interval k = (t1 - t_first) / f - 1; if 0 <= k < n_intervals and the
observation o of the column's series is not NaN, the interval value s goes into  m1 += s, m2 += s * s, m3 += s * o, m4 += (s - o)^2,
one IEEE operation each, in this order.  Nothing leaves the device between steps.

The derivation.  The scored set of a series is: closed[k] and o[k] not NaN.  n, So = sum o and Soo = sum o^2 are formed on the host over
that set in increasing k with plain sequential additions (not numpy.sum, whose pairwise order differs).  Then

    mu_s = m1 / n, mu_o = So / n,  var_s = m2 / n - mu_s^2,  var_o = Soo / n - mu_o^2,  cov = m3 / n - mu_s mu_o
    r = cov / sqrt(var_s var_o),  alpha = sqrt(var_s / var_o),  beta = mu_s / mu_o
    KGE = 1 - sqrt((r - 1)^2 + (alpha - 1)^2 + (beta - 1)^2),  NSE = 1 - m4 / (n var_o),  RMSE = sqrt(m4 / n),  bias = mu_s - mu_o

`_FillValue` stands where the column is not scored, where n < 2, or where a denominator is zero.

Start and restart.  `start` is a multiple of `frequency`.  If the model's clock is past `start` when the run begins -- after a restart --
the next interval boundary becomes interval 0 and the observations before it are dropped.  Without `resume` the moments are not part
of restart files: a continued run scores from where it continues.

Resuming.  With `state.scores.resume = True` every restart file that is written (restart_frequency, and at the end of run()) holds the
group "hip_scores": the moments, the closed flags, the start of interval 0 and the request.  A run that reads such a file with
`resume = True` and the same request -- variables and kinds, frequency, start, the observations' shape, the series map, the grid --
configures the device with the stored start of interval 0, drops no observation and uploads the moments: its `<identifier>.scores.nc`
equals the uninterrupted run's bit for bit, `closed` included.  A different request is a RuntimeError that names the first difference; a
restart file without the group too (set `resume = False` to score from where the run continues).  One rank only: `initialize` refuses
`resume = True` with several ranks (restart files are gathered to rank 0, the moments are not)."""
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, Observer, carried_group, check_map_shape, check_planes, check_resume, check_same_request, claim_output_file,
                        global_attributes, local_mask, map_array, names_array, request_group, svat_only, write_file, xy_variables)

MAX_VARIABLES = 16                # roger_amd/csrc/rh_scores.h: RH_SCORES_MAX_ITEMS
MAX_SERIES = 1024                 # include/roger_hip.h: RH_SCORES_MAX_SERIES
FREQUENCIES = (DAY, 3600, 600)    # the step classes
KINDS = {"sum": 0, "last": 1}
FILL = 9.969209968386869e36       # netCDF's default _FillValue of a double
MOMENTS = ("sum_sim", "sum_sim2", "sum_simobs", "sse")
METRICS = ("bias", "rmse", "r", "nse", "kge")


def sequential_sum(values, counted):
    """Sum of values[..., k] over the counted k in increasing k by plain sequential additions from +0.0 (numpy's accumulate is
    sequential; an uncounted k adds +0.0, which changes no bit of a sum that started at +0.0)."""
    v = np.where(counted, values, 0.0)
    return np.add.accumulate(np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], axis=-1), axis=-1)[..., -1]


def derive(moments, closed, obs, series=None):
    """The maps of ONE variable from its moments (5, n) {acc, m1 ... m4}, the closed flags (K,), its observations (S, K) and the series of
    every column ((n,), < 0: not scored; None: all 0): dict of (n,) arrays -- the raw moments, n (int64) and the metrics, FILL where
    the docstring above says so."""
    moments = np.asarray(moments, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    ncol = moments.shape[1]
    s = np.zeros(ncol, dtype=np.int64) if series is None else np.asarray(series).reshape(-1).astype(np.int64)
    counted = (np.asarray(closed).reshape(-1) != 0)[None, :] & ~np.isnan(obs)
    n_s = counted.sum(axis=1)
    so_s = sequential_sum(obs, counted)
    soo_s = sequential_sum(obs * obs, counted)
    scored = s >= 0
    pick = np.where(scored, s, 0)
    n = np.where(scored, n_s[pick], 0).astype(np.int64)
    so, soo = so_s[pick], soo_s[pick]
    return metrics(moments[1], moments[2], moments[3], moments[4], n, so, soo, scored)


def metrics(m1, m2, m3, m4, n, so, soo, scored):
    """The raw moments, n and the metrics of the docstring above from per-column m1 ... m4, n (int64), So, Soo and the scored flags,
    (ncol,) each: what `derive` returns.  roger_amd/sas_scores.py derives its maps through it with per-column n, So and Soo."""
    ok = scored & (n >= 2)
    out = {key: np.where(scored, m, FILL) for key, m in zip(MOMENTS, (m1, m2, m3, m4))}
    out["n"] = n
    with np.errstate(all="ignore"):
        nf = np.where(ok, n, 1).astype(np.float64)
        mu_s, mu_o = m1 / nf, so / nf
        var_s, var_o = m2 / nf - mu_s * mu_s, soo / nf - mu_o * mu_o
        cov = m3 / nf - mu_s * mu_o
        r = cov / np.sqrt(var_s * var_o)
        alpha = np.sqrt(var_s / var_o)
        beta = mu_s / mu_o
        kge = 1.0 - np.sqrt((r - 1.0) * (r - 1.0) + (alpha - 1.0) * (alpha - 1.0) + (beta - 1.0) * (beta - 1.0))
        nse = 1.0 - m4 / (nf * var_o)
        rmse = np.sqrt(m4 / nf)
        bias = mu_s - mu_o
        has_var_o = ok & (var_o > 0)
        has_r = has_var_o & (var_s * var_o > 0)
    out["bias"] = np.where(ok, bias, FILL)
    out["rmse"] = np.where(ok, rmse, FILL)
    out["r"] = np.where(has_r, r, FILL)
    out["nse"] = np.where(has_var_o, nse, FILL)
    out["kge"] = np.where(has_r & (mu_o != 0), kge, FILL)
    return out


METRIC_NAMES = {"bias": "mean simulated minus mean observed", "rmse": "root mean squared error", "r": "Pearson correlation",
                "nse": "Nash-Sutcliffe efficiency", "kge": "Kling-Gupta efficiency (2009)"}


def check_series(what, series, n_series, settings):
    """A series map over the global interior: of the grid's shape, integers, and none beyond the observations' series."""
    m = np.asarray(series)
    check_map_shape(what, "series map", m, settings)
    if m.dtype.kind not in "iub":
        raise ValueError(f"{what}: the series map holds {m.dtype} values (an integer series index per column, < 0: not scored)")
    if int(m.max()) >= n_series:
        raise ValueError(f"{what}: the series map names series {int(m.max())}, the observations hold {n_series} (0 ... {n_series - 1})")
    return m


def map_variables(variables, maps, items, keys, long_names, series, shape):
    """Into `variables` the (y, x) maps of a scores file: the series of every column (where a map was given), then per item
    (name, variable, kind sentence) its moments, count and metrics `keys`."""
    from .diagnostics import _UNITS

    if series is not None:
        variables["series"] = (("y", "x"), np.ascontiguousarray(series.reshape(shape).T.astype(np.int32)),
                               {"long_name": "series of the column (< 0: not scored)", "units": ""})
    for name, v, kind in items:
        for key in keys:
            attrs = {"long_name": f"{v} ({kind}): {long_names[key]}", "units": _UNITS.get(v, "") if key in ("bias", "rmse") else ""}
            if key != "n":
                attrs["_FillValue"] = np.float64(FILL)
            variables[f"{name}_{key}"] = (("y", "x"), np.ascontiguousarray(maps[f"{name}_{key}"].T), attrs)


class Scores(Observer):
    """`state.scores`: what the script sets (observations, aggregation, frequency, start, series, base_output_path, resume)."""

    group = "hip_scores"

    def __init__(self):
        self.observations = {}
        self.aggregation = {}
        self.frequency = DAY
        self.start = 0
        self.series = None
        self.base_output_path = None
        self.output_path = "{identifier}.scores.nc"
        self._state = None
        self._on = False         # start() configured the device (this rank holds at least one scored column)
        self._names = []
        self._kinds = []
        self._obs = None         # (n_items, n_series, n_intervals) float64 as validated, from `start` on
        self._local = None       # the series of every column of this rank's block, or None
        self._t_first = 0        # the start of interval 0 on the device
        self._dropped = 0        # observations before it
        self._shape = (0, 0)     # (n_series, n_intervals) of the observations as the script gave them
        self._path = None

    @property
    def active(self):
        return bool(self.observations)

    def read(self):
        """Synchronise and return {"closed": (n_intervals,) uint8, "<v>_<map>": (nx, ny) of this rank's block}; None while nothing is
        configured on this rank."""
        if not self._on:
            return None
        return _maps(self._state)

    def _request(self, state):
        """What a resumed run must ask for again (observers.check_same_request)."""
        return {"variables": names_array(self._names), "kinds": np.asarray(self._kinds, dtype=np.int64), "frequency": np.int64(self.frequency),
                "start": np.int64(self.start), "observations_shape": np.asarray(self._shape, dtype=np.int64),
                "series": map_array(self.series, np.int32), "grid": np.asarray([state.settings.nx, state.settings.ny], dtype=np.int64)}

    def restart_state(self, state):
        """The group "hip_scores" of a restart file: the moments, the closed flags, the start of interval 0 and the request."""
        if not self._on:
            return None
        moments, closed = state.backend_context.scores_read()
        return dict(request_group(self._request(state)), moments=np.asarray(moments, dtype=np.float64), closed=np.asarray(closed, dtype=np.uint8),
                    t_first=np.int64(self._t_first))

    def close(self, state):
        """End of run(): the file."""
        if not self._on or not self._path:
            return
        settings = state.settings
        maps = _maps(state)
        x, y, variables = xy_variables(state.variables)
        f = int(self.frequency)
        ends = (self._t_first + (np.arange(len(maps["closed"]), dtype=np.float64) + 1.0) * f) / float(DAY)
        variables["interval"] = (("interval",), ends, {"long_name": "end of the observation interval", "units": "days", "time_origin": str(settings.time_origin)})
        variables["closed"] = (("interval",), maps["closed"].astype(np.int32), {"long_name": "the interval was closed by a step while it was scored", "units": ""})
        long_names = dict(METRIC_NAMES, sum_sim="sum of the simulated interval values", sum_sim2="sum of their squares",
                          sum_simobs="sum of simulated times observed", sse="sum of squared errors", n="scored intervals")
        kinds = ("sum over the interval", "value at the end of the interval")
        map_variables(variables, maps, [(v, v, kinds[k]) for v, k in zip(self._names, self._kinds)], MOMENTS + ("n",) + METRICS, long_names,
                      self._local, (len(x), len(y)))
        write_file(self._path, {"x": len(x), "y": len(y), "interval": len(ends)}, variables, global_attributes(
            settings.identifier, "Moments of simulated against observed interval values per column and the metrics derived from them.",
            {"frequency_seconds": int(f), "first_interval_starts_seconds": int(self._t_first), "observations_dropped": int(self._dropped)}))


def default_kind(name):
    from .diagnostics import _UNITS

    return "sum" if _UNITS.get(name) == "mm/dt" else "last"


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`, once the clock is known."""
    s = state.scores
    s._state = state
    if not s.active:
        return
    settings = state.settings
    check_resume("scores", s)
    svat_only("scores", settings, " and scores its tracers against bulk samples over windows of days through state.transport_scores "
              "(roger_amd/sas_scores.py); the moments of state.scores belong to the SVAT / oneD step")
    names = list(s.observations)
    if len(names) > MAX_VARIABLES:
        raise ValueError(f"scores: {len(names)} variables (at most {MAX_VARIABLES})")
    if int(s.frequency) not in FREQUENCIES:
        raise ValueError(f"scores: frequency = {s.frequency} s (the observation interval is a day, an hour or ten minutes: the step classes)")
    f = int(s.frequency)
    if int(s.start) < 0 or int(s.start) % f:
        raise ValueError(f"scores: start = {s.start} s is not a multiple of the frequency ({f} s)")
    for v in s.aggregation:
        if v not in s.observations:
            raise ValueError(f"scores: aggregation names {v!r}, which has no observations")
        if s.aggregation[v] not in KINDS:
            raise ValueError(f'scores: aggregation of {v!r} is {s.aggregation[v]!r} ("sum" or "last")')
    obs = []
    for v in names:
        check_planes("scores", (v,), state)
        o = np.asarray(s.observations[v], dtype=np.float64)
        if o.ndim not in (1, 2) or not o.size:
            raise ValueError(f"scores: the observations of {v!r} have shape {o.shape} ((n_intervals,) or (n_series, n_intervals))")
        obs.append(o.reshape(1, -1) if o.ndim == 1 else o)
    if any(o.shape != obs[0].shape for o in obs):
        raise ValueError("scores: the observations have shapes " + ", ".join(str(o.shape) for o in obs) + " (one (n_series, n_intervals) for all variables)")
    n_series = obs[0].shape[0]
    if n_series > MAX_SERIES:
        raise ValueError(f"scores: {n_series} series (at most {MAX_SERIES})")
    if s.series is not None:
        check_series("scores", s.series, n_series, settings)
    s._names = names
    s._kinds = [KINDS[s.aggregation.get(v, default_kind(v))] for v in names]
    s._obs = np.ascontiguousarray(np.stack(obs))
    s._shape = tuple(s._obs.shape[1:])


def start(state):
    """Configure the device (after the restart file was read: the clock is known).  Interval 0 starts at `start`, or at the next
    boundary if the clock is past it; the observations before it are dropped.  A resumed run (`resume`, and the restart file holds
    "hip_scores") takes the stored start of interval 0 instead and the moments with it."""
    from . import runtime_state

    s = state.scores
    if not s.active or s._obs is None:
        return
    settings, vs = state.settings, state.variables
    f, now = int(s.frequency), int(vs.time)
    t_first = int(s.start) if now <= int(s.start) else -(-now // f) * f
    held = carried_group("scores", s)
    if held is not None:
        check_same_request("scores", s, held, s._request(state))
        boundary, t_first = max(t_first, int(held["t_first"])), int(held["t_first"])
    s._t_first, s._dropped = t_first, (t_first - int(s.start)) // f
    s._local = None
    if s.series is not None:
        s._local = local_mask(np.asarray(s.series).astype(np.int32), settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        if not (s._local >= 0).any():
            return   # (several ranks: no scored column in this rank's block)
    if s._dropped >= s._obs.shape[2]:
        return       # (a continued run beyond the last observation)
    s._obs = np.ascontiguousarray(s._obs[:, :, s._dropped:])
    vs.flush_to_device()
    if held is not None:
        # rh_scores_configure takes no start of interval 0 behind the clock: any boundary it accepts, then the stored one with the moments
        state.backend_context.scores_configure(s._names, s._kinds, s._obs, s._local, f, boundary)
        state.backend_context.scores_restore(held["moments"], held["closed"], t_first)
    else:
        state.backend_context.scores_configure(s._names, s._kinds, s._obs, s._local, f, t_first)
    s._on = True
    s._path = claim_output_file(s, state, "scores")


def close(state):
    state.scores.close(state)


def _maps(state):
    s = state.scores
    moments, closed = state.backend_context.scores_read()
    nxl, nyl = state.settings.nx // rs.num_proc[0], state.settings.ny // rs.num_proc[1]
    out = {"closed": np.asarray(closed, dtype=np.uint8)}
    for j, v in enumerate(s._names):
        for key, a in derive(moments[j], closed, s._obs[j], s._local).items():
            out[f"{v}_{key}"] = a.reshape(nxl, nyl)
    return out
