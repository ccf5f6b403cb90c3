"""Scores of the offline transport model against observed tracer samples: one goodness-of-fit number per column -- bias, RMSE, r, NSE and
KGE maps of simulated against observed samples -- from per-column moments that stay on the device (include/roger_hip_sas.h,
rh_sas_scores_*; k_sas_scores in roger_amd/csrc/rh_sas_scores.h).  The sibling of roger_amd/scores.py, which belongs to the SVAT / oneD
step.  The workload is the SAS parameter study: the parameters cannot be measured, so every column is one draw of the same plot, and
each draw is judged against delta-18O, delta-2H, bromide or chloride measured in a lysimeter's percolate.

A setup script fills `state.transport_scores` in `set_diagnostics`:

    state.transport_scores.observations = {("C_iso_q_ss", "q_ss"): obs, "C_iso_rz": obs2}   # value or (value, weight); (K,) or (n_series, K); NaN: missing
    state.transport_scores.aggregation  = {"C_iso_rz": "last"}     # default: "bulk" with a weight, "mean" without
    state.transport_scores.windows      = (first, last)            # int (K,) each: model days (itt of the step), inclusive
    state.transport_scores.series       = None                     # or int (nx, ny) over the GLOBAL interior, < 0: column not scored
    state.transport_scores.base_output_path = ...                  # as for the diagnostics

and gets `<identifier>.transport_scores.nc` at the end of the run: dimensions x, y and sample; `window_first(sample)`,
`window_last(sample)`, `closed(sample)` -- 1 for the windows whose last day was stepped while they were open; per item, named `<v>` or
`<v>_by_<w>`, each (y, x): the raw moments `_sum_sim`, `_sum_sim2`, `_sum_simobs`, `_sse`, `_sum_obs`, `_sum_obs2`, the count `_n` and the
metrics `_bias`, `_rmse`, `_r`, `_nse`, `_kge`.  `state.transport_scores.read()` synchronises and returns the same maps at any time.

Samples are BULK samples over irregular windows -- a weekly or fortnightly bottle, a gap of a month.  What is compared with sample k
is, per kind:  "bulk" the flux-weighted mean over the window's days, sum(w v) / sum(w) over the days with w > 0 and v not NaN;  "mean"
the same with w = 1;  "last" the value on the window's last day.  The per-cell concentrations are NaN wherever the day's flux is zero,
so a window may hold water for one column and none for its neighbour: a sample counts for a column only where it has a simulated
value, and n, So = sum o and Soo = sum o^2 are per-column moments beside the four of roger_amd/scores.py.  The derivation is
`scores.metrics` -- the formulas and the `_FillValue` rules of roger_amd/scores.py (n < 2, a zero denominator, a column not scored).

The life cycle is that of roger_amd/sas_totals.py: nothing is scored during the warm-up runs; once `warmup()` has set `warmup_done` --
or `setup()` has read a restart file of a warmed-up run -- the device is configured.  The context counts the days it scores from 0;
the step that follows carries itt + 1, so model day d is day d - (itt + 1) of that count.  A window that began before that step is
dropped (`observations_dropped` in the file): its first days were not seen.  Nothing is drained per step; `close` writes the file.  The
moments are NOT part of restart files: a continued run scores from where it continues.  With several ranks a rank writes one file of
its own for its block, named as the diagnostics name theirs."""
import numpy as np

from . import runtime_settings as rs
from ._native import DAILY_INPUTS, SAS_SCORES_KINDS, totals_item_name
from .observers import Observer, claim_output_file, global_attributes, local_mask, write_file, xy_variables
from .scores import FILL, METRIC_NAMES, METRICS, MOMENTS, check_series, map_variables, metrics

MAX_ITEMS = 16                    # include/roger_hip_sas.h: RH_SAS_SCORES_MAX_ITEMS
MAX_SERIES = 1024                 # RH_SAS_SCORES_MAX_SERIES
OBS_MOMENTS = ("sum_obs", "sum_obs2")


def derive(moments, series=None):
    """The maps of ONE item from its moments (9, n) {num, den, n, m1, m2, m3, m4, so, soo} and the series of every column ((n,), < 0: not
    scored; None: all scored): dict of (n,) arrays -- the raw moments, n (int64) and the metrics, FILL as roger_amd/scores.py says."""
    m = np.asarray(moments, dtype=np.float64)
    scored = np.ones(m.shape[1], dtype=bool) if series is None else np.asarray(series).reshape(-1) >= 0
    n = np.where(scored, m[2], 0).astype(np.int64)
    out = metrics(m[3], m[4], m[5], m[6], n, m[7], m[8], scored)
    out.update({key: np.where(scored, a, FILL) for key, a in zip(OBS_MOMENTS, (m[7], m[8]))})
    return out


class TransportScores(Observer):
    """`state.transport_scores`: what the script sets (observations, aggregation, windows, series, base_output_path)."""

    def __init__(self):
        self.observations = {}
        self.aggregation = {}
        self.windows = None
        self.series = None
        self.base_output_path = None
        self.output_path = "{identifier}.transport_scores.nc"
        self._state = None
        self._on = False         # start() configured the device (this rank holds at least one scored column)
        self._items = []         # [(value, weight or None, kind)] as the script's names
        self._obs = None         # (n_items, n_series, K) float64 as validated; from `start` on the windows kept
        self._first = None       # model days, int64 (K,); from `start` on the windows kept
        self._last = None
        self._local = None       # the series of every column of this rank's block, or None
        self._day0 = 0           # the model day that is day 0 of the context's count
        self._dropped = 0        # windows that began before it
        self._path = None

    @property
    def active(self):
        return bool(self.observations)

    def close(self, state):
        """End of run(): the file."""
        if self._on and self._path:
            _write(self, state)

    def read(self):
        """Synchronise and return {"closed": (K,) uint8, "<item>_<map>": (nx, ny) of this rank's block}; None while nothing is
        configured on this rank."""
        if not self._on:
            return None
        return _maps(self._state)


def _key(k):
    if isinstance(k, str):
        return k, None
    if isinstance(k, (tuple, list)) and len(k) == 2 and all(isinstance(s, str) for s in k):
        return k[0], k[1]
    raise ValueError(f"transport_scores: {k!r} is neither a variable's name nor a pair (value, weight)")


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`."""
    s = state.transport_scores
    s._state = state
    if not s.active:
        return
    settings = state.settings
    if not settings.enable_offline_transport:
        raise NotImplementedError("transport_scores: the scores of the offline transport model against samples over windows of days; "
                                  "the SVAT / oneD step scores through state.scores")
    keys = [_key(k) for k in s.observations]
    if len(keys) > MAX_ITEMS:
        raise ValueError(f"transport_scores: {len(keys)} items (at most {MAX_ITEMS})")
    agg = {_key(k): a for k, a in s.aggregation.items()}
    for k, a in agg.items():
        if k not in keys:
            raise ValueError(f"transport_scores: aggregation names {totals_item_name(*k)!r}, which has no observations")
        if a not in SAS_SCORES_KINDS:
            raise ValueError(f'transport_scores: aggregation of {totals_item_name(*k)!r} is {a!r} ("bulk", "mean" or "last")')
    items, obs = [], []
    for (v, w), o in zip(keys, s.observations.values()):
        meta = state.var_meta.get(v)
        dims = None if meta is None or meta.dims is None else tuple(meta.dims)
        if dims is not None and len(dims) > 2 and dims[-1] in ("ages", "nages"):
            raise NotImplementedError(f"transport_scores: {v!r} is age-resolved (a sample is compared with one value per column)")
        if meta is None or dims not in (("x", "y"), ("x", "y", "timesteps")) or meta.dtype is not None or meta.sas is None:
            raise NotImplementedError(f"transport_scores: {v!r} is not a float64 per-cell variable of the transport step")
        if meta.sas in DAILY_INPUTS:
            raise NotImplementedError(f"transport_scores: {v!r} is a daily input of the transport step, not a result (it can be a weight)")
        if w is not None:
            wmeta = state.var_meta.get(w)
            if wmeta is None or wmeta.sas not in DAILY_INPUTS or wmeta.sas == "C_in":
                raise NotImplementedError(f"transport_scores: the weight {w!r} of {v!r} is not a daily flux input "
                                          f"({', '.join(d for d in DAILY_INPUTS if d != 'C_in')})")
        kind = agg.get((v, w), "bulk" if w is not None else "mean")
        if kind == "bulk" and w is None:
            raise ValueError(f'transport_scores: {v!r} is aggregated as "bulk" and has no weight (give (value, weight))')
        if kind != "bulk" and w is not None:
            raise ValueError(f'transport_scores: {totals_item_name(v, w)!r} is aggregated as "{kind}" and has a weight (only "bulk" takes one)')
        o = np.asarray(o, dtype=np.float64)
        if o.ndim not in (1, 2) or not o.size:
            raise ValueError(f"transport_scores: the observations of {totals_item_name(v, w)!r} have shape {o.shape} ((K,) or (n_series, K))")
        items.append((v, w, kind))
        obs.append(o.reshape(1, -1) if o.ndim == 1 else o)
    if any(o.shape != obs[0].shape for o in obs):
        raise ValueError("transport_scores: the observations have shapes " + ", ".join(str(o.shape) for o in obs) + " (one (n_series, K) for all items)")
    n_series, K = obs[0].shape
    if n_series > MAX_SERIES:
        raise ValueError(f"transport_scores: {n_series} series (at most {MAX_SERIES})")
    if s.windows is None or len(s.windows) != 2:
        raise ValueError("transport_scores: windows = (first, last), the first and the last model day of every sample")
    first, last = (np.asarray(a) for a in s.windows)
    if first.dtype.kind not in "iu" or last.dtype.kind not in "iu" or first.shape != (K,) or last.shape != (K,):
        raise ValueError(f"transport_scores: the windows have shapes {first.shape} and {last.shape} of {first.dtype} and {last.dtype} "
                         f"(two integer arrays ({K},), as the observations hold {K} samples)")
    first, last = first.astype(np.int64), last.astype(np.int64)
    for k in range(K):
        if first[k] > last[k]:
            raise ValueError(f"transport_scores: window {k} is [{first[k]}, {last[k]}]: its last day lies before its first")
        if k and first[k] <= last[k - 1]:
            raise ValueError(f"transport_scores: window {k} starts on day {first[k]}, window {k - 1} ends on day {last[k - 1]} "
                             "(windows are in increasing order and do not overlap)")
    if s.series is not None:
        if int(check_series("transport_scores", s.series, n_series, settings).max()) < 0:
            raise ValueError("transport_scores: the series map scores no column")
    s._items, s._obs, s._first, s._last = items, np.ascontiguousarray(np.stack(obs)), first, last


def start(state):
    """The run proper begins (warmup() is through, or a restart file of a warmed-up run was read): configure the device.  The next
    step is day 0 of the context's count; the windows that began before it are dropped.  Called again, it scores anew."""
    from . import runtime_state

    s = state.transport_scores
    if not s.active or s._obs is None or not state.settings.enable_offline_transport:
        return
    settings, vs = state.settings, state.variables
    s._on = False
    s._day0 = int(vs.itt) + 1
    keep = s._first >= s._day0
    s._dropped += int((~keep).sum())
    s._obs, s._first, s._last = np.ascontiguousarray(s._obs[:, :, keep]), s._first[keep], s._last[keep]
    s._local = None
    if s.series is not None:
        s._local = local_mask(np.asarray(s.series).astype(np.int32), settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        if not (s._local >= 0).any():
            return   # (several ranks: no scored column in this rank's block)
    if not s._first.size:
        return       # (a continued run beyond the last sample)
    vs.flush_to_device()
    state.sas_context.scores_configure([(state.var_meta[v].sas, None if w is None else state.var_meta[w].sas, kind) for v, w, kind in s._items],
                                       s._obs, (s._first - s._day0, s._last - s._day0), s._local)
    s._on = True
    s._path = claim_output_file(s, state, "transport scores")


def _maps(state):
    s = state.transport_scores
    moments, closed, _ = state.sas_context.scores_read()
    nxl, nyl = state.settings.nx // rs.num_proc[0], state.settings.ny // rs.num_proc[1]
    out = {"closed": np.asarray(closed, dtype=np.uint8)}
    for j, (v, w, _) in enumerate(s._items):
        for key, a in derive(moments[j], s._local).items():
            out[f"{totals_item_name(v, w)}_{key}"] = a.reshape(nxl, nyl)
    return out


def _write(s, state):
    """End of run(): the file."""
    maps = _maps(state)
    x, y, variables = xy_variables(state.variables)
    variables["window_first"] = (("sample",), s._first.astype(np.int64), {"long_name": "first model day (itt) of the sample's window", "units": ""})
    variables["window_last"] = (("sample",), s._last.astype(np.int64), {"long_name": "last model day (itt) of the sample's window", "units": ""})
    variables["closed"] = (("sample",), maps["closed"].astype(np.int32), {"long_name": "the window's last day was stepped while it was open", "units": ""})
    long_names = dict(METRIC_NAMES, sum_sim="sum of the simulated samples", sum_sim2="sum of their squares", sum_simobs="sum of simulated times observed",
                      sse="sum of squared errors", sum_obs="sum of the observed samples", sum_obs2="sum of their squares", n="counted samples")
    kinds = {"bulk": "mean over the window weighted by {w}", "mean": "mean over the window's days", "last": "value on the window's last day"}
    map_variables(variables, maps, [(totals_item_name(v, w), v, kinds[kind].format(w=w)) for v, w, kind in s._items],
                  MOMENTS + OBS_MOMENTS + ("n",) + METRICS, long_names, s._local, (len(x), len(y)))
    write_file(s._path, {"x": len(x), "y": len(y), "sample": len(s._first)}, variables, global_attributes(
        state.settings.identifier, "Moments of simulated against observed samples per column and the metrics derived from them.",
        {"first_scored_model_day": int(s._day0), "observations_dropped": int(s._dropped)}))
