"""Duration curves: the distribution over time of a variable per column -- the flow duration curve of the percolation or the runoff
(Q5 / Q50 / Q95, the share of days without flow), the days the root zone spent below a stress threshold, the longest dry spell, the
number of saturation episodes -- from a per-column histogram with exact extremes and run lengths that stays on the device
(include/roger_hip.h, rh_durations_*; k_durations in roger_amd/csrc/rh_durations.h).  A few hundred bytes per column instead of
ten-minute output of every column.

A setup script fills `state.durations` in `set_diagnostics`:

    state.durations.variables   = {"q_ss": edges, "theta_rz": edges2}   # ascending finite edges, at most 63; log_edges(lo, hi, n) helps
    state.durations.aggregation = {"theta_rz": "last"}                  # default: "sum" for the names diagnostics._UNITS gives "mm/dt", else "last"
    state.durations.spells      = {"theta_rz": ("below", 0.15)}         # optional, one per variable; or ("at_or_above", x)
    state.durations.frequency   = 24 * 60 * 60                          # or 3600, 600
    state.durations.start       = 0                                     # seconds, a multiple of frequency
    state.durations.mask        = None                                  # or (nx, ny) over the GLOBAL interior, 0: column not counted
    state.durations.quantiles   = (0.05, 0.5, 0.95)
    state.durations.base_output_path = ...                              # as for the diagnostics

and gets `<identifier>.durations.nc` at the end of the run: dimensions x, y, quantile and per variable v `v_edge`, `v_bin`;
`v_edges(v_edge)`, `v_count(v_bin, y, x)` (the NaN bin last), and (y, x) each `v_n` (the sum of the finite bins), `v_nan`, `v_min`,
`v_max`; `v_exceed(v_edge, y, x)`, the share of v_n with a value >= the edge; `v_q(quantile, y, x)`; for a variable with a spell
`v_longest`, `v_spells` and `v_run` (the run under way at the end).  A variable without edges has one finite bin and neither `v_edges`
nor `v_exceed`.  `state.durations.read()` synchronises and returns the same maps at any time.  With several ranks a rank writes one
file of its own for its block, named as the diagnostics name theirs.

The device rule.  After a step over (t0, t1], with f the frequency: a "sum" variable is accumulated as the output accumulators
accumulate a rate (the first step of an interval overwrites, every other adds), a "last" variable is taken at the interval's end.  A
step with t1 on a boundary (and no longer than f) closes interval k = (t1 - t_first) / f - 1; if k >= 0 the interval value s is counted:
bin #{q : e_q <= s} of the variable's edges gains 1 (a value on an edge goes to the upper bin; a NaN goes to the NaN bin), the extremes
take it (min = s < min ? s : min, max likewise, from +inf / -inf), and a spell advances: in = s < x ("below") or s >= x
("at_or_above"), run = in ? run + 1 : 0, a run that reaches 1 is one more spell, longest = max(longest, run).  Counters are uint32.
Spells run over consecutive COUNTED intervals: an hourly or ten-minute interval under a longer step (a dry day the model takes in one
step) is never started -- it is neither counted nor does it break a run.  Nothing leaves the device between steps.

The quantile rule (`derive`).  Over the finite bins 0 ... m (m edges) take the smallest b whose cumulative count reaches p * v_n;
p = 0 is v_min and p = 1 is v_max.  Otherwise interpolate linearly inside [lo, hi] by the fraction of the bin's count that is needed,
(p * v_n - cumulative count below b) / count of b: lo is e_{b-1}, or v_min for bin 0, and never below v_min; hi is e_b, or v_max for
the last bin, and never above v_max.  `_FillValue` stands where v_n == 0 (min, max, exceed and the quantiles).

Start and restart.  `start` is a multiple of `frequency`.  If the model's clock is past `start` when the run begins -- after a restart
-- the next interval boundary starts the first counted interval.  Without `resume` the counters are not part of restart files: a
continued run counts from where it continues.

Resuming.  With `state.durations.resume = True` every restart file that is written holds the group "hip_durations": the counters, the
float planes (the interval's sum under way, the extremes), the spell planes (the run under way, the longest, the number), the start of the
first counted interval and the request.  A run that reads such a file with `resume = True` and the same request -- variables and kinds,
frequency, start, edges, spells, mask, grid -- configures the device with the stored start and uploads the state: its
`<identifier>.durations.nc` equals the uninterrupted run's bit for bit.  A different request is a RuntimeError that names the first
difference; a restart file without the group too (set `resume = False` to count from where the run continues).  One rank only:
`initialize` refuses `resume = True` with several ranks (restart files are gathered to rank 0, the counters are not)."""
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, Observer, carried_group, check_mask, check_planes, check_resume, check_same_request, claim_output_file,
                        global_attributes, local_mask, map_array, names_array, request_group, svat_only, write_file, xy_variables)
from .scores import FILL, default_kind

MAX_VARIABLES = 16                # roger_amd/csrc/rh_durations.h: RH_DURATIONS_MAX_ITEMS
MAX_EDGES = 63                    # ... RH_DURATIONS_MAX_EDGES
FREQUENCIES = (DAY, 3600, 600)    # the step classes
KINDS = {"sum": 0, "last": 1}
SIDES = {"below": 0, "at_or_above": 1}


def log_edges(lo, hi, n):
    """n edges from lo to hi (both positive) at equal ratios."""
    if not (0 < lo < hi) or int(n) < 2:
        raise ValueError(f"log_edges: 0 < lo < hi and n >= 2 (lo = {lo}, hi = {hi}, n = {n})")
    return np.geomspace(float(lo), float(hi), int(n))


def derive(counts, vals, edges, quantiles=(), spells=None):
    """The maps of ONE variable from its counts (m + 2, n), its float planes (3, n) {acc, min, max}, its m edges and, with a spell, its
    spell planes (3, n) {run, longest, n_spells}: dict of arrays -- count (m + 2, n), n and nan (n,) int64, min and max (n,),
    exceed (m, n), q (len(quantiles), n), and longest, spells, run (n,) int64 -- by the rules of the docstring above."""
    counts = np.asarray(counts).astype(np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    m, ncol = e.size, counts.shape[1]
    assert counts.shape[0] == m + 2
    finite = counts[:m + 1]
    n = finite.sum(axis=0)
    have = n > 0
    vmin, vmax = vals[1], vals[2]
    out = {"count": counts, "n": n, "nan": counts[m + 1].copy(), "min": np.where(have, vmin, FILL), "max": np.where(have, vmax, FILL)}
    nf = np.where(have, n, 1).astype(np.float64)
    above = np.cumsum(finite[::-1], axis=0)[::-1]                   # above[b]: the count of the bins b ... m
    out["exceed"] = np.where(have[None, :], above[1:] / nf[None, :], FILL)
    cum = np.cumsum(finite, axis=0)
    q = np.full((len(quantiles), ncol), FILL)
    cols = np.arange(ncol)
    with np.errstate(all="ignore"):
        for iq, p in enumerate(quantiles):
            p = float(p)
            if p <= 0.0 or p >= 1.0:
                q[iq] = np.where(have, vmin if p <= 0.0 else vmax, FILL)
                continue
            target = p * n.astype(np.float64)
            b = np.minimum((cum < target[None, :]).sum(axis=0), m)  # the smallest bin whose cumulative count reaches the target
            below = np.where(b > 0, cum[np.maximum(b - 1, 0), cols], 0).astype(np.float64)
            inside = np.where(have, finite[b, cols], 1).astype(np.float64)
            lo = np.where(b > 0, e[np.maximum(b - 1, 0)] if m else vmin, vmin)
            hi = np.where(b < m, e[np.minimum(b, m - 1)] if m else vmax, vmax)
            lo, hi = np.maximum(lo, vmin), np.minimum(hi, vmax)
            q[iq] = np.where(have, lo + (target - below) / inside * (hi - lo), FILL)
    out["q"] = q
    if spells is not None:
        sp = np.asarray(spells).astype(np.int64)
        out["run"], out["longest"], out["spells"] = sp[0], sp[1], sp[2]
    return out


class Durations(Observer):
    """`state.durations`: what the script sets (variables, aggregation, spells, frequency, start, mask, quantiles, base_output_path,
    resume)."""

    group = "hip_durations"

    def __init__(self):
        self.variables = {}
        self.aggregation = {}
        self.spells = {}
        self.frequency = DAY
        self.start = 0
        self.mask = None
        self.quantiles = (0.05, 0.5, 0.95)
        self.base_output_path = None
        self.output_path = "{identifier}.durations.nc"
        self._state = None
        self._on = False         # start() configured the device (this rank holds at least one counted column)
        self._names = []
        self._kinds = []
        self._edges = []
        self._spells = []        # per variable None or (side, threshold)
        self._local = None       # the mask of this rank's block, or None
        self._t_first = 0        # the start of the first counted interval on the device
        self._path = None

    @property
    def active(self):
        return bool(self.variables)

    def read(self):
        """Synchronise and return {"<v>_<map>": array over this rank's block, (nx, ny) last}; None while nothing is configured on this
        rank."""
        if not self._on:
            return None
        return _maps(self._state)

    def _request(self, state):
        """What a resumed run must ask for again (observers.check_same_request)."""
        spells = [(-1, np.nan) if sp is None else sp for sp in self._spells]
        return {"variables": names_array(self._names), "kinds": np.asarray(self._kinds, dtype=np.int64), "frequency": np.int64(self.frequency),
                "start": np.int64(self.start), "n_edges": np.asarray([e.size for e in self._edges], dtype=np.int64),
                "edges": np.concatenate(list(self._edges) + [np.zeros(0)]), "sides": np.asarray([sp[0] for sp in spells], dtype=np.int64),
                "thresholds": np.asarray([sp[1] for sp in spells], dtype=np.float64),
                "mask": map_array(None if self.mask is None else np.asarray(self.mask) != 0, np.uint8),
                "grid": np.asarray([state.settings.nx, state.settings.ny], dtype=np.int64)}

    def restart_state(self, state):
        """The group "hip_durations" of a restart file: the counters (the items' bins one behind the other), the float planes, the spell
        planes, the start of the first counted interval and the request."""
        if not self._on:
            return None
        counts, vals, spells = state.backend_context.durations_read()
        return dict(request_group(self._request(state)), counts=np.concatenate([np.asarray(c, dtype=np.uint32) for c in counts]),
                    values=np.asarray(vals, dtype=np.float64), spells=np.asarray(spells, dtype=np.uint32), t_first=np.int64(self._t_first))

    def close(self, state):
        """End of run(): the file."""
        if not self._on or not self._path:
            return
        from .diagnostics import _UNITS

        maps = _maps(state)
        x, y, variables = xy_variables(state.variables)
        dims = {"x": len(x), "y": len(y), "quantile": len(self._quantiles)}
        variables["quantile"] = (("quantile",), np.asarray(self._quantiles, dtype=np.float64), {"long_name": "non-exceedance probability", "units": ""})
        if self._local is not None:
            variables["mask"] = (("y", "x"), np.ascontiguousarray(self._local.reshape(len(x), len(y)).T.astype(np.int32)),
                                 {"long_name": "the column is counted", "units": ""})
        fill = {"_FillValue": np.float64(FILL)}
        for j, v in enumerate(self._names):
            kind = "sum over the interval" if self._kinds[j] == 0 else "value at the end of the interval"
            unit = _UNITS.get(v, "")
            e = self._edges[j]

            def t(key):   # (..., x, y) -> (..., y, x)
                return np.ascontiguousarray(np.swapaxes(maps[f"{v}_{key}"], -1, -2))

            dims[f"{v}_bin"] = e.size + 2
            variables[f"{v}_count"] = ((f"{v}_bin", "y", "x"), t("count"), {"long_name": f"{v} ({kind}): intervals per bin, bin b holds edge b-1 <= value < edge b, the NaN bin last", "units": ""})
            variables[f"{v}_n"] = (("y", "x"), t("n"), {"long_name": f"{v} ({kind}): counted intervals with a number", "units": ""})
            variables[f"{v}_nan"] = (("y", "x"), t("nan"), {"long_name": f"{v} ({kind}): counted intervals with a NaN", "units": ""})
            variables[f"{v}_min"] = (("y", "x"), t("min"), dict(fill, long_name=f"{v} ({kind}): smallest interval value", units=unit))
            variables[f"{v}_max"] = (("y", "x"), t("max"), dict(fill, long_name=f"{v} ({kind}): largest interval value", units=unit))
            variables[f"{v}_q"] = (("quantile", "y", "x"), t("q"), dict(fill, long_name=f"{v} ({kind}): quantiles of the interval values", units=unit))
            if e.size:
                dims[f"{v}_edge"] = e.size
                variables[f"{v}_edges"] = ((f"{v}_edge",), e, {"long_name": f"{v}: bin edges", "units": unit})
                variables[f"{v}_exceed"] = ((f"{v}_edge", "y", "x"), t("exceed"), dict(fill, long_name=f"{v} ({kind}): share of the intervals at or above the edge", units=""))
            if self._spells[j] is not None:
                side, thr = self._spells[j]
                what = f"{v} ({kind}) {'<' if side == 0 else '>='} {thr!r}"
                variables[f"{v}_longest"] = (("y", "x"), t("longest"), {"long_name": f"longest run of consecutive counted intervals with {what}", "units": ""})
                variables[f"{v}_spells"] = (("y", "x"), t("spells"), {"long_name": f"number of runs with {what}", "units": ""})
                variables[f"{v}_run"] = (("y", "x"), t("run"), {"long_name": f"the run with {what} under way at the end", "units": ""})
        write_file(self._path, dims, variables, global_attributes(
            state.settings.identifier, "Histograms of interval values per column, their extremes, exceedance shares, quantiles and threshold spells.",
            {"frequency_seconds": int(self.frequency), "first_interval_starts_seconds": int(self._t_first)}))


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`, once the clock is known."""
    d = state.durations
    d._state = state
    if not d.active:
        return
    settings = state.settings
    check_resume("durations", d)
    svat_only("durations", settings, " over its own arrays; the histograms of state.durations belong to the SVAT / oneD step (a sibling for "
              "the transport model is not built)")
    names = list(d.variables)
    if len(names) > MAX_VARIABLES:
        raise ValueError(f"durations: {len(names)} variables (at most {MAX_VARIABLES})")
    if int(d.frequency) not in FREQUENCIES:
        raise ValueError(f"durations: frequency = {d.frequency} s (the interval is a day, an hour or ten minutes: the step classes)")
    f = int(d.frequency)
    if int(d.start) < 0 or int(d.start) % f:
        raise ValueError(f"durations: start = {d.start} s is not a multiple of the frequency ({f} s)")
    for v in d.aggregation:
        if v not in d.variables:
            raise ValueError(f"durations: aggregation names {v!r}, which has no edges")
        if d.aggregation[v] not in KINDS:
            raise ValueError(f'durations: aggregation of {v!r} is {d.aggregation[v]!r} ("sum" or "last")')
    spells = {}
    for v, sp in d.spells.items():
        if v not in d.variables:
            raise ValueError(f"durations: spells names {v!r}, which has no edges")
        if not isinstance(sp, (tuple, list)) or len(sp) != 2 or sp[0] not in SIDES:
            raise ValueError(f'durations: the spell of {v!r} is {sp!r} (("below", x) or ("at_or_above", x))')
        if not np.isfinite(float(sp[1])):
            raise ValueError(f"durations: the threshold of {v!r} is {sp[1]!r} (a finite number)")
        spells[v] = (SIDES[sp[0]], float(sp[1]))
    edges = []
    for v in names:
        check_planes("durations", (v,), state)
        e = np.asarray(d.variables[v], dtype=np.float64)
        if e.ndim != 1:
            raise ValueError(f"durations: the edges of {v!r} have shape {e.shape} (one ascending list per variable, shared by all columns)")
        if e.size > MAX_EDGES:
            raise ValueError(f"durations: {e.size} edges for {v!r} (at most {MAX_EDGES})")
        if not np.isfinite(e).all():
            raise ValueError(f"durations: the edges of {v!r} are not all finite")
        if not (np.diff(e) > 0).all():
            raise ValueError(f"durations: the edges of {v!r} are not strictly ascending")
        edges.append(np.ascontiguousarray(e))
    check_mask("durations", d.mask, settings)
    qs = tuple(float(p) for p in d.quantiles)
    if any(not 0.0 <= p <= 1.0 for p in qs):
        raise ValueError(f"durations: quantiles = {tuple(d.quantiles)!r} (each within [0, 1])")
    d._names = names
    d._kinds = [KINDS[d.aggregation.get(v, default_kind(v))] for v in names]
    d._edges = edges
    d._spells = [spells.get(v) for v in names]
    d._quantiles = qs


def start(state):
    """Configure the device (after the restart file was read: the clock is known).  The first counted interval starts at `start`, or
    at the next boundary if the clock is past it.  A resumed run (`resume`, and the restart file holds "hip_durations") takes the stored
    start instead and the counters with it."""
    from . import runtime_state

    d = state.durations
    if not d.active or not d._names:
        return
    settings, vs = state.settings, state.variables
    f, now = int(d.frequency), int(vs.time)
    d._t_first = int(d.start) if now <= int(d.start) else -(-now // f) * f
    held = carried_group("durations", d)
    if held is not None:
        check_same_request("durations", d, held, d._request(state))
        d._t_first = int(held["t_first"])
    d._local = None
    if d.mask is not None:
        d._local = local_mask((np.asarray(d.mask) != 0).astype(np.uint8), settings.nx, settings.ny, rs.num_proc, runtime_state.proc_rank)
        if not d._local.any():
            return   # (several ranks: no counted column in this rank's block)
    vs.flush_to_device()
    state.backend_context.durations_configure(d._names, d._kinds, d._edges, d._spells, d._local, f, d._t_first)
    if held is not None:
        offs = np.concatenate([[0], np.cumsum([e.size + 2 for e in d._edges])]).astype(int)
        state.backend_context.durations_restore([held["counts"][offs[j]:offs[j + 1]] for j in range(len(d._names))], held["values"], held["spells"])
    d._on = True
    d._path = claim_output_file(d, state, "durations")


def _maps(state):
    d = state.durations
    counts, vals, spells = state.backend_context.durations_read()
    nxl, nyl = state.settings.nx // rs.num_proc[0], state.settings.ny // rs.num_proc[1]
    out = {}
    for j, v in enumerate(d._names):
        for key, a in derive(counts[j], vals[j], d._edges[j], d._quantiles, spells[j] if d._spells[j] is not None else None).items():
            out[f"{v}_{key}"] = a.reshape(a.shape[:-1] + (nxl, nyl))
    return out
