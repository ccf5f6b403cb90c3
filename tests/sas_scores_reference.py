"""The scores of the SAS context (rh_sas_scores_*, k_sas_scores in roger_amd/csrc/rh_sas_scores.h) restated on the host in plain numpy:
the host's window clock (`Windows`), one day of the kernel (`score_day`), the two together (`HostSasScores`), the derivation of the maps
(`derive`, which calls the formulas of roger_amd.scores on first use) and the oracle double with the scores_* methods of
`_native.SasContext`.  Importing this module imports nothing from roger_amd.

A sample k is a bulk sample over the days [first_day[k], last_day[k]] of the context's count of scored days.  Column i has
s = series[i] (no map: 0); s < 0 is never touched.  Per item (value, weight, kind), v the value after the day:
    BULK (0): wd = the day's weight;  MEAN (1): wd = 1.0.  On the window's first day num and den restart from +0.0; the day is eligible if
              wd > 0 and v == v: num = num + fl(v * wd), den = den + wd; a day that is not eligible leaves both as they are
    LAST (2): nothing before the closing day
    on the closing day of an open window with o = obs[j, s, k]: BULK / MEAN counted if o == o and den > 0, sim = num / den; LAST counted
    if o == o and v == v, sim = v.  A counted sample, one IEEE operation each, in this order:
        n += 1.0;  m1 += sim;  m2 += sim * sim;  m3 += sim * o;  d = sim - o;  m4 += d * d;  so += o;  soo += o * o
moments (J, 9, n) = {num, den, n, m1, m2, m3, m4, so, soo}.  numpy evaluates `a * b` and `x + y` as separate IEEE operations on float64
arrays, which is the rule.  The `variant` argument of score_day exists for the tests that show the inputs have teeth."""
from fractions import Fraction

import numpy as np

BULK, MEAN, LAST = 0, 1, 2
KINDS = {"bulk": BULK, "mean": MEAN, "last": LAST}
NMOM = 9
MAX_ITEMS, MAX_SERIES = 16, 1024
FLUX_INPUTS = ("inf_mat_rz", "inf_pf_rz", "inf_pf_ss", "evap_soil", "transp", "q_rz", "q_ss", "cpr_rz")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def check_windows(first_day, last_day):
    """The windows as two int64 (K,) arrays, or ValueError: in increasing order, not overlapping, last >= first."""
    first, last = (np.asarray(a).reshape(-1).astype(np.int64) for a in (first_day, last_day))
    if first.size != last.size or not first.size:
        raise ValueError(f"windows: {first.size} first and {last.size} last days (at least one window)")
    for k in range(first.size):
        if first[k] > last[k]:
            raise ValueError(f"window {k} is [{first[k]}, {last[k]}]: its last day lies before its first")
        if k and first[k] <= last[k - 1]:
            raise ValueError(f"window {k} starts on day {first[k]}, window {k - 1} ends on day {last[k - 1]}")
    return first, last


class Windows:
    """The host side of the C library: the count of scored days and which window it stands in.  `next()` advances the count by one day
    and returns None (nothing is launched) or (k, first, closes)."""

    def __init__(self, first_day, last_day):
        self.first, self.last = check_windows(first_day, last_day)
        self.closed = np.zeros(self.first.size, dtype=np.uint8)
        self.days, self.k, self.open = 0, 0, -1

    def next(self):
        t = self.days
        self.days += 1
        while self.k < self.first.size and self.last[self.k] < t:
            self.k += 1
        k = self.k
        if k >= self.first.size or t < self.first[k]:
            return None
        first, closes = bool(t == self.first[k]), bool(t == self.last[k])
        if first:
            self.open = k
        if self.open != k:
            return None                      # (its first day was never scored: never compared)
        if closes:
            self.closed[k] = 1
            self.open = -1
            self.k += 1
        return k, first, closes


def _fused(num, v, wd):
    """num + v * wd rounded once, element by element (the variant the rule excludes)."""
    out = np.empty_like(num)
    for i in range(num.size):
        if not (np.isfinite(num[i]) and np.isfinite(v[i]) and np.isfinite(wd[i])):
            out[i] = num[i] + v[i] * wd[i]
        else:
            out[i] = float(Fraction(float(num[i])) + Fraction(float(v[i])) * Fraction(float(wd[i])))
    return out


def score_day(moments, kinds, values, weights, obs, series, k, first, closes, variant=None):
    """One launch of k_sas_scores: moments (J, 9, n) advanced in place.  values[j] (n,) after the day, weights[j] (n,) the day's row of
    the weight or None, obs (J, S, K), series (n,) int or None.  variant: None (the rule), "fma", "add_zero" or "swap34"."""
    n = moments.shape[2]
    s = np.zeros(n, dtype=np.int64) if series is None else np.asarray(series).reshape(-1).astype(np.int64)
    on = s >= 0
    pick = np.where(on, s, 0)
    p3, p4 = (6, 5) if variant == "swap34" else (5, 6)
    with np.errstate(all="ignore"):
        for j, kind in enumerate(kinds):
            if kind == LAST and not closes:
                continue
            m = moments[j]
            v = np.asarray(values[j], dtype=np.float64).reshape(-1)
            sim, counted = v, v == v
            if kind != LAST:
                wd = np.asarray(weights[j], dtype=np.float64).reshape(-1) if kind == BULK else np.ones(n)
                num, den = (np.zeros(n), np.zeros(n)) if first else (m[0].copy(), m[1].copy())
                e = (wd > 0.0) & (v == v)                      # (NaN > 0 is False)
                t = v * wd                                      # rounded before it is added
                added = _fused(num, v, wd) if variant == "fma" else num + t
                if variant == "add_zero":
                    num, den = num + np.where(e, t, 0.0), den + np.where(e, wd, 0.0)
                else:
                    num, den = np.where(e, added, num), np.where(e, den + wd, den)
                m[0], m[1] = np.where(on, num, m[0]), np.where(on, den, m[1])
                if not closes:
                    continue
                counted = den > 0.0
                sim = num / den
            o = obs[j, pick, k]
            c = on & counted & (o == o)
            d = sim - o
            for plane, term in ((2, np.ones(n)), (3, sim), (4, sim * sim), (p3, sim * o), (p4, d * d), (7, o), (8, o * o)):
                m[plane] = np.where(c, m[plane] + term, m[plane])


class HostSasScores:
    """What a configured context holds: the windows' clock and the moments.  items: [(value, weight or None, kind int)]."""

    def __init__(self, items, obs, windows, n, series=None):
        self.items = [(v, w, int(k)) for v, w, k in items]
        self.obs = np.array(obs, dtype=np.float64)
        assert self.obs.ndim == 3 and self.obs.shape[0] == len(self.items)
        self.win = Windows(*windows)
        assert self.obs.shape[2] == self.win.first.size
        self.series = None if series is None else np.asarray(series).reshape(-1).astype(np.int64)
        self.moments = np.zeros((len(self.items), NMOM, int(n)))

    def add(self, held, weights=None, variant=None):
        """The next day of the count.  held: {name: (n,)} values after the day; weights: {name: (n,)} the day's rows (default: held)."""
        weights = held if weights is None else weights
        now = self.win.next()
        if now is None:
            return
        k, first, closes = now
        score_day(self.moments, [kd for _, _, kd in self.items], [held[v] for v, _, _ in self.items],
                  [None if w is None else np.asarray(weights[w]).reshape(-1) for _, w, _ in self.items], self.obs, self.series, k, first, closes,
                  variant)

    @property
    def closed(self):
        return self.win.closed


def window_samples(days, kind, windows, obs_row=None):
    """The simulated sample of every window of ONE item and one column by a plain two-pass computation, for the derivation's checks:
    days = [(v, wd)] per day of the count.  (K,) float64, NaN where the window has no sample."""
    out = np.full(len(windows[0]), np.nan)
    for k, (a, b) in enumerate(zip(*windows)):
        if a < 0 or b >= len(days):
            continue
        if kind == LAST:
            out[k] = days[b][0]
            continue
        pairs = [(v, w if kind == BULK else 1.0) for v, w in days[a:b + 1]]
        pairs = [(v, w) for v, w in pairs if w > 0 and v == v]
        if pairs and sum(w for _, w in pairs) > 0:
            out[k] = sum(v * w for v, w in pairs) / sum(w for _, w in pairs)
    return out


def derive(moments, series=None):
    """The maps of ONE item from its moments (9, n): roger_amd.sas_scores.derive."""
    from roger_amd.sas_scores import derive as d

    return d(moments, series)


def item_key(value, weight=None):
    return value if weight is None else f"{value}_by_{weight}"


def check_items(items, held):
    """The refusals of rh_sas_scores_configure on [(value, weight, kind)] against the arrays `held` ({name: array}), as ValueError (an
    array the context does not hold: LookupError)."""
    if len(items) > MAX_ITEMS:
        raise ValueError(f"n_items = {len(items)} (0 ... {MAX_ITEMS})")
    for j, (v, w, kind) in enumerate(items):
        if kind not in (BULK, MEAN, LAST):
            raise ValueError(f"kind {kind} of array {v}")
        if (v, w, kind) in items[:j]:
            raise ValueError(f"array {v} is given twice with the same weight and kind")
        if v in ("maskCatch", "lu_id"):
            raise ValueError(f"array {v} is int32")
        if v.startswith("sas_params_"):
            raise ValueError(f"array {v} is a parameter block")
        if v in FLUX_INPUTS or v == "C_in":
            raise ValueError(f"array {v} is a daily input")
        if w is not None and w not in FLUX_INPUTS:
            raise ValueError(f"weight {w} is not a daily flux input")
        if kind == BULK and w is None:
            raise ValueError(f"array {v} is BULK and has no weight")
        if kind != BULK and w is not None:
            raise ValueError(f"array {v} is {('BULK', 'MEAN', 'LAST')[kind]} and has the weight {w}")
        if v not in held:
            raise LookupError(f"array {v} is not held by this context")
        if np.asarray(held[v]).ndim != 1:
            raise ValueError(f"array {v} is age-resolved")


def __getattr__(name):
    """ScoresOracleSasContext: the oracle double with the three scores_* methods of `_native.SasContext`, for the host-package tests.
    Built on first use, so that importing this module imports nothing from roger_amd."""
    if name != "ScoresOracleSasContext":
        raise AttributeError(name)
    from sas_zonal_reference import ZonalOracleSasContext

    class ScoresOracleSasContext(ZonalOracleSasContext):
        _sc = None

        def scores_configure(self, items, obs=None, windows=None, series=None):
            items = [(v, w, KINDS[k] if isinstance(k, str) else int(k)) for v, w, k in items]
            if not items:
                self._sc = None
                return
            check_items(items, self._arrays())
            o = np.asarray(obs, dtype=np.float64)
            first, last = check_windows(*windows)
            if o.ndim != 3 or o.shape[0] != len(items) or not 1 <= o.shape[1] <= MAX_SERIES or o.shape[2] != first.size:
                raise ValueError(f"scores_configure: observations of shape {o.shape}")
            if series is not None:
                sr = np.asarray(series).reshape(-1)
                if sr.size != self.n or sr.max() >= o.shape[1]:
                    raise ValueError("scores_configure: series")
                if not (sr >= 0).any():
                    raise ValueError("scores_configure: the series map scores no cell")
            self._sc = HostSasScores(items, o, (first, last), self.n, series)

        def _scores_on(self):
            if self._sc is None:
                raise RuntimeError("rh_sas_scores_configure has not been called")
            return self._sc

        def scores_record(self, day=0):
            self._scores_on().add(self._arrays())

        def scores_read(self):
            sc = self._scores_on()
            return sc.moments.copy(), sc.closed.copy(), sc.win.days

        def step(self, day):
            super().step(day)
            if self._sc is not None:
                self.scores_record(day)

    globals()[name] = ScoresOracleSasContext
    return ScoresOracleSasContext


# ---- the inputs of the pure tests (no day kernel): what tests/test_sas_scores_reference.py shows to have teeth --------------------------
ITEMS16 = [("C_iso_q_ss", "q_ss", BULK), ("C_rz", None, MEAN), ("C_rz", None, LAST), ("C_q_ss", "q_ss", BULK), ("C_iso_transp", "transp", BULK),
           ("C_iso_rz", None, MEAN), ("C_iso_ss", None, LAST), ("C_q_rz", "q_rz", BULK), ("C_ss", None, MEAN), ("C_s", None, LAST),
           ("C_iso_q_ss", "transp", BULK), ("C_iso_q_ss", None, MEAN), ("C_iso_q_ss", None, LAST), ("C_iso_cpr_rz", "cpr_rz", BULK),
           ("C_iso_s", None, LAST), ("C_evap_soil", None, MEAN)]
PURE_DAYS = 7
PURE_WINDOWS = (np.array([0, 1, 4, 6]), np.array([0, 2, 5, 9]))     # first == closes; two days; a gap day (3); one that never closes


def pure_series(n):
    """Three series with -1 columns; column 0 is scored."""
    return ((np.arange(n) + 1) % 4 - 1).astype(np.int32)


def make_pure(n, items, n_series):
    """(values, weights, obs): values[d] {name: (n,)} for the days 0 ... 6 -- negative delta-like numbers whose products with the weights
    are not exact, NaN on some days for some columns; column 0 is NaN on the days 1 and 2 only (den == 0 in window 1 only) --
    weights {name: (3, n)} the three rows of the daily inputs with zeros, a negative and a NaN weight; obs (J, S, 4) with NaN."""
    rng = np.random.default_rng(1000 * n + 10 * len(items) + n_series)
    names = sorted({v for v, _, _ in items})
    wnames = sorted({w for _, w, _ in items if w is not None})
    values = []
    for d in range(PURE_DAYS):
        day = {}
        for v in names:
            a = -12.0 + 9.0 * rng.random(n) + np.where(rng.random(n) < 0.1, 20.0, 0.0)
            a[rng.random(n) < 0.2] = np.nan
            a[0] = np.nan if d in (1, 2) else -7.0 - d / 3.0 - len(v) / 7.0
            day[v] = a
        values.append(day)
    weights = {}
    for w in wnames:
        a = rng.random((3, n)) * 3.0 + 0.1
        a[rng.random((3, n)) < 0.3] = 0.0
        a[:, 0] = [0.7, 1.3, 2.1]
        if n > 2:
            a[1, 2] = np.nan
            a[2, 1] = -0.5
        weights[w] = a
    obs = -10.0 + 6.0 * rng.random((len(items), n_series, len(PURE_WINDOWS[0])))
    obs[1::2, 0, 2] = np.nan
    if n_series > 1:
        obs[:, 1, 0] = np.nan
    return values, weights, obs


def restate_pure(n, items, n_series, variant=None, windows=PURE_WINDOWS, days=PURE_DAYS):
    values, weights, obs = make_pure(n, items, n_series)
    h = HostSasScores(items, obs, windows, n, pure_series(n) if n_series > 1 else None)
    for d in range(days):
        h.add(values[d], {w: a[d % 3] for w, a in weights.items()}, variant)
    return h
