"""The window means of the transport bands by age (rh_sas_age_window_bands_*, roger_amd/csrc/rh_sas_age_bands.h) restated on the host.
Importing this module imports nothing from roger_amd.

The rule is one promise: block (item j, [zone z,] age class a) of window k -- rows[k][[z]][a][probability], hdr[k][[z]][a] = {m, n_nan, W} of
item j -- is what THE RULE of tests/sas_bands_reference.py records for the width-1 values A_j[:, a] with the same item weight and kind
(BULK by a daily flux, or MEAN), under the same mask, weights, probabilities and windows; with zones, mask = (zones == z) & mask.  So
`HostSasAgeWindowBands` holds one sas_bands_reference.HostSasBands per (item, zone, age class), feeds it the width-1 slices day by day, and
restates nothing of the accumulation or the selection.  The wrong variants that show the inputs to have teeth live where the accumulation is
spelt out: in the brute-force loop of tests/test_sas_age_window_bands_reference.py."""
import functools

import numpy as np

from sas_bands_reference import MAX_WEIGHT, PROBS8, HostSasBands, pure_probs  # noqa: F401
from sas_scores_reference import BULK, MEAN, Windows, same_bits  # noqa: F401

KIND_NAMES = {BULK: "bulk", MEAN: "mean"}


class HostSasAgeWindowBands:
    """What a configured context holds.  items: [(value, weight or None, kind int)]; zones: (n,) integers or None (the plain form)."""

    def __init__(self, items, probs, windows, n, mask=None, weights=None, zones=None, n_zones=0):
        self.items = [(v, w, int(k)) for v, w, k in items]
        self.probs, self.windows, self.n = [float(p) for p in probs], windows, int(n)
        self.weights = weights
        mask = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        self.masks = [mask] if zones is None else [(np.asarray(zones).reshape(-1) == z) & mask for z in range(int(n_zones))]
        self.zonal = zones is not None
        self.win = Windows(*windows)          # (for the closed flags and the day count: every host below has the same clock)
        self.hosts = {}                       # {value: [zone][age class] HostSasBands}

    def add(self, held, daily):
        """The next day of the count.  held: {name: (n, W)} values after the day; daily: {weight name: (n,)} the day's rows."""
        self.win.next()
        for item in self.items:
            v = item[0]
            A = np.asarray(held[v], dtype=np.float64)
            if v not in self.hosts:
                self.hosts[v] = [[HostSasBands([item], self.probs, self.windows, self.n, m, self.weights) for _ in range(A.shape[1])] for m in self.masks]
            for per_age in self.hosts[v]:
                for a, h in enumerate(per_age):
                    h.add({v: A[:, a]}, daily)

    def result(self, widths):
        """(rows {name: (K, [Z,] W, P)}, hdr {name: (K, [Z,] W, 3)}); before the first day NaN and 0: widths {name: W}."""
        K, P, Z = self.win.first.size, len(self.probs), len(self.masks)
        rows, hdr = {}, {}
        for v, _, _ in self.items:
            if v in self.hosts:
                r = np.stack([np.stack([h.rows[:, 0] for h in per_age], axis=1) for per_age in self.hosts[v]], axis=1)
                hd = np.stack([np.stack([h.hdr[:, 0] for h in per_age], axis=1) for per_age in self.hosts[v]], axis=1)
            else:
                r, hd = np.full((K, Z, widths[v], P), np.nan), np.zeros((K, Z, widths[v], 3), dtype=np.int64)
            rows[v], hdr[v] = (r, hd) if self.zonal else (r[:, 0], hd[:, 0])
        return rows, hdr

    @property
    def closed(self):
        return self.win.closed


# ---- the inputs of the pure tests (no day kernel): what tests/test_sas_age_window_bands_reference.py shows to have teeth and to meet its
# conditions ----
ITEMS4 = (("TT_q_ss", "q_ss", BULK), ("sa_rz", None, MEAN), ("tt_q_ss", "transp", BULK), ("sa_s", None, MEAN))   # widths ages + 1, ages, ages, ages
WINDOWS = (np.array([0, 1, 5]), np.array([0, 3, 6]))    # one day (first == closes); three days; a gap day (4); two days
DAYS = 7                                                # ... and as many rows of the daily weights: day d reads row d
NAN_DAYS_AGE, FIRST_NAN_AGE, TIE_AGE, ZERO_AGE, EDGE_AGE = 2, 4, 7, 11, 13   # age classes with a purpose (every width here is >= 30)
(P_NUMBER, P_DRY_WINDOW, P_DRY_FIRST, P_NEGATIVE, P_NAN_WEIGHT, P_NAN_DAYS, P_INF, P_FIRST_NAN, P_SUBNORMAL) = range(9)   # participants with one


def named(items):
    """The items as the binding takes them: the kind by its name."""
    return [(v, w, KIND_NAMES[k]) for v, w, k in items]


def width_of(name, ages):
    return ages + 1 if name.startswith("TT_") else ages


def participation(n_part, weighted):
    """(n, mask, weights) with exactly n_part participating columns, as sas_age_bands_reference.age_participation builds them."""
    from sas_age_bands_reference import age_participation

    return age_participation(n_part, weighted)


def make_window_pure(n, ages, items, part=None):
    """(values[d] {name: (n, W)} for the days 0 ... 6, daily {weight name: (7, n)}).  Values are negative delta-like numbers whose products with
    the weights are not exact, NaN scattered over elements and days; the daily weights hold zeros in three of ten places.  Where the sizes
    allow, by index among the PARTICIPATING columns (every item, every weight):
      P_NUMBER       a number in every age class on every day, and a weight > 0
      P_DRY_WINDOW   weight 0 on the days 1 ... 3: the second window of a BULK item is NaN in every age class
      P_DRY_FIRST    weight 0 on day 1, the first day of the second window, > 0 on day 0 and on the days 2 and 3: a stale accumulator shows
      P_NEGATIVE     a negative weight on day 2;   P_NAN_WEIGHT  a NaN weight on day 5
      P_NAN_DAYS     age class NAN_DAYS_AGE is NaN on day 2 only, its neighbours are numbers: den differs along the age axis of the column
      P_INF          age class EDGE_AGE is +inf on day 1 and -inf on day 2 under weights > 0: num is NaN
      P_FIRST_NAN    age class FIRST_NAN_AGE is a number on day 0, NaN on day 1 and a number on the days 2 and 3 (a MEAN's ineligible first day)
      P_SUBNORMAL    age class EDGE_AGE is the smallest subnormal on every day
      age class TIE_AGE    two values only, the same on every day: the MEAN of many columns ties across every selected rank
      age class ZERO_AGE   thirds of negative numbers, zeros and positive numbers; a zero column is -5e-324 on a window's first day and then
                           -0.0 and +0.0 by turns, so that the mean underflows to -0.0 before the + 0.0"""
    cols = np.arange(n) if part is None else np.flatnonzero(part)
    c = np.arange(cols.size)
    names = [v for v, _, _ in items]
    wnames = sorted({w for _, w, _ in items if w is not None})
    first_days = set(int(f) for f in WINDOWS[0])
    values = []
    for d in range(DAYS):
        day = {}
        for j, v in enumerate(names):
            W = width_of(v, ages)
            rng = np.random.default_rng(100003 * n + 1009 * ages + 31 * d + j)
            A = -12.0 + 9.0 * rng.random((n, W)) + np.where(rng.random((n, W)) < 0.1, 20.0, 0.0)
            A[rng.random((n, W)) < 0.15] = np.nan
            A[cols[P_NUMBER], :] = -7.0 - d / 3.0 - j / 7.0 - np.arange(W) / 64.0
            A[cols, TIE_AGE] = np.where(c % 2 == 0, -3.5, 2.25)
            zero = -5e-324 if d in first_days else (-0.0 if d % 2 else 0.0)
            A[cols, ZERO_AGE] = np.where(c % 3 == 0, -1.0 - (c % 5) - d / 8.0, np.where(c % 3 == 1, zero, 2.5 + (c % 4) + d / 8.0))
            if cols.size > P_SUBNORMAL:
                A[cols[P_NAN_DAYS], NAN_DAYS_AGE - 1:NAN_DAYS_AGE + 2] = -6.5 + d / 7.0
                if d == 2:
                    A[cols[P_NAN_DAYS], NAN_DAYS_AGE] = np.nan
                A[cols[P_INF], EDGE_AGE] = np.inf if d == 1 else -np.inf if d == 2 else -4.25
                A[cols[P_FIRST_NAN], FIRST_NAN_AGE] = np.nan if d == 1 else -5.75 + d / 9.0
                A[cols[P_SUBNORMAL], EDGE_AGE] = 5e-324
            day[v] = A
        values.append(day)
    daily = {}
    for q, w in enumerate(wnames):
        rng = np.random.default_rng(7919 * n + 13 * ages + q)
        a = rng.random((DAYS, n)) * 3.0 + 0.1
        a[rng.random((DAYS, n)) < 0.3] = 0.0
        a[:, cols[P_NUMBER]] = 0.7 + 0.2 * np.arange(DAYS)
        if cols.size > P_SUBNORMAL:
            a[:, cols[P_DRY_WINDOW]] = [1.3, 0.0, 0.0, 0.0, 0.9, 0.4, 2.2]
            a[:, cols[P_DRY_FIRST]] = [1.7, 0.0, 0.6, 1.1, 0.3, 0.8, 0.0]
            a[:, cols[P_NEGATIVE]] = [0.9, 1.2, -0.5, 0.4, 1.0, 2.0, 0.3]
            a[:, cols[P_NAN_WEIGHT]] = [0.2, 1.9, 0.8, 0.0, 1.0, np.nan, 1.5]
            a[:, cols[P_NAN_DAYS]] = a[:, cols[P_FIRST_NAN]] = [1.1, 0.9, 1.4, 0.6, 0.5, 1.6, 0.7]
            a[:, cols[P_INF]] = [0.8, 1.5, 0.7, 0.0, 1.0, 1.2, 0.9]
        daily[w] = a
    return values, daily


@functools.lru_cache(maxsize=None)
def restate_pure(n_part, ages, weighted, kind=None):
    """The restated run of all of ITEMS4 with PROBS8 over the seven days, once per shape: (host, (n, mask, weights, zones, n_zones), values,
    daily).  kind: a map of sas_age_bands_zonal_reference.zone_map (n_part is then the map's); None: the plain form.  The cases of fewer items
    and of the one probability 0.5 are slices of it (`sliced`).  Treat the result as read-only."""
    if kind is None:
        n, mask, w = participation(n_part, weighted)
        zones, n_zones = None, 0
    else:
        from sas_age_bands_zonal_reference import zone_map

        n, mask, w, zones, n_zones = zone_map(kind, weighted)
    part = (np.ones(n, dtype=bool) if mask is None else mask != 0) & (True if w is None else w > 0)
    values, daily = make_window_pure(n, ages, ITEMS4, part)
    h = HostSasAgeWindowBands(ITEMS4, PROBS8, WINDOWS, n, mask, w, zones, n_zones)
    for d in range(DAYS):
        h.add(values[d], {wn: a[d] for wn, a in daily.items()})
    return h, (n, mask, w, zones, n_zones), values, daily


def sliced(h, ages, items, n_probs):
    """(rows, hdr) of restate_pure's host for `items` (of ITEMS4) and pure_probs(n_probs)."""
    rows, hdr = h.result({v: width_of(v, ages) for v, _, _ in ITEMS4})
    at = [PROBS8.index(p) for p in pure_probs(n_probs)]
    return {v: rows[v][..., at] for v, _, _ in items}, {v: hdr[v] for v, _, _ in items}
