"""The transport bands by age of the SAS context (rh_sas_age_bands_*, roger_amd/csrc/rh_sas_age_bands.h) restated on the host in plain
numpy.  Importing this module imports nothing from roger_amd.

The rule is one promise: block (item j, age class a) of window k -- rows[k][j][a][probability], hdr[k][j][a] = {m, n_nan, W} -- is what
THE RULE of tests/sas_bands_reference.py gives for the width-1 values A_j[:, a] under the same mask, weights and probabilities with kind
LAST: s = v + 0.0; a NaN element is counted in that age class's n_nan and takes no further part; +-inf are values; a column with
mask == 0 or weight 0 is never touched; T = clip(int(ceil(p * float(W))), 1, W) and the value is the smallest s whose cumulative weight
reaches T; m == 0 gives NaN rows and W = 0.  So `select_ages` calls sas_bands_reference.select once per age class and restates nothing of
it.  Windows and clock are `Windows` of sas_scores_reference; every item is LAST, so only the closing day of an open window does anything.
rows (K, W, P) float64 are NaN and hdr (K, W, 3) int64 is 0 until the window closes.
The `variant` arguments exist for the tests that show the inputs have teeth."""
import numpy as np

from sas_bands_reference import A9, B9, MAX_WEIGHT, PROBS8, pure_probs, select  # noqa: F401
from sas_scores_reference import PURE_DAYS, PURE_WINDOWS, Windows, same_bits  # noqa: F401

VARIANTS = ("next_age", "weight_at_column", "nan_per_column", "one_W", "no_add_zero")


def select_ages(A, part, w, probs, variant=None):
    """A (n, W) values after the day, part (n,) bool, w (n,) integer weights (ones without a plane): (rows (W, P), hdr (W, 3)).
    Variants -- next_age: age class a reads a + 1 (the last one wraps); weight_at_column: the two index spaces of a weight confused -- the
    device reads the COMPACTED weights wts_c at the compacted index i, which is the plane at the column index part_cols[i]; the variant
    reads the plane at i itself, one index space where the other belongs (on the device: wts_c[col] for wts_c[i], or weights[i] for
    weights[col]); nan_per_column: a column with a NaN anywhere is a NaN in every age class;
    one_W: T of every age class from the W of age class 0; no_add_zero: no + 0.0."""
    A = np.asarray(A, dtype=np.float64)
    n, W = A.shape
    cols = np.flatnonzero(part)
    wc = np.asarray(w).astype(np.int64)[np.arange(cols.size) if variant == "weight_at_column" else cols]
    rows, hdr = np.full((W, len(probs)), np.nan), np.zeros((W, 3), dtype=np.int64)
    bad_col = np.isnan(A[cols]).any(axis=1)
    W0 = None
    for a in range(W):
        v = A[cols, (a + 1) % W if variant == "next_age" else a]
        if variant == "nan_per_column":
            v = np.where(bad_col, np.nan, v)
        s = v if variant == "no_add_zero" else v + 0.0
        pr = list(probs)
        if variant == "one_W":   # (the selection is not restated: T0 = T(p, W0) is asked of it as the probability (T0 - 0.5) / W_a)
            Wa = int(wc[s == s].sum())
            W0 = Wa if a == 0 else W0
            if Wa and W0:
                pr = [min(1.0, (min(max(int(np.ceil(float(p) * float(W0))), 1), W0) - 0.5) / Wa) for p in probs]
        rows[a], m, n_nan, Wsum = select(s, wc, pr, "no_add_zero" if variant == "no_add_zero" else None)
        hdr[a] = (m, n_nan, Wsum)
    return rows, hdr


class HostSasAgeBands:
    """What a configured context holds: the windows' clock and the result.  items: the arrays' names."""

    def __init__(self, items, probs, windows, n, mask=None, weights=None):
        self.items, self.probs, self.win, self.n = list(items), [float(p) for p in probs], Windows(*windows), int(n)
        self.w = np.ones(self.n, dtype=np.int64) if weights is None else np.asarray(weights).reshape(-1).astype(np.int64)
        self.part = (np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0) & (self.w > 0)
        self.rows, self.hdr = {}, {}

    def add(self, held, variant=None):
        """The next day of the count.  held: {name: (n, W)} values after the day (read on a closing day only)."""
        now = self.win.next()
        if now is None or not now[2]:
            return
        K, P = self.win.first.size, len(self.probs)
        for v in self.items:
            A = np.asarray(held[v], dtype=np.float64)
            if v not in self.rows:
                self.rows[v], self.hdr[v] = np.full((K, A.shape[1], P), np.nan), np.zeros((K, A.shape[1], 3), dtype=np.int64)
            self.rows[v][now[0]], self.hdr[v][now[0]] = select_ages(A, self.part, self.w, self.probs, variant)

    def result(self, widths):
        """(rows, hdr) with the blocks of items that no window closed yet: widths {name: W}."""
        K, P = self.win.first.size, len(self.probs)
        return ({v: self.rows.get(v, np.full((K, widths[v], P), np.nan)) for v in self.items},
                {v: self.hdr.get(v, np.zeros((K, widths[v], 3), dtype=np.int64)) for v in self.items})

    @property
    def closed(self):
        return self.win.closed


# ---- the inputs of the pure tests (no day kernel): what tests/test_sas_age_bands_reference.py shows to have teeth and to meet its conditions ----
ITEMS4 = ("TT_q_ss", "sa_rz", "tt_q_ss", "sa_s")     # widths ages + 1, ages, ages, ages; the first alone is the one-item case
NAN_AGE, SHIFT_AGE, TIE_AGE, NINE_AGE, ZERO_AGE, EDGE_AGE = 3, 5, 7, 9, 11, 13   # age classes with a purpose (every width here is >= 30)
NAN_COLUMN = 2                                        # index among the PARTICIPATING columns of the column that is NaN at every age


def width_of(name, ages):
    return ages + 1 if name.startswith("TT_") else ages


def age_participation(n_part, weighted):
    """(n, mask, weights) with exactly n_part participating columns: n_part, None, None -- or a byte mask that leaves every fifth column
    out and uint16 likelihoods with zeros, ones and the largest weight, n the smallest size that holds n_part participants plus two
    trailing columns that take no part."""
    if not weighted:
        return n_part, None, None
    big = 2 * n_part + 16
    rng = np.random.default_rng(91 + n_part)
    w = rng.integers(2, MAX_WEIGHT + 1, size=big)
    w[::7] = 0
    w[1::7] = 1
    w[2::11] = MAX_WEIGHT
    mask = np.arange(big) % 5 != 4
    n = int(np.flatnonzero(np.cumsum(mask & (w > 0)) == n_part)[0]) + 3
    w[n - 2:] = 0
    return n, mask[:n].astype(np.uint8), w[:n].astype(np.uint16)


def make_age_pure(n, ages, items, part=None):
    """values[d] {name: (n, W)} for the days 0 ... 6.  Values come from a small pool (ties), of both signs, with NaN scattered over the
    elements, a different pattern in every age class; and, where the sizes allow, in every item and on every day:
      participant NAN_COLUMN   NaN at every age                        age class NAN_AGE    NaN in every column: m == 0
      age class SHIFT_AGE      age class SHIFT_AGE - 1 shifted by one participating column (the same values under other weights)
      age class TIE_AGE        two values only, many ties across every selected rank
      age class NINE_AGE       A9 and B9 alternating: keys that differ in the lowest 9 bits only
      age class ZERO_AGE       thirds of negative numbers, zeros of both signs (three -0.0 to one +0.0) and positive numbers
      age class EDGE_AGE       +inf, -inf and a subnormal among the columns"""
    cols = np.arange(n) if part is None else np.flatnonzero(part)
    c = np.arange(cols.size)
    values = []
    for d in range(PURE_DAYS):
        day = {}
        for j, v in enumerate(items):
            W = width_of(v, ages)
            rng = np.random.default_rng(100003 * n + 1009 * ages + 31 * d + j)
            pool = -12.0 + 9.0 * rng.random(max(3, n // 3)) + np.where(rng.random(max(3, n // 3)) < 0.15, 20.0, 0.0)
            A = pool[rng.integers(0, pool.size, size=(n, W))]
            A[rng.random((n, W)) < 0.15] = np.nan
            A[cols[0], :] = -7.0 - d / 3.0 - j / 7.0 - np.arange(W) / 64.0      # a number in every age class
            A[cols, SHIFT_AGE] = np.roll(A[cols, SHIFT_AGE - 1], 1)
            A[cols, TIE_AGE] = np.where(rng.random(cols.size) < 0.5, -3.5, 2.25)
            A[cols, NINE_AGE] = np.where(c % 2 == 0, A9, B9)
            A[cols, ZERO_AGE] = np.where(c % 3 == 0, -1.0 - (c % 5), np.where(c % 3 == 1, np.where((c // 3) % 4 != 3, -0.0, 0.0), 2.5 + (c % 4)))
            if cols.size > 8:
                A[cols[5], EDGE_AGE], A[cols[6], EDGE_AGE], A[cols[8], EDGE_AGE] = np.inf, -np.inf, 5e-324
            if cols.size > NAN_COLUMN:
                A[cols[NAN_COLUMN], :] = np.nan
            A[:, NAN_AGE] = np.nan
            day[v] = A
        values.append(day)
    return values


def restate_age_pure(n_part, ages, items, n_probs, weighted, variant=None, windows=PURE_WINDOWS, days=PURE_DAYS):
    n, mask, w = age_participation(n_part, weighted)
    h = HostSasAgeBands(items, pure_probs(n_probs), windows, n, mask, w)
    values = make_age_pure(n, ages, items, h.part)
    for d in range(days):
        h.add(values[d], variant)
    return h, (n, mask, w, values)
