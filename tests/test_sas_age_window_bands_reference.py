"""CPU: tests/sas_age_window_bands_reference.py, the numpy twin of the window means of the bands by age (rh_sas_age_window_bands_*), has
teeth.  The twin restates nothing: it feeds sas_bands_reference.HostSasBands the width-1 slices.  Here the rule is spelt out once more, as a
brute-force loop in python floats per column and age class over the days, then np.sort(np.repeat(s, w))[T - 1]; the twin equals it bit for
bit, the pure inputs meet every condition the device tests rely on, and every wrong variant of the loop changes a recorded bit of them."""
from fractions import Fraction

import numpy as np
import pytest

import sas_age_window_bands_reference as R
from sas_scores_reference import BULK, MEAN

VARIANTS = ("fma", "no_restart", "one_den", "nan_poisons", "skip_closing", "row_before", "mean_weighted", "no_add_zero")
ITEMS = R.ITEMS4[:2]      # TT_q_ss BULK by q_ss (width ages + 1) and sa_rz MEAN (width ages)
AGES = 30


def fused(num, v, wd):
    if not (np.isfinite(num) and np.isfinite(v) and np.isfinite(wd)):
        return num + v * wd
    return float(Fraction(num) + Fraction(v) * Fraction(wd))


def brute(cfg, values, daily, items, probs, variant=None):
    """(rows {name: (K, W, P)}, hdr {name: (K, W, 3)}) by the rule in python floats.  Variants -- fma: num + v * wd rounded once; no_restart:
    an ineligible first day leaves the accumulators of the window before; one_den: den per column, added to whenever wd > 0; nan_poisons:
    eligible iff wd > 0; skip_closing: the closing day's value is left out; row_before: wd of row day - 1; mean_weighted: MEAN takes the
    daily weight q_ss; no_add_zero: no + 0.0."""
    n, mask, w = cfg[:3]
    wi = np.ones(n, dtype=np.int64) if w is None else np.asarray(w).astype(np.int64)
    cols = np.flatnonzero((np.ones(n, dtype=bool) if mask is None else np.asarray(mask) != 0) & (wi > 0))
    K, P = len(R.WINDOWS[0]), len(probs)
    rows, hdr = {}, {}
    for v, wn, kind in items:
        W = values[0][v].shape[1]
        rows[v], hdr[v] = np.full((K, W, P), np.nan), np.zeros((K, W, 3), dtype=np.int64)
        for a in range(W):
            acc = {int(c): (0.0, 0.0) for c in cols}       # (kept between the windows only for the variant that fails to restart)
            for k, (f, l) in enumerate(zip(*R.WINDOWS)):
                s = []
                for c in cols:
                    num, den = acc[int(c)]
                    for d in range(int(f), int(l) + 1):
                        x = float(values[d][v][c, a])
                        row = (d - 1) % R.DAYS if variant == "row_before" else d
                        wd = float(daily[wn][row, c]) if kind == BULK else float(daily["q_ss"][row, c]) if variant == "mean_weighted" else 1.0
                        eligible = wd > 0.0 and (x == x or variant == "nan_poisons")
                        if d == f and not (variant == "no_restart" and not eligible):
                            num = den = 0.0
                        if variant == "skip_closing" and d == l:
                            continue
                        if eligible:
                            num = fused(num, x, wd) if variant == "fma" else num + x * wd
                        if eligible or (variant == "one_den" and wd > 0.0):
                            den = den + wd
                    acc[int(c)] = (num, den)
                    sc = num / den if den > 0.0 else float("nan")
                    s.append(sc if variant == "no_add_zero" else sc + 0.0)
                s = np.array(s)
                number = s == s
                m, n_nan, Wsum = int(number.sum()), int((~number).sum()), int(wi[cols][number].sum())
                hdr[v][k, a] = (m, n_nan, Wsum)
                if m:
                    ordered = np.sort(np.repeat(s[number], wi[cols][number]))
                    for q, p in enumerate(probs):
                        rows[v][k, a, q] = ordered[min(max(int(np.ceil(float(p) * float(Wsum))), 1), Wsum) - 1]
    return rows, hdr


def bits_differ(a, b):
    return any(not R.same_bits(a[0][v], b[0][v]) or (a[1][v] != b[1][v]).any() for v in a[0])


@pytest.fixture(scope="module")
def pure():
    """The unweighted shape the variants run on: the twin's run, once, and the loop's."""
    h, cfg, values, daily = R.restate_pure(65, AGES, False)
    return h, cfg, values, daily, brute(cfg, values, daily, ITEMS, R.PROBS8)


def test_the_twin_is_the_loop(pure):
    h, cfg, values, daily, loop = pure
    twin = R.sliced(h, AGES, ITEMS, 8)
    for v, _, _ in ITEMS:
        assert R.same_bits(twin[0][v], loop[0][v]) and (twin[1][v] == loop[1][v]).all(), v
    assert list(h.closed) == [1, 1, 1] and h.win.days == R.DAYS


def test_the_twin_is_the_loop_under_a_mask_and_weights():
    """A few columns only: np.repeat expands every weight.  W != m, so a quantile's rank is one of weights and not of columns."""
    h, cfg, values, daily = R.restate_pure(12, AGES, True)
    loop = brute(cfg, values, daily, ITEMS, R.PROBS8)
    twin = R.sliced(h, AGES, ITEMS, 8)
    for v, _, _ in ITEMS:
        assert R.same_bits(twin[0][v], loop[0][v]) and (twin[1][v] == loop[1][v]).all(), v
        assert (twin[1][v][..., 2] != twin[1][v][..., 0]).any(), v
    assert cfg[0] > 12 and (cfg[1] == 0).any() and (cfg[2] == 0).any()


def test_the_zonal_twin_is_the_plain_one_under_the_zone_masks():
    """The zone axis stands in front of the age axis, and zone z is the plain form with mask = (zones == z) & mask."""
    n, mask, w = R.participation(40, True)
    zones = (np.arange(n) % 4 - 1).astype(np.int32)
    part = (mask != 0) & (w > 0)
    values, daily = R.make_window_pure(n, AGES, ITEMS, part)
    hz = R.HostSasAgeWindowBands(ITEMS, (0.5,), R.WINDOWS, n, mask, w, zones, 3)
    plain = [R.HostSasAgeWindowBands(ITEMS, (0.5,), R.WINDOWS, n, (zones == z) & (mask != 0), w) for z in range(3)]
    for d in range(R.DAYS):
        for h in [hz] + plain:
            h.add(values[d], {wn: a[d] for wn, a in daily.items()})
    widths = {v: R.width_of(v, AGES) for v, _, _ in ITEMS}
    rows, hdr = hz.result(widths)
    for v, _, _ in ITEMS:
        assert rows[v].shape == (3, 3, widths[v], 1) and hdr[v].shape == (3, 3, widths[v], 3)
        for z in range(3):
            pr, ph = plain[z].result(widths)
            assert R.same_bits(rows[v][:, z], pr[v]) and (hdr[v][:, z] == ph[v]).all() and ph[v][..., 0].any()


def test_the_pure_inputs_meet_their_conditions(pure):
    h, (n, mask, w, _, _), values, daily, loop = pure
    cols = np.arange(n)
    bulk, mean = ITEMS[0][0], ITEMS[1][0]
    q = daily["q_ss"]
    assert ITEMS[0][2] == BULK and ITEMS[1][2] == MEAN
    # an element that is NaN on some days of a window only: den differs along the age axis within one column
    c = cols[R.P_NAN_DAYS]
    for v in (bulk, mean):
        assert np.isnan(values[2][v][c, R.NAN_DAYS_AGE]) and not np.isnan([values[d][v][c, R.NAN_DAYS_AGE] for d in (1, 3)]).any()
        assert not np.isnan([values[d][v][c, R.NAN_DAYS_AGE + 1] for d in (1, 2, 3)]).any() and (q[1:4, c] > 0).all()
    # a column whose weight is 0 on every day of a window: every age class NaN and counted
    c = cols[R.P_DRY_WINDOW]
    assert not q[1:4, c].any() and q[0, c] > 0
    assert (loop[1][bulk][1, :, 1] >= 1).all()
    # a column whose weight is 0 on the first day of the second window after a non-zero first window
    c = cols[R.P_DRY_FIRST]
    assert q[0, c] > 0 and q[1, c] == 0 and (q[2:4, c] > 0).all() and not np.isnan(values[0][bulk][c]).all()
    # ... and for a MEAN, an element that is a number on day 0, NaN on day 1 and a number behind it
    c = cols[R.P_FIRST_NAN]
    assert np.isnan(values[1][mean][c, R.FIRST_NAN_AGE]) and not np.isnan([values[d][mean][c, R.FIRST_NAN_AGE] for d in (0, 2, 3)]).any()
    # a negative and a NaN daily weight
    assert q[2, cols[R.P_NEGATIVE]] < 0 and np.isnan(q[5, cols[R.P_NAN_WEIGHT]])
    # a window of one day, where fl(v * wd) / wd != v for some element
    assert R.WINDOWS[0][0] == R.WINDOWS[1][0] == 0
    v0, w0 = values[0][bulk], q[0][:, None]
    with np.errstate(all="ignore"):
        assert ((w0 > 0) & (v0 == v0) & ((v0 * w0) / np.where(w0 > 0, w0, 1.0) != v0)).any()
    # a recorded day between two windows
    assert R.WINDOWS[1][1] == 3 and R.WINDOWS[0][2] == 5 and R.DAYS == 7
    # +inf on one day and -inf on another in one element: num is NaN
    c = cols[R.P_INF]
    assert values[1][bulk][c, R.EDGE_AGE] == np.inf and values[2][bulk][c, R.EDGE_AGE] == -np.inf and (q[1:3, c] > 0).all()
    # both zeros, and a subnormal
    zeros = np.concatenate([values[d][mean][:, R.ZERO_AGE] for d in range(R.DAYS)])
    assert ((zeros == 0) & np.signbit(zeros)).any() and ((zeros == 0) & ~np.signbit(zeros)).any()
    assert all(values[d][bulk][cols[R.P_SUBNORMAL], R.EDGE_AGE] == 5e-324 for d in range(R.DAYS))
    # ties across a selected rank: fewer distinct values than probabilities pick
    assert len(set(loop[0][mean][1, R.TIE_AGE].tolist())) == 2 and loop[1][mean][1, R.TIE_AGE, 0] == n - 0
    # a product v * wd that is inexact
    x, wd = float(values[0][bulk][0, 0]), float(q[0, 0])
    assert Fraction(x) * Fraction(wd) != Fraction(x * wd)
    # every block of the three windows has members, and NaN is counted somewhere
    assert all(loop[1][v][..., 0].all() and loop[1][v][..., 1].any() for v in (bulk, mean))


def test_w_differs_from_m_under_weights():
    h, _, _, _ = R.restate_pure(65, AGES, True)
    hdr = R.sliced(h, AGES, ITEMS, 8)[1]
    assert all((hdr[v][..., 2] > hdr[v][..., 0]).any() for v, _, _ in ITEMS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_variant_changes_a_recorded_bit(pure, variant):
    h, cfg, values, daily, loop = pure
    assert bits_differ(loop, brute(cfg, values, daily, ITEMS, R.PROBS8, variant)), variant
