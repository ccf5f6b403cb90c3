"""CPU: the scores' rule of the SAS context restated (tests/sas_scores_reference.py) on hand-worked windows, the order of its operations
pinned by inputs that another order sums differently -- the inputs tests/test_hip_sas_scores.py runs on the device -- the host package's
derivation (roger_amd/sas_scores.py: derive) against a plain two-pass numpy computation over each column's counted samples, its FILL
cases, the window validation and the refusals of the double."""
from fractions import Fraction

import numpy as np
import pytest

import sas_scores_reference as S
from sas_scores_reference import BULK, LAST, MEAN
from test_scores_reference import cancellation_bound, two_pass

NAN = np.nan


def test_the_window_clock():
    w = S.Windows([0, 1, 4, 6], [0, 2, 5, 9])
    got = [w.next() for _ in range(8)]
    assert got == [(0, True, True), (1, True, False), (1, False, True), None, (2, True, False), (2, False, True), (3, True, False), (3, False, False)]
    assert list(w.closed) == [1, 1, 1, 0] and w.days == 8
    # a window that began before the count did is never open: nothing is launched for it and it is never closed
    w = S.Windows([-2, 3], [1, 3])
    assert [w.next() for _ in range(5)] == [None, None, None, (1, True, True), None] and list(w.closed) == [0, 1]
    # days beyond the last window
    w = S.Windows([1], [1])
    assert [w.next() for _ in range(4)] == [None, (0, True, True), None, None]


def test_hand_worked_windows():
    """Two columns, one series, the windows [0, 1] and [3, 3] (day 2 lies outside every window).  Column 0: v = -8, -4 with the weights
    1, 3 -> (-8 - 12) / 4 = -5; column 1 has no flux on day 0 (v NaN, w 0) -> -4 alone.  Day 3: column 0 has no flux at all."""
    items = [("C", "q", BULK), ("C", None, MEAN), ("C", None, LAST)]
    obs = np.array([[[-6.0, -1.0]], [[-6.0, -1.0]], [[-6.0, NAN]]])
    h = S.HostSasScores(items, obs, ([0, 3], [1, 3]), 2)
    days = [({"C": [-8.0, NAN]}, {"q": [1.0, 0.0]}), ({"C": [-4.0, -4.0]}, {"q": [3.0, 2.0]}), ({"C": [100.0, 100.0]}, {"q": [9.0, 9.0]}),
            ({"C": [NAN, -2.0]}, {"q": [0.0, 0.5]})]
    for held, wts in days[:2]:
        h.add({k: np.array(a) for k, a in held.items()}, {k: np.array(a) for k, a in wts.items()})
    assert list(h.closed) == [1, 0]
    bulk, mean, last = h.moments
    assert list(bulk[:, 0]) == [-20.0, 4.0, 1.0, -5.0, 25.0, 30.0, 1.0, -6.0, 36.0]
    assert list(bulk[:, 1]) == [-8.0, 2.0, 1.0, -4.0, 16.0, 24.0, 4.0, -6.0, 36.0]
    assert list(mean[:, 0]) == [-12.0, 2.0, 1.0, -6.0, 36.0, 36.0, 0.0, -6.0, 36.0]
    assert list(mean[:, 1]) == [-4.0, 1.0, 1.0, -4.0, 16.0, 24.0, 4.0, -6.0, 36.0]
    assert list(last[:, 0]) == [0.0, 0.0, 1.0, -4.0, 16.0, 24.0, 4.0, -6.0, 36.0]
    for held, wts in days[2:]:
        h.add({k: np.array(a) for k, a in held.items()}, {k: np.array(a) for k, a in wts.items()})
    assert list(h.closed) == [1, 1] and h.win.days == 4
    # day 2 touched nothing; day 3: column 0 restarts to +0.0 / +0.0 and is not counted (den == 0), column 1 counts -2
    assert list(bulk[:, 0]) == [0.0, 0.0, 1.0, -5.0, 25.0, 30.0, 1.0, -6.0, 36.0] and not np.signbit(bulk[:2, 0]).any()
    assert list(bulk[:, 1]) == [-1.0, 0.5, 2.0, -6.0, 20.0, 26.0, 5.0, -7.0, 37.0]
    assert list(mean[2:, 0]) == [1.0, -6.0, 36.0, 36.0, 0.0, -6.0, 36.0] and list(mean[2:, 1]) == [2.0, -6.0, 20.0, 26.0, 5.0, -7.0, 37.0]
    assert list(last[:, 1]) == [0.0, 0.0, 1.0, -4.0, 16.0, 24.0, 4.0, -6.0, 36.0]           # its second observation is missing


def test_series_and_columns_that_are_not_scored():
    items = [("C", None, LAST)]
    obs = np.array([[[1.0], [NAN], [3.0]]])
    h = S.HostSasScores(items, obs, ([0], [0]), 4, series=[2, -1, 1, 0])
    h.add({"C": np.array([5.0, 5.0, 5.0, NAN])})
    assert list(h.moments[0, 2]) == [1.0, 0.0, 0.0, 0.0] and list(h.moments[0, 6]) == [4.0, 0.0, 0.0, 0.0] and list(h.moments[0, 7]) == [3.0, 0, 0, 0]
    assert not np.signbit(h.moments).any()


def test_the_rounded_product_is_added_not_a_fused_one():
    """num = 2, then v * wd with v = wd = 2^27 + 1: the product 2^54 + 2^28 + 1 rounds to 2^54 + 2^28, and 2 + that is a tie that goes
    to even; a fused multiply-add rounds 2^54 + 2^28 + 3 once, to 2^54 + 2^28 + 4."""
    a = 2.0 ** 27 + 1.0
    separate, fused = 2.0 ** 54 + 2.0 ** 28, float(Fraction(2) + Fraction(a) * Fraction(a))
    assert fused == separate + 4.0
    for variant, want in ((None, separate), ("fma", fused)):
        m = np.zeros((1, 9, 1))
        S.score_day(m, [BULK], [np.array([2.0])], [np.array([1.0])], np.zeros((1, 1, 1)), None, 0, True, False, variant)
        S.score_day(m, [BULK], [np.array([a])], [np.array([a])], np.zeros((1, 1, 1)), None, 0, False, False, variant)
        assert S.same_bits(m[0, 0, 0], want) and m[0, 1, 0] == 1.0 + a


@pytest.mark.parametrize("n_series", [1, 3])
@pytest.mark.parametrize("n_items", [1, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_the_device_tests_inputs_have_teeth(n, n_items, n_series):
    """What tests/test_hip_sas_scores.py::test_pure uploads: every item counts a sample in some column, the count differs between
    columns, and -- from one wavefront on -- a fused num + v * wd differs in at least one column, while adding +0.0 on a day that is
    not eligible does not (a sum that starts at +0.0 is never -0.0), and moments written to each other's planes (m3 / m4) differ."""
    items = S.ITEMS16[:n_items]
    h = S.restate_pure(n, items, n_series)
    counted = h.moments[:, 2, :]
    scored = S.pure_series(n) >= 0 if n_series > 1 else np.ones(n, dtype=bool)
    assert (counted.max(axis=1) >= 1).all() and list(h.closed) == [1, 1, 1, 0]
    assert not h.moments[:, :, ~scored].any()
    assert (h.moments[:, 3].min(axis=1) < 0).all()                  # negative sums
    assert S.same_bits(S.restate_pure(n, items, n_series, "add_zero").moments, h.moments)
    assert not S.same_bits(S.restate_pure(n, items, n_series, "swap34").moments, h.moments)
    if n > 1:
        assert len(np.unique(counted[0][scored])) > 1
        fused = S.restate_pure(n, items, n_series, "fma").moments
        assert (fused != h.moments).any(axis=(0, 1)).sum() >= 1     # (in at least one column)
    # column 0: NaN on the days 1 and 2 only -- den == 0 in window 1 and in no other
    early = S.restate_pure(n, items, n_series, days=3)              # the windows 0 and 1 are through
    for j, (_, _, kind) in enumerate(items):
        assert early.moments[j, 2, 0] == 1.0 and counted[j, 0] >= 1.0 and (kind == LAST or early.moments[j, 1, 0] == 0.0)


def study(ndays=60, ncol=5, seed=4):
    """Fortnightly-ish windows over `ndays` days: per day and column a delta value (NaN on dry days) and a flux."""
    rng = np.random.default_rng(seed)
    first = np.array([0, 5, 12, 14, 21, 30, 33, 40, 47, 52])
    last = np.array([4, 11, 13, 20, 27, 32, 39, 46, 51, 59])
    truth = -9.0 + 2.5 * np.sin(np.arange(ndays) / 9.0)
    v = truth[:, None] + rng.normal(0.0, 0.4, size=(ndays, ncol)) + np.linspace(-1.0, 1.0, ncol)[None, :]
    w = rng.gamma(1.5, 1.0, size=(ndays, ncol))
    dry = rng.random((ndays, ncol)) < 0.35
    dry[12:14, 1] = True                                        # column 1 has no water in the window [12, 13]
    v[dry], w[dry] = NAN, 0.0
    obs = np.array([truth[a:b + 1].mean() for a, b in zip(first, last)]) + rng.normal(0.0, 0.3, size=first.size)
    obs[6] = NAN
    return v, w, obs, (first, last)


def test_derived_metrics_against_two_pass():
    """Per column, over ITS counted samples.  The tolerance is that of tests/test_scores_reference.py for the same comparison: the
    cancellation bound of the raw-moment variance, 8 n eps (mu^2 + var) / var, the larger of the two series', relative (for nse and
    kge relative to 1; for the bias relative to the two means)."""
    from roger_amd.scores import FILL
    from roger_amd.sas_scores import derive

    v, w, obs, windows = study()
    ncol = v.shape[1]
    for kind in (BULK, MEAN, LAST):
        h = S.HostSasScores([("C", "q" if kind == BULK else None, kind)], obs[None, None, :], windows, ncol)
        for d in range(v.shape[0]):
            h.add({"C": v[d]}, {"q": w[d]})
        assert list(h.closed) == [1] * obs.size
        got = derive(h.moments[0])
        counts = set()
        for c in range(ncol):
            sim = S.window_samples(list(zip(v[:, c], w[:, c])), kind, windows)
            keep = ~np.isnan(sim) & ~np.isnan(obs)
            assert got["n"][c] == keep.sum() >= 3
            counts.add(int(keep.sum()))
            tol = max(cancellation_bound(sim[keep]), cancellation_bound(obs[keep]))
            assert tol < 1e-6
            for key, want in two_pass(sim[keep], obs[keep]).items():
                g = got[key][c]
                assert g != FILL and abs(g - want) <= tol * max(abs(want), 1.0 if key in ("nse", "kge") else 0.0) + (
                    tol * (abs(sim[keep].mean()) + abs(obs[keep].mean())) if key == "bias" else 0.0), (kind, key, c, g, want, tol)
            assert S.same_bits(got["sum_obs"][c], np.add.accumulate(np.concatenate([[0.0], obs[keep]]))[-1])
        assert kind == MEAN or len(counts) > 1                   # the number of counted samples differs between columns
    assert np.isnan(S.window_samples(list(zip(v[:, 1], w[:, 1])), BULK, windows)[2])


def test_fill_values_of_the_derivation():
    from roger_amd.sas_scores import FILL, derive

    m = np.zeros((9, 4))
    m[2:, 0] = [2.0, 3.0, 5.0, 3.0, 2.0, 2.0, 2.0]          # two samples 1 and 2 against the observations 1, 1: var_o == 0
    m[2:, 1] = [1.0, 3.0, 9.0, 3.0, 4.0, 1.0, 1.0]          # one sample
    m[2:, 2] = [2.0, 3.0, 5.0, 8.0, 5.0, 5.0, 13.0]         # not scored: whatever its planes hold
    m[2:, 3] = [2.0, -3.0, 5.0, 8.0, 1.0, -5.0, 13.0]       # two samples -1, -2 against -2, -3
    got = derive(m, np.array([0, 1, -1, 0]))
    assert list(got["n"]) == [2, 1, 0, 2]
    assert got["bias"][0] == 0.5 and got["rmse"][0] == 1.0 and got["nse"][0] == FILL and got["r"][0] == FILL and got["kge"][0] == FILL
    assert all(got[k][1] == FILL for k in ("bias", "rmse", "r", "nse", "kge")) and got["sum_sim"][1] == 3.0 and got["sum_obs"][1] == 1.0
    assert all(got[k][2] == FILL for k in ("sum_sim", "sse", "sum_obs", "sum_obs2", "bias", "kge"))
    assert all(got[k][3] != FILL for k in ("bias", "rmse", "r", "nse", "kge")) and got["bias"][3] == 1.0 and got["r"][3] == 1.0
    assert list(derive(m)["n"]) == [2, 1, 2, 2]


def test_window_validation():
    assert [list(a) for a in S.check_windows([0, 3], [2, 3])] == [[0, 3], [2, 3]]
    assert [list(a) for a in S.check_windows([-4, 3], [2, 3])] == [[-4, 3], [2, 3]]          # began before the count did: accepted, never open
    for first, last, text in (([0, 2], [2, 3], "window 1 starts on day 2, window 0 ends on day 2"),
                              ([3, 0], [4, 1], "window 1 starts on day 0, window 0 ends on day 4"),
                              ([0, 5], [1, 4], "window 1 is [5, 4]: its last day lies before its first"),
                              ([], [], "at least one window"), ([0, 1], [0], "2 first and 1 last days")):
        with pytest.raises(ValueError, match="windows?") as e:
            S.check_windows(first, last)
        assert text in str(e.value)


def test_refusals_of_the_double():
    held = {"C_rz": np.zeros(3), "sa_rz": np.zeros((3, 30)), "maskCatch": np.zeros(3, dtype=np.int32), "q_ss": np.zeros(3)}
    S.check_items([("C_rz", "q_ss", BULK), ("C_rz", None, MEAN), ("C_rz", None, LAST)], held)
    for items, exc, text in (([("C_rz", None, BULK)], ValueError, "array C_rz is BULK and has no weight"),
                             ([("C_rz", "q_ss", MEAN)], ValueError, "array C_rz is MEAN and has the weight q_ss"),
                             ([("C_rz", "q_ss", LAST)], ValueError, "array C_rz is LAST and has the weight q_ss"),
                             ([("C_rz", "C_in", BULK)], ValueError, "weight C_in is not a daily flux input"),
                             ([("C_rz", None, 3)], ValueError, "kind 3"),
                             ([("C_rz", None, MEAN), ("C_rz", None, MEAN)], ValueError, "given twice"),
                             ([("maskCatch", None, MEAN)], ValueError, "int32"), ([("q_ss", None, MEAN)], ValueError, "daily input"),
                             ([("sas_params_q_ss", None, MEAN)], ValueError, "parameter block"), ([("sa_rz", None, MEAN)], ValueError, "age-resolved"),
                             ([("tt50_q_ss", None, MEAN)], LookupError, "not held"), ([("C_rz", None, MEAN)] * 17, ValueError, "n_items = 17")):
        with pytest.raises(exc) as e:
            S.check_items(items, held)
        assert text in str(e.value)
