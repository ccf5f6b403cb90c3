"""CPU: the numpy twin of the transport bands by age (tests/sas_age_bands_reference.py) against brute force, the conditions the pure inputs
of tests/test_hip_sas_age_bands.py are built to meet, and the wrong variants that each change a recorded bit of those inputs."""
import numpy as np
import pytest

import sas_age_bands_reference as R

CASES = [(65, 30, R.ITEMS4, 8, True), (65, 30, R.ITEMS4, 8, False), (257, 63, R.ITEMS4[:1], 1, True), (64, 64, R.ITEMS4, 8, True)]


def brute(A, part, w, probs):
    """np.sort(np.repeat(A[part, a] + 0.0, w))[T - 1] per age class, T = clip(ceil(p W), 1, W); NaN where no number takes part."""
    cols = np.flatnonzero(part)
    rows, hdr = np.full((A.shape[1], len(probs)), np.nan), np.zeros((A.shape[1], 3), dtype=np.int64)
    for a in range(A.shape[1]):
        s, wa = A[cols, a] + 0.0, w[cols]
        ok = s == s
        members = np.sort(np.repeat(s[ok], wa[ok]))
        hdr[a] = (ok.sum(), (~ok).sum(), members.size)
        for q, p in enumerate(probs):
            if members.size:
                rows[a, q] = members[min(max(int(np.ceil(p * float(members.size))), 1), members.size) - 1]
    return rows, hdr


@pytest.mark.parametrize("n_part,ages,items,n_probs,weighted", CASES)
def test_restatement_is_brute_force(n_part, ages, items, n_probs, weighted):
    h, (n, mask, w, values) = R.restate_age_pure(n_part, ages, items, n_probs, weighted)
    assert list(h.closed) == [1, 1, 1, 0] and int(h.part.sum()) == n_part
    wb = np.minimum(h.w, 40)   # (np.repeat of 65535 x 257 members per age class is needless: the rule is the same for small weights)
    small = R.HostSasAgeBands(items, R.pure_probs(n_probs), R.PURE_WINDOWS, n, mask, wb if weighted else None)
    for d in range(R.PURE_DAYS):
        small.add(values[d])
    for k, d in ((0, 0), (1, 2), (2, 5)):
        for v in items:
            rows, hdr = brute(values[d][v], small.part, small.w, small.probs)
            assert R.same_bits(small.rows[v][k], rows) and (small.hdr[v][k] == hdr).all(), (k, v)
            assert (h.hdr[v][k][:, :2] == hdr[:, :2]).all()
    for v in items:
        assert np.isnan(h.rows[v][3]).all() and not h.hdr[v][3].any()   # the window that never closes


def test_the_pure_inputs_meet_their_conditions():
    h, (n, mask, w, values) = R.restate_age_pure(65, 30, R.ITEMS4, 8, True)
    cols = np.flatnonzero(h.part)
    assert mask is not None and (mask == 0).any() and (w == 0).any() and (w == 1).any() and (w == R.MAX_WEIGHT).any() and cols.size == 65 < n
    keys = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)   # noqa: E731
    for k, d in ((0, 0), (1, 2), (2, 5)):
        for v in R.ITEMS4:
            A, hdr, rows = values[d][v][cols], h.hdr[v][k], h.rows[v][k]
            nan = np.isnan(A)
            assert nan[R.NAN_COLUMN].all() and nan[:, R.NAN_AGE].all() and hdr[R.NAN_AGE].tolist() == [0, 65, 0] and np.isnan(rows[R.NAN_AGE]).all()
            scattered = nan.sum(axis=0)
            assert len(set(scattered.tolist())) > 3 and (hdr[:, 1] == scattered).all() and (hdr[:, 0] + hdr[:, 1] == 65).all()   # n_nan differs along the age axis
            live = hdr[:, 0] > 0
            assert (hdr[live, 2] != hdr[live, 0]).all() and len(set(hdr[live, 2].tolist())) > 3                                  # W != m, and W is per age class
            both = ~nan[1:, R.SHIFT_AGE] & ~nan[:-1, R.SHIFT_AGE - 1]   # (the all-NaN column is written behind the shift)
            assert both.sum() > 40 and (A[1:, R.SHIFT_AGE] == A[:-1, R.SHIFT_AGE - 1])[both].all() and not R.same_bits(rows[R.SHIFT_AGE], rows[R.SHIFT_AGE - 1])
            assert set(rows[R.TIE_AGE].tolist()) == {-3.5, 2.25}                                                                  # ties across the selected ranks
            nine = keys(rows[R.NINE_AGE])
            assert set(rows[R.NINE_AGE].tolist()) == {R.A9, R.B9} and len({int(x) >> 9 for x in nine}) == 1                       # the lowest 9 bits decide
            z = A[:, R.ZERO_AGE]
            assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any() and 0.0 in rows[R.ZERO_AGE]
            assert not np.signbit(rows[R.ZERO_AGE][rows[R.ZERO_AGE] == 0]).any()                                                  # + 0.0: one zero
            e = A[:, R.EDGE_AGE]
            assert np.inf in e and -np.inf in e and 5e-324 in e and rows[R.EDGE_AGE][0] == -np.inf and rows[R.EDGE_AGE][-1] == np.inf


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_changes_a_recorded_bit(variant):
    for n_part, ages, items, n_probs, weighted in CASES[:1]:
        good, _ = R.restate_age_pure(n_part, ages, items, n_probs, weighted)
        bad, _ = R.restate_age_pure(n_part, ages, items, n_probs, weighted, variant)
        differs = [not R.same_bits(good.rows[v], bad.rows[v]) or bool((good.hdr[v] != bad.hdr[v]).any()) for v in items]
        assert all(differs), (variant, differs)
    if variant not in ("weight_at_column",):   # without a weight plane every weight is 1 at either index
        good, _ = R.restate_age_pure(65, 30, R.ITEMS4, 8, False)
        bad, _ = R.restate_age_pure(65, 30, R.ITEMS4, 8, False, variant)
        assert any(not R.same_bits(good.rows[v], bad.rows[v]) or bool((good.hdr[v] != bad.hdr[v]).any()) for v in R.ITEMS4), variant
