"""CPU: the likelihood-weighted bands' restatement (tests/bands_weighted_reference.py) against itself -- the two formulations of the pick
-- and against the plain bands' restatement (tests/bands_reference.py) where the weights are 0 or 1."""
import numpy as np
import pytest

from bands_reference import LAST, SUM, HostBands, quantiles_of, rank_of
from bands_weighted_reference import HostWeightedBands, target_of, weighted_quantiles_by_repeat, weighted_quantiles_of

PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
DAY = 86400


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)).all()


def draw(rng, n, wmax):
    """Values with ties, +-inf, +-0.0 and NaN; weights 0 ... wmax with zeros."""
    pool = np.concatenate([rng.normal(size=max(n // 3, 1)), [np.inf, -np.inf, 0.0, -0.0, np.nan, 1.5, 1.5]])
    s = rng.choice(pool, n)
    w = rng.integers(0, wmax + 1, n).astype(np.uint16)
    w[rng.random(n) < 0.2] = 0
    return s, w


@pytest.mark.parametrize("seed", range(40))
def test_the_two_formulations_agree_by_bits(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    s, w = draw(rng, n, int(rng.choice([1, 2, 7, 300])))
    probs = PROBS + tuple(rng.random(3))
    a, b = weighted_quantiles_of(s, w, probs), weighted_quantiles_by_repeat(s, w, probs)
    assert same_bits(a[0], b[0]) and a[1:] == b[1:], (s, w, a, b)
    on = w != 0
    assert a[1] == int((~np.isnan(s[on])).sum()) and a[2] == int(np.isnan(s[on]).sum()) and a[3] == int(w[on & ~np.isnan(s)].astype(np.int64).sum())
    if a[1]:
        x = s[on & ~np.isnan(s)] + 0.0
        assert same_bits(a[0][0], x.min()) and same_bits(a[0][4], x.max())                 # p = 0, p = 1: the participants' extremes
        assert not np.signbit(a[0][~np.isnan(a[0]) & (a[0] == 0.0)]).any()               # the + 0.0 rule
    else:
        assert np.isnan(a[0]).all() and a[3] == 0


@pytest.mark.parametrize("seed", range(20))
def test_weights_0_and_1_reproduce_the_plain_rule_under_the_mask(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 80))
    s, w = draw(rng, n, 1)
    want, m, n_nan = quantiles_of(s[w != 0], PROBS)
    got = weighted_quantiles_of(s, w, PROBS)
    assert same_bits(got[0], want) and got[1:] == (m, n_nan, m)
    for p in PROBS:                                                                       # T - 1 is the plain rank
        assert m == 0 or target_of(p, m) - 1 == rank_of(p, m)


def test_the_target_at_p_0_and_p_1_and_on_a_boundary():
    for W in (1, 2, 20, 65535, 70000 * 65535, 2 ** 47 - 1):
        assert target_of(0.0, W) == 1 and target_of(1.0, W) == W
    assert target_of(0.05, 20) == 1 and target_of(0.95, 20) == 19 and target_of(0.5, 3) == 2 and target_of(0.25, 8) == 2
    # one heavy column is the answer for every p above its left cumulative share; equal values with different weights add up
    s, w = np.array([3.0, 1.0, 2.0, 2.0]), np.array([1, 2, 60, 37], dtype=np.uint16)      # cumulative: 2 | 99 | 100
    v = weighted_quantiles_of(s, w, (0.0, 0.02, 0.0201, 0.5, 0.99, 0.9901, 1.0))[0]
    assert v.tolist() == [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0]


def test_the_trajectory_form_is_the_plain_one_under_0_1_weights_and_differs_under_others():
    rng = np.random.default_rng(7)
    n = 50
    w01 = (rng.random(n) < 0.7).astype(np.uint16)
    w = (w01 * rng.integers(1, 65536, n)).astype(np.uint16)
    plain, same, other = HostBands((SUM, LAST), PROBS, n, w01, DAY, 0), HostWeightedBands((SUM, LAST), PROBS, n, w01, DAY, 0), HostWeightedBands((SUM, LAST), PROBS, n, w, DAY, 0)
    for k in range(6):
        planes = [rng.normal(size=n), rng.normal(size=n)]
        for h in (plain, same, other):
            h.add(k * DAY // 2, (k + 1) * DAY // 2, planes)
    (hdr, values), (shdr, svalues, swsum), (ohdr, ovalues, owsum) = plain.rows(), same.rows(), other.rows()
    assert hdr.shape == (3, 6) and (shdr == hdr).all() and same_bits(svalues, values) and (swsum == hdr[:, 2::2]).all()
    assert (ohdr == hdr).all() and (owsum == int(w.astype(np.int64).sum())).all() and not same_bits(ovalues, values)
    assert same_bits(ovalues[:, :, 0], values[:, :, 0]) and same_bits(ovalues[:, :, -1], values[:, :, -1])    # the extremes do not weigh
    assert same_bits(plain.acc, other.acc)
