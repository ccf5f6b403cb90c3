"""CPU: the restatement of the observation rule (tests/bands_obs_reference.py) has teeth: the pairs are tied to the quantiles that
tests/bands_reference.py and tests/bands_weighted_reference.py select, at the edges of the rule as well."""
import numpy as np
import pytest

from bands_obs_reference import MISSING, HostObsBands, HostObsWeightedBands, HostObsZonalBands, inside_of, obs_at, pair_of
from bands_reference import LAST, SUM, key_of, quantiles_of
from bands_weighted_reference import target_of, weighted_quantiles_of

DAY = 86400
PROBS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


def assert_tied_to_the_quantiles(q, total, pair, o, probs=PROBS):
    below, equal = pair
    assert 0 <= below and 0 <= equal and below + equal <= total
    for p, qp in zip(probs, q):
        T = target_of(p, total)
        assert (qp <= o) == (below + equal >= T), (p, qp, o, pair, T)
        assert (qp < o) == (below >= T), (p, qp, o, pair, T)
    for lo in range(len(probs)):
        for hi in range(lo, len(probs)):
            assert inside_of(below, equal, total, probs[lo], probs[hi]) == (q[lo] <= o <= q[hi]), (probs[lo], probs[hi], o)


@pytest.mark.parametrize("seed", range(6))
def test_the_two_inequalities_on_seeded_inputs_with_many_ties(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 200))
    s = np.round(rng.normal(size=n) * 3) / 2                      # a few distinct values: ties everywhere
    s[rng.random(n) < 0.1] = np.nan
    w = rng.integers(0, 6, n).astype(np.uint16)
    q, m, n_nan = quantiles_of(s, PROBS)
    qw, mw, _, W = weighted_quantiles_of(s, w, PROBS)
    candidates = np.unique(np.concatenate([s[s == s], s[s == s] + 0.25, [-100.0, 100.0, np.inf, -np.inf, 0.0, -0.0]]))
    for o in candidates:
        pair = pair_of(s, o)
        assert pair == (int((s < o).sum()), int((s == o).sum()))
        if m:
            assert_tied_to_the_quantiles(q, m, pair, o)
        pw = pair_of(s, o, w)
        assert pw == (int(w[s < o].astype(np.int64).sum()), int(w[s == o].astype(np.int64).sum()))
        if mw:
            assert_tied_to_the_quantiles(qw, W, pw, o)
    assert m + n_nan == n


def test_the_edges_of_the_order():
    s = np.array([3.0, -1.0, 3.0, 7.5, -1.0, 0.25])
    assert pair_of(s, -1.0) == (0, 2) and pair_of(s, 7.5) == (5, 1)                 # the minimum and the maximum
    assert pair_of(s, -1.5) == (0, 0) and pair_of(s, 8.0) == (6, 0)                 # below and above all values
    assert pair_of(s, np.inf) == (6, 0) and pair_of(s, -np.inf) == (0, 0)
    t = np.array([np.inf, -np.inf, 1.0, np.inf])
    assert pair_of(t, np.inf) == (2, 2) and pair_of(t, -np.inf) == (0, 1) and pair_of(t, 1.0) == (1, 1)
    assert pair_of(s, 3.0, np.array([2, 5, 0, 1, 7, 3])) == (15, 2)                  # weights: 5 + 7 + 3 below, 2 (+ 0) equal


def test_both_zeros_are_one_value():
    s = np.array([-0.0, 0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324])
    for o in (-0.0, 0.0):
        assert pair_of(s, o) == (2, 3)
    assert pair_of(s, 5e-324) == (5, 1) and pair_of(s, -5e-324) == (1, 1)
    # the device compares keys: the + 0.0 on both sides makes the unsigned order of keys the float order
    o = np.float64(-0.0)
    keys, ko = key_of(s), key_of(np.array([o]))[0]
    assert (int((keys < ko).sum()), int((keys == ko).sum())) == pair_of(s, o)
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.normal(size=50) * 10.0 ** rng.integers(-300, 300, 50), [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324]])
    for o in x:
        ko = key_of(np.array([o]))[0]
        assert (int((key_of(x) < ko).sum()), int((key_of(x) == ko).sum())) == pair_of(x, o), o


def test_nan_columns_take_no_part_and_an_all_nan_ensemble_gives_0_0():
    s = np.array([np.nan, 2.0, np.nan, 1.0, 2.0])
    assert pair_of(s, 2.0) == (1, 2) and pair_of(s, 9.0) == (3, 0)
    assert pair_of(np.full(4, np.nan), 1.0) == (0, 0) and pair_of(np.zeros(0), 1.0) == (0, 0)
    assert pair_of(np.full(4, np.nan), 1.0, np.array([1, 2, 3, 4])) == (0, 0)
    assert pair_of(s, 2.0, np.array([0, 0, 0, 0, 0])) == (0, 0)


def test_a_missing_observation_and_an_index_beyond_the_series():
    s = np.arange(5.0)
    assert pair_of(s, np.nan) == MISSING == (-1, -1) and pair_of(s, np.nan, np.ones(5, dtype=int)) == MISSING
    series = np.array([10.0, np.nan, 30.0])
    assert obs_at(series, 0) == 10.0 and np.isnan(obs_at(series, 1)) and obs_at(series, 2) == 30.0
    assert np.isnan(obs_at(series, 3)) and np.isnan(obs_at(series, -1)) and obs_at(series, 0, first_index=2) == 30.0 and np.isnan(obs_at(series, 1, 2))
    # through the double: the series is indexed from the request's start, k + first_index
    h = HostObsBands([LAST], (0.5,), 5, None, DAY, 2 * DAY)                          # t_first: the third day
    h.observe(np.array([[9.0, 9.0, 1.0, np.nan, 3.0]]), first_index=2)
    for d in range(6):
        h.add(d * DAY, (d + 1) * DAY, [s])
    assert h.rows()[0][:, 0].tolist() == [0, 1, 2, 3] and h.pair_rows()[:, 0].tolist() == [[1, 1], [-1, -1], [3, 1], [-1, -1]]
    bare = HostObsBands([LAST], (0.5,), 5, None, DAY, 0)
    bare.add(0, DAY, [s])
    assert bare.pair_rows().tolist() == [[[-1, -1]]]                                 # no observations: no pair


def test_weights_0_and_1_give_the_plain_pairs_under_the_mask():
    rng = np.random.default_rng(5)
    n = 64
    w = (rng.random(n) < 0.6).astype(np.uint16)
    obs = np.round(rng.normal(size=(2, 5)))
    plain, weighted = HostObsBands([SUM, LAST], PROBS, n, w != 0, DAY, 0), HostObsWeightedBands([SUM, LAST], PROBS, n, w, DAY, 0)
    for h in (plain, weighted):
        h.observe(obs)
    for k in range(10):                                                              # two steps a day
        planes = [np.round(rng.normal(size=n)), np.round(rng.normal(size=n) * 2)]
        planes[1][rng.random(n) < 0.1] = np.nan
        for h in (plain, weighted):
            h.add(k * DAY // 2, (k + 1) * DAY // 2, planes)
    assert (plain.pair_rows() == weighted.pair_rows()).all() and plain.pair_rows().shape == (5, 2, 2) and (plain.pair_rows()[..., 1] > 0).any()
    assert (weighted.rows()[2] == plain.rows()[0][:, 2::2]).all()


def test_block_z_is_the_plain_pair_under_the_zones_mask_and_a_zone_without_a_column():
    rng = np.random.default_rng(8)
    n = 40
    zone = rng.integers(-1, 3, n)
    zone[zone == 1] = -1                                                             # zone 1 of 0 ... 3 has no column, and neither has zone 3
    obs = np.round(rng.normal(size=(1, 4, 3)))
    obs[0, 2, 1] = np.nan
    h = HostObsZonalBands([LAST], (0.5,), n, zone, 4, DAY, 0)
    h.observe(obs)
    per = [HostObsBands([LAST], (0.5,), n, zone == z, DAY, 0) for z in range(4)]
    for z, p in enumerate(per):
        p.observe(obs[:, z])
    for d in range(4):
        x = np.round(rng.normal(size=n))
        h.add(d * DAY, (d + 1) * DAY, [x])
        for p in per:
            p.add(d * DAY, (d + 1) * DAY, [x])
    pairs = h.pair_rows()
    assert pairs.shape == (4, 1, 4, 2)
    for z, p in enumerate(per):
        assert (pairs[:, :, z] == p.pair_rows()).all()
    assert (pairs[:3, 0, 1] == 0).all() and (pairs[:3, 0, 3] == 0).all() and (pairs[3] == -1).all() and (pairs[1, 0, 2] == -1).all()
    assert (h.rows()[1][:, 0, 1] == 0).all()
