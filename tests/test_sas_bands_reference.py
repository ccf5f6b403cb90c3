"""CPU: the numpy restatement of the transport bands (tests/sas_bands_reference.py) against brute force, and the pure inputs of
tests/test_hip_sas_bands.py on the restatement alone: every wrong variant of the rule changes a recorded bit on them, and they meet the
conditions without which the GPU test could pass vacuously."""
import numpy as np
import pytest

import sas_bands_reference as B

SIZES = [1, 63, 64, 65, 255, 256, 257]
BIG = 256 * 256 + 1


def recorded(h):
    """Everything a context records, as bit patterns."""
    return np.concatenate([h.rows.view(np.uint64).reshape(-1), h.hdr.view(np.uint64).reshape(-1), h.pairs.view(np.uint64).reshape(-1)])


@pytest.mark.parametrize("seed", range(6))
def test_the_selection_is_the_sorted_repeated_sample(seed):
    """argsort / cumsum / searchsorted equals np.sort(np.repeat(s, w))[T - 1] bit for bit: ties, both signs, infinities, a subnormal, NaN."""
    rng = np.random.default_rng(seed)
    n = [1, 2, 17, 64, 257, 1000][seed]
    pool = np.concatenate([rng.normal(size=max(2, n // 4)), [0.0, np.inf, -np.inf, 5e-324, -5e-324, B.A9, B.B9]])
    s = pool[rng.integers(0, pool.size, size=n)]
    s[rng.random(n) < 0.15] = np.nan
    w = rng.integers(1, 10, size=n)
    if seed % 2:
        w[:] = 1
    probs = list(B.PROBS8) + list(rng.random(8))
    values, m, n_nan, W = B.select(s, w, probs)
    x = s[s == s]
    assert (m, n_nan, W) == (x.size, n - x.size, int(w[s == s].sum()))
    if not m:
        assert np.isnan(values).all()
        return
    brute = np.sort(np.repeat(x, w[s == s]))
    for p, v in zip(probs, values):
        T = min(max(int(np.ceil(p * float(W))), 1), W)
        assert B.same_bits(v, brute[T - 1]), (p, v, brute[T - 1])
        if seed % 2:   # all weights 1: the plain rule of the ensemble bands
            assert B.same_bits(v, np.sort(x)[min(max(int(np.ceil(p * m)) - 1, 0), m - 1)])
    for o in (x[0], -1e300, 1e300, 0.25, -0.0):
        below, equal = B.obs_pair(s, w, o)
        assert (below, equal) == (int((brute < o).sum()), int((brute == o).sum()))
    assert B.obs_pair(s, w, np.nan) == (-1, -1)
    assert B.same_bits(B.values_of(B.keys_of(x)), x) and (np.argsort(B.keys_of(brute), kind="stable") == np.arange(brute.size)).all()


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_the_pure_inputs_have_teeth(variant):
    """no `+ 0.0`, floor for ceil in T, a fused num + v * wd, NaN counted as a member, a zero-weight column taking part, the last 9-bit
    pass dropped: each changes at least one recorded bit of the pure inputs at full width (n = 257, 8 items, 8 probabilities; a zero-weight
    column can only show with a weight plane, the others show without one)."""
    changed = {}
    for weighted in (False, True):
        want = B.restate_pure(257, B.ITEMS8, 8, weighted)
        changed[weighted] = int((recorded(B.restate_pure(257, B.ITEMS8, 8, weighted, variant=variant)) != recorded(want)).sum())
    assert changed[True] > 0 if variant == "zero_weight" else changed[False] > 0, changed
    # ... and at every size the GPU test runs beyond a single column, some case of that size shows it
    for n in SIZES[1:]:
        shows = False
        for n_items, n_probs, weighted in ((8, 8, True), (8, 8, False), (8, 1, True), (1, 8, True)):
            a, b = (B.restate_pure(n, B.ITEMS8[:n_items], n_probs, weighted, variant=v) for v in (None, variant))
            shows = shows or bool((recorded(a) != recorded(b)).any())
        assert shows, (variant, n)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [257, BIG])
def test_the_pure_inputs_meet_their_conditions(n, weighted):
    h = B.restate_pure(n, B.ITEMS8, 8, weighted)
    values, _, obs = B.make_pure(n, B.ITEMS8)
    mask, w = B.pure_participation(n, weighted)
    part = np.ones(n, dtype=bool) if mask is None else (mask != 0) & (w > 0)
    wi = np.ones(n, dtype=np.int64) if w is None else w.astype(np.int64)
    assert list(h.closed) == [1, 1, 1, 0] and h.win.days == B.PURE_DAYS
    assert np.isnan(h.rows[3]).all() and not h.hdr[3].any() and (h.pairs[3] == -1).all()          # the window that never closes
    for j in range(8):   # per item at least three distinct values among the recorded quantiles of some window
        assert max(len(np.unique(h.rows[k, j][~np.isnan(h.rows[k, j])])) for k in range(3)) >= 3, j
    assert (h.hdr[:3, :, 1] > 0).any()                                                              # some window with n_nan > 0
    assert h.hdr[1, 6, 0] == 0 and h.hdr[1, 6, 2] == 0 and np.isnan(h.rows[1, 6]).all() and h.hdr[1, 6, 1] == part.sum()   # m == 0
    assert (h.pairs[1, 6] == 0).all() or np.isnan(obs[6, 1])                                         # ... whose pair is (0, 0)
    assert (h.rows[:3] < 0).any() and (h.rows[:3] > 0).any()                                         # negative and positive values
    # both zeros present among C_s's participants, and the median falls among them: ties that straddle a selected rank
    cs = values[0]["C_s"][part]
    assert (np.signbit(cs) & (cs == 0)).any() and (~np.signbit(cs) & (cs == 0)).any()
    assert B.same_bits(h.rows[0, 7, 3], 0.0)
    s0, tot = np.sort(cs), int(wi[part].sum())
    below = int(wi[part][cs < 0].sum())
    T = min(max(int(np.ceil(0.5 * tot)), 1), tot)
    assert below < T - 1 and T < below + int(wi[part][cs == 0].sum()) and s0.size == h.hdr[0, 7, 0]   # members tie on both sides of rank T - 1
    # +-inf and a subnormal present
    ci = values[0]["C_iso_rz"]
    assert part[5] and part[6] and part[8] and ci[5] == np.inf and ci[6] == -np.inf and 0 < ci[8] < 2.3e-308
    assert h.rows[0, 5, 0] == -np.inf and h.rows[0, 5, 7] == np.inf
    # two members whose keys differ only in the lowest 9 bits on either side of a selected rank: C_rz (LAST, item 2) in window 2
    ka, kb = B.keys_of(np.array([B.A9])), B.keys_of(np.array([B.B9]))
    assert ka[0] != kb[0] and ka[0] >> np.uint64(9) == kb[0] >> np.uint64(9)
    assert B.same_bits(h.rows[2, 2, 0], B.A9) and B.same_bits(h.rows[2, 2, 7], B.B9)
    q = [B.same_bits(v, B.B9) for v in h.rows[2, 2]]
    assert q == sorted(q) and 0 < sum(q) < 8
    if weighted:
        assert (h.hdr[:3, :, 2] != h.hdr[:3, :, 0]).any() and (w == 0).any() and (w == 1).any() and (w == B.MAX_WEIGHT).any() and (mask == 0).any()
    else:
        assert (h.hdr[:, :, 2] == h.hdr[:, :, 0]).all()
    # observations below all members, above all, exactly on a member, and one missing
    m, W = h.hdr[:, :, 0], h.hdr[:, :, 2]
    assert tuple(h.pairs[0, 0]) == (0, 0) and m[0, 0] > 0
    assert tuple(h.pairs[1, 0]) == (W[1, 0], 0) and m[1, 0] > 0
    assert h.pairs[0, 2, 1] > 0 and h.pairs[0, 2, 0] > 0 and obs[2, 0] == B.ON_A_MEMBER
    assert np.isnan(obs[1, 2]) and tuple(h.pairs[2, 1]) == (-1, -1)
    assert ((h.pairs[:3, :, 0] >= 0) == ~np.isnan(obs[:, :3].T)).all()
    assert (h.pairs[:3].sum(axis=2) <= W[:3])[h.pairs[:3, :, 0] >= 0].all()


@pytest.mark.parametrize("n", SIZES)
def test_weights_of_zero_and_one_are_a_mask(n):
    """With every weight in {0, 1} the rows are those of mask = (w != 0), bit for bit, and W == m."""
    values, weights, obs = B.make_pure(n, B.ITEMS8)
    w = (np.arange(n) % 3 != 1).astype(np.uint16)
    a = B.HostSasBands(B.ITEMS8, B.PROBS8, B.PURE_WINDOWS, n, None, w, obs)
    b = B.HostSasBands(B.ITEMS8, B.PROBS8, B.PURE_WINDOWS, n, w != 0, None, obs)
    for d in range(B.PURE_DAYS):
        for h in (a, b):
            h.add(values[d], {wn: x[d % 3] for wn, x in weights.items()})
    assert (recorded(a) == recorded(b)).all() and (a.hdr[:, :, 2] == a.hdr[:, :, 0]).all()


def test_the_clock_is_the_scores_clock():
    """A day outside every window, and a window whose first day was never recorded, record nothing; LAST items wait for the closing day."""
    n = 5
    v = {"C_rz": np.arange(n) - 2.0}
    h = B.HostSasBands([("C_rz", None, B.LAST)], (0.0, 1.0), (np.array([-1, 3]), np.array([1, 4])), n)
    for d in range(5):
        h.add(v)
        assert list(h.closed) == [0, int(d >= 4)]
    assert np.isnan(h.rows[0]).all() and list(h.rows[1, 0]) == [-2.0, 2.0] and list(h.hdr[1, 0]) == [5, 0, 5] and (h.pairs == -1).all()
