"""CPU: the numpy restatement of the transport bands per zone (tests/sas_bands_zonal_reference.py) against brute force per zone, the pure
inputs of tests/test_hip_sas_bands_zonal.py on the restatement alone -- every wrong variant changes a recorded bit on them, and they meet
the conditions without which the GPU test could pass vacuously -- and the zone axis through roger_amd.bands' elementwise helpers."""
import numpy as np
import pytest

import sas_bands_reference as B
import sas_bands_zonal_reference as Z

CASES = ["contiguous", "interleaved1", "interleaved3", "interleaved1024"]


def case_of(name, weighted):
    return Z.contiguous_case(weighted) if name == "contiguous" else Z.interleaved_case(int(name[len("interleaved"):]))


def recorded_zonal(h):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint64).reshape(-1) for a in (h.rows, h.hdr, h.pairs)])


@pytest.mark.parametrize("weighted", [False, True])
def test_the_restatement_is_brute_force_per_zone(weighted):
    """np.sort(np.repeat(s, w))[T - 1] per zone on LAST items (s = v + 0.0): an empty zone, a zone of one column, a zone whose values are
    all NaN, ties across a selected rank inside one zone with the same values in another, zone == -1 columns, mask == 0 and weight 0
    inside a zone."""
    n, nz = 61, 6
    rng = np.random.default_rng(3)
    zone = np.full(n, -1)
    zone[0:20], zone[20:40], zone[40], zone[41:50], zone[50:56] = 0, 1, 2, 4, 5     # zone 3 is empty, zone 2 one column; 56 ... 60: -1
    v = rng.normal(size=n).round(1)
    v[0:20] = np.repeat([-1.0, 0.5, -0.0, 0.0, 2.0], 4)                               # ties across the ranks of 0.25, 0.5, 0.75 ...
    v[20:40] = v[0:20][::-1]                                                           # ... and the same values in another zone
    v[41:50] = np.nan                                                                  # a zone whose values are all NaN
    v[52] = np.nan
    v[58] = -100.0                                                                     # (outside every zone: must not show)
    mask = np.ones(n, dtype=np.uint8)
    mask[[3, 25]] = 0
    w = rng.integers(1, 10, size=n) if weighted else None
    if weighted:
        w[[5, 30, 51]] = 0
    probs = (0.0, 0.25, 0.5, 0.75, 1.0)
    obs = np.array([[[-1.0], [0.0], [v[40]], [1.0], [np.nan], [0.3]]])
    h = Z.HostSasBandsZonal([("C_rz", None, B.LAST)], probs, (np.array([0]), np.array([0])), n, zone, nz, mask, w, obs)
    h.add({"C_rz": v})
    wi = np.ones(n, dtype=np.int64) if w is None else w
    for z in range(nz):
        part = (zone == z) & (mask != 0) & (wi > 0)
        s = v[part] + 0.0
        num = s == s
        brute = np.sort(np.repeat(s[num], wi[part][num]))
        m, W = int(num.sum()), int(brute.size)
        assert tuple(h.hdr[0, 0, z]) == (m, int(part.sum()) - m, W), z
        if not m:
            assert np.isnan(h.rows[0, 0, z]).all() and W == 0
        for q, p in enumerate(probs):
            if m:
                assert B.same_bits(h.rows[0, 0, z, q], brute[min(max(int(np.ceil(p * float(W))), 1), W) - 1]), (z, p)
        o = obs[0, z, 0]
        assert tuple(h.pairs[0, 0, z]) == ((-1, -1) if o != o else (int((brute < o + 0.0).sum()), int((brute == o + 0.0).sum()))), z
    assert h.hdr[0, 0, 3].tolist() == [0, 0, 0] and h.pairs[0, 0, 3].tolist() == [0, 0]       # the empty zone, observed
    assert h.hdr[0, 0, 4, 0] == 0 and h.hdr[0, 0, 4, 1] > 0 and h.pairs[0, 0, 4].tolist() == [-1, -1]
    assert h.hdr[0, 0, 2].tolist()[:2] == [1, 0] and h.pairs[0, 0, 2, 1] == wi[40]             # one column, observed on it
    assert np.nanmin(h.rows) > -100.0
    off, cols = Z.zone_lists(zone, nz, Z.participation(n, zone, mask, w))
    assert off[-1] == cols.size and all((np.diff(cols[off[z]:off[z + 1]]) > 0).all() and (zone[cols[off[z]:off[z + 1]]] == z).all() for z in range(nz))


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_the_pure_inputs_have_teeth(variant):
    """The weight read at the list position instead of the column, a column counted in its neighbour's zone, the W of the whole domain
    used for T: each changes a recorded bit of the pure inputs (the first needs a weight plane), in the 3-zone and the contiguous case."""
    for name in ("interleaved3", "contiguous"):
        changed = {}
        for weighted in (False, True):
            n, zone, nz = case_of(name, weighted)
            a, b = (Z.restate_zonal(n, zone, nz, B.ITEMS8, 8, weighted, variant=v)[0] for v in (None, variant))
            changed[weighted] = int((recorded_zonal(a) != recorded_zonal(b)).sum())
        assert changed[True] > 0 and (variant == "weight_by_position" or changed[False] > 0), (name, changed)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_the_pure_inputs_meet_their_conditions(name, weighted):
    n, zone, nz = case_of(name, weighted)
    items, n_probs = (B.ITEMS8, 8) if nz < 1024 else (B.ITEMS8[:3], 3)
    h, (values, _, mask, w, obs) = Z.restate_zonal(n, zone, nz, items, n_probs, weighted)
    part = Z.participation(n, zone, mask, w)
    off, _ = Z.zone_lists(zone, nz, part)
    sizes = np.diff(off)
    rows, hdr, pairs = h.rows, h.hdr, h.pairs
    assert list(h.closed) == [1, 1, 1, 0] and rows.shape == (4, len(items), nz, n_probs)
    assert np.isnan(rows[3]).all() and not hdr[3].any() and (pairs[3] == -1).all()
    assert (hdr[:3, :, :, 0] + hdr[:3, :, :, 1] == sizes[None, None, :]).all()                 # every participant is in exactly one zone's counts
    if name == "contiguous":
        assert tuple(sizes) == Z.SIZES and (zone == -1).any()
        if weighted:   # mask == 0 and weight 0 inside a zone
            assert ((zone >= 0) & (mask == 0)).any() and ((zone >= 0) & (w == 0)).any()
        assert np.isnan(rows[:3, :, 0]).all() and not hdr[:3, :, 0].any()                      # the empty zone ...
        assert ((pairs[:3, :, 0] == 0) | np.isnan(obs[:, 0, :3].T)[..., None]).all()             # ... whose pair is (0, 0) where observed
    if name == "interleaved1":
        assert sizes[0] == (2049 if not weighted else part.sum())
    if weighted:
        assert (hdr[:3, :, :, 2] != hdr[:3, :, :, 0]).any()
    else:
        assert (hdr[..., 2] == hdr[..., 0]).all()
    assert (hdr[:3, :, :, 1] > 0).any() and (rows[:3] < 0).any()
    # zones differ: some quantile of some item is not the same in every zone with a number
    if nz > 1:
        assert any(len(np.unique(rows[k, j, hdr[k, j, :, 0] > 0, q])) > 1 for k in range(3) for j in range(len(items)) for q in range(n_probs))
    # observations: below all members, above all, on a member (item 2, window 0), missing -- per zone
    big = sizes > 0
    W0 = hdr[0, 0, :, 2]
    assert (pairs[0, 0, 0::2] == 0).all() and (pairs[0, 0, 1::2, 0] == W0[1::2]).all() and (pairs[0, 0, 1::2, 1] == 0).all()
    assert (pairs[0, 2, big, 1] > 0).any()
    assert ((pairs[:3, :, :, 0] >= 0) == ~np.isnan(np.moveaxis(obs[:, :, :3], 2, 0))).all() and (pairs[:3] == -1).any()


def test_the_helpers_of_roger_amd_bands_take_the_zone_axis():
    """bands.inside, bands.pit and bands.rank_histogram are elementwise: on (K, items, zones) arrays they give what they give zone by zone."""
    from roger_amd import bands

    n, zone, nz = case_of("interleaved3", True)
    h, _ = Z.restate_zonal(n, zone, nz, B.ITEMS8, 8, True)
    below, equal, total = h.pairs[..., 0], h.pairs[..., 1], h.hdr[..., 2]
    ins, pit = bands.inside(below, equal, total, 0.05, 0.95), bands.pit(below, equal, total)
    assert ins.shape == pit.shape == below.shape == (4, 8, 3)
    for z in range(nz):
        assert (ins[:, :, z] == bands.inside(below[:, :, z], equal[:, :, z], total[:, :, z], 0.05, 0.95)).all()
        assert B.same_bits(pit[:, :, z], bands.pit(below[:, :, z], equal[:, :, z], total[:, :, z]))
    assert ins.any() and not ins.all()
    assert (bands.rank_histogram(pit) == sum(bands.rank_histogram(pit[:, :, z]) for z in range(nz))).all() and bands.rank_histogram(pit).sum() > 0
