"""CPU: the restatement of the transport bands by age per zone (tests/sas_age_bands_zonal_reference.py) equals brute force per zone and
age class, its pure inputs meet the conditions the GPU tests rely on, and each wrong variant changes a recorded bit of those inputs."""
import numpy as np
import pytest

import sas_age_bands_reference as R
import sas_age_bands_zonal_reference as Z

AGES = 30


def participation(cfg):
    n, mask, w, zones, n_zones = cfg
    wts = np.ones(n, dtype=np.int64) if w is None else w.astype(np.int64)
    part = (np.ones(n, dtype=bool) if mask is None else mask != 0) & (wts > 0)
    return part, wts


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["sizes_interleaved", "three", "short_only"])
def test_restatement_is_brute_force_per_zone_and_age_class(kind, weighted):
    """np.sort(np.repeat(A[cols_z, a], w))[T - 1] with T = clip(ceil(p W), 1, W) over the numbers of the zone's participating columns."""
    items = R.ITEMS4[:2]
    cfg, values = Z.make_zonal_pure(kind, AGES, items, weighted)
    n, mask, w, zones, n_zones = cfg
    if weighted:   # (the same participation under weights 0 ... 6: np.repeat writes every member out)
        w = np.where(w > 0, w % 6 + 1, 0).astype(np.uint16)
        cfg = (n, mask, w, zones, n_zones)
    part, wts = participation(cfg)
    h = Z.HostSasAgeBandsZonal(items, R.PROBS8, Z.ZONAL_WINDOWS, n, zones, n_zones, mask, w)
    for d in range(Z.ZONAL_DAYS):
        h.add(values[d])
    rows, hdr = h.result({v: R.width_of(v, AGES) for v in items})
    assert list(h.closed) == [1, 1, 0]
    for k, d in ((0, 0), (1, 2)):
        for v in items:
            A = values[d][v]
            assert rows[v].shape == (3, n_zones, A.shape[1], 8) and hdr[v].shape == (3, n_zones, A.shape[1], 3)
            for z in range(n_zones):
                cols = np.flatnonzero(part & (zones == z))
                for a in range(A.shape[1]):
                    s = A[cols, a] + 0.0
                    ok = s == s
                    m, W = int(ok.sum()), int(wts[cols][ok].sum())
                    assert hdr[v][k, z, a].tolist() == [m, int(cols.size) - m, W], (v, k, z, a)
                    if not m:
                        assert np.isnan(rows[v][k, z, a]).all()
                        continue
                    flat = np.sort(np.repeat(s[ok], wts[cols][ok]))
                    want = [flat[min(max(int(np.ceil(p * float(W))), 1), W) - 1] for p in R.PROBS8]
                    assert Z.same_bits(rows[v][k, z, a], np.array(want)), (v, k, z, a)
    assert np.isnan(rows[items[0]][2]).all() and not hdr[items[0]][2].any()


@pytest.mark.parametrize("kind", Z.MAPS)
def test_maps_meet_their_conditions(kind):
    """The sizes the maps are named for, in participating columns; columns with zones == -1 that would take part; with weights, columns of
    mask 0 and of weight 0 inside a zone; and zone orders that differ from the column order where the map says so."""
    for weighted in (False, True):
        cfg = Z.zone_map(kind, weighted)
        n, mask, w, zones, n_zones = cfg
        part, wts = participation(cfg)
        sizes = np.bincount(zones[part & (zones >= 0)], minlength=n_zones)
        assert zones.dtype == np.int32 and zones.min() == -1 and zones.max() == n_zones - 1 and (part & (zones == -1)).sum() >= 2
        if kind.startswith("sizes"):
            assert tuple(sizes) == Z.SIZES
        if kind == "sizes_interleaved":
            cols, off = Z.zone_order(zones, part, n_zones)
            assert (np.diff(cols) < 0).any() and all((np.diff(cols[off[z]:off[z + 1]]) > 0).all() for z in range(n_zones))
        if kind == "one":
            assert n_zones == 1 and sizes[0] == 2100
        if kind == "three":
            assert tuple(sizes) == (150, Z.SHORT, 1694)
        if kind == "many":
            assert n_zones == 1024 and sizes.sum() == 2100 and (sizes == 0).any() and (sizes == 1).any() and sizes.max() < Z.SHORT
        if kind == "short_only":
            assert sizes.min() == 1 and sizes.max() == Z.SHORT
        if kind == "long_only":
            assert sizes.min() == Z.SHORT + 1
        if weighted:
            inside = zones >= 0
            assert (inside & (mask == 0)).any() and (inside & (w == 0) & (mask != 0)).any() and (wts[part] > 1).any()
        if Z.NAN_ZONE[kind] is not None:
            assert sizes[Z.NAN_ZONE[kind]] > 0 and sizes[(Z.NAN_ZONE[kind] + 1) % n_zones] > 0


@pytest.mark.parametrize("weighted", [False, True])
def test_pure_values_meet_their_conditions(weighted):
    """On the map of all sizes: an empty zone and a zone of one column; a zone that is NaN in one age class (m == 0 there, not in the age
    class beside it and not in the zone beside it); ties across a selected rank in a zone, with the same two values in another zone; W != m
    under weights; both zeros, +-inf and a subnormal among the participants of some zone."""
    items = R.ITEMS4[:1]
    h, cfg, values = Z.restate_zonal_pure("sizes", AGES, weighted)
    n, mask, w, zones, n_zones = cfg
    part, wts = participation(cfg)
    rows, hdr = Z.sliced(h, AGES, 1, 8)
    rows, hdr = rows[items[0]], hdr[items[0]]
    A = values[0][items[0]]
    assert not hdr[0, 0].any() and np.isnan(rows[0, 0]).all()                       # the empty zone: what configure wrote
    assert hdr[0, 1, :, 0].max() == 1 and hdr[0, 1, :, 0].min() == 0               # one column, NaN in the NaN age class
    nz = Z.NAN_ZONE["sizes"]
    assert hdr[0, nz, Z.ZONE_NAN_AGE, 0] == 0 and hdr[0, nz, Z.ZONE_NAN_AGE, 1] == Z.SIZES[nz] and hdr[0, nz, Z.ZONE_NAN_AGE, 2] == 0
    assert hdr[0, nz, Z.ZONE_NAN_AGE + 1, 0] > 0 and hdr[0, nz + 1, Z.ZONE_NAN_AGE, 0] > 0
    for z in (4, 8):   # two values only: a selected rank falls among equal members, here and in the other zone
        tie = A[part & (zones == z), R.TIE_AGE]
        assert set(np.unique(tie)) == {-3.5, 2.25} and set(rows[0, z, R.TIE_AGE]) == {-3.5, 2.25}
    if weighted:
        assert (hdr[0, 2:, :, 2] != hdr[0, 2:, :, 0]).any()
    inside = A[part & (zones >= 0)]
    zero = inside[:, R.ZERO_AGE]
    assert (np.signbit(zero) & (zero == 0)).any() and (~np.signbit(zero) & (zero == 0)).any()
    edge = inside[:, R.EDGE_AGE]
    assert np.isposinf(edge).any() and np.isneginf(edge).any() and (edge == 5e-324).any()


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_each_wrong_variant_changes_a_recorded_bit(variant):
    """weight_at_column needs weights whose zone-ordered index is not the column index; the other three show on either participation."""
    items = R.ITEMS4[:1]
    for weighted in ((True,) if variant == "weight_at_column" else (False, True)):
        cfg, values = Z.make_zonal_pure("sizes_interleaved", AGES, items, weighted)
        n, mask, w, zones, n_zones = cfg
        got = []
        for v in (None, variant):
            h = Z.HostSasAgeBandsZonal(items, R.PROBS8, Z.ZONAL_WINDOWS, n, zones, n_zones, mask, w)
            for d in range(Z.ZONAL_DAYS):
                h.add(values[d], v)
            got.append(h.result({items[0]: R.width_of(items[0], AGES)}))
        (rows, hdr), (vrows, vhdr) = got
        changed = not Z.same_bits(rows[items[0]], vrows[items[0]]) or (hdr[items[0]] != vhdr[items[0]]).any()
        assert changed, (variant, weighted)
