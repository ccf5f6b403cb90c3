"""CPU: the restatement of the zonal recorder (tests/sas_zonal_reference.py) against the shipped rule of the catchment totals: for every
zone z the walk over the zone's slots gives, bit for bit, sas_totals_reference.item_block(values, weight, zone == z) -- and the inputs
can tell a wrong order of summation from the right one."""
import numpy as np
import pytest

import sas_totals_reference as R
import sas_zonal_reference as Z

SIZES = [1, 5, 255, 256, 257, 300, 1000, 65837]


def nansum_block(values, weight, mask):
    """The row block by plain np.nansum over the counted cells: the right cells in some other order."""
    v = np.asarray(values, dtype=np.float64)
    e = R.eligible(v.shape[0], weight, mask)
    w = np.ones(v.shape[0]) if weight is None else np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if v.ndim == 1:
            c = e & ~np.isnan(v)
            return np.array([w[c].sum(), c.sum(), (v[c] * w[c] if weight is not None else v[c]).sum(), 0.0, 0.0])
        t = v[e] * w[e][:, None] if weight is not None else v[e]
        return np.concatenate([[w[e].sum(), e.sum()], np.nansum(t, axis=0)])


@pytest.mark.parametrize("n", SIZES)
def test_the_walk_is_the_totals_rule_of_every_zone(n):
    ages = 30
    d = R.make_inputs(n, ages)
    maps = Z.zone_maps(n)
    assert ("many" in maps) == (n == 1000)
    differs = 0
    for mname, (zone, nz) in maps.items():
        ix = Z.Index(zone, nz)
        assert (ix.ncells == 0).any() and ix.ncells.sum() == np.count_nonzero(zone >= 0)
        for day in ((1, -1) if n <= 1000 else (1,)):
            got = Z.want_rows(ix, d, R.ITEMS, day)
            for z in range(nz):
                want = R.want_row(d, R.ITEMS, zone == z, day)
                for key, block in want.items():
                    assert R.same_bits(got[key][z], block), (n, mname, day, z, key, got[key][z][:6], block[:6])
                if day == 1:
                    for it in R.ITEMS[:5]:
                        v, w = (it, None) if isinstance(it, str) else it
                        key = v if w is None else f"{v}_by_{w}"
                        plain = nansum_block(d[v], None if w is None else d[w][1], zone == z)
                        k = slice(0, 3) if d[v].ndim == 1 else slice(0, None)
                        differs += not R.same_bits(plain[k], want[key][k])
    if n >= 255:
        assert differs, "np.nansum gives the rule's bits everywhere: these inputs cannot tell a wrong order from the right one"


def test_the_maps_hold_what_they_promise():
    zone, nz = Z.zone_maps(65837)["sparse"]
    far = np.flatnonzero(zone == 3)              # (ids above the empty one are shifted by one)
    assert far.size and far.min() >= 65536 and np.count_nonzero(zone == 4) == 1 and not (zone == 2).any() and nz == 5
    zone, nz = Z.zone_maps(1000)["many"]
    assert nz == 300 and np.unique(zone[zone >= 0]).size > 250
    zone, nz = Z.zone_maps(300)["blocks"]
    edges = np.flatnonzero(np.diff(zone[zone >= 0]) != 0)
    assert edges.size and (zone == -1).any()
    ix = Z.Index(Z.zone_maps(65837)["mix"][0], 7)
    assert max(len(a) for z in ix.acc for a in z) == 2          # a second round of accumulators
    assert ix.slot_tile[ix.runs[0][-1]] // 256 == 1             # ... and a second group of runs: three levels


def test_a_wrong_order_is_seen():
    """The walk with the slots of a zone taken in DEcreasing run order differs from the rule in some bit."""
    n = 65837
    d = R.make_inputs(n, 30)
    zone, nz = Z.zone_maps(n)["mix"]
    ix = Z.Index(zone, nz)
    right = Z.zone_blocks(ix, d["sa_s"])
    for r in ix.runs:
        r.reverse()
    assert not R.same_bits(Z.zone_blocks(ix, d["sa_s"]), right)
