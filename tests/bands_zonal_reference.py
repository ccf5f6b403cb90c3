"""The ensemble bands per zone (rh_bands_configure_zonal, roger_amd/csrc/rh_bands.h) restated through the ONE rule they promise: block z
of a row is the row tests/bands_reference.py's HostBands records with mask = (zone == z).  Imports nothing from roger_amd.

`zone`: an index 0 ... n_zones - 1 per column, negative: the column takes no part (a mask is folded into it by the caller, as the C ABI
has it).  A zone without a column gives m = 0, n_nan = 0 and NaN."""
import numpy as np

from bands_reference import HostBands, quantiles_of


def fold(zone, mask=None):
    """The zone index with a mask folded in: -1 where mask == 0."""
    zone = np.asarray(zone).reshape(-1).astype(np.int64)
    return zone if mask is None else np.where(np.asarray(mask).reshape(-1) != 0, zone, -1)


def zonal_quantiles_of(s, zone, n_zones, probs):
    """(values (Z, P), counts (Z, 2) {m, n_nan}) of the interval values s (n,)."""
    s, zone = np.asarray(s, dtype=np.float64).reshape(-1), np.asarray(zone).reshape(-1)
    values, counts = np.full((n_zones, len(probs)), np.nan), np.zeros((n_zones, 2), dtype=np.int64)
    for z in range(n_zones):
        values[z], counts[z, 0], counts[z, 1] = quantiles_of(s[zone == z], probs)
    return values, counts


class HostZonalBands:
    """A HostBands per zone, each under mask = (zone == z); rows(): hdr (rows, 2) {k, t1}, counts (rows, J, Z, 2), values (rows, J, Z, P)."""

    def __init__(self, kinds, probs, n, zone, n_zones, interval=86400, t_first=0):
        zone = np.asarray(zone).reshape(-1)
        assert zone.size == int(n) and 1 <= int(n_zones) <= 1024 and zone.max() < int(n_zones)
        self.nv, self.np = len(kinds), len(probs)
        self.per_zone = [HostBands(kinds, probs, n, zone == z, interval, t_first) for z in range(int(n_zones))]

    def add(self, t0, t1, planes):
        for h in self.per_zone:
            h.add(t0, t1, planes)

    def rows(self):
        per = [h.rows() for h in self.per_zone]
        hdr = per[0][0][:, :2].copy()
        assert all(np.array_equal(p[0][:, :2], hdr) for p in per)
        counts = np.stack([p[0][:, 2:].reshape(-1, self.nv, 2) for p in per], axis=2)
        values = np.stack([p[1] for p in per], axis=2)
        return hdr, counts, values
