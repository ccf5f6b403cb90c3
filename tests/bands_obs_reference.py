"""Where the observation falls in the ensemble (rh_bands_observations, roger_amd/csrc/rh_bands.h) restated on the host in plain numpy,
on top of tests/bands_reference.py, tests/bands_weighted_reference.py and tests/bands_zonal_reference.py: their clocks, their SUM / LAST
aggregation and their participants.  Imports nothing from roger_amd.

Everything is the bands' rule as it stands.  On top of it an item may carry observations: one float64 series per item without zones, one
per zone with zones; NaN means missing.  The series is indexed from the request's start, not from the first counted interval: for row
interval number k the element is o = obs[k + first_index], first_index = (t_first - start) / frequency; an index beyond the series means
missing.  On a counted step, per item (and zone), an int64 pair (below, equal):
    o a NaN (missing, or the item has no observations):  below = equal = -1
    else o' = o + 0.0 and, with x, wx the participants that are numbers (wx: ones, or the integer weights):
        below = int(wx[x < o'].sum());  equal = int(wx[x == o'].sum())          (m == 0: (0, 0))
The total is T_tot = m (plain, zonal) or W (weighted): 0 <= below, 0 <= equal, below + equal <= T_tot, and for a recorded probability p
with T = clamp(ceil(p * T_tot), 1, T_tot) and recorded quantile q:  q <= o <=> below + equal >= T,  q < o <=> below >= T  -- so
"inside [q_lo, q_hi]" <=> below + equal >= T_lo and below < T_hi (`inside_of`).
The host doubles record the pairs beside their classes' rows: one row of pairs per counted interval, -1 while no observations are set."""
import numpy as np

from bands_reference import LAST, SUM, HostBands
from bands_weighted_reference import HostWeightedBands, target_of
from bands_zonal_reference import HostZonalBands
from durations_reference import clock

MISSING = (-1, -1)


def pair_of(s, o, w=None):
    """(below, equal) of the interval values s (n,) of the masked-in columns against the observation o; w: integer weights (n,), 0: the
    column takes no part, None: every column counts 1."""
    o = float(o)
    if o != o:
        return MISSING
    x = np.asarray(s, dtype=np.float64).reshape(-1) + 0.0
    wx = np.ones(x.size, dtype=np.int64) if w is None else np.asarray(w).reshape(-1).astype(np.int64)
    assert wx.size == x.size and (wx >= 0).all()
    number = (x == x) & (wx != 0)
    x, wx = x[number], wx[number]
    o = o + 0.0
    return int(wx[x < o].sum()), int(wx[x == o].sum())


def obs_at(series, k, first_index=0):
    """The element of a series for row interval number k: NaN beyond the series (and in front of it)."""
    series = np.asarray(series, dtype=np.float64).reshape(-1)
    at = int(k) + int(first_index)
    return float(series[at]) if 0 <= at < series.size else float("nan")


def inside_of(below, equal, total, p_lo, p_hi):
    """q(p_lo) <= o <= q(p_hi) from the counts alone; total >= 1 and the pair is not MISSING."""
    return below + equal >= target_of(p_lo, total) and below < target_of(p_hi, total)


class _Observed:
    """The mix-in in front of HostBands / HostWeightedBands: `observe(obs, first_index)` with obs (J, intervals), and from then on
    self.pairs gains one row (J, 2) per counted interval.  The interval value of a column is what the class in use has just formed: the
    SUM accumulator after its `add`, or the plane itself."""

    obs, first_index = None, 0

    def observe(self, obs, first_index=0):
        self.obs = None if obs is None else np.asarray(obs, dtype=np.float64).reshape(len(self.kinds), -1)
        self.first_index = int(first_index)

    def _weights(self):
        return None

    def add(self, t0, t1, planes):
        super().add(t0, t1, planes)
        if not hasattr(self, "pairs"):
            self.pairs = []
        _, _, k, counted = clock(int(t0), int(t1), self.iv, self.t_first)
        if not counted:
            return
        row = []
        for j, kind in enumerate(self.kinds):
            s = self.acc[j, self.on] if kind == SUM else np.asarray(planes[j], dtype=np.float64).reshape(-1)[self.on]
            row.append(MISSING if self.obs is None else pair_of(s, obs_at(self.obs[j], k, self.first_index), self._weights()))
        self.pairs.append(row)

    def pair_rows(self):
        """(rows, J, 2) int64."""
        return np.array(getattr(self, "pairs", []), dtype=np.int64).reshape(-1, len(self.kinds), 2)


class HostObsBands(_Observed, HostBands):
    pass


class HostObsWeightedBands(_Observed, HostWeightedBands):
    def _weights(self):
        return self.w[self.on]


class HostObsZonalBands(HostZonalBands):
    """A HostObsBands per zone, each under mask = (zone == z) with that zone's series: obs (J, Z, intervals)."""

    def __init__(self, kinds, probs, n, zone, n_zones, interval=86400, t_first=0):
        super().__init__(kinds, probs, n, zone, n_zones, interval, t_first)
        zone = np.asarray(zone).reshape(-1)
        self.per_zone = [HostObsBands(kinds, probs, n, zone == z, interval, t_first) for z in range(int(n_zones))]

    def observe(self, obs, first_index=0):
        obs = None if obs is None else np.asarray(obs, dtype=np.float64).reshape(self.nv, len(self.per_zone), -1)
        for z, h in enumerate(self.per_zone):
            h.observe(None if obs is None else obs[:, z], first_index)

    def pair_rows(self):
        """(rows, J, Z, 2) int64."""
        return np.stack([h.pair_rows() for h in self.per_zone], axis=2)


__all__ = ["LAST", "SUM", "MISSING", "pair_of", "obs_at", "inside_of", "HostObsBands", "HostObsWeightedBands", "HostObsZonalBands"]
