"""The transport bands per zone (rh_sas_bands_configure_zonal, roger_amd/csrc/rh_sas_bands_zonal.h) restated through the ONE rule they
promise: block (item, zone z) of a window is what tests/sas_bands_reference.py's HostSasBands records with mask = (zone == z) & mask, the
same weights, probabilities and windows, and obs = obs[:, z].  Imports nothing from roger_amd.

`zone`: -1: the column is outside every zone, else 0 ... n_zones - 1.  A zone without a participating column gives m = 0, n_nan = 0,
W = 0, NaN rows and, with an observation that is not missing, the pair (0, 0).
The `variant` argument exists for the tests that show the inputs have teeth: three ways a per-zone kernel can go wrong."""
import numpy as np

import sas_bands_reference as B
from sas_bands_reference import HostSasBands

VARIANTS = ("weight_by_position", "neighbour_zone", "domain_W")


def participation(n, zone, mask=None, weights=None):
    """bool (n,): zone >= 0, mask != 0, weight != 0."""
    part = np.asarray(zone).reshape(-1) >= 0
    if mask is not None:
        part = part & (np.asarray(mask).reshape(-1) != 0)
    if weights is not None:
        part = part & (np.asarray(weights).reshape(-1) != 0)
    return part


def zone_lists(zone, n_zones, part):
    """The stable counting sort over the participating columns: (zone_off (n_zones + 1,), zone_cols ascending within a zone)."""
    zone = np.asarray(zone).reshape(-1)
    cols = np.flatnonzero(part)
    cols = cols[np.argsort(zone[cols], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(zone[cols], minlength=n_zones))]).astype(np.int64)
    return off, cols.astype(np.int32)


class _DomainW(HostSasBands):
    """HostSasBands whose target T is taken from the W of ALL zones' participants (`domain`, bool (n,)) instead of the zone's own."""

    def __init__(self, *a, domain=None, **kw):
        super().__init__(*a, **kw)
        self.domain = domain

    def add(self, held, weights=None, variant=None):
        weights = held if weights is None else weights
        now = self.win.next()
        if now is None:
            return
        k, first, closes = now
        kinds = [kd for _, _, kd in self.items]
        if not closes and all(kd == B.LAST for kd in kinds):
            return
        w = np.ones(self.n, dtype=np.int64) if self.weights is None else self.weights
        part = self.mask & (w > 0)
        both = part | self.domain
        s = B.band_day(self.acc, kinds, [held[v] for v, _, _ in self.items],
                       [None if wn is None else np.asarray(weights[wn]).reshape(-1) for _, wn, _ in self.items], both, first, closes)
        if not closes:
            return
        for j in range(len(self.items)):
            x, wx = s[j][part], w[part]
            ok = x == x
            x, wx = x[ok], wx[ok]
            dom = s[j][self.domain]
            W_all = int(w[self.domain][dom == dom].sum())
            m, W = int(x.size), int(wx.sum())
            self.hdr[k, j] = (m, int(ok.size - m), W)
            if m:
                o = np.argsort(x, kind="stable")
                cw = np.cumsum(wx[o])
                for q, p in enumerate(self.probs):
                    T = min(max(int(np.ceil(p * float(W_all))), 1), W)
                    self.rows[k, j, q] = x[o][np.searchsorted(cw, T, side="left")]
            if self.obs is not None:
                self.pairs[k, j] = B.obs_pair(s[j][part], w[part], self.obs[j, k])


class HostSasBandsZonal:
    """A HostSasBands per zone, each under mask = (zone == z) & mask and obs[:, z]: rows (K, J, Z, P), hdr (K, J, Z, 3), pairs (K, J, Z, 2)."""

    def __init__(self, items, probs, windows, n, zone, n_zones, mask=None, weights=None, obs=None, variant=None):
        zone = np.asarray(zone).reshape(-1).astype(np.int64)
        n_zones = int(n_zones)
        assert variant is None or variant in VARIANTS
        assert zone.size == int(n) and 1 <= n_zones <= 1024 and zone.min() >= -1 and zone.max() < n_zones
        mask = np.ones(int(n), dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        obs = None if obs is None else np.asarray(obs, dtype=np.float64).reshape(len(items), n_zones, -1)
        part = participation(n, zone, mask, weights)
        off, cols = zone_lists(zone, n_zones, part)
        self.per_zone = []
        for z in range(n_zones):
            mz, wz, cls, kw = (zone == z) & mask, weights, HostSasBands, {}
            mine = cols[off[z]:off[z + 1]]
            if variant == "weight_by_position" and weights is not None:
                # the weight is read at the entry's position in the list, not at its column; a wrong weight of 0 leaves the column out
                # here where a kernel would keep it in m with nothing in the bins: either way the recorded bits differ from the rule's
                wz = np.asarray(weights).reshape(-1).copy()
                wz[mine] = np.asarray(weights).reshape(-1)[np.arange(off[z], off[z + 1])]
                mz = np.zeros(int(n), dtype=bool)
                mz[mine] = True
            elif variant == "neighbour_zone" and off[z + 1] < cols.size:
                mz = mz.copy()
                mz[cols[off[z + 1]]] = True                 # the list read one entry too far: the first column of the next zone
            elif variant == "domain_W":
                cls, kw = _DomainW, dict(domain=part)
            self.per_zone.append(cls(items, probs, windows, n, mz, wz, None if obs is None else obs[:, z], **kw))

    def add(self, held, weights=None):
        for h in self.per_zone:
            h.add(held, weights)

    rows = property(lambda self: np.stack([h.rows for h in self.per_zone], axis=2))
    hdr = property(lambda self: np.stack([h.hdr for h in self.per_zone], axis=2))
    pairs = property(lambda self: np.stack([h.pairs for h in self.per_zone], axis=2))
    closed = property(lambda self: self.per_zone[0].closed)
    win = property(lambda self: self.per_zone[0].win)


# ---- the inputs of the pure GPU tests: the values, weights and windows of sas_bands_reference.make_pure under a zone map ----
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2049)   # participating columns per zone; 2049 = 256 x 8 + 1: the second trip of the in-flight loop


def contiguous_case(weighted):
    """(n, zone, n_zones): zone z holds exactly SIZES[z] PARTICIPATING columns under pure_participation(n, weighted), one zone after the
    other; a column that does not participate carries the zone of its neighbourhood (mask == 0 and weight 0 inside a zone); what is left
    over is outside every zone (-1)."""
    n = 4600 if weighted else sum(SIZES) + 7
    mask, w = B.pure_participation(n, weighted)
    part = np.ones(n, dtype=bool) if mask is None else (mask != 0) & (w != 0)
    rank = np.cumsum(part) - part                       # participating columns before this one
    edges = np.cumsum(SIZES)
    assert part.sum() > edges[-1]
    zone = np.searchsorted(edges, rank, side="right")
    zone = np.where(zone < len(SIZES), zone, -1).astype(np.int32)
    return n, zone, len(SIZES)


def interleaved_case(n_zones):
    """(n, zone, n_zones): zone = i % n_zones; one zone of 2049 columns, three of 257, or 1024 of two and one."""
    n = {1: 2049, 3: 3 * 257, 1024: 1024 + 513}[n_zones]
    return n, (np.arange(n) % n_zones).astype(np.int32), n_zones


def zonal_obs(items, values, zone, n_zones, part):
    """obs (J, Z, K) from make_pure's (J, K): per zone shifted, below all members in window 0 of the even zones and above all in the odd
    ones (item 0), missing in a pattern over (item, zone) in window 2, and exactly on a member -- C_rz (LAST) of the zone's first
    participating column on day 0 -- for item 2 in window 0."""
    _, _, obs = B.make_pure(zone.size, items)
    out = np.repeat(obs[:, None, :], n_zones, axis=1) + 0.125 * (np.arange(n_zones) % 7)[None, :, None]
    out[0, 0::2, 0], out[0, 1::2, 0] = -1e6, 1e6
    jz = np.add.outer(np.arange(len(items)), np.arange(n_zones))
    out[:, :, 2] = np.where(jz % 2 == 1, np.nan, out[:, :, 2])
    if len(items) > 2:
        off, cols = zone_lists(zone, n_zones, part)
        for z in range(n_zones):
            if off[z + 1] > off[z]:
                v = values[0]["C_rz"][cols[off[z]]]
                out[2, z, 0] = v if v == v else out[2, z, 0]
    return out


def restate_zonal(n, zone, n_zones, items, n_probs, weighted, observed=True, variant=None):
    """(the restatement after the seven pure days, the inputs it was given)"""
    values, weights, _ = B.make_pure(n, items)
    mask, w = B.pure_participation(n, weighted)
    obs = zonal_obs(items, values, zone, n_zones, participation(n, zone, mask, w)) if observed else None
    h = HostSasBandsZonal(items, B.pure_probs(n_probs), B.PURE_WINDOWS, n, zone, n_zones, mask, w, obs, variant)
    for d in range(B.PURE_DAYS):
        h.add(values[d], {wn: a[d % 3] for wn, a in weights.items()})
    return h, (values, weights, mask, w, obs)
