"""The transport bands by age per zone of the SAS context (rh_sas_age_bands_configure_zonal, roger_amd/csrc/rh_sas_age_bands.h) restated on
the host in plain numpy.  Importing this module imports nothing from roger_amd.

The rule is one promise: block (item j, zone z, age class a) of window k -- rows[k][z][a][probability], hdr[k][z][a] = {m, n_nan, W} of item
j -- is what tests/sas_age_bands_reference.py records for item j and age class a with mask = (zones == z) & mask and the same weights,
probabilities and windows.  So `HostSasAgeBandsZonal` holds one HostSasAgeBands per zone and restates nothing of the selection.  A column
with zones == -1, mask == 0 or weight 0 is in no zone's counts; a zone with m == 0 in an age class gives NaN rows and W = 0 there.
The `variant` arguments exist for the tests that show the inputs have teeth: each is a mistake the device code could make."""
import functools

import numpy as np

from sas_age_bands_reference import (EDGE_AGE, ITEMS4, NAN_AGE, TIE_AGE, ZERO_AGE, HostSasAgeBands, age_participation, make_age_pure,  # noqa: F401
                                     select_ages, width_of)
from sas_bands_reference import PROBS8, pure_probs  # noqa: F401
from sas_scores_reference import same_bits  # noqa: F401

VARIANTS = ("weight_at_column", "zone_off_shifted", "domain_W", "less_than")
SHORT = 256                                                 # RH_SELECT_BLOCK: zones of 1 ... SHORT participating columns take the one-key-per-thread kernel
ZONAL_WINDOWS = (np.array([0, 1, 5]), np.array([0, 2, 9]))  # first == closes; two days; one that closes on a day never reached
ZONAL_DAYS = 3
ZONE_NAN_AGE = 15                                           # the age class in which zone NAN_ZONE of a map holds NaN only
MANY_SAMPLE = tuple(range(3, 1024, 64))                     # the zones of the 1024-zone map that are restated on every day


def days_of(kind):
    """The days over which EVERY zone of the map is restated: the 1024 zones stop behind the first closing day, because the restatement is a
    call per zone and age class; behind it the zones MANY_SAMPLE are restated (restate_sampled)."""
    return 1 if kind == "many" else ZONAL_DAYS


def zone_order(zones, part, n_zones):
    """(part_cols, zone_off): the participating columns in zone order, ascending within a zone (a stable sort), and where each zone starts."""
    cols = np.flatnonzero(part & (zones >= 0))
    cols = cols[np.argsort(zones[cols], kind="stable")]
    return cols, np.concatenate([[0], np.cumsum(np.bincount(zones[cols], minlength=n_zones))])


def _less_than(s, w, probs):
    """The variant `<` for `<=`: the smallest s whose weight STRICTLY below it reaches T; none: the key of all bits set, a NaN pattern."""
    number = s == s
    x, wx = s[number], w[number]
    out = np.full(len(probs), np.nan)
    W = int(wx.sum())
    o = np.argsort(x, kind="stable")
    uniq, first = np.unique(x[o], return_index=True)
    below = np.concatenate([[0], np.cumsum(wx[o])])[first]   # the weight strictly below every distinct value
    for q, p in enumerate(probs):
        T = min(max(int(np.ceil(float(p) * float(W))), 1), W) if W else 1
        ok = uniq[below >= T]
        out[q] = ok[0] if ok.size else np.nan
    return out


def select_zone_variant(A, zones, n_zones, part, w, probs, z, variant):
    """(rows (W, P), hdr (W, 3)) of zone z under a mistake.  weight_at_column: the weight of the participant at zone-ordered index i read
    from the plane at i itself, where the plane at part_cols[i] belongs; zone_off_shifted: the zone's run starts and ends one entry late,
    so its first column is lost and the next zone's first column is counted; domain_W: T from the W of all zones together; less_than:
    the cumulative weight over the members strictly below."""
    A, w = np.asarray(A, dtype=np.float64), np.asarray(w).astype(np.int64)
    cols, off = zone_order(zones, part, n_zones)
    lo, hi = int(off[z]), int(off[z + 1])
    if variant == "zone_off_shifted":
        lo, hi = min(lo + 1, cols.size), min(hi + 1, cols.size)
    mine = np.zeros(part.size, dtype=bool)
    mine[cols[lo:hi]] = True
    wv = w.copy()
    if variant == "weight_at_column":
        wv[cols[lo:hi]] = np.maximum(w[lo:hi], 1)
    rows, hdr = select_ages(A, mine, wv, probs)
    if variant == "domain_W":
        every = np.zeros(part.size, dtype=bool)
        every[cols] = True
        for a in range(A.shape[1]):
            s = A[:, a] + 0.0
            Wa, Wd = int(w[mine & (s == s)].sum()), int(w[every & (s == s)].sum())
            if Wa:   # (the selection is not restated: T_d = T(p, W_d) is asked of it as the probability (T_d - 0.5) / W_a)
                pr = [min(1.0, (min(max(int(np.ceil(float(p) * float(Wd))), 1), Wd) - 0.5) / Wa) for p in probs]
                rows[a] = select_ages(A[:, a:a + 1], mine, wv, pr)[0][0]
    if variant == "less_than":
        for a in range(A.shape[1]):
            if hdr[a, 0]:
                rows[a] = _less_than(A[cols[lo:hi], a] + 0.0, wv[cols[lo:hi]], probs)
    return rows, hdr


class HostSasAgeBandsZonal:
    """What a context configured with zones holds: HostSasAgeBands once per zone with mask = (zones == z) & mask."""

    def __init__(self, items, probs, windows, n, zones, n_zones, mask=None, weights=None):
        self.items, self.probs, self.n, self.n_zones = list(items), [float(p) for p in probs], int(n), int(n_zones)
        self.zones = np.asarray(zones).reshape(-1).astype(np.int64)
        self.w = np.ones(self.n, dtype=np.int64) if weights is None else np.asarray(weights).reshape(-1).astype(np.int64)
        self.part = (np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0) & (self.w > 0)
        self.hosts = [HostSasAgeBands(items, probs, windows, n, (self.zones == z) & self.part, weights) for z in range(self.n_zones)]
        self.win = self.hosts[0].win

    def add(self, held, variant=None):
        """The next day of the count.  held: {name: (n, W)} values after the day (read on a closing day only)."""
        for z, h in enumerate(self.hosts):
            if variant is None:
                h.add(held)
                continue
            now = h.win.next()
            if now is None or not now[2]:
                continue
            K, P = h.win.first.size, len(self.probs)
            for v in self.items:
                A = np.asarray(held[v], dtype=np.float64)
                if v not in h.rows:
                    h.rows[v], h.hdr[v] = np.full((K, A.shape[1], P), np.nan), np.zeros((K, A.shape[1], 3), dtype=np.int64)
                h.rows[v][now[0]], h.hdr[v][now[0]] = select_zone_variant(A, self.zones, self.n_zones, self.part, self.w, self.probs, z, variant)

    def result(self, widths):
        """(rows {name: (K, Z, W, P)}, hdr {name: (K, Z, W, 3)}), with the blocks of what no window closed yet."""
        per_zone = [h.result(widths) for h in self.hosts]
        return ({v: np.stack([r[v] for r, _ in per_zone], axis=1) for v in self.items},
                {v: np.stack([hd[v] for _, hd in per_zone], axis=1) for v in self.items})

    @property
    def closed(self):
        return self.win.closed


# ---- the inputs of the pure tests: zone maps by name, and the values of sas_age_bands_reference.make_age_pure over the whole domain ----
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2049)   # participating columns of the zones: both selections and the boundary between them
NAN_ZONE = {"sizes": 3, "sizes_interleaved": 3, "one": None, "three": 1, "many": 5, "short_only": 1, "long_only": 1}
MAPS = tuple(NAN_ZONE)


def zone_map(kind, weighted):
    """(n, mask, weights, zones int32 (n,), n_zones).  Every map holds participating columns with zones == -1 (one in 500 of them); with
    weights a zone also holds columns with mask == 0 and with weight 0, which carry the zone index of their neighbour.
      sizes / sizes_interleaved   zones of SIZES participating columns, contiguous / shuffled over the domain
      one, three, many            1, 3 and 1024 zones over about 2100 columns (three: 150, 256 and the rest; many: drawn at random, so
                                  some zones are empty and most hold one to four columns)
      short_only, long_only       zones of 1, 100, 256, 30 and of 257, 300, 1000 participating columns: one of the two launches is skipped"""
    sizes = {"sizes": SIZES, "sizes_interleaved": SIZES, "one": (2100,), "three": (150, 256, 1694), "many": None, "short_only": (1, 100, 256, 30),
             "long_only": (257, 300, 1000)}[kind]
    n_zones = 1024 if sizes is None else len(sizes)
    inside = 2100 if sizes is None else sum(sizes)
    outside = max(2, inside // 500)
    n, mask, w = age_participation(inside + outside, weighted)
    part = (np.ones(n, dtype=bool) if mask is None else mask != 0) & (True if w is None else w > 0)
    cols = np.flatnonzero(part)
    rng = np.random.default_rng(17 + inside + n_zones)
    out = np.zeros(cols.size, dtype=bool)
    out[np.round(np.linspace(3, cols.size - 2, outside)).astype(np.int64)] = True
    label = rng.integers(0, n_zones, size=inside) if sizes is None else np.repeat(np.arange(n_zones), sizes)
    if kind == "sizes_interleaved":
        label = rng.permutation(label)
    of_part = np.full(cols.size, -1, dtype=np.int64)
    of_part[~out] = label
    zones = np.full(n, -1, dtype=np.int32)
    zones[cols] = of_part
    idle = np.flatnonzero(~part)                       # mask == 0 or weight 0: inside the zone of the participant in front of them
    zones[idle] = zones[cols][np.clip(np.searchsorted(cols, idle) - 1, 0, cols.size - 1)]
    return n, mask, w, zones, n_zones


def make_zonal_pure(kind, ages, items, weighted):
    """((n, mask, weights, zones, n_zones), values[d] {name: (n, W)} for the days 0 ... ZONAL_DAYS - 1): make_age_pure's values -- NaN
    scattered, the NaN age class, ties, both zeros, +-inf, a subnormal -- and zone NAN_ZONE[kind] all NaN in age class ZONE_NAN_AGE."""
    cfg = zone_map(kind, weighted)
    n, mask, w, zones, _ = cfg
    part = (np.ones(n, dtype=bool) if mask is None else mask != 0) & (True if w is None else w > 0)
    values = make_age_pure(n, ages, items, part)[:ZONAL_DAYS]
    if NAN_ZONE[kind] is not None:
        for day in values:
            for A in day.values():
                A[zones == NAN_ZONE[kind], ZONE_NAN_AGE] = np.nan
    return cfg, values


@functools.lru_cache(maxsize=None)
def restate_zonal_pure(kind, ages, weighted):
    """The restated run of a map with all of ITEMS4 and PROBS8, once: the cases of fewer items and of the one probability 0.5 are slices of
    it (an item's values do not depend on the items beside it, and a probability's row not on the others).  Treat the result as read-only."""
    cfg, values = make_zonal_pure(kind, ages, ITEMS4, weighted)
    n, mask, w, zones, n_zones = cfg
    h = HostSasAgeBandsZonal(ITEMS4, PROBS8, ZONAL_WINDOWS, n, zones, n_zones, mask, w)
    for d in range(days_of(kind)):
        h.add(values[d])
    return h, cfg, values


@functools.lru_cache(maxsize=None)
def restate_sampled(kind, ages, weighted, sample=MANY_SAMPLE):
    """{z: (rows, hdr)} of the zones `sample` over all ZONAL_DAYS, ITEMS4 and PROBS8: HostSasAgeBands with mask = (zones == z) & mask each.
    Read-only, as restate_zonal_pure's."""
    (n, mask, w, zones, n_zones), values = make_zonal_pure(kind, ages, ITEMS4, weighted)
    widths = {v: width_of(v, ages) for v in ITEMS4}
    out = {}
    for z in sample:
        h = HostSasAgeBands(ITEMS4, PROBS8, ZONAL_WINDOWS, n, (zones == z) & (True if mask is None else mask != 0), w)
        for d in range(ZONAL_DAYS):
            h.add(values[d])
        out[z] = h.result(widths)
    return out


def sliced(h, ages, n_items, n_probs):
    """(rows, hdr) of restate_zonal_pure's host for the first n_items items and pure_probs(n_probs)."""
    widths = {v: width_of(v, ages) for v in ITEMS4}
    rows, hdr = h.result(widths)
    at = [PROBS8.index(p) for p in pure_probs(n_probs)]
    return {v: rows[v][..., at] for v in ITEMS4[:n_items]}, {v: hdr[v] for v in ITEMS4[:n_items]}
