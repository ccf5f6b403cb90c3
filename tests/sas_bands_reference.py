"""The transport bands of the SAS context (rh_sas_bands_*, roger_amd/csrc/rh_sas_bands.h) restated on the host in plain numpy: the host's
window clock (`Windows` of sas_scores_reference, the clock the scores have), one day of the day kernel (`band_day`), the selection as
argsort / cumsum / searchsorted (`select`), where the observation falls (`obs_pair`) and the three together (`HostSasBands`).  Importing this module imports nothing from roger_amd.

The rule.  Window k is the days [first_day[k], last_day[k]] of the context's count of recorded days.  A column takes part iff mask != 0
and its integer weight w_i (0 ... 65535; without a weight plane 1) is > 0; one that does not is never touched.  Per item (value, weight,
kind), v the value after the day:
    BULK (0): wd = the day's weight;  MEAN (1): wd = 1.0.  On the window's first day num and den restart from +0.0; the day is eligible iff
              wd > 0 and v == v: num = num + fl(v * wd), den = den + wd; a day that is not eligible leaves both as they are
    LAST (2): nothing before the closing day
    closing day:  BULK / MEAN  s = num / den if den > 0 else NaN;  LAST  s = v;  then s = s + 0.0 (-0.0 becomes +0.0)
m = participants with a number, n_nan = participants with a NaN, W = sum of w_i over the m.  For a probability p
    T = clip(int(ceil(p * float(W))), 1, W);   o = argsort(s, stable);  cw = cumsum(w[o]);  value = s[o][searchsorted(cw, T, "left")]
which is np.sort(np.repeat(s, w))[T - 1] bit for bit; with m == 0 NaN and W = 0.  With observations, per item and window the int64 pair
(below, equal) = (sum w_i [s_i < o + 0.0], sum w_i [s_i == o + 0.0]); a missing o gives (-1, -1), m == 0 gives (0, 0).
rows (K, J, P) float64 are NaN, hdr (K, J, 3) = {m, n_nan, W} is 0 and pairs (K, J, 2) are -1 until the window closes.
The `variant` arguments exist for the tests that show the inputs have teeth."""
import numpy as np

from sas_scores_reference import BULK, LAST, MEAN, PURE_DAYS, PURE_WINDOWS, Windows, _fused, same_bits  # noqa: F401

MAX_WEIGHT = 65535
VARIANTS = ("no_add_zero", "floor", "fma", "nan_member", "zero_weight", "drop9")


def band_day(acc, kinds, values, weights, part, first, closes, variant=None):
    """One launch of k_sas_bands_day: acc (J, 2, n) = {num, den} advanced in place for the participating columns `part` (bool (n,)).  On a
    closing day the window values s (J, n) float64 -- after + 0.0, NaN where there is none -- else None."""
    n = acc.shape[2]
    s = np.full((len(kinds), n), np.nan)
    with np.errstate(all="ignore"):
        for j, kind in enumerate(kinds):
            if kind == LAST and not closes:
                continue
            v = np.asarray(values[j], dtype=np.float64).reshape(-1)
            sj = v
            if kind != LAST:
                wd = np.asarray(weights[j], dtype=np.float64).reshape(-1) if kind == BULK else np.ones(n)
                num, den = (np.zeros(n), np.zeros(n)) if first else (acc[j, 0].copy(), acc[j, 1].copy())
                e = (wd > 0.0) & (v == v)                       # (NaN > 0 is False)
                t = v * wd                                       # rounded before it is added
                added = _fused(num, v, wd) if variant == "fma" else num + t
                num, den = np.where(e, added, num), np.where(e, den + wd, den)
                acc[j, 0], acc[j, 1] = np.where(part, num, acc[j, 0]), np.where(part, den, acc[j, 1])
                if not closes:
                    continue
                sj = np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), np.nan)
            s[j] = sj if variant == "no_add_zero" else sj + 0.0
    return s if closes else None


def keys_of(x):
    """The order-preserving uint64 key of every value (none a NaN): unsigned comparison of keys is < on the values."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def values_of(keys):
    k = np.asarray(keys, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def select(s, w, probs, variant=None):
    """The selection over the participating columns: s (n,) window values, w (n,) integer weights > 0.  (values (P,), m, n_nan, W)."""
    s, w = np.asarray(s, dtype=np.float64), np.asarray(w).astype(np.int64)
    number = np.ones(s.size, dtype=bool) if variant == "nan_member" else s == s
    x, wx = s[number], w[number]
    m, n_nan, W = int(x.size), int(s.size - x.size), int(wx.sum())
    values = np.full(len(probs), np.nan)
    if m:
        # (argsort orders the bit patterns only under the + 0.0 rule; without it the keys decide between -0.0 and +0.0, as on the device)
        o = np.argsort(keys_of(x), kind="stable") if variant == "no_add_zero" else np.argsort(x, kind="stable")
        cw = np.cumsum(wx[o])
        for q, p in enumerate(probs):
            t = np.floor(float(p) * float(W)) if variant == "floor" else np.ceil(float(p) * float(W))
            T = min(max(int(t), 1), W)
            values[q] = x[o][np.searchsorted(cw, T, side="left")]
        if variant == "drop9":   # (five passes of 11 bits: the lowest 9 bits of the key are never looked at)
            ok = values == values
            values[ok] = values_of(keys_of(values[ok]) & ~np.uint64(0x1ff))
    return values, m, n_nan, W


def obs_pair(s, w, o):
    """(below, equal) of the observation o among the participants' window values s with integer weights w."""
    if o != o:
        return -1, -1
    s, w = np.asarray(s, dtype=np.float64), np.asarray(w).astype(np.int64)
    o = o + 0.0
    number = s == s
    return int(w[number & (s < o)].sum()), int(w[number & (s == o)].sum())


class HostSasBands:
    """What a configured context holds: the windows' clock, num / den and the result.  items: [(value, weight or None, kind int)]."""

    def __init__(self, items, probs, windows, n, mask=None, weights=None, obs=None):
        self.items = [(v, w, int(k)) for v, w, k in items]
        self.probs = [float(p) for p in probs]
        self.win = Windows(*windows)
        K, J = self.win.first.size, len(self.items)
        self.n = int(n)
        self.mask = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        self.weights = None if weights is None else np.asarray(weights).reshape(-1).astype(np.int64)
        self.obs = None if obs is None else np.array(obs, dtype=np.float64).reshape(J, K)
        self.acc = np.zeros((J, 2, self.n))
        self.rows = np.full((K, J, len(self.probs)), np.nan)
        self.hdr = np.zeros((K, J, 3), dtype=np.int64)
        self.pairs = np.full((K, J, 2), -1, dtype=np.int64)

    def add(self, held, weights=None, variant=None):
        """The next day of the count.  held: {name: (n,)} values after the day; weights: {name: (n,)} the day's rows (default: held)."""
        weights = held if weights is None else weights
        now = self.win.next()
        if now is None:
            return
        k, first, closes = now
        kinds = [kd for _, _, kd in self.items]
        if not closes and all(kd == LAST for kd in kinds):
            return
        w = np.ones(self.n, dtype=np.int64) if self.weights is None else self.weights
        part = self.mask if variant == "zero_weight" else self.mask & (w > 0)
        s = band_day(self.acc, kinds, [held[v] for v, _, _ in self.items],
                     [None if wn is None else np.asarray(weights[wn]).reshape(-1) for _, wn, _ in self.items], part, first, closes, variant)
        if not closes:
            return
        for j in range(len(self.items)):
            self.rows[k, j], m, n_nan, W = select(s[j][part], w[part], self.probs, variant)
            self.hdr[k, j] = (m, n_nan, W)
            if self.obs is not None:
                self.pairs[k, j] = obs_pair(s[j][part], w[part], self.obs[j, k])

    @property
    def closed(self):
        return self.win.closed


# ---- the inputs of the pure tests (no day kernel): what tests/test_sas_bands_reference.py shows to have teeth and to meet its conditions ----
ITEMS8 = [("C_iso_q_ss", "q_ss", BULK), ("C_rz", None, MEAN), ("C_rz", None, LAST), ("C_q_ss", "q_ss", BULK), ("C_iso_transp", "transp", BULK),
          ("C_iso_rz", None, MEAN), ("C_iso_ss", None, LAST), ("C_s", None, LAST)]
PROBS8 = (0.0, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 1.0)
A9 = 1.5                                                    # the lowest 9 bits of its key are 0 ...
B9 = float(np.array(np.array(A9).view(np.uint64) + np.uint64(3)).view(np.float64))   # ... and this one differs from it in them only
ON_A_MEMBER = -7.25                                         # C_rz of column 1 on day 0: the observation that falls exactly on a member


def pure_probs(n_probs):
    return PROBS8 if n_probs == 8 else (0.5,) if n_probs == 1 else PROBS8[:n_probs]


def pure_participation(n, weighted):
    """(mask, weights): None, None -- or a byte mask that leaves every fifth column out and uint16 likelihoods with zeros, ones and the
    largest weight; the columns 0 and 1 take part."""
    if not weighted:
        return None, None
    rng = np.random.default_rng(77 + n)
    w = rng.integers(2, MAX_WEIGHT + 1, size=n)
    w[::7] = 0
    w[1::7] = 1
    w[2::11] = MAX_WEIGHT
    w[0] = 3
    mask = (np.arange(n) % 5 != 4).astype(np.uint8)
    return mask, w.astype(np.uint16)


def make_pure(n, items):
    """(values, weights, obs): values[d] {name: (n,)} for the days 0 ... 6, weights {name: (3, n)} the three rows of the daily inputs with
    zeros, a negative and a NaN weight, obs (J, 4).  Values are drawn from a small pool (ties), of both signs, with NaN; and by name:
      C_s       thirds of negative numbers, zeros of both signs (three -0.0 to one +0.0) and positive numbers: the median falls among the zeros
      C_iso_rz  +inf, -inf and a subnormal among the columns
      C_iso_ss  all NaN on day 2: window 1 closes with m == 0
      C_rz      on day 5 the two values A9 and B9, alternating: the median is the last A9, the next member B9; column 1 holds ON_A_MEMBER
                on day 0"""
    rng = np.random.default_rng(1000 * n + len(items))
    names = sorted({v for v, _, _ in items})
    wnames = sorted({w for _, w, _ in items if w is not None})
    c = np.arange(n)
    values = []
    for d in range(PURE_DAYS):
        day = {}
        for v in names:
            pool = -12.0 + 9.0 * rng.random(max(3, n // 3)) + np.where(rng.random(max(3, n // 3)) < 0.15, 20.0, 0.0)
            a = pool[rng.integers(0, pool.size, size=n)]
            a[rng.random(n) < 0.2] = np.nan
            a[0] = -7.0 - d / 3.0 - len(v) / 7.0
            if v == "C_s":
                a = np.where(c % 3 == 0, -1.0 - (c % 5), np.where(c % 3 == 1, np.where((c // 3) % 4 != 3, -0.0, 0.0), 2.5 + (c % 4)))
            elif v == "C_iso_rz" and n > 8:
                a[5], a[6], a[8] = np.inf, -np.inf, 5e-324
            elif v == "C_iso_ss" and d == 2:
                a[:] = np.nan
            elif v == "C_rz" and d == 5:
                a = np.where(c % 2 == 0, A9, B9)
            elif v == "C_rz" and d == 0 and n > 1:
                a[1] = ON_A_MEMBER
            day[v] = a
        values.append(day)
    weights = {}
    for w in wnames:
        a = rng.random((3, n)) * 3.0 + 0.1
        a[rng.random((3, n)) < 0.3] = 0.0
        a[:, 0] = [0.7, 1.3, 2.1]
        if n > 2:
            a[1, 2] = np.nan
            a[2, 1] = -0.5
        weights[w] = a
    obs = -10.0 + 6.0 * rng.random((len(items), len(PURE_WINDOWS[0])))
    obs[0, 0], obs[0, 1] = -1e6, 1e6                       # below all members, above all
    obs[1::2, 2] = np.nan                                  # missing
    if len(items) > 2:
        obs[2, 0] = ON_A_MEMBER
    return values, weights, obs


def restate_pure(n, items, n_probs, weighted, observed=True, variant=None, windows=PURE_WINDOWS, days=PURE_DAYS):
    values, weights, obs = make_pure(n, items)
    mask, w = pure_participation(n, weighted)
    h = HostSasBands(items, pure_probs(n_probs), windows, n, mask, w, obs if observed else None)
    for d in range(days):
        h.add(values[d], {wn: a[d % 3] for wn, a in weights.items()}, variant)
    return h
