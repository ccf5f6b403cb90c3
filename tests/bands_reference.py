"""The ensemble bands' device rule (rh_bands_*, roger_amd/csrc/rh_bands.h) restated on the host in plain numpy over a list of
(t0, t1, planes), and the CPU double with it.  Imports nothing from roger_amd.

The clock is the duration curves' (tests/durations_reference.py: clock).  A column with mask 0 takes no part.  Per item j with value v:
    SUM (0):  acc = v if first else acc + v, on every step
    LAST (1): nothing on a step that is not counted
    on a counted step  s = (acc if SUM else v) + 0.0        (-0.0 becomes +0.0)
        n_nan = #{masked-in columns with s != s};  x = np.sort(the others);  m = x.size
        per probability p:  r = clamp(int(ceil(p * float(m))) - 1, 0, m - 1);  value = x[r]  (NaN if m == 0)
    one row per counted interval: header {k, t1, then per item m, n_nan}, values (item, probability).
`key_of` / `value_of` are the order-preserving key map of the device's radix selection, restated for the CPU checks."""
import math

import numpy as np

from durations_reference import clock

SUM, LAST = 0, 1
KEY_MASKED = np.uint64(0xFFFFFFFFFFFFFFFF)
KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFE)


def rank_of(p, m):
    """The rank of probability p among m values (m >= 1)."""
    return min(max(int(math.ceil(float(p) * float(m))) - 1, 0), int(m) - 1)


def quantiles_of(s, probs):
    """(values (P,), m, n_nan) of the interval values s (n,) of the masked-in columns."""
    s = np.asarray(s, dtype=np.float64).reshape(-1) + 0.0
    nan = s != s
    x = np.sort(s[~nan])
    m = int(x.size)
    out = np.full(len(probs), np.nan)
    if m:
        out[:] = [x[rank_of(p, m)] for p in probs]
    return out, m, int(nan.sum())


def key_of(s):
    """The uint64 key of float64 values (not NaN): u = bits(s + 0.0); u ^ (all ones if the sign bit is set else the sign bit)."""
    u = (np.asarray(s, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u ^ np.uint64(1 << 63))


def value_of(key):
    key = np.asarray(key, dtype=np.uint64)
    return np.where(key >> np.uint64(63) != 0, key ^ np.uint64(1 << 63), ~key).view(np.float64)


class HostBands:
    """hdr: list of rows [k, t1, m_0, nan_0, ...]; values: list of (J, P) arrays; acc (J, n), advanced by `add` after every step."""

    def __init__(self, kinds, probs, n, mask=None, interval=86400, t_first=0):
        self.kinds = [int(k) for k in kinds]
        self.probs = [float(p) for p in probs]
        assert 1 <= len(self.kinds) <= 8 and 1 <= len(self.probs) <= 8 and all(0.0 <= p <= 1.0 for p in self.probs)
        self.n, self.iv, self.t_first = int(n), int(interval), int(t_first)
        self.on = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        assert self.on.size == self.n
        self.acc = np.zeros((len(self.kinds), self.n))
        self.hdr, self.values = [], []

    def add(self, t0, t1, planes):
        """planes: one (n,) array per item, the values after the step over (t0, t1]."""
        first, _, k, counted = clock(int(t0), int(t1), self.iv, self.t_first)
        on = self.on
        row, hdr = np.full((len(self.kinds), len(self.probs)), np.nan), [int(k), int(t1)]
        for j, kind in enumerate(self.kinds):
            if kind == LAST and not counted:
                continue
            v = np.asarray(planes[j], dtype=np.float64).reshape(-1)[on]
            s = v.copy()
            if kind == SUM:
                if not first:
                    with np.errstate(invalid="ignore"):
                        s = self.acc[j, on] + v
                self.acc[j, on] = s
            if counted:
                row[j], m, n_nan = quantiles_of(s, self.probs)
                hdr += [m, n_nan]
        if counted:
            self.hdr.append(hdr)
            self.values.append(row)

    def rows(self):
        nv, npr = len(self.kinds), len(self.probs)
        return (np.array(self.hdr, dtype=np.int64).reshape(-1, 2 + 2 * nv), np.array(self.values, dtype=np.float64).reshape(-1, nv, npr))


def oracle_double():
    """tests/oracle_context.py's double with the three bands_* methods of `_native.Context`: the refusals of rh_bands_configure as
    ValueError, a read before it as RuntimeError.  (A function: importing this module must not need the oracle's library.)"""
    from oracle_context import OracleContext

    class BandsOracleContext(OracleContext):
        _bands = None

        def bands_configure(self, names, kinds=(), probs=(0.05, 0.5, 0.95), interval=86400, t_first=0, mask=None, capacity=4096):
            names = list(names)
            if not names:
                self._bands = None
                return
            if len(names) > 8 or not 1 <= len(probs) <= 8 or any(not 0.0 <= float(p) <= 1.0 for p in probs):
                raise ValueError("bands_configure: counts or probabilities")
            if any(self.st.planes[v].dtype != np.float64 for v in names):
                raise ValueError("bands_configure: float64 planes only")
            if int(interval) not in (86400, 3600, 600) or int(t_first) % int(interval) or int(capacity) < 1:
                raise ValueError("bands_configure: interval or capacity")
            self._bands = HostBands(kinds, probs, self.n, mask, interval, t_first)
            self._bnames = names

        def bands_count(self):
            if self._bands is None:
                raise RuntimeError("bands_configure has not been called")
            return len(self._bands.hdr)

        def bands_read(self, first, n):
            if self._bands is None:
                raise RuntimeError("bands_configure has not been called")
            hdr, values = self._bands.rows()
            return hdr[first:first + n].copy(), values[first:first + n].copy()

        def _accumulate(self):
            super()._accumulate()
            if self._bands is None:
                return
            s = self.st.scal
            self._bands.add(int(s.time) - int(s.dt_secs), int(s.time), [self.st.planes[v] for v in self._bnames])

    return BandsOracleContext
