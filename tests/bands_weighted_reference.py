"""The likelihood-weighted ensemble bands' device rule (rh_bands_configure_weighted, roger_amd/csrc/rh_bands.h) restated on the host in
plain numpy, on tests/bands_reference.py's clock and aggregation, and the CPU double with it.  Imports nothing from roger_amd.

Everything is bands_reference's rule except: a column takes part iff its integer weight w_i (uint16, 0 ... 65535) is > 0; m and n_nan
count participating columns; W = sum of w_i over the m columns with a number; per probability p
    T = clamp(int(ceil(p * float(W))), 1, W);   value = the smallest s with sum_{s_i <= s} w_i >= T   (NaN if m == 0)
in two formulations that must agree by bits: cumsum / searchsorted over the stably sorted values, and np.sort(np.repeat(s, w))[T - 1].
One row per counted interval: header {k, t1, then per item m, n_nan}, values (item, probability), weight sums (item,)."""
import math

import numpy as np

from bands_reference import LAST, SUM, HostBands
from durations_reference import clock

MAX_WEIGHT = 65535


def target_of(p, W):
    """T of probability p under the weight sum W (W >= 1): one double multiplication, one ceil."""
    return min(max(int(math.ceil(float(p) * float(W))), 1), int(W))


def _participants(s, w):
    s = np.asarray(s, dtype=np.float64).reshape(-1) + 0.0
    w = np.asarray(w).reshape(-1)
    assert s.size == w.size and w.dtype.kind in "iu" and (w.size == 0 or (0 <= int(w.min()) and int(w.max()) <= MAX_WEIGHT))
    on = w != 0
    s, w = s[on], w[on].astype(np.int64)
    nan = s != s
    return s[~nan], w[~nan], int(nan.sum())


def weighted_quantiles_of(s, w, probs):
    """(values (P,), m, n_nan, W) of the interval values s (n,) under the integer weights w (n,): cumsum / searchsorted."""
    x, wx, n_nan = _participants(s, w)
    m, W = int(x.size), int(wx.sum())
    out = np.full(len(probs), np.nan)
    if m:
        o = np.argsort(x, kind="stable")
        cw = np.cumsum(wx[o])
        out[:] = [x[o][np.searchsorted(cw, target_of(p, W), side="left")] for p in probs]
    return out, m, n_nan, W


def weighted_quantiles_by_repeat(s, w, probs):
    """The same through np.repeat: column i counts as w_i identical members.  (Memory: W values -- for small weights only.)"""
    x, wx, n_nan = _participants(s, w)
    m, W = int(x.size), int(wx.sum())
    out = np.full(len(probs), np.nan)
    if m:
        members = np.sort(np.repeat(x, wx))
        out[:] = [members[target_of(p, W) - 1] for p in probs]
    return out, m, n_nan, W


class HostWeightedBands(HostBands):
    """HostBands under mask = (w != 0) -- its clock, its SUM / LAST aggregation and its accumulators -- with the weighted pick in place of
    quantiles_of.  wsum: list of rows [W_0, W_1, ...]."""

    def __init__(self, kinds, probs, n, weights, interval=86400, t_first=0):
        w = np.asarray(weights).reshape(-1)
        assert w.size == int(n) and w.dtype.kind in "iu" and 0 <= int(w.min()) and int(w.max()) <= MAX_WEIGHT
        super().__init__(kinds, probs, n, w != 0, interval, t_first)
        self.w = w.astype(np.int64)
        self.wsum = []

    def add(self, t0, t1, planes):
        first, _, k, counted = clock(int(t0), int(t1), self.iv, self.t_first)
        on = self.on
        row, hdr, wsum = np.full((len(self.kinds), len(self.probs)), np.nan), [int(k), int(t1)], []
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
                row[j], m, n_nan, W = weighted_quantiles_of(s, self.w[on], self.probs)
                hdr += [m, n_nan]
                wsum.append(W)
        if counted:
            self.hdr.append(hdr)
            self.values.append(row)
            self.wsum.append(wsum)

    def rows(self):
        """(hdr (rows, 2 + 2 J), values (rows, J, P), wsum (rows, J))."""
        return super().rows() + (np.array(self.wsum, dtype=np.int64).reshape(-1, len(self.kinds)),)


def oracle_double():
    """bands_reference's oracle double with `bands_configure(..., weights=)` and `bands_weight_sums` of `_native.Context`: a uint16 per
    column of this block, a mask folded in.  (A function: importing this module must not need the oracle's library.)"""
    import bands_reference

    class WeightedBandsOracleContext(bands_reference.oracle_double()):
        _weighted = False

        def bands_configure(self, names, kinds=(), probs=(0.05, 0.5, 0.95), interval=86400, t_first=0, mask=None, capacity=4096, weights=None):
            if weights is None or not list(names):
                super().bands_configure(names, kinds, probs, interval, t_first, mask, capacity)
                self._weighted = False
                return
            w = np.asarray(weights).reshape(-1)
            if w.size != self.n or w.dtype.kind not in "iu" or int(w.min()) < 0 or int(w.max()) > MAX_WEIGHT:
                raise ValueError("bands_configure: the weights are integers 0 ... 65535, one per column")
            if mask is not None:
                w = np.where(np.asarray(mask).reshape(-1) != 0, w, 0)
            if not w.any():
                raise ValueError("bands_configure: no participating column (every weight is 0)")
            super().bands_configure(names, kinds, probs, interval, t_first, None, capacity)      # (its refusals)
            self._bands = HostWeightedBands(kinds, probs, self.n, w.astype(np.uint16), interval, t_first)
            self._weighted = True

        def bands_read(self, first, n):
            if self._bands is None:
                raise RuntimeError("bands_configure has not been called")
            hdr, values = self._bands.rows()[:2]
            return hdr[first:first + n].copy(), values[first:first + n].copy()

        def bands_weight_sums(self, first, n):
            if self._bands is None or not self._weighted:
                raise RuntimeError("bands_configure has not been called with weights")
            return self._bands.rows()[2][first:first + n].copy()

    return WeightedBandsOracleContext
