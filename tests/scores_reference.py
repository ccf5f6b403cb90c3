"""The scores' device rule (rh_scores_*, k_scores in roger_amd/csrc/rh_scores.h) restated on the host in plain numpy over a list of
(t0, t1, planes), and the CPU double with it.  Imports nothing from roger_amd.

After a step over (t0, t1], iv the interval in seconds:
    first  = t0 % iv == 0
    closes = t1 % iv == 0 and t1 - t0 <= iv          (a step longer than the interval never closes one)
    k      = t1 // iv - 1 - t_first // iv,  scored only when 0 <= k < n_intervals
Column i has s = series[i] (no map: 0); s < 0 is never touched.  Per item j with value v:
    SUM (0):  acc = v if first else acc + v, on every step
    LAST (1): acc = v on a closing step; its acc plane stays +0.0 in memory
    on a scored closing step with o = obs[j, s, k] not NaN, one IEEE operation each, in this order:
        m1 += acc;  m2 += acc * acc;  m3 += acc * o;  d = acc - o;  m4 += d * d
numpy evaluates `a * b` and `x + y` as separate IEEE operations on float64 arrays, which is the rule.
`ScoresOracleContext` is tests/oracle_context.py's double with the two scores_* methods of `_native.Context`."""
import numpy as np

from oracle_context import OracleContext

SUM, LAST = 0, 1


def clock(t0, t1, iv, t_first, n_intervals):
    """(first, closes, k, scored) of a step over (t0, t1]."""
    first = t0 % iv == 0
    closes = t1 % iv == 0 and t1 - t0 <= iv
    k = t1 // iv - 1 - t_first // iv
    return first, closes, k, closes and 0 <= k < n_intervals


class HostScores:
    """moments (J, 5, n) float64 {acc, m1, m2, m3, m4} and closed (K,) uint8, advanced by `add` after every step."""

    def __init__(self, kinds, obs, n, series=None, interval=86400, t_first=0):
        self.kinds = [int(k) for k in kinds]
        self.obs = np.array(obs, dtype=np.float64)
        assert self.obs.ndim == 3 and self.obs.shape[0] == len(self.kinds)
        self.n, self.iv, self.t_first = int(n), int(interval), int(t_first)
        self.series = np.zeros(self.n, dtype=np.int64) if series is None else np.asarray(series).reshape(-1).astype(np.int64)
        assert self.series.size == self.n and self.series.max() < self.obs.shape[1]
        self.moments = np.zeros((len(self.kinds), 5, self.n))
        self.closed = np.zeros(self.obs.shape[2], dtype=np.uint8)

    def add(self, t0, t1, planes):
        """planes: one (n,) array per item, the values after the step over (t0, t1]."""
        first, closes, k, scored = clock(int(t0), int(t1), self.iv, self.t_first, self.obs.shape[2])
        if scored:
            self.closed[k] = 1
        on = self.series >= 0
        s = self.series[on]
        for j, kind in enumerate(self.kinds):
            if kind == LAST and not scored:
                continue
            m = self.moments[j]
            v = np.asarray(planes[j], dtype=np.float64).reshape(-1)[on]
            acc = v.copy()
            if kind == SUM:
                if not first:
                    acc = m[0, on] + v
                m[0, on] = acc
            if not scored:
                continue
            o = self.obs[j, s, k]
            have = o == o
            cols = np.flatnonzero(on)[have]
            a, o = acc[have], o[have]
            m[1, cols] = m[1, cols] + a
            sq = a * a
            m[2, cols] = m[2, cols] + sq
            so = a * o
            m[3, cols] = m[3, cols] + so
            d = a - o
            dd = d * d
            m[4, cols] = m[4, cols] + dd


def interval_series(steps, kind, iv, t_first, n_intervals):
    """The aggregated series of one item over `steps` = [(t0, t1, values (n,))]: (K, n) interval values (NaN where interval k was not
    closed while scored) -- the same additions as the rule, kept per interval for the two-pass checks."""
    out, acc = None, None
    for t0, t1, v in steps:
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if out is None:
            out, acc = np.full((n_intervals, v.size), np.nan), np.zeros(v.size)
        first, closes, k, scored = clock(int(t0), int(t1), iv, t_first, n_intervals)
        if kind == SUM:
            acc = v.copy() if first else acc + v
        elif closes:
            acc = v.copy()
        if scored:
            out[k] = acc
    return out


class ScoresOracleContext(OracleContext):
    """The double with scores: the refusals of rh_scores_configure as ValueError, rh_scores_read before it as RuntimeError."""

    _scores = None

    def scores_configure(self, names, kinds=(), obs=None, series=None, interval=86400, t_first=0):
        names = list(names)
        if not names:
            self._scores = None
            return
        if len(names) > 16:
            raise ValueError("scores_configure: n_items")
        if any(self.st.planes[v].dtype != np.float64 for v in names):
            raise ValueError("scores_configure: float64 planes only")
        o = np.asarray(obs, dtype=np.float64)
        if o.ndim != 3 or o.shape[0] != len(names) or not 1 <= o.shape[1] <= 1024 or o.shape[2] < 1 or len(kinds) != len(names):
            raise ValueError("scores_configure: observations")
        if int(interval) not in (86400, 3600, 600):
            raise ValueError("scores_configure: interval")
        if int(t_first) % int(interval) or int(t_first) < int(self.st.scal.time):
            raise ValueError("scores_configure: t_first")
        if series is not None and (np.asarray(series).size != self.n or np.asarray(series).max() >= o.shape[1]):
            raise ValueError("scores_configure: series")
        self._scores = HostScores(kinds, o, self.n, series, interval, t_first)
        self._snames = names

    def scores_read(self):
        if self._scores is None:
            raise RuntimeError("scores_configure has not been called")
        return self._scores.moments.copy(), self._scores.closed.copy()

    def _accumulate(self):
        super()._accumulate()
        if self._scores is None:
            return
        s = self.st.scal
        self._scores.add(int(s.time) - int(s.dt_secs), int(s.time), [self.st.planes[v] for v in self._snames])
