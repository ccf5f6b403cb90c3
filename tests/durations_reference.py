"""The duration curves' device rule (rh_durations_*, k_durations in roger_amd/csrc/rh_durations.h) restated on the host in plain numpy
over a list of (t0, t1, planes), and the CPU double with it.  Imports nothing from roger_amd.

After a step over (t0, t1], iv the interval in seconds:
    first   = t0 % iv == 0
    closes  = t1 % iv == 0 and t1 - t0 <= iv          (a step longer than the interval never closes one)
    k       = t1 // iv - 1 - t_first // iv
    counted = closes and k >= 0                       (no upper bound)
A column with mask 0 is never touched.  Per item j with value v:
    SUM (0):  acc = v if first else acc + v, on every step; s = acc
    LAST (1): nothing on a step that is not counted; s = v on a counted one; its acc plane stays +0.0
    on a counted step, with the item's m edges e (ascending):
        bin = m + 1 if s != s else #{q : e[q] <= s};  count[j][bin] += 1 (uint32)
        mn = s if s < mn else mn;  mx = s if s > mx else mx          (from +inf / -inf; a NaN compares false)
        with a spell (side, thr):  in = s < thr if side == BELOW else s >= thr;  run = run + 1 if in else 0;
                                   n_spells += 1 if in and run == 1;  longest = max(longest, run)
Spells run over consecutive counted intervals: an hourly interval under a daily step is neither counted nor does it break a run.
`DurationsOracleContext` is tests/oracle_context.py's double with the two durations_* methods of `_native.Context`."""
import numpy as np

SUM, LAST = 0, 1
BELOW, AT_OR_ABOVE = 0, 1
RUN, LONGEST, NSPELLS = 0, 1, 2


def clock(t0, t1, iv, t_first):
    """(first, closes, k, counted) of a step over (t0, t1]."""
    first = t0 % iv == 0
    closes = t1 % iv == 0 and t1 - t0 <= iv
    k = t1 // iv - 1 - t_first // iv
    return first, closes, k, closes and k >= 0


class HostDurations:
    """counts: one (m_j + 2, n) uint32 per item; vals (J, 3, n) float64 {acc, mn, mx}; spells (J, 3, n) uint32 {run, longest,
    n_spells}, advanced by `add` after every step.  spells_cfg[j]: None or (side, threshold)."""

    def __init__(self, kinds, edges, n, spells=None, mask=None, interval=86400, t_first=0):
        self.kinds = [int(k) for k in kinds]
        self.edges = [np.array(e, dtype=np.float64).reshape(-1) for e in edges]
        assert len(self.edges) == len(self.kinds)
        for e in self.edges:
            assert e.size <= 63 and np.isfinite(e).all() and (np.diff(e) > 0).all()
        self.cfg = list(spells) if spells is not None else [None] * len(self.kinds)
        self.n, self.iv, self.t_first = int(n), int(interval), int(t_first)
        self.on = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        assert self.on.size == self.n
        self.counts = [np.zeros((e.size + 2, self.n), dtype=np.uint32) for e in self.edges]
        self.vals = np.zeros((len(self.kinds), 3, self.n))
        self.vals[:, 1], self.vals[:, 2] = np.inf, -np.inf
        self.spells = np.zeros((len(self.kinds), 3, self.n), dtype=np.uint32)

    def add(self, t0, t1, planes):
        """planes: one (n,) array per item, the values after the step over (t0, t1]."""
        first, _, _, counted = clock(int(t0), int(t1), self.iv, self.t_first)
        on, cols = self.on, np.flatnonzero(self.on)
        for j, kind in enumerate(self.kinds):
            if kind == LAST and not counted:
                continue
            v = np.asarray(planes[j], dtype=np.float64).reshape(-1)[on]
            s = v.copy()
            if kind == SUM:
                if not first:
                    s = self.vals[j, 0, on] + v
                self.vals[j, 0, on] = s
            if not counted:
                continue
            e = self.edges[j]
            with np.errstate(invalid="ignore"):
                b = np.where(s != s, e.size + 1, (e[None, :] <= s[:, None]).sum(axis=1))
                self.counts[j][b, cols] += np.uint32(1)
                mn, mx = self.vals[j, 1, on], self.vals[j, 2, on]
                self.vals[j, 1, on] = np.where(s < mn, s, mn)
                self.vals[j, 2, on] = np.where(s > mx, s, mx)
                if self.cfg[j] is not None:
                    side, thr = self.cfg[j]
                    inside = s < thr if int(side) == BELOW else s >= thr
                    run = np.where(inside, self.spells[j, RUN, on] + np.uint32(1), np.uint32(0)).astype(np.uint32)
                    self.spells[j, RUN, on] = run
                    self.spells[j, NSPELLS, on] += (inside & (run == 1)).astype(np.uint32)
                    self.spells[j, LONGEST, on] = np.maximum(self.spells[j, LONGEST, on], run)


def interval_series(steps, kind, iv, t_first):
    """The interval values of one item over `steps` = [(t0, t1, values (n,))]: (counted intervals, n), in the order they were counted --
    the same additions as the rule, kept per interval for the checks of the derivation."""
    out, acc = [], None
    for t0, t1, v in steps:
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        first, _, _, counted = clock(int(t0), int(t1), iv, t_first)
        if acc is None:
            acc = np.zeros(v.size)
        if kind == SUM:
            acc = v.copy() if first else acc + v
        if counted:
            out.append(acc.copy() if kind == SUM else v.copy())
    return np.array(out)


def oracle_double():
    """tests/oracle_context.py's double with durations: the refusals of rh_durations_configure as ValueError, rh_durations_read before
    it as RuntimeError.  (A function: importing this module must not need the oracle's library.)"""
    from oracle_context import OracleContext

    class DurationsOracleContext(OracleContext):
        _durations = None

        def durations_configure(self, names, kinds=(), edges=(), spells=(), mask=None, interval=86400, t_first=0):
            names = list(names)
            if not names:
                self._durations = None
                return
            if len(names) > 16:
                raise ValueError("durations_configure: n_items")
            if any(self.st.planes[v].dtype != np.float64 for v in names):
                raise ValueError("durations_configure: float64 planes only")
            edges = [np.asarray(e, dtype=np.float64).reshape(-1) for e in edges]
            if any(e.size > 63 or not np.isfinite(e).all() or not (np.diff(e) > 0).all() for e in edges):
                raise ValueError("durations_configure: edges")
            if int(interval) not in (86400, 3600, 600) or int(t_first) % int(interval):
                raise ValueError("durations_configure: interval")
            self._durations = HostDurations(kinds, edges, self.n, list(spells) or None, mask, interval, t_first)
            self._dnames = names

        def durations_read(self):
            if self._durations is None:
                raise RuntimeError("durations_configure has not been called")
            d = self._durations
            return [c.copy() for c in d.counts], d.vals.copy(), d.spells.copy()

        def _accumulate(self):
            super()._accumulate()
            if self._durations is None:
                return
            s = self.st.scal
            self._durations.add(int(s.time) - int(s.dt_secs), int(s.time), [self.st.planes[v] for v in self._dnames])

    return DurationsOracleContext
