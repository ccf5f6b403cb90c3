"""The CPU double for resuming the scores, the duration curves, the event outputs and the bands from a restart file: tests/oracle_context.py's
double with all four observers' restatements (tests/scores_reference.py, durations_reference.py, events_reference.py, bands_reference.py,
bands_zonal_reference.py) and the calls ABI version 18 adds to `_native.Context` -- scores_restore, durations_restore, events_state,
events_restore, bands_state, bands_restore -- with the rules of the C side: a restore is valid after the observer's configure call and
before the next step (RuntimeError for RH_ERR_STATE), checks its sizes (ValueError for RH_ERR_ARG) and changes nothing when it refuses.
Imports nothing from roger_amd."""
import numpy as np


def resume_double():
    """(A function: importing this module must not need the oracle's library.)"""
    import bands_reference
    import durations_reference
    from bands_zonal_reference import HostZonalBands
    from events_reference import EventsOracleContext
    from scores_reference import ScoresOracleContext

    class ResumeOracleContext(ScoresOracleContext, EventsOracleContext, durations_reference.oracle_double(), bands_reference.oracle_double()):
        _fresh = frozenset()
        _bands_row0 = 0
        _bands_zonal = False

        def _configured(self, which, on):
            self._fresh = (self._fresh | {which}) if on else (self._fresh - {which})

        def _restorable(self, which, held):
            if held is None:
                raise RuntimeError(f"{which}_restore: {which}_configure has not been called")
            if which not in self._fresh:
                raise RuntimeError(f"{which}_restore: a step has run since {which}_configure")

        def _accumulate(self):
            self._fresh = frozenset()
            super()._accumulate()

        # -- scores --
        def scores_configure(self, names, *a, **k):
            super().scores_configure(names, *a, **k)
            self._configured("scores", bool(list(names)))

        def scores_restore(self, moments, closed, t_first):
            self._restorable("scores", self._scores)
            h = self._scores
            m, c = np.asarray(moments, dtype=np.float64), np.asarray(closed, dtype=np.uint8)
            if m.shape != h.moments.shape or c.shape != h.closed.shape or int(t_first) < 0 or int(t_first) % h.iv:
                raise ValueError("scores_restore: size mismatch, or t_first")
            h.moments, h.closed, h.t_first = m.copy(), c.copy(), int(t_first)

        # -- durations --
        def durations_configure(self, names, *a, **k):
            super().durations_configure(names, *a, **k)
            self._configured("durations", bool(list(names)))

        def durations_restore(self, counts, values, spells):
            self._restorable("durations", self._durations)
            h = self._durations
            counts = [np.asarray(c, dtype=np.uint32) for c in counts]
            v, sp = np.asarray(values, dtype=np.float64), np.asarray(spells, dtype=np.uint32)
            if [c.shape for c in counts] != [c.shape for c in h.counts] or v.shape != h.vals.shape or sp.shape != h.spells.shape:
                raise ValueError("durations_restore: size mismatch")
            h.counts, h.vals, h.spells = [c.copy() for c in counts], v.copy(), sp.copy()

        # -- events --
        def events_configure(self, names, *a, **k):
            super().events_configure(names, *a, **k)
            self._configured("events", bool(list(names)))

        def events_state(self):
            if self._events is None:
                raise RuntimeError("events_configure has not been called")
            h = self._events
            return h.hdr[:, 0].copy(), int(h.running), int(h.drained)   # (the restatement keeps a slot's id in its header)

        def events_restore(self, hdr, ids, running, drained, lost=False, values=None):
            self._restorable("events", self._events)
            h = self._events
            hdr, ids, values = np.asarray(hdr, dtype=np.int64), np.asarray(ids, dtype=np.int64), dict(values or {})
            if hdr.shape != h.hdr.shape or ids.shape != (h.ns,) or any(not 0 <= int(s) < h.ns or np.asarray(v).shape != h.values.shape[1:]
                                                                       for s, v in values.items()):
                raise ValueError("events_restore: size mismatch")
            h.hdr = hdr.copy()
            h.hdr[:, 0] = ids
            for s, v in values.items():
                h.values[int(s)] = np.asarray(v, dtype=np.float64)
            h.running, h.drained, h.lost = int(running), int(drained), bool(lost)

        # -- bands, plain and per zone --
        def bands_configure(self, names, kinds=(), probs=(0.05, 0.5, 0.95), interval=86400, t_first=0, mask=None, capacity=4096, zones=None, n_zones=None):
            self._bands_row0, self._bands_zonal = 0, bool(list(names)) and zones is not None
            if self._bands_zonal:
                if mask is not None or int(interval) not in (86400, 3600, 600) or int(t_first) % int(interval) or int(capacity) < 1:
                    raise ValueError("bands_configure: zones")
                self._bands = HostZonalBands(kinds, probs, self.n, np.asarray(zones).reshape(-1), int(n_zones), interval, t_first)
                self._bnames = list(names)
            else:
                super().bands_configure(names, kinds, probs, interval, t_first, mask, capacity)
            self._configured("bands", bool(list(names)))

        def _bands_parts(self):
            return self._bands.per_zone if self._bands_zonal else [self._bands]

        def bands_count(self):
            if self._bands is None:
                raise RuntimeError("bands_configure has not been called")
            return self._bands_row0 + len(self._bands.rows()[0])

        def bands_read(self, first, n):
            if self._bands is None or self._bands_zonal:
                raise RuntimeError("bands_read: not configured, or configured per zone")
            first = int(first) - self._bands_row0
            assert first >= 0
            return tuple(a[first:first + n].copy() for a in self._bands.rows())

        def bands_zonal_read(self, first, n):
            if self._bands is None or not self._bands_zonal:
                raise RuntimeError("bands_zonal_read: not configured, or configured without zones")
            first = int(first) - self._bands_row0
            assert first >= 0
            return tuple(a[first:first + n].copy() for a in self._bands.rows())

        def bands_state(self):
            if self._bands is None:
                raise RuntimeError("bands_configure has not been called")
            acc = np.zeros_like(self._bands_parts()[0].acc)
            for h in self._bands_parts():
                acc[:, h.on] = h.acc[:, h.on]
            return acc

        def bands_restore(self, acc, rows):
            self._restorable("bands", self._bands)
            acc = np.asarray(acc, dtype=np.float64)
            if acc.shape != self._bands_parts()[0].acc.shape or int(rows) < 0:
                raise ValueError("bands_restore: size mismatch, or rows")
            for h in self._bands_parts():
                h.acc[:, h.on] = acc[:, h.on]
            self._bands_row0 = int(rows)

    return ResumeOracleContext
