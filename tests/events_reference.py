"""The event outputs' device rule (rh_events_*, k_events in roger_amd/csrc/rh_events.h) restated on the host in plain numpy over a list
of (e, t0, t1, dt, planes), and the CPU double with it.  Imports nothing from roger_amd.

After a step over (t0, t1] of dt hours whose event id is e (0: no event, nothing happens): slot = e % n_slots; the step is the first of
its event in the slot when the slot's header id differs from e.  Header per slot, int64 {event id, steps, t0 of the first step, t1 of the
last step, steps of 600 s, steps of 3600 s}, -1 each until a step touches the slot; the event that was running at the configuration
(`running`) keeps t0 = -1.  Per item with value v and slot element p:
    SUM (0):    p = v if first else p + v
    PEAK (1):   r = v / dt;  p = r if first else (r if r > p or (p is NaN and r is not) else p)
    FIRST (2):  p = v on the first step only
    LAST (3):   p = v on every step
A step of event e with e - drained > n_slots stores nothing and sets `lost`.  numpy's `/` and `+` on float64 arrays are single IEEE
operations, which is the rule.
`EventsOracleContext` is tests/oracle_context.py's double with the three events_* methods of `_native.Context`."""
import numpy as np

from oracle_context import OracleContext

SUM, PEAK, FIRST, LAST = 0, 1, 2, 3
DT_HOURS = {600: 1.0 / 6, 3600: 1.0, 86400: 24.0}     # S.dt of the three step classes (rh_control.h, scalars_update)


class HostEvents:
    """hdr (n_slots, 6) int64, values (n_slots, J, n) float64 and `lost`, advanced by `add` after every step."""

    def __init__(self, kinds, n, n_slots=1, running=0, drained=0):
        self.kinds = [int(k) for k in kinds]
        self.n, self.ns = int(n), int(n_slots)
        self.running, self.drained = int(running), int(drained)
        self.hdr = np.full((self.ns, 6), -1, dtype=np.int64)
        self.values = np.zeros((self.ns, len(self.kinds), self.n))
        self.lost = False

    def add(self, e, t0, t1, dt, planes):
        """planes: one (n,) array per item, the values after the step over (t0, t1] of dt hours with event id e."""
        e, t0, t1 = int(e), int(t0), int(t1)
        if e == 0:
            return
        if e - self.drained > self.ns:
            self.lost = True
            return
        slot = e % self.ns
        h = self.hdr[slot]
        first = int(h[0]) != e
        ten, hour = int(t1 - t0 == 600), int(t1 - t0 == 3600)
        if first:
            h[:] = (e, 1, -1 if e == self.running else t0, t1, ten, hour)
        else:
            h[1] += 1
            h[3] = t1
            h[4] += ten
            h[5] += hour
        dt = np.float64(dt)
        for j, kind in enumerate(self.kinds):
            if kind == FIRST and not first:
                continue
            v = np.asarray(planes[j], dtype=np.float64).reshape(-1)
            p = self.values[slot, j]
            if kind == SUM:
                p[:] = v if first else p + v
            elif kind == PEAK:
                with np.errstate(all="ignore"):
                    r = v / dt
                if first:
                    p[:] = r
                else:
                    take = (r > p) | ((p != p) & (r == r))
                    p[take] = r[take]
            else:
                p[:] = v


class EventsOracleContext(OracleContext):
    """The double with event outputs: the refusals of rh_events_configure as ValueError, a read before it as RuntimeError."""

    _events = None

    def events_configure(self, names, kinds=(), n_slots=1):
        names = list(names)
        if not names:
            self._events = None
            return
        if len(names) > 16 or len(kinds) != len(names):
            raise ValueError("events_configure: n_items")
        if any(self.st.planes[v].dtype != np.float64 for v in names):
            raise ValueError("events_configure: float64 planes only")
        if any(int(k) not in (SUM, PEAK, FIRST, LAST) for k in kinds) or not 1 <= int(n_slots) <= 65536:
            raise ValueError("events_configure: kinds, n_slots")
        s = self.st.scal
        running = int(s.event_id[1])
        self._events = HostEvents(kinds, self.n, n_slots, running, (running if running > 0 else int(s.event_id_counter)) - 1)
        self._enames = names

    def events_read(self, slots=None):
        if self._events is None:
            raise RuntimeError("events_configure has not been called")
        h = self._events
        if slots is None:
            slots = [s for s in range(h.ns) if h.hdr[s, 0] >= 0]
        return h.hdr.copy(), {int(s): h.values[int(s)].copy() for s in slots}, bool(h.lost)

    def events_set_drained(self, event_id):
        if self._events is None:
            raise RuntimeError("events_configure has not been called")
        self._events.drained = int(event_id)

    def _accumulate(self):
        super()._accumulate()
        if self._events is None:
            return
        s = self.st.scal
        self._events.add(int(s.event_id[1]), int(s.time) - int(s.dt_secs), int(s.time), float(s.dt), [self.st.planes[v] for v in self._enames])
