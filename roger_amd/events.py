"""Event outputs: one map per rainfall event and item -- the event's sum, its peak intensity, the value it started from, the value it
ended with -- accumulated on the device after every step (include/roger_hip.h, rh_events_*; k_events in roger_amd/csrc/rh_events.h).
The adaptive time stepping numbers the events (`event_id`); here the accumulators' slot is the event, not the day.  The event runoff
coefficient of every column is `(q_hof + q_sof) / prec` of two or three "sum" items, without ten-minute output of the whole run.

A setup script fills `state.events` in `set_diagnostics`:

    state.events.items = [("prec", "sum"), ("q_hof", "sum"), ("q_sof", "sum"), ("q_sur", "peak"), ("theta_rz", "first")]
    state.events.n_slots = 16                     # events resident on the device between two read-outs
    state.events.base_output_path = ...           # as for the diagnostics

and gets `<identifier>.events.nc`: dimensions event (unlimited), y and x; per event `event_id`, `event_start` and `event_end` (days, with
`time_origin`; the start of its first and the end of its last step), `event_steps`, `event_steps_10min`, `event_steps_hourly`; per
item a variable `<name>_<kind>` (event, y, x) float64.  The kinds: "sum" adds the value of every step of the event, "peak" keeps the
largest value / dt in mm/h (a NaN is never taken over a number), "first" keeps the value after the event's first step, "last" the value
after its last.

An event is complete once a later step ran under another event id (0, between events, included), or at the end of run().  Completed
events are read out after every round of device steps and after each step of the host loops, and their slots are handed back to the
device.  The device overwrites no slot that has not been read: if more than `n_slots` events pass between two read-outs, the run stops
with an error that names the remedy.  With several ranks a rank writes one file of its own for its block, named as the diagnostics
name theirs.

Start and restart.  An event that is already running when the observer is configured -- a run continued from a restart file written
in mid-event -- is written with `event_start = -1`: its maps cover the steps from the configuration on.  Without `resume` the maps are
not part of restart files.

Resuming.  With `state.events.resume = True` every restart file that is written holds the group "hip_events": the slots' headers and ids,
`running`, `drained`, `lost`, the maps of the events that are not complete yet (the one that is running: the completed ones are read out
and `<identifier>.events.nc` is written at that moment -- they can be many times the size of the arena and do not go into the restart
file), the host's bookkeeping and the request.  A run that reads such a file with `resume = True` and the same request -- items, n_slots,
grid -- uploads all of it: the event that was running at the restart appears ONCE, in the continued run's file, with its true
`event_start` and its sums and peak over the whole event, and the interrupted run's file followed by the continued run's along the `event`
axis is the uninterrupted run's.  A run whose last act is the restart file of the end of run() leaves the running event to the continued
run: its own file ends with the last completed event.  A different request is a RuntimeError that names the first difference; a restart
file without the group too (set `resume = False` for the behaviour above).  One rank only: `initialize` refuses `resume = True` with
several ranks (restart files are gathered to rank 0, the maps are not)."""
import numpy as np

from . import runtime_settings as rs
from .observers import (DAY, WRITE_BYTES, Observer, carried_group, check_planes, check_resume, check_same_request, claim_output_file,
                        global_attributes, names_array, request_group, svat_only, write_file, xy_variables)

MAX_ITEMS = 16                    # roger_amd/csrc/rh_events.h: RH_EVENTS_MAX_ITEMS
MAX_SLOTS = 65536                 # include/roger_hip.h: RH_EVENTS_MAX_SLOTS
KINDS = {"sum": 0, "peak": 1, "first": 2, "last": 3}


class Events(Observer):
    """`state.events`: what the script sets (items, n_slots, base_output_path, resume) and the events drained so far."""

    group = "hip_events"

    def __init__(self):
        self.items = []
        self.n_slots = 16
        self.base_output_path = None
        self.output_path = "{identifier}.events.nc"
        self._on = False         # start() configured the device
        self._items = []         # [(name, kind string)] as validated
        self._hdr = []           # drained headers, (6,) int64 each
        self._values = []        # drained maps, (n_items, n) float64 each
        self._drained = None     # the highest event id read out (None: as the configuration left it)
        self._last_id = 0        # the event id of the last step a host loop looked at
        self._unwritten = 0
        self._handed_over = None # resume: the time step at which the running event went into a restart file
        self._path = None

    @property
    def active(self):
        return bool(self.items)

    def _request(self, state):
        """What a resumed run must ask for again (observers.check_same_request)."""
        return {"items": names_array(f"{v} {k}" for v, k in self._items), "n_slots": np.int64(self.n_slots),
                "grid": np.asarray([state.settings.nx, state.settings.ny], dtype=np.int64)}

    def restart_state(self, state):
        """The group "hip_events" of a restart file.  The completed events are read out and the file is written first: what is left on
        the device is the event that is running, and only its maps go into the restart file."""
        if not self._on:
            return None
        self.drain(state, final=True)
        ctx = state.backend_context
        hdr, _, lost = ctx.events_read(slots=())
        ids, running, drained = ctx.events_state()
        live = [s for s in range(hdr.shape[0]) if int(hdr[s, 0]) > 0 and int(hdr[s, 0]) > int(drained)]
        out = dict(request_group(self._request(state)), hdr=np.asarray(hdr, dtype=np.int64), ids=np.asarray(ids, dtype=np.int64),
                   scalars=np.asarray([running, drained, int(bool(lost)), self._last_id], dtype=np.int64), slots=np.asarray(live, dtype=np.int32))
        if live:
            _, values, _ = ctx.events_read(slots=live)
            out["maps"] = np.stack([values[s] for s in live])
        self._handed_over = int(state.variables.itt)
        return out

    def drain(self, state, final=False, end=False):
        """Read out the completed events: every resident event but the one the last step belonged to (end, the end of run(): that one
        too; it stays on the device until it ends or run() does).  final: the file is written now (otherwise when enough has been
        read out)."""
        if not self._on:
            return
        ctx = state.backend_context
        hdr, _, lost = ctx.events_read(slots=())
        if lost:
            raise RuntimeError(f"events: more than {int(self.n_slots)} rainfall events passed between two read-outs and the device kept no "
                               "slot for the last ones: raise state.events.n_slots (more slots), or call run_device() in shorter pieces")
        current = 0 if end else int(ctx.get_scalars().event_id[1])
        self._last_id = current
        done = sorted((int(hdr[s, 0]), s) for s in range(hdr.shape[0])
                      if hdr[s, 0] > 0 and int(hdr[s, 0]) != current and (self._drained is None or int(hdr[s, 0]) > self._drained))
        if done:
            _, values, _ = ctx.events_read(slots=[s for _, s in done])
            for e, s in done:
                self._hdr.append(hdr[s].copy())
                self._values.append(values[s])
                self._unwritten += values[s].nbytes
            self._drained = done[-1][0]
            ctx.events_set_drained(self._drained)
        if end or final or self._unwritten > WRITE_BYTES:
            self._unwritten = 0
            if self._path:
                self._write(state)

    def stepped(self, state):
        """A host loop made one step: read out when the step ran under another event id than the one before it (an event ended)."""
        if not self._on:
            return
        e = int(state.variables._get_scalars().event_id[1])
        if e != self._last_id:
            if self._last_id > 0:
                self.drain(state)
            self._last_id = e

    def close(self, state):
        """End of run(): the event that is still running counts as complete, and the file -- unless this very step's restart file took
        the running event over (`resume`): then it belongs to the run that continues."""
        if self.resume and self._on and self._handed_over is not None and self._handed_over == int(state.variables.itt):
            return self.drain(state, final=True)
        self.drain(state, end=True)

    def _write(self, state):
        """The whole file from the events held in memory, through roger_amd.nc4lite."""
        from .diagnostics import _UNITS

        settings = state.settings
        nxl, nyl = settings.nx // rs.num_proc[0], settings.ny // rs.num_proc[1]
        x, y, variables = xy_variables(state.variables)
        hdr = np.stack(self._hdr) if self._hdr else np.zeros((0, 6), dtype=np.int64)
        days = lambda t: np.where(t < 0, -1.0, t / float(DAY))   # noqa: E731  (-1: the event was running when the observer was configured)
        time_attrs = {"units": "days", "time_origin": str(settings.time_origin)}
        variables.update({
            "event_id": (("event",), hdr[:, 0].astype(np.int64), {"long_name": "event id of the adaptive time stepping", "units": ""}),
            "event_start": (("event",), days(hdr[:, 2].astype(np.float64)), dict(time_attrs, long_name="start of the event's first step (-1: before the run was (re)started)")),
            "event_end": (("event",), days(hdr[:, 3].astype(np.float64)), dict(time_attrs, long_name="end of the event's last step")),
            "event_steps": (("event",), hdr[:, 1].astype(np.int64), {"long_name": "time steps of the event", "units": ""}),
            "event_steps_10min": (("event",), hdr[:, 4].astype(np.int64), {"long_name": "ten-minute steps of the event", "units": ""}),
            "event_steps_hourly": (("event",), hdr[:, 5].astype(np.int64), {"long_name": "hourly steps of the event", "units": ""}),
        })
        long_names = {"sum": "sum over the event", "peak": "peak intensity of the event", "first": "value after the event's first step",
                      "last": "value after the event's last step"}
        for j, (v, kind) in enumerate(self._items):
            a = np.stack([m[j].reshape(nxl, nyl).T for m in self._values]) if self._values else np.zeros((0, nyl, nxl))
            unit = _UNITS.get(v, "")
            if kind == "peak":
                unit = "mm/h" if unit == "mm/dt" else (unit + "/h" if unit else "1/h")
            elif kind == "sum" and unit == "mm/dt":
                unit = "mm"
            variables[f"{v}_{kind}"] = (("event", "y", "x"), np.ascontiguousarray(a), {"long_name": f"{v}: {long_names[kind]}", "units": unit})
        write_file(self._path, {"event": None, "y": len(y), "x": len(x)}, variables, global_attributes(
            settings.identifier, "One record per rainfall event of the adaptive time stepping, accumulated on the device after every step."))


def initialize(state):
    """Validate what the script asked for (after set_diagnostics); the device is configured by `start`, once the event ids are known."""
    ev = state.events
    if not ev.active:
        return
    check_resume("events", ev)
    svat_only("events", state.settings, " and knows no rainfall events; the event outputs belong to the SVAT / oneD step")
    items = []
    for item in ev.items:
        if not isinstance(item, (tuple, list)) or len(item) != 2:
            raise ValueError(f"events: item {item!r} (a pair (variable, kind), kind one of " + ", ".join(f'"{k}"' for k in KINDS) + ")")
        v, kind = item
        if kind not in KINDS:
            raise ValueError(f"events: kind of {v!r} is {kind!r} (" + ", ".join(f'"{k}"' for k in KINDS) + ")")
        check_planes("events", (v,), state)
        if (v, kind) in items:
            raise ValueError(f"events: item ({v!r}, {kind!r}) is given twice")
        items.append((v, kind))
    if len(items) > MAX_ITEMS:
        raise ValueError(f"events: {len(items)} items (at most {MAX_ITEMS})")
    if not 1 <= int(ev.n_slots) <= MAX_SLOTS:
        raise ValueError(f"events: n_slots = {ev.n_slots} (1 ... {MAX_SLOTS} events resident on the device)")
    ev._items = items


def start(state):
    """Configure the device (after the restart file was read: an event that is running now keeps event_start = -1).  A resumed run
    (`resume`, and the restart file holds "hip_events") uploads the slots as they were instead: the running event keeps its start."""
    ev = state.events
    if not ev.active or not ev._items:
        return
    held = carried_group("events", ev)
    if held is not None:
        check_same_request("events", ev, held, ev._request(state))
    state.variables.flush_to_device()
    state.backend_context.events_configure([v for v, _ in ev._items], [KINDS[k] for _, k in ev._items], int(ev.n_slots))
    ev._on, ev._hdr, ev._values, ev._drained, ev._unwritten, ev._handed_over = True, [], [], None, 0, None
    ev._last_id = int(state.backend_context.get_scalars().event_id[1])
    if held is not None:
        running, drained, lost, last_id = (int(v) for v in held["scalars"])
        maps = {int(s): held["maps"][k] for k, s in enumerate(np.asarray(held["slots"]).reshape(-1))}
        state.backend_context.events_restore(held["hdr"], held["ids"], running, drained, bool(lost), maps)
        ev._drained, ev._last_id = drained, last_id
    ev._path = claim_output_file(ev, state, "events")


def drain(state, final=False):
    state.events.drain(state, final=final)


def close(state):
    state.events.close(state)
