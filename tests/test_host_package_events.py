"""CPU: `state.events` (roger_amd/events.py) on the oracle double with the restatement (tests/events_reference.py): a setup script ends
with an `.events.nc` whose records are the restatement applied to the double's planes after every step, on the device-rounds loop and on
the host loop; the validation messages; the read-out and the lost-events error on a fake context."""
import types

import numpy as np
import pytest

from events_reference import FIRST, LAST, PEAK, SUM, EventsOracleContext, HostEvents
from golden_util import load_case

ITEMS = [("prec", "sum"), ("q_ss", "sum"), ("q_sur", "peak"), ("theta_rz", "first"), ("S_rz", "last")]
KINDS = (SUM, SUM, PEAK, FIRST, LAST)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


@pytest.fixture
def events_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []

    def make(*a, **k):
        made.append(EventsOracleContext(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


def make_model(tmp_path, ndays=6, script_hooks=None, **settings):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks=script_hooks)
    cfg = dict(items=ITEMS, base_output_path=str(tmp_path))
    cfg.update(settings)

    def set_diagnostics(self, state):
        for k, v in cfg.items():
            setattr(state.events, k, v)

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model


@pytest.mark.parametrize("script_hooks,by_routine,n_slots", [(None, False, 16), ("plain", True, 1)])
def test_script_writes_the_events_of_the_doubles_planes(events_backend, tmp_path, monkeypatch, script_hooks, by_routine, n_slots):
    """The device-rounds loop with 16 slots, and the host loop with ONE slot: the read-out after the step that ends an event frees it."""
    from nc_util import netcdf_file

    from roger_amd import h5lite

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    model = make_model(tmp_path, script_hooks=script_hooks, n_slots=n_slots)
    model.setup()
    ctx = events_backend[-1]
    steps = []
    accumulate = ctx._accumulate

    def recording():
        accumulate()
        s = ctx.st.scal
        steps.append((int(s.event_id[1]), int(s.time) - int(s.dt_secs), int(s.time), float(s.dt), {v: ctx.download(v).copy() for v, _ in ITEMS}))

    ctx._accumulate = recording
    model.run()
    ids = [e for e, *_ in steps]
    events = sorted(set(ids) - {0})
    assert len(events) >= 3 and {t1 - t0 for e, t0, t1, *_ in steps if e} >= {600, 3600}
    h = HostEvents(KINDS, 16, n_slots=64)
    for e, t0, t1, dt, p in steps:
        h.add(e, t0, t1, dt, [p[v] for v, _ in ITEMS])
    path = tmp_path / "GoldenSVAT.events.nc"
    assert h5lite.is_hdf5(str(path))
    f = netcdf_file(str(path))
    assert f.variables["event_id"].dimensions == ("event",) and list(f.variables["event_id"][:]) == events
    want = h.hdr[events]
    np.testing.assert_array_equal(f.variables["event_start"][:], want[:, 2] / 86400.0)
    np.testing.assert_array_equal(f.variables["event_end"][:], want[:, 3] / 86400.0)
    assert f.variables["event_start"].units == b"days" and f.variables["event_end"].time_origin == f.variables["event_start"].time_origin
    for key, col in (("event_steps", 1), ("event_steps_10min", 4), ("event_steps_hourly", 5)):
        np.testing.assert_array_equal(f.variables[key][:], want[:, col])
    for j, (v, kind) in enumerate(ITEMS):
        var = f.variables[f"{v}_{kind}"]
        a = np.asarray(var[:])
        assert var.dimensions == ("event", "y", "x") and a.shape == (len(events), 4, 4)
        for k, e in enumerate(events):
            assert same_bits(a[k], h.values[e, j].reshape(4, 4).T), (v, kind, e)
    assert np.any(np.asarray(f.variables["prec_sum"][:]) != 0) and f.variables["q_sur_peak"].units == b"mm/h" and f.variables["prec_sum"].units == b"mm"


def test_an_event_running_at_the_start_keeps_no_start_and_the_last_event_is_written_at_close(events_backend, tmp_path):
    """The double's scalars say an event is running when the observer is configured (as a restart file written in mid-event does):
    event_start = -1 for it.  A run that ends inside an event writes that event at close()."""
    from nc_util import netcdf_file

    from roger_amd import events

    model = make_model(tmp_path, ndays=3)
    model.setup()
    ctx, state = events_backend[-1], model.state
    ctx.st.scal.event_id[1] = ctx.st.scal.event_id_counter = 5
    events.start(state)                      # (what setup() does behind restart.read_restart)
    v = np.arange(16.0)
    ctx._events.add(5, 600, 1200, 1.0 / 6, [v] * len(ITEMS))
    ctx._events.add(6, 7200, 10800, 1.0, [v + 1] * len(ITEMS))
    ctx.st.scal.event_id[1] = 6              # the run ends inside event 6
    events.drain(state)
    assert [int(h[0]) for h in state.events._hdr] == [5] and ctx._events.drained == 5
    events.close(state)
    f = netcdf_file(str(tmp_path / "GoldenSVAT.events.nc"))
    assert list(f.variables["event_id"][:]) == [5, 6]
    assert list(f.variables["event_start"][:]) == [-1.0, 7200 / 86400.0] and list(f.variables["event_end"][:]) == [1200 / 86400.0, 10800 / 86400.0]
    assert list(f.variables["event_steps_10min"][:]) == [1, 0] and list(f.variables["event_steps_hourly"][:]) == [0, 1]
    assert same_bits(f.variables["S_rz_last"][:][1], (v + 1).reshape(4, 4).T) and same_bits(f.variables["q_sur_peak"][:][0], (v / (1.0 / 6)).reshape(4, 4).T)


def test_refusals(events_backend, tmp_path):
    for kw, exc, text in ((dict(items=[("prec", "mean")]), ValueError, r"kind of 'prec' is 'mean' \(\"sum\", \"peak\", \"first\", \"last\"\)"),
                          (dict(items=["prec"]), ValueError, r"item 'prec' \(a pair \(variable, kind\)"),
                          (dict(items=[("prec", "sum"), ("prec", "sum")]), ValueError, r"item \('prec', 'sum'\) is given twice"),
                          (dict(items=[("lu_id", "last")]), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(items=[("no_such_variable", "sum")]), NotImplementedError, "no_such_variable"),
                          (dict(items=[(v, k) for v in ("prec", "q_ss", "aet", "S_rz", "theta") for k in ("sum", "peak", "first", "last")][:17]),
                           ValueError, r"17 items \(at most 16\)"),
                          (dict(n_slots=0), ValueError, r"n_slots = 0 \(1 \.\.\. 65536"),
                          (dict(n_slots=65537), ValueError, "n_slots = 65537")):
        model = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model = make_model(tmp_path, ndays=1, items=[])
    model.setup()
    model.run()
    assert events_backend[-1]._events is None and not model.state.events._on and not list(tmp_path.iterdir())


def test_the_offline_transport_is_refused():
    from roger_amd import events
    from roger_amd.state import RogerState

    st = RogerState()
    assert not st.events.active
    events.initialize(st)
    st.events.items = [("q_ss", "sum")]
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    with pytest.raises(NotImplementedError, match="offline transport"):
        events.initialize(st)


class FakeContext:
    """events_read / events_set_drained / get_scalars over a HostEvents, counting the calls."""

    def __init__(self, n_slots):
        self.h = HostEvents((SUM,), 3, n_slots)
        self.current, self.reads, self.published = 0, [], []

    def step(self, e, k):
        self.current = e
        self.h.add(e, 600 * k, 600 * (k + 1), 1.0 / 6, [np.full(3, float(k))])

    def events_read(self, slots=None):
        self.reads.append(None if slots is None else list(slots))
        return self.h.hdr.copy(), {int(s): self.h.values[int(s)].copy() for s in (slots or ())}, self.h.lost

    def events_set_drained(self, e):
        self.published.append(int(e))
        self.h.drained = int(e)

    def get_scalars(self):
        return types.SimpleNamespace(event_id=[self.current, self.current])


def fake_state(n_slots, rank=None):
    from roger_amd import events

    ev = events.Events()
    ev._on, ev.n_slots, ev._items = True, n_slots, [("q_ss", "sum")]
    return types.SimpleNamespace(events=ev, backend_context=FakeContext(n_slots))


def test_draining_on_a_fake_context():
    """Only completed events are read, in the order of their ids, each once; the highest id is published; the running event stays."""
    from roger_amd import events

    state = fake_state(2)
    ctx, ev = state.backend_context, state.events
    for k, e in enumerate((0, 1, 1, 0, 2)):
        ctx.step(e, k)
    events.drain(state)                                   # event 1 is complete, event 2 is running
    assert [int(h[0]) for h in ev._hdr] == [1] and ctx.published == [1] and ctx.reads == [[], [1]]
    assert list(ev._values[0][0]) == [3.0, 3.0, 3.0]      # steps 1 and 2: 1 + 2
    events.drain(state)                                   # nothing new: the headers only
    assert len(ev._hdr) == 1 and ctx.published == [1] and ctx.reads[2:] == [[]]
    for k, e in enumerate((2, 3, 0), start=5):            # event 2 ends, event 3 takes the slot event 1 had
        ctx.step(e, k)
    assert not ctx.h.lost
    events.drain(state)
    assert [int(h[0]) for h in ev._hdr] == [1, 2, 3] and ctx.published == [1, 3] and ctx.reads[-1] == [0, 1]
    assert list(ev._hdr[1]) == [2, 2, 2400, 3600, 2, 0] and list(ev._values[2][0]) == [6.0] * 3


def test_the_lost_events_error_names_the_remedy():
    from roger_amd import events

    state = fake_state(1)
    ctx = state.backend_context
    for k, e in enumerate((1, 0, 2)):                     # event 2 finds the only slot unread
        ctx.step(e, k)
    assert ctx.h.lost and ctx.h.hdr[0, 0] == 1
    with pytest.raises(RuntimeError, match=r"more than 1 rainfall events passed between two read-outs.*raise state\.events\.n_slots "
                                           r"\(more slots\), or call run_device\(\) in shorter pieces"):
        events.drain(state)
    assert not state.events._hdr and not ctx.published


def test_two_rank_file_name(monkeypatch, tmp_path):
    """With several ranks a rank writes one file of its own, named as the diagnostics name theirs."""
    from roger_amd import events, runtime_state

    calls = []
    ctx = types.SimpleNamespace(events_configure=lambda *a: calls.append(a), get_scalars=lambda: types.SimpleNamespace(event_id=[0, 0]))
    meta = types.SimpleNamespace(plane=7, dtype=None)
    state = types.SimpleNamespace(settings=types.SimpleNamespace(nx=6, ny=4, enable_offline_transport=False, identifier="run"),
                                  var_meta={"q_ss": meta}, variables=types.SimpleNamespace(flush_to_device=lambda: None),
                                  backend_context=ctx, events=events.Events())
    state.events.items, state.events.n_slots, state.events.base_output_path = [("q_ss", "peak")], 3, str(tmp_path)
    monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self: 1))
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
    events.initialize(state)
    events.start(state)
    assert calls == [(["q_ss"], [1], 3)] and state.events._on and state.events._path.endswith("run.events.0001.nc")
