"""roger_amd/observers.py: the registry RogerSetup walks instead of naming the observers, and the one drain of the rings.  The orders
are spelled out here as they stood in roger.py when every observer was named there, nine times."""
import importlib
import types

import numpy as np
import pytest

ALL = ["points", "totals", "zonal_totals", "scores", "events", "durations", "bands",
       "transport_points", "transport_totals", "transport_zonal_totals", "transport_scores"]
MODULES = {"transport_points": "sas_points", "transport_totals": "sas_totals", "transport_zonal_totals": "sas_zonal_totals",
           "transport_scores": "sas_scores"}
SVAT_RINGS = ["points", "totals", "zonal_totals", "bands"]
TRANSPORT_RINGS = ["transport_points", "transport_totals", "transport_zonal_totals"]


def module_of(attribute):
    return importlib.import_module("roger_amd." + MODULES.get(attribute, attribute))


def test_every_entry_is_on_a_fresh_state_and_the_calls_keep_their_order(monkeypatch):
    from roger_amd import observers
    from roger_amd.state import RogerState

    assert [e.attribute for e in observers.REGISTRY] == ALL
    state = RogerState()
    calls = []
    for e in observers.REGISTRY:
        module, obj = module_of(e.attribute), getattr(state, e.attribute)
        assert e.module == module.__name__.rsplit(".", 1)[1] and type(obj) is getattr(module, e.cls)
        assert isinstance(obj, observers.RingSeries) == e.ring and obj.output_path.endswith(f".{e.attribute}.nc")
        for name in ("initialize", "start"):
            if hasattr(module, name):
                monkeypatch.setattr(module, name, lambda st, a=e.attribute, n=name: calls.append((n, a)))
        for name in ("close", "stepped", "drain", "check_call"):
            if hasattr(obj, name):
                monkeypatch.setattr(type(obj), name, lambda self, *args, a=e.attribute, n=name, **kw: calls.append((n, a, args[1:], kw)))

    def called(f, *args, **kw):
        calls.clear()
        f(state, *args, **kw)
        return [c[:2] for c in calls], [c[2:] for c in calls]

    assert called(observers.initialize)[0] == [("initialize", a) for a in ALL]
    assert called(observers.start, transport=False)[0] == [("start", a) for a in ("scores", "events", "durations", "bands")]
    assert called(observers.start, transport=True)[0] == [("start", a) for a in TRANSPORT_RINGS + ["transport_scores"]]
    assert called(observers.close)[0] == [("close", a) for a in ALL]
    assert called(observers.stepped)[0] == [("stepped", a) for a in SVAT_RINGS + ["events"]]
    assert called(observers.stepped, transport=True)[0] == [("stepped", a) for a in TRANSPORT_RINGS]
    assert called(observers.check_call, 7) == ([("check_call", a) for a in SVAT_RINGS], [((), {})] * 4)
    assert called(observers.drain_rings)[0] == [("drain", a) for a in SVAT_RINGS + TRANSPORT_RINGS]
    who, how = called(observers.drain_round, final=True)
    assert who == [("drain", a) for a in SVAT_RINGS + ["events"]] and how == [((), {"final": True})] * 5


def configure(state, attribute):
    """The least a script sets for `state.<attribute>.active`."""
    o = getattr(state, attribute)
    if attribute in ("points", "transport_points"):
        o.cells, o.output_variables = [(0, 0)], ["q_ss"]
    elif attribute in ("totals", "transport_totals"):
        o.output_variables = ["q_ss"]
    elif attribute in ("zonal_totals", "transport_zonal_totals"):
        o.zones, o.output_variables = np.ones((4, 2), dtype=int), ["q_ss"]
    elif attribute in ("scores", "transport_scores"):
        o.observations = {"q_ss": np.zeros(3)}
    elif attribute == "events":
        o.items = [("q_ss", "sum")]
    else:
        o.variables = {"q_ss": [1.0]} if attribute == "durations" else ["q_ss"]
    assert o.active


@pytest.mark.parametrize("attribute", [None] + ALL)
def test_needs_end_of_step_is_the_expression_the_lean_loop_had(attribute):
    from roger_amd import observers
    from roger_amd.state import RogerState

    state = RogerState()
    if attribute:
        configure(state, attribute)
    was = state.points.active or state.totals.active or state.zonal_totals.active or state.events.active or state.bands.active
    assert observers.needs_end_of_step(state) is bool(was) and bool(was) == (attribute in SVAT_RINGS + ["events"])


def test_ring_capacity_is_the_same_on_a_rank_without_a_zone(monkeypatch):
    """4 x 2 columns on two ranks, every zone and every band column in the block of rank 0: rank 1 configures neither ring (_on is False)
    and still takes the rounds of its peer -- the smallest capacity the script asked for."""
    from roger_amd import bands, observers, runtime_state, totals, zonal_totals

    zones = np.array([[1, 2], [2, 1], [0, 0], [0, 0]])
    on, capacity = {}, {}
    for rank in (0, 1):
        configured = []
        ctx = types.SimpleNamespace(**{f"{k}_configure": (lambda *a, k=k: configured.append(k)) for k in ("totals", "zonal", "bands")})
        state = types.SimpleNamespace(
            settings=types.SimpleNamespace(nx=4, ny=2, enable_offline_transport=False, identifier="run", time_origin="1900-01-01"),
            var_meta={"q_ss": types.SimpleNamespace(plane=7, dtype=None)}, backend_context=ctx,
            variables=types.SimpleNamespace(time=0, itt=0, flush_to_device=lambda: None, q_ss=np.zeros((6, 6))))   # (the rank's block)
        observers.create(state)
        for module in (totals, zonal_totals, bands):
            monkeypatch.setattr(module, "rs", types.SimpleNamespace(num_proc=(2, 1)))
        monkeypatch.setattr(observers, "rs", types.SimpleNamespace(diskless_mode=True))
        monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self, r=rank: r))
        monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
        assert observers.ring_capacity(state) is None
        state.totals.output_variables, state.totals.capacity = ["q_ss"], 48
        state.zonal_totals.output_variables, state.zonal_totals.zones, state.zonal_totals.capacity = ["q_ss"], zones, 24
        state.bands.variables, state.bands.mask, state.bands.capacity = ["q_ss"], zones > 0, 12
        for module in (totals, zonal_totals, bands):
            module.initialize(state)
        bands.start(state)
        on[rank] = (configured, [getattr(state, a)._on for a in ("totals", "zonal_totals", "bands")])
        capacity[rank] = observers.ring_capacity(state)
    assert on == {0: (["totals", "zonal", "bands"], [True, True, True]), 1: (["totals"], [True, False, False])}
    assert capacity == {0: 12, 1: 12}


@pytest.mark.parametrize("attribute,label,count", [("points", "points", lambda n: n), ("totals", "totals", lambda n: (n, 3)),
                                                   ("zonal_totals", "zonal totals", lambda n: (n, [3])), ("bands", "bands", lambda n: n)])
def test_a_ring_that_wrapped_is_refused_in_the_words_every_ring_had(attribute, label, count):
    from roger_amd import observers
    from roger_amd.state import RogerState

    state = RogerState()
    ring = getattr(state, attribute)
    kind = {"zonal_totals": "zonal"}.get(attribute, attribute)
    rows = types.SimpleNamespace(n=0)
    state._ctx = types.SimpleNamespace(**{f"{kind}_count": lambda: count(rows.n),
                                          f"{kind}_read": lambda first, n: (np.zeros((n, 3), dtype=np.int64), np.zeros((n, 1, 1)))})
    ring.capacity, ring._on = 4, True
    rows.n = 3
    ring.drain(state)
    assert ring._read == 3 and [len(h) for h in ring._hdr] == [3] and ring._unwritten == 3 * 32
    rows.n = 8   # five rows since the last drain, four resident
    with pytest.raises(RuntimeError) as e:
        observers.drain_rings(state)
    assert str(e.value) == f"5 rows of the {label} recorded since the last drain but only 4 are resident on the device"
    with pytest.raises(RuntimeError) as e:
        observers.check_call(state, 5)
    assert str(e.value) == (f"5 steps in one call but only 4 rows of the {label} are resident on the device: "
                            f"call run_device() in shorter pieces, or raise state.{attribute}.capacity")
    ring.check_call(4)
    for _ in range(3):
        ring.stepped(state)
    assert ring._steps == 3
    rows.n = 7
    ring.stepped(state)   # the fourth step call since the last drain: the capacity
    assert ring._steps == 0 and ring._read == 7
