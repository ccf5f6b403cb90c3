"""GPU: event outputs (rh_events_*, k_events in roger_amd/csrc/rh_events.h) against the host restatement (tests/events_reference.py),
values as bits, headers and the lost flag exactly.

The reference is tests/test_hip_points.py's pattern: a context WITHOUT observers steps one call per step and the items' planes and the
scalars (the event id among them, rh_get_scalars) are downloaded after every step; the restatement forms the expectation from them.
Grids 3 x 2, 257 x 1 and 40 x 25, each for SVAT and oneD, over the 8 days of the combo forcing: 150 steps, four events (steps 3-10 and
29-43 hourly, 58-116 of ten minutes, 131-145 hourly) with daily and hourly steps between them.  No DAILY step lies inside an event, in
8 days or in 30 (checked on the CPU oracle): a daily step is chosen on a dry day without snow, where the event clock runs past
end_event and the step ends the event.  `test_the_reference_run` therefore asserts the two classes that occur inside events and the
daily class between them; a daily step inside an event is covered by the restatement's own test (tests/test_events_reference.py).

Pieces (case 2).  With n_slots = 2 and pieces of 1, 2, 37 steps and the rest, the last piece holds the end of event 2 and events 3 and
4: event 4 finds slot 0 unread and is lost -- by the rule.  The test replays the same read-outs on the restatement and compares the
device with it exactly (events 1-3 intact, the lost flag set); a second set of pieces (1, 2, 37, 60 and the rest) loses nothing and
gives all four events bit-equal to the one-call run."""
import functools
import types

import numpy as np
import pytest

from events_reference import DT_HOURS, FIRST, LAST, PEAK, SUM, HostEvents
from test_hip_points import CASES, NDAYS, NSTEPS, make_ctx, same_bits

pytestmark = pytest.mark.gpu

# pure outputs (q_ss, aet, theta, q_hof, q_sur), stored planes (S_rz, theta_rz) and a forcing plane; all four kinds
ITEMS = (("prec", SUM), ("q_hof", SUM), ("q_sur", PEAK), ("theta_rz", FIRST), ("S_rz", LAST), ("q_ss", SUM), ("aet", PEAK), ("theta", LAST))
NAMES, KINDS = tuple(v for v, _ in ITEMS), tuple(k for _, k in ITEMS)
SLOTS = 8


class Steps:
    """Per step of a context without observers: e, t0, t1, dt (hours) and planes[name] (steps, n)."""

    def __init__(self, nx, ny, lateral):
        import hip_util as H

        ctx, forcing = make_ctx(nx, ny, lateral)
        drv = H.HipForcingDriver(ctx, forcing)
        rows, planes = [], {v: [] for v in set(NAMES)}
        while not rows or rows[-1][2] < NDAYS * 86400:
            ctx.step(drv.before_step())
            s = ctx.get_scalars()
            assert s.sanity_ok == 1 and float(s.dt) == DT_HOURS[int(s.dt_secs)]
            rows.append((int(s.event_id[1]), int(s.time - s.dt_secs), int(s.time), int(s.event_id_counter)))
            for v in planes:
                planes[v].append(ctx.download(v))
        ctx.close()
        self.rows = np.array(rows, dtype=np.int64)
        self.planes = {v: np.stack(a) for v, a in planes.items()}
        self.n = nx * ny

    def __len__(self):
        return len(self.rows)

    def feed(self, h, first, stop, names=NAMES):
        for k in range(first, stop):
            e, t0, t1, _ = (int(x) for x in self.rows[k])
            h.add(e, t0, t1, DT_HOURS[t1 - t0], [self.planes[v][k] for v in names])
        return h


@functools.lru_cache(maxsize=None)
def reference(nx, ny, lateral):
    ref = Steps(nx, ny, lateral)
    assert len(ref) == NSTEPS
    return ref


def whole(ref):
    """Every event of the run in a slot of its own."""
    return ref.feed(HostEvents(KINDS, ref.n, SLOTS), 0, len(ref))


def assert_state(ctx, want, what):
    """Headers and the lost flag exactly, every slot's maps as bits (an untouched slot is +0.0)."""
    hdr, values, lost = ctx.events_read(slots=range(want.ns))
    np.testing.assert_array_equal(hdr, want.hdr, err_msg=f"{what}: headers")
    assert lost == want.lost, (what, "lost", lost)
    for s in range(want.ns):
        ok = values[s].view(np.uint64) == want.values[s].view(np.uint64)
        assert ok.all(), (what, "slot", s, "(item, column)", np.argwhere(~ok)[:5], values[s][~ok][:3], want.values[s][~ok][:3])


def configured(nx, ny, lateral, n_slots=SLOTS):
    ctx, forcing = make_ctx(nx, ny, lateral)
    assert {"q_ss", "aet", "theta"} <= set(ctx.pure_output_planes()) and "S_rz" not in ctx.pure_output_planes()
    ctx.events_configure(NAMES, KINDS, n_slots)
    return ctx, forcing


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_the_reference_run(nx, ny, lateral):
    """At least three events; ten-minute and hourly steps inside events, daily steps between them; sums that are not all zero."""
    ref = reference(nx, ny, lateral)
    e, dts = ref.rows[:, 0], ref.rows[:, 2] - ref.rows[:, 1]
    assert len(set(e[e > 0])) >= 3, set(e)
    assert {600, 3600} <= set(dts[e > 0]) and 86400 in set(dts[e == 0]), (set(dts[e > 0]), set(dts[e == 0]))
    assert 86400 not in set(dts[e > 0]), "a daily step inside an event: assert all three classes inside events now"
    w = whole(ref)
    assert sorted(w.hdr[w.hdr[:, 0] > 0, 0]) == sorted(set(e[e > 0])) and not w.lost
    for j, v in enumerate(NAMES):
        if v != "q_hof":     # (no Hortonian overland flow on every parameter set)
            assert np.any(w.values[:, j] != 0), v


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_call_against_the_restatement(nx, ny, lateral):
    """1. One rh_run_steps call."""
    ref = reference(nx, ny, lateral)
    ctx, _ = configured(nx, ny, lateral)
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_state(ctx, whole(ref), f"{nx} x {ny} lateral={lateral}")
    ctx.close()


def read_out(ctx, h, current, drained, got, what):
    """What roger_amd/events.py's drain does, on the device and on the restatement alike: the resident events other than `current` and
    above `drained` are read, compared and handed back."""
    assert int(ctx.get_scalars().event_id[1]) == current
    hdr, _, lost = ctx.events_read(slots=())
    np.testing.assert_array_equal(hdr, h.hdr, err_msg=f"{what}: headers")
    assert lost == h.lost, (what, "lost", lost)
    done = sorted((int(hdr[s, 0]), s) for s in range(h.ns) if hdr[s, 0] > 0 and hdr[s, 0] != current and hdr[s, 0] > drained)
    if not done:
        return drained
    values = ctx.events_read(slots=[s for _, s in done])[1]
    for e, s in done:
        assert same_bits(values[s], h.values[s]), (what, "event", e)
        got[e] = (hdr[s].copy(), values[s])
    ctx.events_set_drained(done[-1][0])
    h.drained = done[-1][0]
    return done[-1][0]


@pytest.mark.parametrize("pieces,lost", [((1, 2, 37, NSTEPS - 40), True), ((1, 2, 37, 60, NSTEPS - 100), False)])
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces(nx, ny, lateral, pieces, lost):
    """2. n_slots = 2, read out between the pieces (the module's docstring on the two sets of pieces)."""
    ref = reference(nx, ny, lateral)
    ctx, _ = configured(nx, ny, lateral, 2)
    h, got, drained, k = HostEvents(KINDS, ref.n, 2), {}, 0, 0
    for n in pieces:
        ctx.run_steps(n)
        ref.feed(h, k, k + n)
        k += n
        drained = read_out(ctx, h, int(ref.rows[k - 1, 0]), drained, got, f"{nx} x {ny} lateral={lateral} after {k} steps")
    assert k == NSTEPS and h.lost == lost
    assert_state(ctx, h, f"{nx} x {ny} lateral={lateral} in pieces")
    w = whole(ref)
    assert sorted(got) == ([1, 2, 3] if lost else [1, 2, 3, 4])
    for e, (hdr, values) in got.items():
        np.testing.assert_array_equal(hdr, w.hdr[e % SLOTS])
        assert same_bits(values, w.values[e % SLOTS]), e
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_configured_in_the_middle_of_an_event(nx, ny, lateral):
    """3. 80 steps without the observer end inside event 3: that event keeps t0 = -1 and its sums are the restatement's from step 80 on."""
    ref = reference(nx, ny, lateral)
    k0 = 80
    assert ref.rows[k0 - 1, 0] == 3 == ref.rows[k0, 0]
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.run_steps(k0)
    ctx.events_configure(NAMES, KINDS, SLOTS)
    ctx.run_steps(NSTEPS - k0)
    want = ref.feed(HostEvents(KINDS, ref.n, SLOTS, running=3, drained=2), k0, NSTEPS)
    assert want.hdr[3, 0] == 3 and want.hdr[3, 2] == -1 and want.hdr[4, 2] > 0 and (want.hdr[1] == -1).all()
    assert_state(ctx, want, f"{nx} x {ny} lateral={lateral} configured at step {k0}")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_slot_and_two_events_in_one_call(nx, ny, lateral):
    """4. n_slots = 1, 50 steps: event 1 is intact and bit-equal, event 2 stores nothing, the lost flag is set, and the host package's
    read-out raises with the remedy."""
    from roger_amd import events

    ref = reference(nx, ny, lateral)
    assert set(ref.rows[:50, 0]) == {0, 1, 2}
    ctx, _ = configured(nx, ny, lateral, 1)
    ctx.run_steps(50)
    want = ref.feed(HostEvents(KINDS, ref.n, 1), 0, 50)
    assert want.lost and want.hdr[0, 0] == 1
    assert_state(ctx, want, f"{nx} x {ny} lateral={lateral} one slot")
    w = whole(ref)
    hdr, values, _ = ctx.events_read()
    np.testing.assert_array_equal(hdr[0], w.hdr[1])
    assert same_bits(values[0], w.values[1])
    ev = events.Events()
    ev._on, ev.n_slots = True, 1
    with pytest.raises(RuntimeError, match=r"raise state\.events\.n_slots \(more slots\), or call run_device\(\) in shorter pieces"):
        events.drain(types.SimpleNamespace(events=ev, backend_context=ctx))
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_entry_points(path, lateral):
    """5. rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step at 257 x 1: the restatement of the context's own planes and
    scalars after every step (items are planes rh_after_timestep does not assign)."""
    from test_hip_points import host_hooks

    names, kinds = ("q_ss", "aet", "S_rz", "S_rz"), (SUM, PEAK, FIRST, LAST)
    ctx, forcing = make_ctx(257, 1, lateral)
    ctx.events_configure(names, kinds, 4)
    h = HostEvents(kinds, ctx.n, 4)
    classes = set()
    for _ in range(70):
        monthly = host_hooks(ctx, forcing)
        if path == "routines":
            ctx.call("rh_adaptive_dt")
            if monthly:
                ctx.call("rh_params_surface")
            ctx.call("rh_step_core")
            ctx.call("rh_after_timestep")
        else:
            ctx.step(monthly)
        s = ctx.get_scalars()
        h.add(s.event_id[1], s.time - s.dt_secs, s.time, s.dt, [ctx.download(v) for v in names])
        if s.event_id[1] > 0:
            classes.add(int(s.dt_secs))
    assert classes == {600, 3600} and (h.hdr[1:4, 0] == (1, 2, 3)).all() and np.any(h.values[:, 0] != 0)
    assert_state(ctx, h, f"{path} lateral={lateral}")
    ctx.close()


@pytest.mark.parametrize("front", ["one_launch", "old_front"])
@pytest.mark.parametrize("nx,ny", [(4, 3), (40, 25)])
def test_per_cell_forcing(nx, ny, front, monkeypatch):
    """6. The Eberbaechle weights tiled over the grid, behind the one-launch front and behind the predicate-kernel front: fifteen events
    in 400 steps, the ids and step lengths from the golden run's scalars."""
    import per_cell_observers as P
    from golden_util import load_case
    from test_hip_per_cell_observers import FRONTS, default_env

    case = "svat_eberbaechle_weights"
    default_env(monkeypatch)
    rec, n = P.reference(case, nx, ny), P.prefix_steps(case)
    if front != "one_launch":
        for k, v in FRONTS[front][0].items():
            monkeypatch.setenv(k, v)
    scal = load_case(case)[0]["scal"][:n]
    assert (scal[:, :3].astype(np.int64) == rec.hdr).all()
    e, dt = scal[:, 9].astype(np.int64), scal[:, 7]
    names, kinds = ("prec", "q_ss", "aet", "S_rz", "theta"), (SUM, SUM, PEAK, FIRST, LAST)
    h = HostEvents(kinds, nx * ny, 16)
    for k in range(n):
        t1, dts = int(rec.hdr[k, 1]), int(rec.hdr[k, 2])
        h.add(e[k], t1 - dts, t1, dt[k], [rec.planes[v][k] for v in names])
    assert len(set(e[e > 0])) == 15 and not h.lost and np.any(h.values[:, 1] != 0)
    ctx = P.make_ctx(case, nx, ny)
    ctx.events_configure(names, kinds, 16)
    ctx.run_steps(n)
    assert ctx.sparse_steps() > 0
    assert_state(ctx, h, f"{case} {nx} x {ny} {front}")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES[2:])
def test_one_rank_communicator(nx, ny, lateral):
    """7. rh_run_steps_dist with a one-rank RCCL communicator (more than one rank: tests/test_hip_ranks_observers.py)."""
    from roger_amd import _native as native

    ref = reference(nx, ny, lateral)
    ctx, _ = configured(nx, ny, lateral)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.run_steps_dist(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_state(ctx, whole(ref), f"rh_run_steps_dist, one rank, {nx} x {ny} lateral={lateral}")
    ctx.close()


def test_routed_steps(monkeypatch):
    """8. The routed step on the smallest routing golden (4 x 6): rh_step_routed step by step against the restatement of the context's
    own planes and scalars after every step, then the device-driven routed steps of rh_run_steps (and RH_ROUTED_BY_ROUTINE=1) against
    that state.  140 steps: event 1 (120 steps of ten minutes), four hourly steps and a daily one outside, the beginning of event 2."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    names, kinds, nsteps = ("prec", "q_sur_out", "aet", "S", "q_ss", "z0"), (SUM, SUM, PEAK, FIRST, SUM, LAST), 140
    ctx = routed_ctx(native, g, names_all)
    ctx.events_configure(names, kinds, 4)
    h = HostEvents(kinds, ctx.n, 4)
    drv = H.HipForcingDriver(ctx, forcing)
    outside = set()
    for _ in range(nsteps):
        ctx.step_routed(drv.before_step())
        s = ctx.get_scalars()
        h.add(s.event_id[1], s.time - s.dt_secs, s.time, s.dt, [ctx.download(v) for v in names])
        if s.event_id[1] == 0:
            outside.add(int(s.dt_secs))
    assert (h.hdr[1:3, 0] == (1, 2)).all() and h.hdr[1, 4] == 120 and outside == {3600, 86400} and not h.lost
    assert all(np.any(h.values[:, j] != 0) for j in range(len(names))), "a routed item never held a value"
    assert_state(ctx, h, "rh_step_routed")
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.events_configure(names, kinds, 4)
        ctx.run_steps(nsteps)
        assert_state(ctx, h, f"rh_run_steps on a routing context, by_routine={by_routine}")
        ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """End to end: a RogerSetup script with the reference's hook bodies and `state.events` writes the same `.events.nc` on the device
    rounds (one round holds the whole run: sixteen slots) as the same script stepped routine by routine with ONE slot (read out when an
    event ends)."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    items = [("prec", "sum"), ("q_ss", "sum"), ("q_sur", "peak"), ("theta_rz", "first"), ("S_rz", "last")]
    keys = ["event_id", "event_start", "event_end", "event_steps", "event_steps_10min", "event_steps_hourly"] + [f"{v}_{k}" for v, k in items]
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, 6, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path, n_slots=16 if mode == "device" else 1):
            state.events.items = items
            state.events.n_slots = n_slots
            state.events.base_output_path = str(path)

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        model.run()
        f = netcdf_file(str(path / "GoldenSVAT.events.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in keys}
        model.state.backend_context.close()
    d = out["device"]
    for k, a in d.items():
        b = out["routine"][k]
        assert (same_bits(a, b) if a.dtype.kind == "f" else (a.shape == b.shape and np.array_equal(a, b))), k
    assert len(d["event_id"]) >= 3 and (np.diff(d["event_id"]) == 1).all() and (d["event_start"] > 0).all()
    assert (d["event_steps"] >= d["event_steps_10min"] + d["event_steps_hourly"]).all() and d["event_steps_10min"].any()
    assert np.any(d["prec_sum"] != 0) and np.any(d["q_sur_peak"] != 0) and d["prec_sum"].shape == (len(d["event_id"]), 4, 4)


def test_refusals_and_release():
    """RH_ERR_ARG with the offending value in the text, RH_ERR_STATE before the configuration and after the release."""
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    floats = float_planes(ctx)
    with pytest.raises(NativeError, match=r"rh_events_headers failed \(-3\)"):
        ctx.events_read()
    for kw, text in ((dict(names=(ints[0],), kinds=(SUM,)), f"plane {ints[0]} is int32"), (dict(names=floats[:17], kinds=(SUM,) * 17), "n_items = 17"),
                     (dict(names=("q_ss",), kinds=(4,)), "kind 4 of item 0"), (dict(names=("q_ss",), kinds=(SUM,), n_slots=0), "n_slots = 0"),
                     (dict(names=("q_ss",), kinds=(SUM,), n_slots=65537), "n_slots = 65537")):
        with pytest.raises(NativeError, match=r"rh_events_configure failed \(-1\)") as err:
            ctx.events_configure(**kw)
        assert text in str(err.value), (text, str(err.value))
    ctx.events_configure(floats[:16], (LAST,) * 16, 3)
    hdr, values, lost = ctx.events_read(slots=range(3))
    assert (hdr == -1).all() and not lost and all(v.shape == (16, 6) and not v.any() for v in values.values())
    ctx.run_steps(12)
    assert ctx.events_read()[0][1, 0] == 1
    ctx.events_configure(())
    ctx.run_steps(2)
    with pytest.raises(NativeError, match=r"rh_events_lost failed \(-3\)|rh_events_headers failed \(-3\)"):
        ctx.events_read()
    ctx.close()
