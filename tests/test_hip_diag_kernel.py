"""GPU: the output accumulator kernel (k_diag, roger_amd/csrc/rh_control.h) against its host restatement (tests/diag_reference.py),
bit for bit.  Every output file comes from this kernel: it reads planes through the tiled arena addressing, writes a linear
(slot, variable, cell) buffer and is launched with the fused step's grid.  Both sides add the same float64 values in the same order,
so the tolerance is zero -- a tolerance would hide an addressing error of a small flux.

Grids: 40 x 25 (three full 256-column tiles and a ragged fourth, last wavefront of 40 lanes), 257 x 1 (one tile plus one column) and
3 x 2; intervals of a day, an hour and ten minutes with 3 / 5 / 7 resident slots, so that slots wrap and sub-daily intervals are
skipped by longer steps (asserted on the device's own step log, as tests/test_diag_reference.py asserts it on the CPU).

The CPU double over the same 8 days of the combo forcing (4 x 4 and 3 x 2 columns): 150 steps (4 daily, 86 hourly, 60 ten-minute);
every slot reused after wrapping; intervals never started: 0 (daily), 92 (hourly), 1002 (ten-minute).  The step-by-step test prints
the same figures of the device's own step log for every parametrisation (pytest -s)."""
import copy
import functools

import numpy as np
import pytest

from diag_reference import HostAccumulator

pytestmark = pytest.mark.gpu

RATE = ("prec", "aet", "q_ss", "inf_mat_rz", "S_fp_rz")     # four pure outputs (the KEEP variant stores them) and one state plane
COLLECT = ("S_rz", "theta", "swe")
NDAYS = 8
GRIDS = [(40, 25), (257, 1), (3, 2)]
INTERVALS = [(86400, 3), (3600, 5), (600, 7)]
MARKS = (1, 3, 40, 110, 130)     # steps whose reference state the run_steps test compares with (pieces of 1, 2, 37, the rest; the limit)


def make_ctx(nx, ny, lateral):
    """As test_hip_params.test_many_wavefronts_with_a_ragged_last_one: heterogeneous columns, the combo forcing resident."""
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    n = nx * ny
    p = hetero_params(n, seed=5)
    if lateral:
        p.update(slope=0.05, slope_per=5, dmph=50.0)
        p["z_soil"] = np.maximum(p["z_soil"], 800.0)
    forcing = combo_forcing(ndays=NDAYS + 4)
    ctx = create_svat(nx, ny, params=p, lateral=lateral)
    ctx.set_forcing_series(forcing)
    return ctx, forcing


def one_step(ctx, drv):
    """One fused step with the hooks on the host; returns the scalars after it."""
    ctx.step(drv.before_step())
    s = ctx.get_scalars()
    assert s.sanity_ok == 1
    return s


def feed(ref, ctx, s, names=None):
    planes = {v: ctx.download(v) for v in (names or ref.rate + ref.collect)}
    return ref.add(s.time, s.dt_secs, planes), planes


def assert_slot(ctx, ref, slot, what):
    for v in ref.rate + ref.collect:
        np.testing.assert_array_equal(ctx.diag_download(v, slot), ref.data[v][slot], err_msg=f"{what}: {v} slot {slot}")
    assert ctx.diag_steps(slot) == ref.reported_steps(slot), f"{what}: steps of slot {slot}"
    assert ctx.diag_slot_times(slot) == (int(ref.t0[slot]), int(ref.t1[slot])), f"{what}: times of slot {slot}"


def assert_all_slots(ctx, ref, what):
    for slot in range(ref.n_slots):
        assert_slot(ctx, ref, slot, what)


@functools.lru_cache(maxsize=None)
def stepwise(nx, ny, lateral, interval, n_slots):
    """NDAYS days, one step at a time, every step compared; returns (reference, {step: copy of the reference after it})."""
    import hip_util as H

    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=n_slots)
    ctx.diag_set_interval(interval)
    drv = H.HipForcingDriver(ctx, forcing)
    ref = HostAccumulator(RATE, COLLECT, n_slots, ctx.n, interval=interval)
    assert_all_slots(ctx, ref, "before the first step")   # zeros and (-1, -1, -1)
    marks, step, nonzero = {}, 0, set()
    while True:
        s = one_step(ctx, drv)
        step += 1
        slot, planes = feed(ref, ctx, s)
        nonzero |= {v for v, a in planes.items() if np.any(a != 0)}
        what = f"{nx} x {ny} lateral={lateral} interval={interval} step {step}"
        assert_slot(ctx, ref, slot, what)
        if step % 25 == 0:
            assert_all_slots(ctx, ref, what)   # an untouched slot keeps its bits: no write into another slot or variable row
        if step in MARKS:
            marks[step] = copy.deepcopy(ref)
        if s.time >= NDAYS * 86400:
            break
    assert_all_slots(ctx, ref, f"{nx} x {ny} lateral={lateral} interval={interval} at the end")
    ctx.close()
    print(f"k_diag stepwise {nx}x{ny} lateral={lateral} interval={interval} slots={n_slots}: {step} steps, classes "
          f"{ {c: sum(1 for e in ref.log if e[1] == c) for c in sorted(ref.step_classes())} }, slots reused {sorted(ref.slots_reused())}, "
          f"intervals never started {len(ref.intervals_never_started())}")
    assert nonzero == set(RATE + COLLECT), f"variables that never held a value: {set(RATE + COLLECT) - nonzero}"
    return ref, marks


@pytest.mark.parametrize("interval,n_slots", INTERVALS)
@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_every_step_equals_the_host_accumulator(nx, ny, lateral, interval, n_slots):
    """(a) One step at a time: the touched slot after every step, every slot of every variable every 25 steps and at the end."""
    ref, _ = stepwise(nx, ny, lateral, interval, n_slots)
    assert ref.step_classes() == {600, 3600, 86400}, ref.step_classes()
    assert ref.slots_reused(), "no slot was reused after the index wrapped"
    if interval != 86400:
        assert ref.intervals_never_started(), "every interval was started: no longer step covered one"


@pytest.mark.parametrize("interval,n_slots", INTERVALS[:2])
@pytest.mark.parametrize("lateral", [False, True])
def test_calls_of_several_steps_equal_single_steps(lateral, interval, n_slots):
    """(b) rh_run_steps in pieces of 1, 2, 37 and 70 steps (the sparse KEEP kernels, lazy rotation, the tail's control part): at every
    piece end all slots and the bookkeeping equal the reference fed by single steps.  Then a time limit inside the run with 30
    launches too many: the halted launches add nothing, and neither does a further call."""
    nx, ny = GRIDS[0]
    ref, marks = stepwise(nx, ny, lateral, interval, n_slots)
    assert len(ref.log) > MARKS[-1] and set(marks) == set(MARKS)
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=n_slots)
    ctx.diag_set_interval(interval)
    done = 0
    for stop in MARKS[:-1]:
        n = stop - done
        ctx.run_steps(n)
        done = stop
        if n >= 3:
            assert ctx.sparse_steps() >= n - 2, (n, ctx.sparse_steps())   # the KEEP variant ran: four accumulated planes are pure outputs
        s = ctx.get_scalars()
        t_start, dt = marks[stop].log[-1][:2]
        assert (s.itt, s.time, s.dt_secs) == (stop, t_start + dt, dt)
        assert_all_slots(ctx, marks[stop], f"lateral={lateral} interval={interval}: run_steps up to step {stop}")
    assert any(marks[m].log[-1][0] % 86400 != 0 and (marks[m].log[-1][0] + marks[m].log[-1][1]) % 86400 != 0 for m in MARKS), "no piece ends inside a day"
    limit = MARKS[-1]
    t_limit = marks[limit].log[-1][0] + marks[limit].log[-1][1]
    ctx.set_time_limit(t_limit)
    ctx.run_steps(limit - done + 30)
    s = ctx.get_scalars()
    assert (s.itt, s.time) == (limit, t_limit)
    assert_all_slots(ctx, marks[limit], f"lateral={lateral} interval={interval}: at the time limit")
    ctx.run_steps(5)
    assert ctx.get_scalars().itt == limit
    assert_all_slots(ctx, marks[limit], f"lateral={lateral} interval={interval}: after a call beyond the limit")
    ctx.close()


def test_accumulated_m1_planes_switch_the_lazy_rotation_off():
    """(c) An accumulated X_m1 plane: the pending tau -> taum1 copies are materialised and the fused kernel stores those planes again."""
    import hip_util as H

    nx, ny = GRIDS[0]
    with_m1 = dict(rate=["q_ss"], collect=["S_rz_m1", "swe_m1"])
    without = dict(rate=["q_ss"], collect=["S_rz", "swe"])
    ctx, forcing = make_ctx(nx, ny, False)
    single, _ = make_ctx(nx, ny, False)
    drv = H.HipForcingDriver(single, forcing)
    ctx.run_steps(40)
    assert ctx.step_mode()[0], "no accumulator: the rotation stays pending"
    for _ in range(40):
        s = one_step(single, drv)
    assert s.time % 86400 != 0 and s.time == ctx.get_scalars().time
    for cfg, lazy in ((with_m1, False), (without, True)):
        ctx.diag_configure(n_slots=3, **cfg)
        ref = HostAccumulator(cfg["rate"], cfg["collect"], 3, ctx.n)
        ctx.run_steps(30)
        assert ctx.step_mode()[0] == lazy, cfg
        for _ in range(30):
            s = one_step(single, drv)
            feed(ref, single, s)
        assert s.time == ctx.get_scalars().time
        assert_all_slots(ctx, ref, f"collect={cfg['collect']}")
        assert np.any(ref.data[cfg["collect"][0]] != 0)
    ctx.close()
    single.close()


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS[:2])
def test_one_rank_communicator(nx, ny, lateral):
    """(c2) rh_run_steps_dist with a one-rank RCCL communicator: every slot equals the reference fed by single steps (more than one
    rank: tests/test_hip_ranks_observers.py)."""
    from roger_amd import _native as native

    interval, n_slots = INTERVALS[0]
    ref, _ = stepwise(nx, ny, lateral, interval, n_slots)
    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=n_slots)
    ctx.diag_set_interval(interval)
    ctx.run_steps_dist(len(ref.log))
    assert ctx.sparse_steps() > 0
    assert_all_slots(ctx, ref, f"rh_run_steps_dist, one rank, {nx} x {ny} lateral={lateral}")
    ctx.close()


def test_routed_steps(monkeypatch):
    """(c3) The routed step on the smallest routing golden (4 x 6), hourly slots: rh_step_routed step by step against the host
    accumulator fed the context's own planes after every step, then the device-driven routed steps of rh_run_steps (and
    RH_ROUTED_BY_ROUTINE=1) against those slots.  140 steps: 120 of ten minutes, four hourly, a daily one, fifteen of ten minutes."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    rate, collect, nsteps, interval, n_slots = ("prec", "q_sur_out", "aet", "q_ss"), ("S", "z0"), 140, 3600, 5
    ctx = routed_ctx(native, g, names_all)
    ctx.diag_configure(rate=rate, collect=collect, n_slots=n_slots)
    ctx.diag_set_interval(interval)
    ref = HostAccumulator(rate, collect, n_slots, ctx.n, interval=interval)
    drv = H.HipForcingDriver(ctx, forcing)
    for k in range(nsteps):
        ctx.step_routed(drv.before_step())
        s = ctx.get_scalars()
        slot, _ = feed(ref, ctx, s)     # (sanity_ok is not asserted: the reference's own water balance check fails on routed runs)
        assert_slot(ctx, ref, slot, f"rh_step_routed step {k + 1}")
    assert ref.step_classes() == {600, 3600, 86400} and ref.slots_reused() and ref.intervals_never_started() and all(np.any(ref.data[v] != 0) for v in rate + collect)
    assert_all_slots(ctx, ref, "rh_step_routed")
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.diag_configure(rate=rate, collect=collect, n_slots=n_slots)
        ctx.diag_set_interval(interval)
        ctx.run_steps(nsteps)
        assert_all_slots(ctx, ref, f"rh_run_steps on a routing context, by_routine={by_routine}")
        ctx.close()


def same_interval_steps(ctx, drv, ref, iv):
    """Steps until the next one would begin in another interval; yields (k, slot, planes of the step, scalars)."""
    s = ctx.get_scalars()
    k, interval = 0, s.time // iv
    while ctx.get_scalars().time // iv == interval:
        s = one_step(ctx, drv)
        k += 1
        slot, planes = feed(ref, ctx, s)
        yield k, slot, planes, s


@pytest.mark.parametrize("nx,ny", GRIDS[1:])
def test_a_slot_first_touched_inside_its_interval_counts_its_steps(nx, ny):
    """(d) rh_diag_configure and rh_diag_set_interval leave (-1, -1, -1) in every slot.  A slot whose first accumulated step does not
    begin on an interval boundary reports the steps that were accumulated -- 1 after one step, the divisor of the `average`
    diagnostic -- and keeps t_start = -1.  (The kernel counted from the -1: 0 after one step, one short ever after.)"""
    import hip_util as H

    ctx, forcing = make_ctx(nx, ny, False)
    drv = H.HipForcingDriver(ctx, forcing)
    for _ in range(30):
        s = one_step(ctx, drv)
    assert s.time % 86400 != 0, "the model time is not inside a day"
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=3)
    ref = HostAccumulator(RATE, COLLECT, 3, ctx.n)
    for k, slot, planes, s in same_interval_steps(ctx, drv, ref, 86400):
        assert ctx.diag_steps(slot) == k, f"{k} steps accumulated since the configuration inside the day"
        assert ctx.diag_slot_times(slot) == (-1, s.time)
        if k == 1:
            for v in RATE + COLLECT:
                np.testing.assert_array_equal(ctx.diag_download(v, slot), planes[v], err_msg=v)
        assert_slot(ctx, ref, slot, f"step {k} after the configuration")
    assert k >= 3
    # the same after rh_diag_set_interval on the configured context, inside an hour: ten-minute steps of the heavy rain
    for _ in range(200):
        s = one_step(ctx, drv)
        if s.dt_secs == 600 and s.time % 3600 == 600:
            break
    assert s.dt_secs == 600 and s.time % 3600 == 600, "no ten-minute step found that leaves the time inside an hour"
    ctx.diag_set_interval(3600)
    ref = HostAccumulator(RATE, COLLECT, 3, ctx.n, interval=3600)
    for v in RATE + COLLECT:   # (rh_diag_set_interval keeps the values: the reference continues from them)
        for slot in range(3):
            ref.data[v][slot] = ctx.diag_download(v, slot)
    for slot in range(3):
        assert ctx.diag_steps(slot) == 0 and ctx.diag_slot_times(slot) == (-1, -1)
    for k, slot, planes, s in same_interval_steps(ctx, drv, ref, 3600):
        assert ctx.diag_steps(slot) == k, f"{k} steps accumulated since rh_diag_set_interval inside the hour"
        assert ctx.diag_slot_times(slot) == (-1, s.time)
        assert_slot(ctx, ref, slot, f"step {k} after rh_diag_set_interval")
    assert k == 5
    ctx.close()


def test_configuration_limits_and_the_restart_entry_points():
    """(e) 32 variables and no more, float64 planes that the context holds, at least one slot: every refusal is RH_ERR_ARG and leaves the
    previous configuration working.  One resident slot keeps the last day.  rh_diag_upload / rh_diag_set_slot_state (the restart):
    what was put back is read back, and the accumulation goes on from it as the reference does from the same state."""
    import hip_util as H
    from roger_amd._native import NativeError

    ctx, forcing = make_ctx(3, 2, False)
    drv = H.HipForcingDriver(ctx, forcing)
    floats = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if not is_int]
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, is_int in ctx.planes[ctx.planes_held:] if not is_int]
    assert len(floats) >= 33 and ints and not_held
    ctx.diag_configure(rate=floats[:20], collect=floats[20:32], n_slots=2)      # 32 are accepted
    ctx.diag_configure(rate=["prec", "q_ss"], collect=["S_rz"], n_slots=1)
    ref = HostAccumulator(["prec", "q_ss"], ["S_rz"], 1, ctx.n)
    refused = (dict(rate=floats[:20], collect=floats[20:33], n_slots=2), dict(rate=floats[:33], collect=[], n_slots=2),
               dict(rate=["prec", ints[0]], collect=[], n_slots=2), dict(rate=[], collect=[not_held[0]], n_slots=2),
               dict(rate=["aet"], collect=["theta"], n_slots=0), dict(rate=["aet"], collect=["theta"], n_slots=-1))
    s = ctx.get_scalars()
    while s.time < 3 * 86400:    # one resident slot over three days: the third day's sums stay
        if refused and s.itt >= 2:
            with pytest.raises(NativeError, match=r"rh_diag_configure failed \(-1\)"):
                ctx.diag_configure(**refused[0])
            refused = refused[1:]
        s = one_step(ctx, drv)
        slot, _ = feed(ref, ctx, s)
        assert_slot(ctx, ref, slot, f"one slot, step {s.itt}")
    assert not refused and s.time == 3 * 86400 and int(ref.t0[0]) == 2 * 86400 and ref.reported_steps(0) > 1
    # the restart's entry points, on a slot inside its interval (day 3 has begun) and on one with t_start = -1
    ctx.diag_configure(rate=["prec", "q_ss"], collect=["S_rz"], n_slots=4)
    ref = HostAccumulator(["prec", "q_ss"], ["S_rz"], 4, ctx.n)
    for k in range(3):
        s = one_step(ctx, drv)
        feed(ref, ctx, s)
    assert s.time % 86400 != 0
    now = int(s.time // 86400) % 4
    rng = np.random.default_rng(7)
    states = {now: (7, -1, int(s.time)), (now + 1) % 4: (3, 5 * 86400, 5 * 86400 + 1800)}   # (steps, t_start, t_end)
    for slot, (steps, t0, t1) in states.items():
        for v in ref.rate + ref.collect:
            ref.data[v][slot] = rng.uniform(-1.0, 1.0, ctx.n) * 10.0 ** rng.integers(-12, 3, ctx.n)
            ctx.diag_upload(v, slot, ref.data[v][slot])
        ref.steps[slot], ref.t0[slot], ref.t1[slot] = steps, t0, t1
        ctx.diag_set_slot_state(slot, steps, t0, t1)
    assert_all_slots(ctx, ref, "read back")
    while s.time < 4 * 86400 + 7200:   # on through the rest of the day and into the next slot, which is overwritten
        s = one_step(ctx, drv)
        slot, _ = feed(ref, ctx, s)
        assert_slot(ctx, ref, slot, f"after the upload, step {s.itt}")
    assert_all_slots(ctx, ref, "after the upload, at the end")
    assert ref.reported_steps(now) > 8 and int(ref.t0[now]) == -1 and int(ref.t0[(now + 1) % 4]) == 4 * 86400
    ctx.close()
