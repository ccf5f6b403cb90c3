"""CPU: the host restatement of the output accumulators (tests/diag_reference.py) against the CPU double's own accumulators
(tests/oracle_context.py), step by step over the combo forcing -- two implementations of one contract (include/roger_hip.h, the
accumulator section), neither of which imports the other.  The GPU tests (tests/test_hip_diag_kernel.py) hold the device kernel
against the same restatement; what they lean on -- all three step classes, a slot reused after the index wrapped, a sub-daily
interval that is never started because a longer step covers it -- is asserted here on the reference alone."""
import numpy as np
import pytest

from diag_reference import HostAccumulator

RATE = ("prec", "aet", "q_ss", "inf_mat_rz", "S_fp_rz")
COLLECT = ("S_rz", "theta", "swe")
NDAYS = 8
CASES = [(86400, 3), (3600, 5), (600, 7)]


def oracle_svat(nx, ny, seed):
    """roger_amd.svat.create_svat on the double: parameters -> derived parameters -> initial conditions."""
    import oracle_context as OC
    from roger_amd import lookuptables as lut
    from roger_amd.svat import BENCHMARK_PARAMS, hetero_params

    ctx = OC.OracleContext(nx, ny)
    n = ctx.n
    p = dict(BENCHMARK_PARAMS)
    p.update(hetero_params(n, seed=seed))
    ctx.set_luts(lut.ARR_ILU, lut.ARR_GC, lut.ARR_GCM, lut.ARR_RDLU)
    full = lambda v, dtype: np.full(n, v, dtype=dtype) if np.ndim(v) == 0 else np.asarray(v, dtype=dtype).reshape(n)  # noqa: E731
    for k, v in p.items():
        if k not in ("theta_rz", "theta_ss"):
            ctx.upload(k, full(v, ctx.dtype_of(k)))
    for entry in ("rh_topo", "rh_params_surface", "rh_params_soil"):
        ctx.call(entry)
    for k in ("theta_rz", "theta_ss"):
        ctx.upload(k, full(p[k], np.float64))
        ctx.upload(k + "_m1", full(p[k], np.float64))
    ctx.call("rh_initial_conditions")
    return ctx


def assert_conditions(ref, interval):
    """What the comparisons lean on, from the reference's own step log."""
    assert ref.step_classes() == {600, 3600, 86400}, ref.step_classes()
    assert ref.slots_reused(), "no slot was reused after the index wrapped"
    if interval != 86400:
        assert ref.intervals_never_started(), "every interval was started: no longer step covered one"


@pytest.mark.parametrize("interval,n_slots", CASES)
def test_reference_equals_the_double_step_by_step(oracle, interval, n_slots):
    from roger_amd.forcing import combo_forcing

    ctx = oracle_svat(4, 4, seed=5)
    ctx.set_forcing_series(combo_forcing(ndays=NDAYS + 1))
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=n_slots)
    ctx.diag_set_interval(interval)
    ref = HostAccumulator(RATE, COLLECT, n_slots, ctx.n, interval=interval)
    d = ctx._diag
    steps = 0
    while ctx.get_scalars().time < NDAYS * 86400:
        ctx.run_steps(1)
        s = ctx.get_scalars()
        slot = ref.add(s.time, s.dt_secs, {v: ctx.download(v) for v in RATE + COLLECT})
        steps += 1
        assert s.sanity_ok == 1
        for v in RATE + COLLECT:
            np.testing.assert_array_equal(d["data"][v], ref.data[v], err_msg=f"step {steps} slot {slot} {v}")
        np.testing.assert_array_equal(d["steps"], ref.steps, err_msg=f"step {steps}")
        np.testing.assert_array_equal(d["t0"], ref.t0, err_msg=f"step {steps}")
        np.testing.assert_array_equal(d["t1"], ref.t1, err_msg=f"step {steps}")
        assert ctx.diag_steps(slot) == ref.reported_steps(slot) >= 1
        assert ctx.diag_slot_times(slot) == (int(ref.t0[slot]), int(ref.t1[slot]))
    assert ctx.get_scalars().time == NDAYS * 86400 and steps == len(ref.log)
    assert_conditions(ref, interval)
    assert any(np.any(ref.data[v] != 0) for v in ("q_ss", "aet", "swe")), "nothing to accumulate"


def test_a_slot_first_touched_inside_its_interval_counts_its_steps(oracle):
    """Configured mid-day: the slot reports the steps accumulated (1 after one step), keeps t_start = -1, and the double agrees."""
    from roger_amd.forcing import combo_forcing

    ctx = oracle_svat(3, 2, seed=5)
    ctx.set_forcing_series(combo_forcing(ndays=NDAYS + 1))
    ctx.run_steps(30)
    s = ctx.get_scalars()
    assert s.time % 86400 != 0
    ctx.diag_configure(rate=RATE, collect=COLLECT, n_slots=3)
    ref = HostAccumulator(RATE, COLLECT, 3, ctx.n)
    day = s.time // 86400
    k = 0
    while True:
        ctx.run_steps(1)
        s = ctx.get_scalars()
        if (s.time - s.dt_secs) // 86400 != day:
            break
        slot = ref.add(s.time, s.dt_secs, {v: ctx.download(v) for v in RATE + COLLECT})
        k += 1
        assert ctx.diag_steps(slot) == ref.reported_steps(slot) == k
        assert ctx.diag_slot_times(slot) == (-1, s.time)
        for v in RATE:
            np.testing.assert_array_equal(ctx.diag_download(v, slot), ref.data[v][slot])
    assert k >= 2
