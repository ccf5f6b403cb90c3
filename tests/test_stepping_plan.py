"""roger_amd/stepping.py against the decisions it replaced.

The five `old_*` functions below are the reference.  They are transcribed from roger_amd/roger.py as it stood before stepping.py
existed (commit 0878899: `_fused_host_step_possible`, `device_run_possible`, `_lean_host_loop_possible`, the engine branch of
`run_device` and the `limit` expression of `_run_on_device`), condition for condition and in the same order, with the settings,
the environment and the context replaced by the fact that stands for them.  The four `hasattr` probes that both `_native.Context`
and the CPU tests' double satisfy (`step`, `run_steps`, `set_time_limit`, `diag_slot_times`) are transcribed as True.  Nothing here
is derived from stepping.py.
"""
import itertools

from roger_amd import stepping
from roger_amd.stepping import Facts

HOOKS = ("read_data", "set_boundary_conditions", "set_forcing", "set_parameters", "after_timestep")
HOOK_CASES = [dict.fromkeys(HOOKS, True)] + [{**dict.fromkeys(HOOKS, True), h: False} for h in HOOKS[2:]] + [dict.fromkeys(HOOKS, False)]


class Recorder:
    def __init__(self, classes):
        self.classes, self.calls = classes, 0

    def __call__(self):
        self.calls += 1
        return self.classes


def old_fused_host_step_possible(f, hook_classes):
    if f.multi_rank or f.routing or f.offline_transport:
        return False
    if not True or f.step_by_routine:   # hasattr(ctx, "step")
        return False
    classes = hook_classes()
    return classes["set_parameters"] and classes["after_timestep"]


def old_device_run_possible(f, hook_classes):
    if f.offline_transport or f.profile_mode or f.restart_every_step:
        return False
    if not True or f.step_by_routine:   # hasattr(ctx, "run_steps")
        return False
    return all(hook_classes().values())


def old_lean_host_loop_possible(f, hook_classes):
    return (old_fused_host_step_possible(f, hook_classes) and not f.profile_mode and not f.restart_every_step
            and f.has_step_scalars and not f.no_lean_loop)


def old_run_loop(f, hook_classes):   # the if / elif / else of run()
    if old_device_run_possible(f, hook_classes):
        return "device"
    elif old_lean_host_loop_possible(f, hook_classes):
        return "lean"
    return "step"


def old_engine(f):
    if f.multi_rank and f.per_cell_forcing:
        return "three"
    elif f.multi_rank:
        if f.has_run_steps_dist:
            return "run_steps_dist"
        return "one"
    return "run_steps"


def old_limit(f):
    limit = True and not f.per_cell_forcing and not f.routing   # hasattr(ctx, "set_time_limit")
    if f.multi_rank and not f.has_run_steps_dist:
        limit = False
    return limit


LOOPS = {"device": stepping.DEVICE_ROUNDS, "lean": stepping.LEAN_LOOP, "step": stepping.STEP_LOOP}
ENGINES = {"run_steps": stepping.RUN_STEPS, "run_steps_dist": stepping.RUN_STEPS_DIST, "one": stepping.PHASED_ONE,
           "three": stepping.PHASED_THREE}


def _same(new, old, f, classes):
    """`new` and `old` give the same answer and evaluate the hook classes in the same cases."""
    n, o = Recorder(classes), Recorder(classes)
    got, want = new(f, n), old(f, o)
    assert got == want, (new.__name__, f, classes, got, want)
    assert bool(n.calls) is bool(o.calls), (new.__name__, f, classes, n.calls, o.calls)


def test_every_combination_of_facts_decides_as_before():
    assert len(set(LOOPS.values())) == 3 and len(set(ENGINES.values())) == 4 and stepping.FUSED != stepping.BY_ROUTINE
    n = 0
    for bits in itertools.product((False, True), repeat=len(Facts._fields)):
        f = Facts(*bits)
        assert stepping.engine(f) == ENGINES[old_engine(f)], f
        assert stepping.time_limit(f) is old_limit(f), f
        for classes in HOOK_CASES:
            _same(lambda f, h: stepping.step_form(f, h) == stepping.FUSED, old_fused_host_step_possible, f, classes)
            _same(stepping.device_rounds_possible, old_device_run_possible, f, classes)
            _same(stepping.lean_loop_possible, old_lean_host_loop_possible, f, classes)
            _same(stepping.run_loop, lambda f, h: LOOPS[old_run_loop(f, h)], f, classes)
            assert stepping.step_form(f, Recorder(classes)) in (stepping.FUSED, stepping.BY_ROUTINE)
            n += 1
    assert n == 2 ** 10 * 5
