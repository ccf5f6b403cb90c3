"""How a run advances: ONE decision, as plain functions over plain facts (no GPU, no torch, no I/O).  `RogerSetup._facts()` gathers
the `Facts`; `run()`, `step()`, `_run_on_device()` and `run_device()` branch on the answers and decide nothing themselves.

`hook_classes` is a zero-argument callable returning {hook: True if the device performs it}: it probes the script's hooks
(roger_amd/hooks.py) and is evaluated ONLY where the cheaper facts leave the answer open.  `RogerSetup.hook_classes()` also sets
`state._stock_set_forcing`, so whether a restart file written at midnight leaves out the day's forcing arrays depends on whether
a decision here got as far as the callable (`step_form` does not on several ranks).  Kept as it always was, on purpose: evaluating
the callable eagerly would change the restart files of multi-rank runs.
"""
from typing import NamedTuple

DEVICE_ROUNDS, LEAN_LOOP, STEP_LOOP = "device rounds", "lean host loop", "step loop"                # run(): run_loop
FUSED, BY_ROUTINE = "fused", "by routine"                                                           # step(): step_form
RUN_STEPS, RUN_STEPS_DIST, PHASED_ONE, PHASED_THREE = "run_steps", "run_steps_dist", "phased, one exchange", "phased, three phases"


class Facts(NamedTuple):
    offline_transport: bool    # settings.enable_offline_transport
    routing: bool              # settings.enable_routing_1D
    profile_mode: bool         # runtime setting: synchronise and log after every step
    restart_every_step: bool   # settings.restart_frequency > 0
    multi_rank: bool           # more than one rank
    per_cell_forcing: bool     # station weights / several stations (known once the forcing series are on the device)
    step_by_routine: bool      # RH_STEP_BY_ROUTINE: the three-call step, for A/B and for the tests of that path
    no_lean_loop: bool         # RH_NO_LEAN_LOOP: run() through step() where the lean loop would do
    has_step_scalars: bool     # the context's one-call step returns the scalars (the CPU tests' double has none)
    has_run_steps_dist: bool   # the context exchanges the summary word itself, from C (the double does not)


def step_form(f, hook_classes):
    """FUSED: set_parameters and after_timestep are the device's -- the model class's, or a script's that do the same --, one rank, no
    routing: the physics of the step is one native call.  BY_ROUTINE: adaptive time step (phased over several ranks), set_parameters,
    rh_step_core."""
    if f.multi_rank or f.routing or f.offline_transport or f.step_by_routine:
        return BY_ROUTINE
    classes = hook_classes()
    return FUSED if classes["set_parameters"] and classes["after_timestep"] else BY_ROUTINE


def device_rounds_possible(f, hook_classes):
    """Every per-step hook is the device's and nothing was asked for that needs the host after each step."""
    if f.offline_transport or f.profile_mode or f.restart_every_step or f.step_by_routine:
        return False
    return all(hook_classes().values())


def lean_loop_possible(f, hook_classes):
    """The hooks in front of the physics on the host, then the fused step as one call that also returns the scalars."""
    return (step_form(f, hook_classes) == FUSED and not (f.profile_mode or f.restart_every_step)
            and f.has_step_scalars and not f.no_lean_loop)


def run_loop(f, hook_classes):
    if device_rounds_possible(f, hook_classes):
        return DEVICE_ROUNDS
    return LEAN_LOOP if lean_loop_possible(f, hook_classes) else STEP_LOOP   # STEP_LOOP: step() after step(), as in the reference


def engine(f):
    """What run_device() advances with."""
    if not f.multi_rank:
        return RUN_STEPS
    if f.per_cell_forcing:   # every column forms its own prec / ta: both predicate words are evaluated over the columns
        return PHASED_THREE
    return RUN_STEPS_DIST if f.has_run_steps_dist else PHASED_ONE   # shared forcing: one exchange of the summary word per step


def time_limit(f):
    """Whether the rounds of _run_on_device() may be cut short by the device-side time limit: the control parts for per-cell
    forcing and for routing do not observe it, nor does the phased orchestration."""
    return not (f.per_cell_forcing or f.routing) and engine(f) in (RUN_STEPS, RUN_STEPS_DIST)
