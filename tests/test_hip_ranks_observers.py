"""GPU: the six device observers (accumulators, points, catchment totals, zonal totals, scores, event outputs) behind the stepping of MORE
THAN ONE RANK, which is how the product runs them: rh_run_steps_dist on SVAT blocks (all-reduce -> k_ctrl on the received word -> the
fused launch with RH_TAIL_PRE | RH_TAIL_HOOKS -> the observers under `after_fused && D->skipped`), the device-driven routed steps with a
communicator (route_exchange twice per step in front of k_routed_cg<false, false> -> the observers -> k_after_timestep_oned) and
rh_step_routed's phase-1 / all-reduce / phase-2 path.  Ranks are threads of one child process joined by the loopback communicator
(tests/test_hip_loopback_ranks.py); every rank has its own grid size, and with it its own workgroup count for the events' per-workgroup
ids, the totals' tree and the points' gather.

What every rank must hold is the observers' numpy restatements applied to ITS COLUMNS of a single-domain reference without observer and
communicator, bit for bit (tests/ranks_observers.py, where the scenarios are described).  One child process per scenario."""
import os
import subprocess
import sys

import pytest

from test_hip_loopback_ranks import HERE, loopback  # noqa: F401

pytestmark = pytest.mark.gpu


def _child(loopback, scenario, **extra):  # noqa: F811
    env = dict(os.environ, RH_RCCL_LIB=loopback)
    env.pop("RH_ROUTED_BY_ROUTINE", None)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ranks_observers.py"), scenario], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{scenario}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    print(r.stdout.strip())
    return r.stdout


def test_svat_golden_all_six_on_halves_and_slabs(loopback):  # noqa: F811
    """1. svat_hetero_combo under rh_run_steps_dist: two halves, four one-column slabs, the halves with an X_m1 plane."""
    out = _child(loopback, "svat_golden")
    assert out.count("ranks == restatements of the single domain") == 3 and "4 ranks == restatements" in out


def test_svat_golden_every_observer_alone(loopback):  # noqa: F811
    """1. ... and each observer on its own on the two halves: another plane union, has_observers and KEEP bits."""
    out = _child(loopback, "svat_golden_alone")
    assert out.count("alone, two halves: 2 ranks == restatements of the single domain") == 6


def test_svat_more_than_one_workgroup_per_rank(loopback):  # noqa: F811
    """2. 40 x 25 as 275 + 725 columns and 257 x 1 as 256 + 1, SVAT with and without lateral flow."""
    out = _child(loopback, "svat_tiles")
    assert out.count("== restatements of the single domain") == 4 and "[275, 725]" in out and "[256, 1]" in out


def test_routed_steps_with_ranks(loopback):  # noqa: F811
    """3. oned_routing on two halves and on (2, 2), oned_routing_combo on (1, 2): the device-driven routed steps."""
    out = _child(loopback, "routed")
    assert out.count("ranks == restatements of the single domain") == 3 and "on (2, 2): 4 ranks" in out


def test_routed_steps_by_routine_with_ranks(loopback):  # noqa: F811
    """3. ... and the two halves through rh_step_routed (RH_ROUTED_BY_ROUTINE=1)."""
    out = _child(loopback, "routed_by_routine", RH_ROUTED_BY_ROUTINE="1")
    assert "by routine: 2 ranks == restatements of the single domain" in out
