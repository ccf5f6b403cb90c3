"""GPU: the grid split along x AND y (num_proc = (px, py)) with the routing's halo as a one-cell frame -- west / east columns, south /
north rows, corners -- exchanged with up to eight neighbour ranks (rh_comm_set_grid, route_exchange).  As in
tests/test_hip_loopback_ranks.py the ranks are threads of a child process on one GPU, joined by the loopback communicator
(tests/loopback_nccl.cpp through RH_RCCL_LIB), which checks peers, counts and order of every message; the blocks must equal the single
domain bit for bit and the reference's golden runs.  What this does not show: the speed of the exchange over real RCCL between GPUs."""
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def loopback(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is needed to build the loopback communicator")
    so = tmp_path_factory.mktemp("loopback") / "libloopback_nccl.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(HERE, "loopback_nccl.cpp"), "-o", str(so)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return str(so)


def _child(loopback, scenario):
    env = dict(os.environ, RH_RCCL_LIB=loopback)
    r = subprocess.run([sys.executable, os.path.join(HERE, "grid_ranks_child.py"), scenario], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{scenario}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    print(r.stdout.strip())
    return r.stdout


def test_routed_steps_on_process_grids(loopback):
    """oned_routing on (2, 2) (diagonal flow across the corner), (1, 2), (2, 3); oned_routing_combo on (1, 2), (1, 4); the hillslope
    tutorial (1 x 20, draining along +y) on (1, 2), (1, 4): bits of the single domain, the golden run, the exact number of messages, and
    blocks without a communicator that do not reproduce it."""
    out = _child(loopback, "routing")
    assert out.count("== single domain") == 7 and out.count("without a communicator differs") == 3
    assert "oned_routing_tutorial: grid (1, 4) == single domain == golden" in out and "oned_routing: grid (2, 2) == single domain == golden" in out


def test_grid_n_by_1_is_the_default(loopback):
    out = _child(loopback, "unchanged")
    assert "grid (2, 1) set explicitly == default" in out and "grid (4, 1) set explicitly == default" in out


def test_routing_entry_points_on_a_2x2_grid(loopback):
    assert "grid (2, 2) == single domain" in _child(loopback, "routing_by_routine")


def test_run_steps_dist_on_a_2x2_grid(loopback):
    assert "grid (2, 2) == golden" in _child(loopback, "allreduce")


def test_comm_set_grid_errors(loopback):
    assert "errors:" in _child(loopback, "errors")
