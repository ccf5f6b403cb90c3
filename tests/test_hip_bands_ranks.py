"""GPU: the ensemble bands on two loopback ranks under rh_run_steps_dist, 257 x 1 as 256 + 1 columns: each rank's rows equal the
restatement over its own columns of the single-domain reference (tests/bands_ranks_child.py, one child process: the loopback
communicator is chosen when the library is loaded)."""
import os
import subprocess
import sys

import pytest

from test_hip_loopback_ranks import HERE, loopback  # noqa: F401

pytestmark = pytest.mark.gpu


def test_two_ranks_equal_their_columns_of_the_single_domain(loopback):  # noqa: F811
    """256 + 1 columns, in one call and in pieces."""
    env = dict(os.environ, RH_RCCL_LIB=loopback)
    r = subprocess.run([sys.executable, os.path.join(HERE, "bands_ranks_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    print(r.stdout.strip())
    assert r.stdout.count("[256, 1] columns == restatements of the single domain") == 1
