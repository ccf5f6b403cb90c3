"""GPU: zonal totals with two ranks -- two loopback ranks (tests/test_hip_loopback_ranks.py's communicator) record their halves of a domain
over the global zone list; the combined files equal the single domain's within n 2^-52 sum|t| per (row, zone, variable), the bound of
reassociating n additions (tests/test_host_package_sas_totals.py); minimum, maximum, ncells and headers exactly."""
import os
import subprocess
import sys

import pytest

from test_hip_loopback_ranks import HERE, loopback  # noqa: F401

pytestmark = pytest.mark.gpu


def test_two_ranks_combined_equal_the_single_domain(loopback, tmp_path):  # noqa: F811
    env = dict(os.environ, RH_RCCL_LIB=loopback)
    r = subprocess.run([sys.executable, os.path.join(HERE, "zonal_ranks_child.py"), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    print(r.stdout.strip())
    assert "2 ranks combined == single domain" in r.stdout
