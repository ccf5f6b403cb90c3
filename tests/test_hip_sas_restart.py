"""Checkpoint / restart of the offline transport model on the device (roger_amd/restart.py, transport branch): a run interrupted with a
restart file -- half-way, or right after warmup() and its rescale_SA -- and continued in a fresh model equals the uninterrupted run bit for
bit, for the three solvers and for oxygen-18 and bromide; a restart write at 10^5 columns x 1000 ages stays within one age array plus one
block of host memory (the age-resolved storages are streamed in column blocks, never held on the host in full)."""
import json
import os
import subprocess
import sys

import pytest

import sas_binding as sb
from test_host_package_sas_restart import assert_records_continue, assert_same_state, golden_model, on_disk, split_run  # noqa: F401

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case,warmup", [("sas_stats_a30", 0), ("sas_euler_a40", 0), ("sas_rk4_a40", 0), ("sas_bromide_a40", 0),
                                         ("sas_bromide_euler_a30", 0), ("sas_bromide_rk4_a30", 1)])
def test_interrupted_run_equals_uninterrupted_on_the_device(on_disk, tmp_path, case, warmup):
    ndays = sb.SasGolden(case).ndays
    a, c, _ = split_run(tmp_path, lambda: golden_model(case, warmup_days=ndays if warmup else 0)[1], ndays, warmup)
    assert_same_state(a, c)
    assert_records_continue(tmp_path, a.state.settings.identifier)


@pytest.mark.parametrize("case", ["sas_warmup_a30", "sas_bromide_warmup_a30"])
def test_restart_right_after_the_warmup_on_the_device(on_disk, tmp_path, case):
    ndays = sb.SasGolden(case).ndays
    a, c, _ = split_run(tmp_path, lambda: golden_model(case, warmup_days=ndays)[1], ndays, 1, at_warmup=True)
    assert_same_state(a, c)
    assert_records_continue(tmp_path, a.state.settings.identifier)


_CHILD = r"""
import json, resource, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from roger_amd import runtime_settings as rs
rs.update(diskless_mode=False)
from roger_amd import h5lite, restart
from roger_amd.state import RogerState

st = RogerState()
with st.settings.unlock():
    st.settings.update(nx=1000, ny=100, ages=1000, nages=1001, nitt=2, enable_offline_transport=True, enable_oxygen18=True,
                       sas_solver="deterministic")
st.initialize_variables()
sas = st.sas_context
n, ages = sas.n, sas.ages
step = restart._block_cells(sas)
for i, k in enumerate(restart.AGE_STATE):   # a start: column c of array i holds (c % 97 + 1 + i / 8) / ages in every age class
    for first in range(0, n, step):
        cnt = min(step, n - first)
        sas.upload_cells(k, first, np.repeat(((np.arange(first, first + cnt) % 97 + 1 + i / 8.0) / ages)[:, None], ages, axis=1))
sas.sync()
# one day step, as a run leaves the state: every variable the step writes -- the six storages and the tt / mtt / TT distributions among
# them -- is newer on the device than its (still unmapped) host mirror
from roger_amd.core import transport
from roger_amd.sas import BENCHMARK_SAS_K
vs = st.variables
with vs.unlock():
    vs.dt_secs = 86400
    for f, k in BENCHMARK_SAS_K.items():
        p = np.zeros((1004, 104, 8))
        p[..., 0], p[..., 1] = 6, k
        setattr(vs, "sas_params_" + f, p)
        setattr(vs, f, np.full((1004, 104), 0.5))
transport.calculate_storage_selection(st)
sas.sync()
aged = [k for k, v in st.var_meta.items() if v.sas is not None and ("ages" in v.dims or "nages" in v.dims)]   # held by the context
assert all(vs._is_device_newer(k) for k in restart.AGE_STATE)

def rss():
    with open("/proc/self/status") as f:
        return next(int(l.split()[1]) for l in f if l.startswith("VmRSS:")) * 1024

import threading, time
top, done = [0], threading.Event()

def sample():   # VmRSS every millisecond during the write: its peak even where an earlier one masks it in ru_maxrss
    while not done.is_set():
        top[0] = max(top[0], rss())
        time.sleep(0.001)

rss0, peak0 = rss(), resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
t = threading.Thread(target=sample)
t.start()
try:
    restart.write_restart(st, filename=sys.argv[2])
finally:
    done.set()
    t.join()
peak1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
untouched = all(vs._is_device_newer(k) for k in aged)   # no age-resolved host mirror was filled by the write
small, f = h5lite.open_blocks(sys.argv[2], streamed=restart.AGE_STATE)
with f:
    ok = all(f.shape("hip_core", k) == (1000, 100, ages) and   # the file holds what the device holds after the step
             np.array_equal(f.get("hip_core", k, c * ages, ages), sas.download_cells(k, c, 1)[0], equal_nan=True)
             for k in restart.AGE_STATE for c in (0, step - 1, step, n - 1))
print(json.dumps(dict(untouched=untouched, n_aged=len(aged), rss0=rss0, peak0=peak0, peak1=peak1, sampled=max(top[0], rss()), array=n * ages * 8, block=step * ages * 8, ok=ok)))
"""


def test_restart_write_streams_the_age_arrays(tmp_path):
    """Peak RSS of a restart write at 10^5 columns x 1000 ages (six 800 MB age arrays) after a day step -- every age-resolved variable
    newer on the device, as a run leaves them -- in a fresh process, by resource.getrusage and by sampling VmRSS during the write:the write may add at most one age array plus one block to what the process held before it --
    holding the six arrays would add 4.8 GB."""
    out = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(tmp_path / "big.h5")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r["ok"] and r["untouched"] and r["n_aged"] >= 21
    limit = r["array"] + r["block"]
    assert r["sampled"] - r["rss0"] <= limit, r
    # ru_maxrss: the write did not raise the process's peak above what one array plus one block over the start allows (where the
    # process peaked higher before the write -- the HIP runtime's own start-up -- that peak stands and is all ru_maxrss can say)
    assert r["peak1"] <= max(r["peak0"], r["rss0"] + limit), r
