"""The dry paths of the macropore and crack sub-step loops (rh_physics.h: h_inf_mp / h_inf_sc with DryPath<true>, taken by the LAZY
pipelines of the fused step) against the loops themselves, on the host: tools/substep_dry_check.cpp compiles rh_physics.h as host code
with the address and undefined-behaviour sanitizers and runs both on more than 10^7 states -- every input of the two stages replaced in
turn by zeros of both signs, NaN, infinities, tiny, huge and negative values at 1 / 5 / 120 sub-steps, mask on and off, one and two
wetting fronts, and 10^7 random states -- comparing every field of the column bit for bit (NaN for NaN)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dry_paths_equal_the_loops_on_ten_million_states(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "substep_dry_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "roger_amd", "csrc"),
                    os.path.join(REPO, "tools", "substep_dry_check.cpp"), "-o", str(exe), "-lm", "-pthread"], check=True)
    r = subprocess.run([str(exe), "10000000"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    states = int(re.search(r"states (\d+)", r.stdout).group(1))
    assert states >= 10_000_000
    for stage in ("macropores", "cracks"):
        dry, loops = (int(v) for v in re.search(stage + r":\s+dry path (\d+), loops (\d+)", r.stdout).groups())
        assert dry + loops == states
        assert dry > states // 10 and loops > states // 10, (stage, dry, loops)   # both paths well represented
