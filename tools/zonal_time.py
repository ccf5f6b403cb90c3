#!/usr/bin/env python3
"""What the zonal totals recorder (rh_zonal_*, k_zonal_tiles + k_zonal_finish) costs per step: 200 fused steps (rh_run_steps) of the
benchmark's columns at 1000 x 1000 and at 80 x 53, for

    (a)  the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset),
    (b)  this tree's library without observers,
    (t)  this tree's library with the catchment totals (rh_totals_*) of eight variables over every column -- what one zone costs a
         user without the zonal recorder, who pays it once per zone,
    (c1) this tree's library with zonal totals of the same variables, one zone everywhere,
    (c2) ... 16 stripes along x,
    (c3) ... 256 random zone ids (a scattered map: every tile holds nearly every zone).

Every figure is one child process (create, 120 warm-up steps, three timed calls of `steps` steps, the fastest taken); the variants
alternate `repeats` times, and the median and the range over the repeats are printed.

    python3 tools/zonal_time.py [steps [repeats]]"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ["prec", "aet", "q_ss", "S_rz", "S_ss", "swe", "theta_rz", "inf_mat_rz"]   # aet, q_ss: pure outputs (the KEEP variant runs)
GRIDS = [(1000, 1000), (80, 53)]
VARIANTS = [("a", "(a)  parent commit, no observers"), ("b", "(b)  this commit, no observers"),
            ("t", "(t)  this commit, catchment totals over every column"), ("c1", "(c1) this commit, zonal totals, one zone"),
            ("c2", "(c2) this commit, zonal totals, 16 stripes along x"), ("c3", "(c3) this commit, zonal totals, 256 random zones")]


def zone_map(nx, ny, variant):
    import numpy as np

    if variant == "c1":
        return np.zeros(nx * ny, dtype=np.int32), 1
    if variant == "c2":
        return np.repeat(np.arange(nx) * 16 // nx, ny).astype(np.int32), 16
    return np.random.default_rng(256).integers(0, 256, size=nx * ny).astype(np.int32), 256


def child(nx, ny, steps, variant):
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(nx, ny)
    ctx.set_forcing_series(combo_forcing(ndays=400))
    if variant == "t":
        ctx.totals_configure(NAMES, None, capacity=4096)
    elif variant.startswith("c"):
        zone, nz = zone_map(nx, ny, variant)
        ctx.zonal_configure(NAMES, zone, nz, capacity=120 + 3 * steps)
    ctx.run_steps(120)
    ctx.sync()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    if variant == "t":
        assert ctx.totals_count() == (120 + 3 * steps, nx * ny)
    elif variant.startswith("c"):
        assert ctx.zonal_count()[0] == 120 + 3 * steps and int(ctx.zonal_count()[1].sum()) == nx * ny
    ctx.close()
    print(json.dumps(best))


def run_child(nx, ny, steps, variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), variant],
                         env=env, check=True, capture_output=True, text=True).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    print(f"python3 tools/zonal_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else ""))
    for nx, ny in GRIDS:
        got = {key: [] for key, _ in VARIANTS}
        for _ in range(repeats):
            for key, _ in VARIANTS:
                if key == "a":
                    if parent:
                        got[key].append(run_child(nx, ny, steps, "b", parent))
                else:
                    got[key].append(run_child(nx, ny, steps, key))
        print(f"{nx} x {ny}, {steps} fused steps per call, {len(NAMES)} variables, ms per step, median [min ... max] of {repeats} alternating repeats",
              flush=True)
        for key, label in VARIANTS:
            if got[key]:
                v = got[key]
                print(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
        med = {key: statistics.median(v) for key, v in got.items() if v}
        line = "    over (b), us per step: " + ", ".join(f"{key} {1e3 * (med[key] - med['b']):+.1f}" for key in ("t", "c1", "c2", "c3"))
        if "a" in med:
            line += f"; (b) - (a): {1e3 * (med['b'] - med['a']):+.1f}"
        print(line, flush=True)
