#!/usr/bin/env python3
"""What the totals recorder (rh_totals_*, k_totals_tiles + k_totals_finish) costs per step: 200 fused steps (rh_run_steps) of the
benchmark's columns at 1000 x 1000 and at 80 x 53, for

    (a) the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset),
    (b) this tree's library without totals,
    (c) this tree's library with totals of eight variables over every column.

Every figure is one child process (create, 120 warm-up steps, three timed calls of `steps` steps, the fastest taken); the three
variants alternate a, b, c, a, b, c, ... `repeats` times, and the median and the range over the repeats are printed.

    python3 tools/totals_time.py [steps [repeats]]"""
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


def child(nx, ny, steps, with_totals):
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(nx, ny)
    ctx.set_forcing_series(combo_forcing(ndays=400))
    if with_totals:
        ctx.totals_configure(NAMES, None, capacity=4096)
    ctx.run_steps(120)
    ctx.sync()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    if with_totals:
        assert ctx.totals_count() == (120 + 3 * steps, nx * ny)
    ctx.close()
    print(json.dumps(best))


def run_child(nx, ny, steps, with_totals, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), str(int(with_totals))],
                         env=env, check=True, capture_output=True, text=True).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        nx, ny, steps, with_totals = (int(v) for v in sys.argv[2:6])
        child(nx, ny, steps, bool(with_totals))
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    print(f"python3 tools/totals_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else ""))
    for nx, ny in GRIDS:
        got = {"a": [], "b": [], "c": []}
        for _ in range(repeats):
            if parent:
                got["a"].append(run_child(nx, ny, steps, False, parent))
            got["b"].append(run_child(nx, ny, steps, False))
            got["c"].append(run_child(nx, ny, steps, True))
        print(f"{nx} x {ny}, {steps} fused steps per call, ms per step, median [min ... max] of {repeats} alternating repeats", flush=True)
        for key, label in (("a", "(a) parent commit, no observers"), ("b", "(b) this commit, no totals"),
                           ("c", f"(c) this commit, totals of {len(NAMES)} variables over every column")):
            if got[key]:
                v = got[key]
                print(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
        mb, mc = statistics.median(got["b"]), statistics.median(got["c"])
        print(f"    (c) - (b): {1e3 * (mc - mb):+.1f} us per step" + (f"; (b) - (a): {1e3 * (mb - statistics.median(got['a'])):+.1f} us per step"
                                                                       if got["a"] else ""), flush=True)
