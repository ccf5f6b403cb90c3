#!/usr/bin/env python3
"""What the transport recorder (rh_sas_points_*, k_sas_points) costs per day: rh_sas_run_days over 8 days at 10^5 columns x 1000 ages
(oxygen-18, deterministic solver, the benchmark's exponents, 6 sub-steps, age statistics) on a context without points and on one
with 16 cells x {6 scalars, tt_q_ss, TT_q_ss, sa_s} -- 16 x 3007 float64 = 376 KB gathered per day.  Both contexts keep the
distributions (the points context needs them for tt_q_ss / TT_q_ss / sa_s), so the recorder is the only difference.  The two are
stepped alternately in one process; medians and the spread (min ... max) of the repeats are printed.

    python3 tools/sas_points_time.py [repeats]               this tree's library, without and with points
    ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so ...     the no-points run on the parent's library as well, in a child process
                                                             (RH_OLD_VARIANT: an older ABI is accepted)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, AGES, SUBSTEPS, DAYS = 100_000, 1000, 6, 8
SCALARS = ["C_iso_q_ss", "C_iso_transp", "C_iso_rz", "C_iso_ss", "tt50_q_ss", "rt50_s"]
VECTORS = ["tt_q_ss", "TT_q_ss", "sa_s"]


def measure(repeats, with_points=(False, True)):
    """ms per day, `repeats` times: [(one figure per context)] on contexts of one process stepped alternately."""
    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(N, DAYS, seed=42)
    ctxs = []
    for points in with_points:
        ctx = rsas.create_sas(N, AGES, SUBSTEPS, 90.0, 260.0, daily=daily, age_statistics=True, keep_distributions=True)
        if points:
            ctx.points_configure([(k * (N - 1)) // 15 for k in range(16)], SCALARS + VECTORS, capacity=64)
        ctx.run_days(0, DAYS)   # warm-up: first launches, clocks
        ctx.sync()
        ctxs.append(ctx)
    out = []
    for _ in range(repeats):
        row = []
        for ctx in ctxs:
            t0 = time.perf_counter()
            ctx.run_days(0, DAYS)
            ctx.sync()
            row.append((time.perf_counter() - t0) / DAYS * 1e3)
        out.append(row)
    for ctx, points in zip(ctxs, with_points):
        if points:
            assert ctx.points_count() == DAYS * (repeats + 1)
        ctx.close()
    return out


def summary(values):
    return f"{statistics.median(values):.3f} ms per day (median of {len(values)}; {min(values):.3f} ... {max(values):.3f})"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:      # the baseline on another library: the ms per day without points
        print(json.dumps([r[0] for r in measure(int(sys.argv[2]), with_points=(False,))]))
        sys.exit(0)
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rows = measure(repeats)
    base, pts = [r[0] for r in rows], [r[1] for r in rows]
    print(f"{N} columns x {AGES} ages, {SUBSTEPS} sub-steps, rh_sas_run_days over {DAYS} days, keep_distributions on both contexts\n"
          f"    this tree, no points:   {summary(base)}\n"
          f"    this tree, with points: {summary(pts)}   (16 cells x {{6 scalars, tt_q_ss, TT_q_ss, sa_s}})\n"
          f"    difference of the medians: {1e3 * (statistics.median(pts) - statistics.median(base)):+.1f} us per day; "
          f"pairs {[f'{a:.3f}/{b:.3f}' for a, b in rows]}", flush=True)
    parent = os.environ.get("ROGER_HIP_PARENT")
    if parent:
        env = dict(os.environ, ROGER_HIP_LIB=parent, RH_OLD_VARIANT="1")
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(repeats)], env=env, check=True, capture_output=True,
                             text=True).stdout.strip().splitlines()[-1]
        print(f"    parent library, no points: {summary(json.loads(got))}", flush=True)
