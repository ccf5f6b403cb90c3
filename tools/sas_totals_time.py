#!/usr/bin/env python3
"""What the transport totals (rh_sas_totals_*, roger_amd/csrc/rh_sas_totals.h) cost per day: rh_sas_run_days over 8 days at 10^5
columns x 1000 ages (oxygen-18, deterministic solver, the benchmark's exponents, 6 sub-steps, age statistics) on a context without
totals and on one with the tutorial's items -- C_iso_q_ss by q_ss, tt_q_ss by q_ss, sa_s: two age arrays of 0.8 GB read per day.  Both
contexts keep the distributions, so the recorder is the only difference.  The two are stepped alternately in one process; medians and
the spread (min ... max) of the repeats -- the A/B noise -- are printed, and the bytes per second the added time amounts to.

    python3 tools/sas_totals_time.py [repeats]               this tree's library, without and with totals
    ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so ...     the no-totals run on the parent's library as well, in a child process
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
ITEMS = [("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s"]
BYTES = N * 8 * (1 + 3 + 2 * AGES)     # C_iso_q_ss; q_ss for the width-1 item, for the age item's wsum and in its level 1; the two age arrays


def measure(repeats, with_totals=(False, True)):
    """ms per day, `repeats` times: [(one figure per context)] on contexts of one process stepped alternately."""
    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(N, DAYS, seed=42)
    ctxs = []
    for totals in with_totals:
        ctx = rsas.create_sas(N, AGES, SUBSTEPS, 90.0, 260.0, daily=daily, age_statistics=True, keep_distributions=True)
        if totals:
            ctx.totals_configure(ITEMS, None, capacity=64)
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
    for ctx, totals in zip(ctxs, with_totals):
        if totals:
            assert ctx.totals_count()[0] == DAYS * (repeats + 1)
        ctx.close()
    return out


def summary(values):
    return f"{statistics.median(values):.3f} ms per day (median of {len(values)}; {min(values):.3f} ... {max(values):.3f})"


def verdict(base, par):
    """The unconfigured context against the parent: the difference of the medians beside the noise the two series show themselves
    (the larger of their min ... max spreads)."""
    diff = statistics.median(base) - statistics.median(par)
    noise = max(max(base) - min(base), max(par) - min(par))
    return (f"no totals, this tree - parent: {1e3 * diff:+.1f} us per day; noise (larger spread of the two series) {1e3 * noise:.1f} us: "
            + ("within the noise" if abs(diff) <= noise else "OUTSIDE the noise"))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:      # the baseline on another library: the ms per day without totals
        print(json.dumps([r[0] for r in measure(int(sys.argv[2]), with_totals=(False,))]))
        sys.exit(0)
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rows = measure(repeats)
    base, pts = [r[0] for r in rows], [r[1] for r in rows]
    added = statistics.median(pts) - statistics.median(base)
    print(f"{N} columns x {AGES} ages, {SUBSTEPS} sub-steps, rh_sas_run_days over {DAYS} days, keep_distributions on both contexts\n"
          f"    this tree, no totals:   {summary(base)}\n"
          f"    this tree, with totals: {summary(pts)}   ({ITEMS})\n"
          f"    difference of the medians: {1e3 * added:+.1f} us per day = {BYTES / 1e9:.2f} GB at {BYTES / max(added, 1e-9) / 1e9:.2f} TB/s; "
          f"pairs {[f'{a:.3f}/{b:.3f}' for a, b in rows]}", flush=True)
    parent = os.environ.get("ROGER_HIP_PARENT")
    if parent:
        env = dict(os.environ, ROGER_HIP_LIB=parent, RH_OLD_VARIANT="1")
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(repeats)], env=env, check=True, capture_output=True,
                             text=True).stdout.strip().splitlines()[-1]
        par = json.loads(got)
        print(f"    parent library, no totals: {summary(par)}", flush=True)
        print("    " + verdict(base, par), flush=True)
