#!/usr/bin/env python3
"""What the transport zonal totals (rh_sas_zonal_*, roger_amd/csrc/rh_sas_zonal.h) cost per day beside the one-mask recorder they
generalise: rh_sas_run_days over 8 days at 10^5 columns x 1000 ages (oxygen-18, deterministic solver, the benchmark's exponents,
6 sub-steps, age statistics, distributions kept) with the items C_iso_q_ss by q_ss, tt_q_ss by q_ss, sa_s -- two age arrays of 0.8 GB
read per day -- on ONE context whose recorders are switched between

    (a) none
    (b) transport totals with one mask that holds every column (a mask array, not None): the reference point, the same rows read
    (c) zonal totals with 1, 16 and 256 block zones (contiguous, equal), and with a 16-zone interleaved map (zone = column mod 16:
        every tile holds every zone, 16 slots per tile instead of 1 or 2)

The variants are timed in alternating order, each after a warm-up run of its own, with a synchronise around rh_sas_run_days; medians
and the spread (min ... max) of the repeats are printed, and what each recorder adds to (a).

    python3 tools/sas_zonal_time.py [repeats] [--out FILE]"""
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, AGES, SUBSTEPS, DAYS = 100_000, 1000, 6, 8
ITEMS = [("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s"]


def variants():
    c = np.arange(N)
    block = lambda z: (c * z // N).astype(np.int32)       # noqa: E731
    return [("(a) no recorder", None),
            ("(b) transport totals, one mask", ("totals", c >= 0)),
            ("(c) zonal, 1 block zone", ("zonal", block(1), 1)),
            ("(c) zonal, 16 block zones", ("zonal", block(16), 16)),
            ("(c) zonal, 256 block zones", ("zonal", block(256), 256)),
            ("(c) zonal, 16 zones interleaved", ("zonal", (c % 16).astype(np.int32), 16))]


def configure(ctx, what):
    ctx.totals_configure([])
    ctx.zonal_configure([])
    if what is None:
        return
    if what[0] == "totals":
        ctx.totals_configure(ITEMS, what[1], capacity=2 * DAYS)
    else:
        ctx.zonal_configure(ITEMS, what[1], what[2], capacity=2 * DAYS)


def slots(zone):
    return sum(np.unique(zone[b:b + 256]).size for b in range(0, N, 256))


def measure(repeats):
    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(N, DAYS, seed=42)
    ctx = rsas.create_sas(N, AGES, SUBSTEPS, 90.0, 260.0, daily=daily, age_statistics=True, keep_distributions=True)
    todo = variants()
    times = {name: [] for name, _ in todo}
    for r in range(repeats):
        for name, what in (todo if r % 2 == 0 else todo[::-1]):
            configure(ctx, what)
            ctx.run_days(0, DAYS)   # warm-up: first launches, clocks
            ctx.sync()
            t0 = time.perf_counter()
            ctx.run_days(0, DAYS)
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / DAYS * 1e3)
    ctx.close()
    return todo, times


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    repeats = int(args[0]) if args else 7
    todo, times = measure(repeats)
    base = statistics.median(times[todo[0][0]])
    lines = [f"{N} columns x {AGES} ages, {SUBSTEPS} sub-steps, rh_sas_run_days over {DAYS} days, one context, items {ITEMS}",
             f"ms per day: median of {repeats} (min ... max), and the median's difference from (a)"]
    for name, what in todo:
        v = times[name]
        extra = f"   {slots(what[1])} slots" if what and what[0] == "zonal" else ""
        lines.append(f"    {name:34s} {statistics.median(v):8.3f} ({min(v):.3f} ... {max(v):.3f})   {statistics.median(v) - base:+.3f}{extra}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
