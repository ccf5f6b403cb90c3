#!/usr/bin/env python3
"""What the transport scores (rh_sas_scores_*, k_sas_scores in roger_amd/csrc/rh_sas_scores.h) cost per day: rh_sas_run_days over 14
days at 10^5 columns x 1000 ages (oxygen-18, deterministic solver, the benchmark's exponents, 6 sub-steps), for

    (a)  the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset), nothing configured,
    (b)  this tree's library with nothing configured,
    (c)  this tree's library with four BULK items (C_iso_q_ss, C_q_ss, C_iso_q_rz, C_iso_transp by their fluxes) scored against
         weekly windows [0, 6], [7, 13]: every day is inside a window, two of the fourteen close one.

Every figure is one child process (create, a warm-up run of the 14 days, three timed runs with a synchronise around rh_sas_run_days,
the fastest taken); the variants alternate `repeats` times, and the median and the range over the repeats are printed.  Pass
condition: the median of (b) lies inside (a)'s min ... max range of the same run -- an unconfigured context enqueues what it enqueued
before.  (c) has no cap: it is reported next to the bytes rh_sas_scores.h says the kernel moves.

    python3 tools/sas_scores_time.py [repeats]        # writes profiles/sas_scores_cost.txt as well"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, AGES, SUBSTEPS, DAYS = 100_000, 1000, 6, 14
ITEMS = [("C_iso_q_ss", "q_ss", "bulk"), ("C_q_ss", "q_ss", "bulk"), ("C_iso_q_rz", "q_rz", "bulk"), ("C_iso_transp", "transp", "bulk")]
WINDOWS = ([0, 7], [6, 13])
VARIANTS = [("a", "(a) parent commit, nothing configured"), ("b", "(b) this commit, nothing configured"),
            ("c", "(c) this commit, scores: four BULK items, weekly windows")]
# rh_sas_scores.h: a BULK item moves 48 B per column on a non-closing day (32 B on a window's first) and 112 B more on a closing one
BYTES_PER_DAY = len(ITEMS) * N * (2 * 32 + 12 * 48 + 2 * 112) / DAYS


def child(variant):
    import numpy as np

    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(N, DAYS, seed=42)
    ctx = rsas.create_sas(N, AGES, SUBSTEPS, 90.0, 260.0, daily=daily)
    best = None
    for k in range(4):   # the first run is the warm-up
        if variant == "c":
            ctx.scores_configure(ITEMS, np.full((len(ITEMS), 1, 2), -8.0), WINDOWS)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.run_days(0, DAYS)
        ctx.sync()
        ms = (time.perf_counter() - t0) / DAYS * 1e3
        if k:
            best = ms if best is None else min(best, ms)
    if variant == "c":
        moments, closed, days = ctx.scores_read()
        assert list(closed) == [1, 1] and days == DAYS and moments[:, 2].any()
    ctx.close()
    print(json.dumps(best))


def run_child(variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant], env=env, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(sys.argv[2])
        sys.exit(0)
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    lines = [f"python3 tools/sas_scores_time.py {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
                                                              "   (ROGER_HIP_PARENT unset: (a) NOT measured)")]
    print(lines[0], flush=True)
    got = {key: [] for key, _ in VARIANTS}
    for _ in range(repeats):
        for key, _ in VARIANTS:
            if key == "a":
                if parent:
                    got[key].append(run_child("b", parent))
            else:
                got[key].append(run_child(key))
            print(key, got[key][-1:], flush=True)
    lines.append(f"{N} columns x {AGES} ages, {SUBSTEPS} sub-steps, deterministic solver, rh_sas_run_days over {DAYS} days, ms per day, "
                 f"median [min ... max] of {repeats} alternating repeats")
    for key, label in VARIANTS:
        if got[key]:
            v = got[key]
            lines.append(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
    med = {key: statistics.median(v) for key, v in got.items() if v}
    lines.append(f"    (c) - (b): {med['c'] - med['b']:+.4f} ms per day; by rh_sas_scores.h the kernel moves {BYTES_PER_DAY / 1e6:.1f} MB per day "
                 f"on average ({len(ITEMS)} BULK items x {N} columns: 48 B on a non-closing day, 32 B on a first, 112 B more on a closing one)")
    if "a" in med:
        ok = min(got["a"]) <= med["b"] <= max(got["a"])
        lines.append(f"    (b) - (a): {med['b'] - med['a']:+.4f} ms; median of (b) inside (a)'s range: {'PASS' if ok else 'FAIL'}")
    for line in lines[1:]:
        print(line, flush=True)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "sas_scores_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
