#!/usr/bin/env python3
"""What the transport bands (rh_sas_bands_*; the kernels of roger_amd/csrc/rh_sas_bands.h) cost.

ALONE (`alone`).  The STAND-ALONE time of a day's band launches, at 10^5 and 10^6 columns, with 1 and 8 BULK items, 3 probabilities, with
and without a weight plane: rh_sas_bands_record on a context that holds uploaded values (ages = 2, no day kernel), R days enqueued back
to back and one synchronisation at the end.  Closing days: every day is its own window (k_sas_bands_day and the 12 launches of the
selection).  Accumulating days: one window that never closes (k_sas_bands_day alone).  What this is NOT: the same planes (at most about
200 MB) are swept again and again, so they are served from the 256 MiB last-level cache, not from HBM, nothing runs in front of the
launches, and a timed window is 0.1 ... 15 ms of host wall clock.  The bytes-per-second figure beside each time is therefore a
cache-resident, back-to-back enqueue rate; it is printed to show which cases are bound by launches and which by data, not as an HBM figure.

BEHIND THE DAY'S KERNEL (`run`).  Milliseconds ADDED per day where it counts: rh_sas_run_days over 14 days at 10^5 columns x 1000 ages
(oxygen-18, deterministic solver, 6 sub-steps), every figure a process of its own, the minimum of three runs after a warm-up run:
(n) nothing configured, (c) eight BULK items, every day its own window (14 closing days), (a) eight BULK items, one window over the 14
days (13 accumulating days and one closing day).  The transport kernel streams the state in front of every band launch: cold cache.

OFF cost (`off`).  `python bench.py --model sas --steps 8 --warmup 2` (no bands configured), ms per day: the parent's library twice (its own
run-to-run spread is the margin) and this tree's once.  Needs ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so.

    python3 tools/sas_bands_time.py [alone] [run] [off]        (default: all; `off` is skipped without ROGER_HIP_PARENT)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VALUES = ["C_iso_q_ss", "C_q_ss", "C_iso_transp", "C_iso_rz", "C_rz", "C_iso_ss", "C_ss", "C_s"]
PROBS = (0.05, 0.5, 0.95)
R, REPEATS = 20, 5
# rh_sas_bands.h: a BULK item moves 48 B per column on a non-closing day (32 B on a window's first, which every day of the daily band is),
# 8 B more for the key on a closing day; the selection six passes x (8 B key + 2 B weight) per item and column
DAY_FIRST, DAY_NEXT, KEY, PASSES, KEY_READ, WEIGHT_READ = 32, 48, 8, 6, 8, 2


def alone():
    import numpy as np

    from roger_amd._native import SasContext

    lines = []
    for n in (100_000, 1_000_000):
        rng = np.random.default_rng(n)
        ctx = SasContext(n, 2, forcing_days=1)
        ctx.upload("q_ss", rng.random((1, n)) + 0.1)
        for v in VALUES:
            ctx.upload(v, -12.0 + 9.0 * rng.random(n))
        weights = rng.integers(1, 65536, size=n).astype(np.uint16)
        for n_items in (1, 8):
            items = [(v, "q_ss", "bulk") for v in VALUES[:n_items]]
            for w in (None, weights):
                figures = {}
                for what, windows in (("closing", (np.arange(R * (REPEATS + 1)),) * 2), ("accumulating", (np.array([0]), np.array([10 ** 9])))):
                    ctx.bands_configure(items, PROBS, windows, None, w)
                    for _ in range(R):       # warm-up: first launches, clocks
                        ctx.bands_record(0)
                    ctx.sync()
                    ms = []
                    for _ in range(REPEATS):
                        t0 = time.perf_counter()
                        for _ in range(R):
                            ctx.bands_record(0)
                        ctx.sync()
                        ms.append((time.perf_counter() - t0) / R * 1e3)
                    figures[what] = ms
                    if what == "closing":
                        assert ctx.bands_read()[3].all()
                sel = PASSES * (KEY_READ + (WEIGHT_READ if w is not None else 0)) * n_items * n
                moved = {"closing": (DAY_FIRST + KEY) * n_items * n + sel, "accumulating": DAY_NEXT * n_items * n}
                for what, ms in figures.items():
                    med = statistics.median(ms)
                    lines.append(f"    {n:>8d} columns, {n_items} item(s), {'weights' if w is not None else 'no weights':10s} {what:12s} day: "
                                 f"{med:8.4f} ms (median of {REPEATS} x {R} days; {min(ms):.4f} ... {max(ms):.4f}); the rule moves {moved[what] / 1e6:7.1f} MB: "
                                 f"{moved[what] / (med * 1e-3) / 1e12:5.2f} TB/s cache-resident, back to back")
        ctx.bands_configure([])
        ctx.close()
    return lines


RUN_N, RUN_AGES, RUN_SUBSTEPS, RUN_DAYS = 100_000, 1000, 6, 14
RUN_ITEMS = [("C_iso_q_ss", "q_ss", "bulk"), ("C_q_ss", "q_ss", "bulk"), ("C_iso_q_rz", "q_rz", "bulk"), ("C_q_rz", "q_rz", "bulk"),
             ("C_iso_transp", "transp", "bulk"), ("C_transp", "transp", "bulk"), ("C_iso_rz", "q_ss", "bulk"), ("C_rz", "q_ss", "bulk")]
RUN_VARIANTS = [("n", "(n) nothing configured"), ("c", "(c) 8 BULK items, every day its own window: 14 closing days"),
                ("a", "(a) 8 BULK items, one window of 14 days: 13 accumulating days, 1 closing")]


def run_child(variant):
    """ms per day of rh_sas_run_days behind the real day kernel: the minimum of three runs after a warm-up run."""
    import numpy as np

    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(RUN_N, RUN_DAYS, seed=42)
    ctx = rsas.create_sas(RUN_N, RUN_AGES, RUN_SUBSTEPS, 90.0, 260.0, daily=daily)
    windows = {"c": (np.arange(RUN_DAYS),) * 2, "a": (np.array([0]), np.array([RUN_DAYS - 1]))}.get(variant)
    best = None
    for k in range(4):
        if windows is not None:
            ctx.bands_configure(RUN_ITEMS, PROBS, windows)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.run_days(0, RUN_DAYS)
        ctx.sync()
        ms = (time.perf_counter() - t0) / RUN_DAYS * 1e3
        if k:
            best = ms if best is None else min(best, ms)
    if windows is not None:
        rows, hdr, _, closed, days = ctx.bands_read()
        assert closed.all() and days == RUN_DAYS and hdr[:, :, 0].any()
    ctx.close()
    print(json.dumps(best))


def behind_the_day():
    got = {}
    for v, _ in RUN_VARIANTS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v], check=True, capture_output=True, text=True, timeout=280).stdout
        got[v] = float(json.loads(out.strip().splitlines()[-1]))
    lines = [f"    rh_sas_run_days over {RUN_DAYS} days, {RUN_N} columns x {RUN_AGES} ages, {RUN_SUBSTEPS} sub-steps, ms per day (minimum of 3 runs, a process each):"]
    lines += [f"    {text}: {got[v]:.4f}" + ("" if v == "n" else f"   ({got[v] - got['n']:+.4f} ms per day against (n))") for v, text in RUN_VARIANTS]
    return lines


def bench_ms_per_day(lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--model", "sas", "--gpus", "1", "--steps", "8", "--warmup", "2"], env=env,
                         check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
    rec = json.loads(out)
    for key in ("ms_per_step", "ms_per_day", "step_ms"):
        if key in rec:
            return float(rec[key]), key
    return float(rec["wall_s"]) / 8 * 1e3, "wall_s / 8"


def off_cost():
    parent = os.environ.get("ROGER_HIP_PARENT")
    if not parent:
        return ["    off cost: ROGER_HIP_PARENT is not set, skipped"]
    a, key = bench_ms_per_day(parent)
    b, _ = bench_ms_per_day(parent)
    c, _ = bench_ms_per_day()
    return [f"    bench.py --model sas --steps 8 --warmup 2, no bands configured, {key} in ms: parent library {a:.4f} and {b:.4f} "
            f"(its own spread {abs(a - b):.4f}), this tree {c:.4f} ({c - min(a, b):+.4f} against the parent's faster run)"]


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        run_child(sys.argv[2])
        sys.exit(0)
    what = sys.argv[1:] or ["alone", "run", "off"]
    print("transport bands (rh_sas_bands_*), measured once on one MI355X", flush=True)
    if "alone" in what:
        print("\n".join(alone()), flush=True)
    if "run" in what:
        print("\n".join(behind_the_day()), flush=True)
    if "off" in what:
        print("\n".join(off_cost()), flush=True)
