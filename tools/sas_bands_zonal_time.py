#!/usr/bin/env python3
"""What the transport bands per zone (rh_sas_bands_configure_zonal; the kernels of roger_amd/csrc/rh_sas_bands_zonal.h) cost on a CLOSING
day, against the plain configuration (rh_sas_bands_configure; k_sas_bands_hist / _pick, whose code objects are the parent's).

BEHIND THE DAY'S KERNEL (`run`).  Milliseconds ADDED per day where it counts: rh_sas_run_days over 14 days at 10^5 columns x 1000 ages
(oxygen-18, deterministic solver, 6 sub-steps), eight BULK items, three probabilities, no weights, every day its own window (14 closing
days); every figure a process of its own, the minimum of three runs after a warm-up run: (n) nothing configured, (p) the plain
configuration (13 launches a day), (z4) / (z64) / (z1024) that many equal zones, zone = i % Z (2 launches a day), (z90) one zone holding 90 %
of the columns and 63 zones sharing the rest: ONE workgroup per item walks the large zone -- the load-balance note as a number.  The
transport kernel streams the state in front of every band launch: cold cache.

ALONE (`alone`).  The STAND-ALONE time of a closing day's band launches at 10^5 and 10^6 columns, eight BULK items, no weights:
rh_sas_bands_record on a context that holds uploaded values (ages = 2, no day kernel), R days enqueued back to back and one
synchronisation at the end, plain and with 4, 64 and 1024 equal zones; with a weight plane where the bound of 65536 columns per zone
allows it.  The same planes are swept again and again: served from the last-level cache, not from HBM.

OFF cost (`off`).  `python bench.py --model sas --steps 8 --warmup 2` (no bands configured), ms per day: the parent's library twice (its own
run-to-run spread is the margin) and this tree's once.  Needs ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so.

    python3 tools/sas_bands_zonal_time.py [run] [alone] [off]        (default: all; `off` is skipped without ROGER_HIP_PARENT)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sas_bands_time import PROBS, RUN_AGES, RUN_DAYS, RUN_ITEMS, RUN_N, RUN_SUBSTEPS, VALUES, off_cost  # noqa: E402

R, REPEATS = 20, 5
RUN_VARIANTS = [("n", "(n) nothing configured", None), ("p", "(p) plain configuration, 13 launches a closing day", 0),
                ("z4", "(z4) 4 equal zones, 2 launches", 4), ("z64", "(z64) 64 equal zones", 64), ("z1024", "(z1024) 1024 equal zones", 1024),
                ("z90", "(z90) 64 zones, zone 0 holds 90 % of the columns", 64)]


def zone_map(variant, n):
    import numpy as np

    nz = {v: z for v, _, z in RUN_VARIANTS}[variant]
    i = np.arange(n)
    if variant == "z90":
        return np.where(i % 10 != 9, 0, 1 + (i // 10) % (nz - 1)).astype(np.int32), nz
    return (i % nz).astype(np.int32), nz


def run_child(variant):
    """ms per day of rh_sas_run_days behind the real day kernel: the minimum of three runs after a warm-up run."""
    import numpy as np

    from roger_amd import sas as rsas

    daily = rsas.synthetic_daily_inputs(RUN_N, RUN_DAYS, seed=42)
    ctx = rsas.create_sas(RUN_N, RUN_AGES, RUN_SUBSTEPS, 90.0, 260.0, daily=daily)
    windows = (np.arange(RUN_DAYS),) * 2
    kw = {}
    if variant.startswith("z"):
        zone, nz = zone_map(variant, RUN_N)
        kw = dict(zones=zone, n_zones=nz)
    best = None
    for k in range(4):
        if variant != "n":
            ctx.bands_configure(RUN_ITEMS, PROBS, windows, **kw)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.run_days(0, RUN_DAYS)
        ctx.sync()
        ms = (time.perf_counter() - t0) / RUN_DAYS * 1e3
        if k:
            best = ms if best is None else min(best, ms)
    if variant != "n":
        rows, hdr, _, closed, days = ctx.bands_read()
        assert closed.all() and days == RUN_DAYS and hdr[..., 0].any()
        if kw:
            assert hdr[..., 0].sum(axis=2).max() <= RUN_N and rows.shape[2] == kw["n_zones"]
    ctx.close()
    print(json.dumps(best))


def behind_the_day():
    got = {}
    for v, _, _ in RUN_VARIANTS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v], check=True, capture_output=True, text=True, timeout=280).stdout
        got[v] = float(json.loads(out.strip().splitlines()[-1]))
    lines = [f"    rh_sas_run_days over {RUN_DAYS} closing days, {RUN_N} columns x {RUN_AGES} ages, {RUN_SUBSTEPS} sub-steps, 8 BULK items, ms per day "
             "(minimum of 3 runs, a process each):"]
    for v, text, _ in RUN_VARIANTS:
        more = "" if v == "n" else f"   ({got[v] - got['n']:+.4f} ms per day against (n)" + ("" if v == "p" else f", {got[v] - got['p']:+.4f} against (p)") + ")"
        lines.append(f"    {text}: {got[v]:.4f}{more}")
    return lines


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
        items = [(v, "q_ss", "bulk") for v in VALUES]
        windows = (np.arange(R * (REPEATS + 1)),) * 2
        for nz in (0, 4, 64, 1024):
            for w in (None, weights):
                if w is not None and nz and (n + nz - 1) // nz > 65536:
                    lines.append(f"    {n:>8d} columns, {nz:4d} zones, weights   : refused by the bound (a weighted zone holds at most 65536 columns)")
                    continue
                kw = dict(zones=(np.arange(n) % nz).astype(np.int32), n_zones=nz) if nz else {}
                ctx.bands_configure(items, PROBS, windows, None, w, **kw)
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
                assert ctx.bands_read()[3].all()
                what = f"{nz:4d} zones" if nz else "plain     "
                lines.append(f"    {n:>8d} columns, {what}, {'weights' if w is not None else 'no weights':10s}: {statistics.median(ms):8.4f} ms per closing day "
                             f"(median of {REPEATS} x {R} days; {min(ms):.4f} ... {max(ms):.4f}), cache-resident, back to back")
        ctx.bands_configure([])
        ctx.close()
    return lines


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        run_child(sys.argv[2])
        sys.exit(0)
    what = sys.argv[1:] or ["run", "alone", "off"]
    print("transport bands per zone (rh_sas_bands_configure_zonal), measured once on one MI355X", flush=True)
    if "run" in what:
        print("\n".join(behind_the_day()), flush=True)
    if "alone" in what:
        print("\n".join(alone()), flush=True)
    if "off" in what:
        print("\n".join(off_cost()), flush=True)
