#!/usr/bin/env python3
"""What the transport bands by age (rh_sas_age_bands_*; the kernels of roger_amd/csrc/rh_sas_age_bands.h) cost on a CLOSING day -- every
other day enqueues nothing -- at 10^5 columns x 1000 ages, for 1 item (TT_q_ss, 1001 age classes) and 4 items (TT_q_ss, tt_q_ss, sa_s,
sa_rz: 4001 age classes), three probabilities, without weights (every column takes part) and with a weight plane on a mask of 65536
columns (the bound of a weighted configuration).

BEHIND THE DAY'S KERNEL (`run`).  Milliseconds ADDED per day where it counts: rh_sas_run_days over 14 days (oxygen-18, deterministic
solver, 6 sub-steps, keep_distributions on in every variant), every day its own window (14 closing days); every figure a process of its
own, the minimum of three runs after a warm-up run: (n) nothing configured, (a1) / (a4) 1 / 4 items, (a1w) / (a4w) the same with weights.

ALONE (`alone`).  The STAND-ALONE time of a closing day's launches: rh_sas_age_bands_record on a context that holds uploaded values (no
day kernel), R days enqueued back to back and one synchronisation at the end; 1 and 4 items, without and with weights; and the SLOPE over
the participating columns, 1 item without weights under masks of 25 000, 50 000 and 100 000 columns (one workgroup walks an age class).
Beside it THE ALTERNATIVE it replaces, timed in the same process: download the item's (n, ages + 1) array and np.partition on the host
at the three ranks.  10^6 columns (an 8 GB array per item) are not measured here.

OFF cost (`off`).  `python bench.py --model sas --steps 8 --warmup 2` (nothing configured), ms per day: the parent's library and this
tree's ALTERNATING, three runs each; the median of this tree against the parent's own range.  Needs
ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so; ROGER_HIP_OFF_FIRST=tree lets this tree's library open the alternation.

PER ZONE (`zonal`; not part of the default).  rh_sas_age_bands_configure_zonal, 1 item (TT_q_ss), no weights, every column in a zone: the
plain configuration, 1, 8, 64 and 1024 equal contiguous zones, and one map with a zone of 90 % of the columns beside 63 small ones --
stand-alone (R closing days back to back) and behind the day's kernel (14 closing days), every figure a process of its own, the minimum
of three runs after a warm-up run.  THE ALTERNATIVE, stand-alone: the plain call once per zone with mask = zones == z, the sum over the
zones of a closing day each (8 and 64 zones and the 90 % map: every zone; 1024 zones: 16 zones, times 64).  ROGER_HIP_NO_SMALL=/path/to/a/library built
with -DSAS_AGE_SHORT_ZONE=0 (tools/build_variant.py nosmall --unit rh_sas -DSAS_AGE_SHORT_ZONE=0) adds the 1024 zones with every zone
through the six passes: the price of the second path as a measured pair.

WINDOW MEANS (`window`; not part of the default).  rh_sas_age_window_bands_*, 1 item (tt_q_ss BULK by q_ss, 1000 age classes), no weights,
every column takes part.  Stand-alone (record back to back on uploaded values): an ACCUMULATING day (k_sas_age_acc on a day that is neither
a window's first nor its last; 8 B source + 16 B read + 16 B written per element, reported as bytes per second too) and a CLOSING day of
one-day windows (k_sas_age_keys_window and the selection).  Behind the day's kernel, rh_sas_run_days over 14 days: nothing configured, the
snapshot observer with 14 windows, the window means with ONE window of 14 days and with 14 windows of one day.  Every figure a process of
its own, the minimum of three runs after a warm-up run.

    python3 tools/sas_age_bands_time.py [run] [alone] [off] [zonal] [window]   (default: run alone off; `off` is skipped without ROGER_HIP_PARENT)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sas_bands_time import PROBS, RUN_AGES, RUN_DAYS, RUN_N, RUN_SUBSTEPS, bench_ms_per_day  # noqa: E402

R, REPEATS, BOUND = 5, 3, 65536
ITEMS = ["TT_q_ss", "tt_q_ss", "sa_s", "sa_rz"]
RUN_VARIANTS = [("n", "(n) nothing configured", 0, False), ("a1", "(a1) 1 item, 1001 age classes, 2 launches a closing day", 1, False),
                ("a4", "(a4) 4 items, 4001 age classes, 8 launches", 4, False), ("a1w", "(a1w) 1 item, weights on a mask of 65536 columns", 1, True),
                ("a4w", "(a4w) 4 items, weights on a mask of 65536 columns", 4, True)]


def participation(n, weighted, n_part=None):
    """(mask, weights): every column -- or the first n_part columns of a stride over the domain, with likelihoods 1 ... 65535."""
    import numpy as np

    if not weighted and n_part is None:
        return None, None
    n_part = BOUND if n_part is None else n_part
    mask = np.zeros(n, dtype=np.uint8)
    mask[np.round(np.linspace(0, n - 1, n_part)).astype(np.int64)] = 1
    assert int(mask.sum()) == n_part
    return mask, np.random.default_rng(n).integers(1, 65536, size=n).astype(np.uint16) if weighted else None


def run_child(variant):
    """ms per day of rh_sas_run_days behind the real day kernel: the minimum of three runs after a warm-up run."""
    import numpy as np

    from roger_amd import sas as rsas

    _, _, n_items, weighted = next(v for v in RUN_VARIANTS if v[0] == variant)
    daily = rsas.synthetic_daily_inputs(RUN_N, RUN_DAYS, seed=42)
    ctx = rsas.create_sas(RUN_N, RUN_AGES, RUN_SUBSTEPS, 90.0, 260.0, daily=daily, keep_distributions=True)
    windows = (np.arange(RUN_DAYS),) * 2
    mask, w = participation(RUN_N, weighted)
    best = None
    for k in range(4):
        if n_items:
            ctx.age_bands_configure(ITEMS[:n_items], PROBS, windows, mask, w)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.run_days(0, RUN_DAYS)
        ctx.sync()
        ms = (time.perf_counter() - t0) / RUN_DAYS * 1e3
        if k:
            best = ms if best is None else min(best, ms)
    if n_items:
        rows, hdr, closed, days = ctx.age_bands_read()
        assert closed.all() and days == RUN_DAYS and all(hdr[v][..., 0].any() for v in ITEMS[:n_items])
    ctx.close()
    print(json.dumps(best))


def behind_the_day():
    got = {}
    for v, _, _, _ in RUN_VARIANTS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v], check=True, capture_output=True, text=True, timeout=280).stdout
        got[v] = float(json.loads(out.strip().splitlines()[-1]))
    lines = [f"    rh_sas_run_days over {RUN_DAYS} closing days, {RUN_N} columns x {RUN_AGES} ages, {RUN_SUBSTEPS} sub-steps, keep_distributions, "
             "3 probabilities, ms per day (minimum of 3 runs, a process each):"]
    for v, text, _, _ in RUN_VARIANTS:
        lines.append(f"    {text}: {got[v]:.4f}" + ("" if v == "n" else f"   ({got[v] - got['n']:+.4f} ms per closing day against (n))"))
    return lines


def alone():
    import numpy as np

    from roger_amd._native import SasContext

    n, ages = RUN_N, RUN_AGES
    rng = np.random.default_rng(7)
    ctx = SasContext(n, ages, keep_distributions=True)
    for v in ITEMS:
        ctx.upload(v, rng.random(ctx.shape(v)))
    windows = (np.arange(R * (REPEATS + 1)),) * 2
    lines = []

    def timed(n_items, mask, w, what):
        ctx.age_bands_configure(ITEMS[:n_items], PROBS, windows, mask, w)
        for _ in range(R):       # warm-up: first launches, clocks
            ctx.age_bands_record(0)
        ctx.sync()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(R):
                ctx.age_bands_record(0)
            ctx.sync()
            ms.append((time.perf_counter() - t0) / R * 1e3)
        assert ctx.age_bands_read()[2].all()
        lines.append(f"    {what}: {statistics.median(ms):9.4f} ms per closing day (median of {REPEATS} x {R} days; {min(ms):.4f} ... {max(ms):.4f}), back to back")
        return statistics.median(ms)

    for n_items in (1, 4):
        for weighted in (False, True):
            mask, w = participation(n, weighted)
            timed(n_items, mask, w, f"{n} columns x {ages} ages, {n_items} item(s), " + (f"weights on {BOUND} columns" if weighted else f"no weights, {n} columns take part"))
    slope = {}
    for n_part in (25_000, 50_000, 100_000):
        mask, _ = participation(n, False, n_part) if n_part < n else (None, None)
        slope[n_part] = timed(1, mask, None, f"slope: 1 item, no weights, {n_part:6d} participating columns")
    lines.append(f"    slope: {(slope[100_000] - slope[25_000]) / 75.0:.4f} ms per 1000 participating columns and item of 1001 age classes (25 000 -> 100 000)")
    ctx.age_bands_configure([])
    # the alternative: the (n, ages + 1) array to the host, np.partition at the three ranks
    t0 = time.perf_counter()
    A = ctx.download("TT_q_ss")
    t1 = time.perf_counter()
    ranks = sorted({min(max(int(np.ceil(p * n)), 1), n) - 1 for p in PROBS})
    band = np.partition(A, ranks, axis=0)[ranks]
    t2 = time.perf_counter()
    assert band.shape == (len(ranks), ages + 1)
    lines.append(f"    the alternative, 1 item: download of ({n}, {ages + 1}) float64 {1e3 * (t1 - t0):.1f} ms + np.partition at {len(ranks)} ranks on the host "
                 f"{1e3 * (t2 - t1):.1f} ms = {1e3 * (t2 - t0):.1f} ms")
    lines.append("    10^6 columns: not measured")
    ctx.close()
    return lines


ZONAL_VARIANTS = [("plain", "the plain configuration (no zones)"), ("z1", "1 zone"), ("z8", "8 equal zones"), ("z64", "64 equal zones"),
                  ("z1024", "1024 equal zones (97 or 98 columns each: the one-key-per-thread kernel)"),
                  ("z90", "64 zones, one of 90 % of the columns")]


def zone_map(variant, n):
    """int32 (n,) zone indices of a variant, None for the plain configuration; contiguous zones, every column in one."""
    import numpy as np

    if variant == "plain":
        return None
    c = np.arange(n, dtype=np.int64)
    if variant == "z90":
        big = n * 9 // 10
        return np.where(c < big, 0, 1 + (c - big) * 63 // (n - big)).astype(np.int32)
    return (c * int(variant[1:]) // n).astype(np.int32)


def zonal_child(mode, variant):
    """ms per closing day of one variant: `alone` (record back to back), `run` (behind the day's kernel; `none`: nothing configured) or
    `per_zone` (the plain call once per zone, summed); the minimum of three runs after a warm-up run."""
    import numpy as np

    from roger_amd import sas as rsas
    from roger_amd._native import SasContext

    n, ages = RUN_N, RUN_AGES
    zones = None if variant == "none" else zone_map(variant, n)
    if mode == "run":
        daily = rsas.synthetic_daily_inputs(n, RUN_DAYS, seed=42)
        ctx = rsas.create_sas(n, ages, RUN_SUBSTEPS, 90.0, 260.0, daily=daily, keep_distributions=True)
        windows = (np.arange(RUN_DAYS),) * 2
        best = []
        for k in range(4):
            if variant != "none":
                ctx.age_bands_configure(ITEMS[:1], PROBS, windows, zones=zones)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.run_days(0, RUN_DAYS)
            ctx.sync()
            best.append((time.perf_counter() - t0) / RUN_DAYS * 1e3)
        if variant != "none":
            assert ctx.age_bands_read()[2].all()
        ctx.close()
        print(json.dumps(min(best[1:])))
        return
    ctx = SasContext(n, ages, keep_distributions=True)
    ctx.upload(ITEMS[0], np.random.default_rng(7).random(ctx.shape(ITEMS[0])))
    windows = (np.arange(R * 4),) * 2

    def closing_day(**kw):
        ctx.age_bands_configure(ITEMS[:1], PROBS, windows, **kw)
        ms = []
        for k in range(4):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(R):
                ctx.age_bands_record(0)
            ctx.sync()
            ms.append((time.perf_counter() - t0) / R * 1e3)
        assert ctx.age_bands_read()[2].all()
        return min(ms[1:])

    if mode == "alone":
        out = closing_day(zones=zones)
    else:   # per_zone: the plain call under the mask of every zone (1024 zones: 16 of them, scaled)
        nz = int(zones.max()) + 1
        sample = range(nz) if nz <= 64 else range(0, nz, nz // 16)
        out = sum(closing_day(mask=zones == z) for z in sample) * (nz / len(sample))
    ctx.close()
    print(json.dumps(out))


def zonal_cost():
    def child(mode, variant, lib=None):
        env = dict(os.environ, **({"ROGER_HIP_LIB": lib} if lib else {}))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--zonal-child", mode, variant], check=True, capture_output=True, text=True,
                             timeout=280, env=env).stdout
        return float(json.loads(out.strip().splitlines()[-1]))

    lines = [f"    per zone: {RUN_N} columns x {RUN_AGES} ages, 1 item (1001 age classes), 3 probabilities, no weights, ms per closing day "
             "(minimum of 3 runs, a process each)"]
    none = child("run", "none")
    lines.append(f"    behind the day's kernel, nothing configured: {none:.4f} ms per day")
    for v, text in ZONAL_VARIANTS:
        alone, run = child("alone", v), child("run", v)
        lines.append(f"    {text}: stand-alone {alone:.4f}; behind the day's kernel {run:.4f} ({run - none:+.4f} against nothing configured)")
    for v in ("z8", "z64", "z90", "z1024"):
        lines.append(f"    the alternative, the plain call once per zone, {'64 zones with one of 90 % of the columns' if v == 'z90' else v[1:] + ' zones'}, stand-alone, summed"
                     + (" (16 zones x 64)" if v == "z1024" else "") + f": {child('per_zone', v):.4f}")
    lib = os.environ.get("ROGER_HIP_NO_SMALL")
    if lib:
        lines.append(f"    1024 equal zones with every zone through the six passes (a build with SAS_AGE_SHORT_ZONE=0): stand-alone {child('alone', 'z1024', lib):.4f}; "
                     f"behind the day's kernel {child('run', 'z1024', lib):.4f}")
    else:
        lines.append("    ROGER_HIP_NO_SMALL is not set: the 1024 zones through the six passes were not measured")
    return lines


WINDOW_ITEM = [("tt_q_ss", "q_ss", "bulk")]
WINDOW_RUNS = [("none", "nothing configured"), ("snapshot", "the snapshot observer, 1 item, 14 windows of one day"),
               ("w1", "the window means, 1 item, ONE window of 14 days (13 accumulating days, 1 closing day)"),
               ("w14", "the window means, 1 item, 14 windows of one day (14 closing days)")]


def window_child(mode, variant):
    """ms per day of one variant of the window means: `alone` acc / close (record back to back) or `run` (behind the day's kernel)."""
    import numpy as np

    from roger_amd import sas as rsas
    from roger_amd._native import SasContext

    n, ages = RUN_N, RUN_AGES
    one_long, every_day = (np.array([0]), np.array([RUN_DAYS - 1])), (np.arange(RUN_DAYS),) * 2
    if mode == "run":
        daily = rsas.synthetic_daily_inputs(n, RUN_DAYS, seed=42)
        ctx = rsas.create_sas(n, ages, RUN_SUBSTEPS, 90.0, 260.0, daily=daily, keep_distributions=True)
        best = []
        for k in range(4):
            if variant == "snapshot":
                ctx.age_bands_configure(["tt_q_ss"], PROBS, every_day)
            elif variant != "none":
                ctx.age_window_bands_configure(WINDOW_ITEM, PROBS, one_long if variant == "w1" else every_day)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.run_days(0, RUN_DAYS)
            ctx.sync()
            best.append((time.perf_counter() - t0) / RUN_DAYS * 1e3)
        if variant in ("w1", "w14"):
            rows, hdr, closed, days = ctx.age_window_bands_read()
            assert closed.all() and days == RUN_DAYS and hdr["tt_q_ss"][..., 0].any()
        ctx.close()
        print(json.dumps(min(best[1:])))
        return
    rng = np.random.default_rng(7)
    ctx = SasContext(n, ages, keep_distributions=True)
    ctx.upload("tt_q_ss", rng.random(ctx.shape("tt_q_ss")))
    ctx.upload("q_ss", rng.random(ctx.shape("q_ss")) + 0.1)
    days = R * 4 + 2
    # acc: one window that the days below never close; close: every day a window of its own
    ctx.age_window_bands_configure(WINDOW_ITEM, PROBS, (np.array([0]), np.array([days])) if variant == "acc" else (np.arange(days),) * 2)
    ctx.age_window_bands_record(0)   # (acc: the window's first day, which reads no accumulator)
    ms = []
    for k in range(4):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(R):
            ctx.age_window_bands_record(0)
        ctx.sync()
        ms.append((time.perf_counter() - t0) / R * 1e3)
    ctx.close()
    print(json.dumps(min(ms[1:])))


def window_cost():
    def child(mode, variant):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--window-child", mode, variant], check=True, capture_output=True, text=True,
                             timeout=280).stdout
        return float(json.loads(out.strip().splitlines()[-1]))

    elems = RUN_N * RUN_AGES
    acc, close = child("alone", "acc"), child("alone", "close")
    lines = [f"    window means: {RUN_N} columns x {RUN_AGES} ages, 1 item (tt_q_ss BULK by q_ss, {RUN_AGES} age classes), 3 probabilities, no weights, ms per "
             "day (minimum of 3 runs, a process each)",
             f"    stand-alone, an accumulating day (k_sas_age_acc): {acc:.4f} ms; {elems} elements x 40 B = {elems * 40 / 1e9:.2f} GB, {elems * 40 / acc / 1e9:.3f} TB/s",
             f"    stand-alone, a closing day of a one-day window (k_sas_age_keys_window, k_sas_age_bands): {close:.4f} ms"]
    got = {v: child("run", v) for v, _ in WINDOW_RUNS}
    for v, text in WINDOW_RUNS:
        lines.append(f"    behind the day's kernel over {RUN_DAYS} days, {text}: {got[v]:.4f}" + ("" if v == "none" else f" ({got[v] - got['none']:+.4f} against nothing configured)"))
    return lines


def off_cost():
    parent = os.environ.get("ROGER_HIP_PARENT")
    if not parent:
        return ["    off cost: ROGER_HIP_PARENT is not set, skipped"]
    old, new, key = [], [], ""
    first = os.environ.get("ROGER_HIP_OFF_FIRST", "parent")   # which library opens the alternation: an order effect shows when it is swapped
    for _ in range(3):
        for lib in ((parent, None) if first == "parent" else (None, parent)):
            ms, key = bench_ms_per_day(lib)
            (old if lib else new).append(ms)
    med = statistics.median(new)
    verdict = "within or below the parent's range" if med <= max(old) else "ABOVE the parent's range"
    return [f"    bench.py --model sas --steps 8 --warmup 2, nothing configured, {key} in ms, alternating: parent library "
            + ", ".join(f"{x:.4f}" for x in old) + f" (range {min(old):.4f} ... {max(old):.4f}); this tree " + ", ".join(f"{x:.4f}" for x in new)
            + f" (median {med:.4f}): {verdict}"]


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        run_child(sys.argv[2])
        sys.exit(0)
    if sys.argv[1:2] == ["--zonal-child"]:
        zonal_child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if sys.argv[1:2] == ["--window-child"]:
        window_child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    what = sys.argv[1:] or ["run", "alone", "off"]
    print("transport bands by age (rh_sas_age_bands_*), measured once on one MI355X", flush=True)
    if "run" in what:
        print("\n".join(behind_the_day()), flush=True)
    if "alone" in what:
        print("\n".join(alone()), flush=True)
    if "off" in what:
        print("\n".join(off_cost()), flush=True)
    if "zonal" in what:
        print("\n".join(zonal_cost()), flush=True)
    if "window" in what:
        print("\n".join(window_cost()), flush=True)
