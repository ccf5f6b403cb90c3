#!/usr/bin/env python3
"""What the likelihood-weighted ensemble bands (rh_bands_configure_weighted; k_bands_select_w in roger_amd/csrc/rh_bands.h) cost per
COUNTED step: fused steps (rh_run_steps) of the benchmark's columns under a forcing without precipitation, where every step is a day and
closes a daily interval.  Two items (q_ss summed, theta_rz at the interval's end), three probabilities.  Per shape:
    (n)  nothing configured,
    (a)  the parent commit's library, plain bands with one mask over every column (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped
         if unset),
    (p)  this tree's library, the same plain bands,
    (w)  this tree's library, weighted bands: seeded weights 1 ... 65535 on every column.
Shapes: 80 x 53 columns (launch-bound) and 1000 x 1000 columns.

Every figure is one child process (create, 60 warm-up steps, three timed calls of `steps` steps that end in a synchronise, the fastest
taken); the variants alternate `repeats` times, and the median and the range over the repeats are printed.

    python3 tools/bands_weighted_time.py [steps [repeats]]        # writes profiles/bands_weighted_cost.txt as well"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(80, 53), (1000, 1000)]
ITEMS, KINDS = ["q_ss", "theta_rz"], [0, 1]
PROBS = (0.05, 0.5, 0.95)
PASSES = 6
VARIANTS = [("n", "(n) nothing configured"), ("a", "(a) parent commit, plain bands, one mask"), ("p", "(p) this commit, plain bands, one mask"),
            ("w", "(w) this commit, weighted bands")]


def child(nx, ny, steps, variant):
    import numpy as np

    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    n = nx * ny
    ctx = create_svat(nx, ny)
    forcing = combo_forcing(ndays=3 * steps + 100)
    forcing["PREC"] = np.zeros_like(forcing["PREC"])
    forcing["TA"] = np.full_like(forcing["TA"], 12.0)
    ctx.set_forcing_series(forcing)
    if variant == "p":
        ctx.bands_configure(ITEMS, KINDS, PROBS, 86400, 0, np.ones(n, dtype=np.uint8), 4096)
    elif variant == "w":
        ctx.bands_configure(ITEMS, KINDS, PROBS, 86400, 0, None, 4096, weights=np.random.default_rng(1).integers(1, 65536, n).astype(np.uint16))
    ctx.run_steps(60)
    ctx.sync()
    rows0 = ctx.bands_count() if variant != "n" else 0
    t_before = int(ctx.get_scalars().time)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    days = (int(ctx.get_scalars().time) - t_before) // 86400
    assert days == 3 * steps, (days, "not every step was a day")
    if variant != "n":
        assert ctx.bands_count() - rows0 == 3 * steps, (variant, ctx.bands_count() - rows0)
    ctx.close()
    print(json.dumps(best))


def run_child(nx, ny, steps, variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), variant],
                         env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    lines = [f"python3 tools/bands_weighted_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
                                                                       "   (ROGER_HIP_PARENT unset: (a) NOT measured)")]
    print(lines[0], flush=True)
    for nx, ny in SHAPES:
        n = nx * ny
        got = {key: [] for key, _ in VARIANTS}
        for _ in range(repeats):
            for key, _ in VARIANTS:
                if key == "a":
                    if parent:
                        got[key].append(run_child(nx, ny, steps, "p", parent))
                else:
                    got[key].append(run_child(nx, ny, steps, key))
        block = [f"{nx} x {ny} columns, {len(ITEMS)} items x {len(PROBS)} probabilities, every step counted, {steps} fused steps per call, ms per step, "
                 f"median [min ... max] of {repeats} alternating repeats"]
        for key, label in VARIANTS:
            if got[key]:
                v = got[key]
                block.append(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
        med = {key: statistics.median(v) for key, v in got.items() if v}
        add_p, add_w = (1e3 * (med[key] - med["n"]) for key in "pw")
        if "a" in med:
            block.append(f"    plain bands, this commit against the parent: (p) - (a) = {1e3 * (med['p'] - med['a']):+.1f} us; the parent's own repeats "
                         f"spread over {1e3 * (max(got['a']) - min(got['a'])):.1f} us (max - min)")
        block.append(f"    a counted step over (n): plain (p) {add_p:+.1f} us, weighted (w) {add_w:+.1f} us, both with 7 launches: (w) - (p) = {add_w - add_p:+.1f} us "
                     f"(spread of (w): {1e3 * (max(got['w']) - min(got['w'])):.1f} us, of (p): {1e3 * (max(got['p']) - min(got['p'])):.1f} us)")
        extra = PASSES * 2 * n * len(ITEMS)
        block.append(f"    the cost model's added traffic: {PASSES} passes x 2 B x {n} weights x {len(ITEMS)} items = {extra / 1e6:.2f} MB on top of the plain "
                     f"selection's {PASSES * 8 * n * len(ITEMS) / 1e6:.2f} MB of keys (+25 %), and 8-byte merges in place of 4-byte ones; at the "
                     f"{add_w - add_p:.1f} us of (w) - (p) the added bytes alone would move at {extra / max(add_w - add_p, 1e-3) / 1e6:.3f} TB/s")
        for line in block:
            print(line, flush=True)
        lines += block
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "bands_weighted_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
