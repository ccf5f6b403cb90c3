#!/usr/bin/env python3
"""What the ensemble bands (rh_bands_*, k_bands and k_bands_select in roger_amd/csrc/rh_bands.h) cost per step: fused steps
(rh_run_steps) of the benchmark's columns at 1000 x 1000 and at 80 x 53.

Unconfigured, under the combo forcing (all three step classes):
    (a)  the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset),
    (b)  this tree's library with nothing configured.
Configured, under a forcing without precipitation, where EVERY step is a day -- so a variant's steps are all of one kind and the
difference to (n) is the added time of one such step:
    (n)  nothing configured,
    (l)  bands, one LAST item, first interval far in the future: k_bands and the six k_bands_select launches all end after the scalar
         loads -- seven empty launches; a seventh of the difference is the per-launch gap,
    (u)  bands, one SUM item, three probabilities, first interval far in the future: the step that is not counted (24 B per column),
    (v)  durations, one SUM item without edges, first interval far in the future: its step that is not counted, the same 24 B,
    (k)  bands, one SUM item, three probabilities, daily interval from 0: every step is counted.

Every figure is one child process (create, 60 warm-up steps, three timed calls of `steps` steps, the fastest taken); the variants
alternate `repeats` times, and the median and the range over the repeats are printed.

    python3 tools/bands_time.py [steps [repeats]]        # writes profiles/bands_cost.txt as well"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GRIDS = [(1000, 1000), (80, 53)]
ITEM = "q_ss"
PROBS = (0.05, 0.5, 0.95)
FAR = 10 ** 6 * 86400
PASSES, LAUNCHES = 6, 7
HBM_TBS = 8.0   # MI355X peak HBM rate, TB/s
VARIANTS = [("a", "(a) parent commit, combo forcing, no observers"), ("b", "(b) this commit, combo forcing, nothing configured"),
            ("n", "(n) dry days, nothing configured"), ("l", "(l) dry days, bands: seven launches that end after the scalar loads"),
            ("u", "(u) dry days, bands: one SUM item, no step counted"), ("v", "(v) dry days, durations: one SUM item, no step counted"),
            ("k", "(k) dry days, bands: one SUM item, three probabilities, every step counted")]


def child(nx, ny, steps, variant):
    import numpy as np

    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(nx, ny)
    forcing = combo_forcing(ndays=3 * steps + 100 if variant not in "ab" else 400)
    if variant not in "ab":
        forcing["PREC"] = np.zeros_like(forcing["PREC"])
        forcing["TA"] = np.full_like(forcing["TA"], 12.0)
    ctx.set_forcing_series(forcing)
    if variant == "l":
        ctx.bands_configure([ITEM], [1], PROBS, 86400, FAR, None, 4096)
    elif variant == "u":
        ctx.bands_configure([ITEM], [0], PROBS, 86400, FAR, None, 4096)
    elif variant == "v":
        ctx.durations_configure([ITEM], [0], [[]], [None], None, 86400, FAR)
    elif variant == "k":
        ctx.bands_configure([ITEM], [0], PROBS, 86400, 0, None, 4096)
    ctx.run_steps(60)
    ctx.sync()
    rows0 = ctx.bands_count() if variant in "luk" else 0
    t_before = int(ctx.get_scalars().time)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    days = (int(ctx.get_scalars().time) - t_before) // 86400
    rows = (ctx.bands_count() - rows0) if variant in "luk" else 0
    if variant not in "ab":
        assert days == 3 * steps, (days, "not every step was a day")
    assert rows == (3 * steps if variant == "k" else 0), (variant, rows)
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
    lines = [f"python3 tools/bands_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
                                                              "   (ROGER_HIP_PARENT unset: (a) NOT measured)")]
    print(lines[0], flush=True)
    for nx, ny in GRIDS:
        n = nx * ny
        got = {key: [] for key, _ in VARIANTS}
        for _ in range(repeats):
            for key, _ in VARIANTS:
                if key == "a":
                    if parent:
                        got[key].append(run_child(nx, ny, steps, "b", parent))
                else:
                    got[key].append(run_child(nx, ny, steps, key))
        block = [f"{nx} x {ny}, {steps} fused steps per call, ms per step, median [min ... max] of {repeats} alternating repeats"]
        for key, label in VARIANTS:
            if got[key]:
                v = got[key]
                block.append(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
        med = {key: statistics.median(v) for key, v in got.items() if v}
        if "a" in med:
            spread = max(got["a"]) - min(got["a"])
            ok = abs(med["b"] - med["a"]) <= spread
            block.append(f"    unconfigured: (b) - (a) = {1e3 * (med['b'] - med['a']):+.1f} us; the parent's own repeats spread over {1e3 * spread:.1f} us "
                         f"(max - min): {'within' if ok else 'NOT within'} that spread")
        gap = 1e3 * (med["l"] - med["n"]) / LAUNCHES
        add_u, add_v, add_k = (1e3 * (med[key] - med["n"]) for key in "uvk")
        block.append(f"    per-launch gap: ((l) - (n)) / {LAUNCHES} launches = {gap:.2f} us")
        block.append(f"    a step that is NOT counted, one SUM item (24 B per column), over (n): bands (u) {add_u:+.1f} us, durations (v) {add_v:+.1f} us; "
                     f"{LAUNCHES} launches x the gap explain {LAUNCHES * gap:.1f} us of (u), 1 x the gap {gap:.1f} us of (v); "
                     f"(u) beyond its launches and (v)'s own time beyond its launch: {add_u - LAUNCHES * gap - (add_v - gap):+.1f} us")
        moved = PASSES * 8 * n
        sel = add_k - add_u
        block.append(f"    a COUNTED step, one SUM item, three probabilities, over (n): (k) {add_k:+.1f} us ({sel:+.1f} us over the step that is not counted); "
                     f"{LAUNCHES} launches per step; the selection must read {PASSES} passes x 8 B x {n} keys = {moved / 1e6:.2f} MB"
                     + (f": {moved / (sel * 1e-6) / 1e12:.2f} TB/s over those {sel:.1f} us, {100.0 * moved / (sel * 1e-6) / 1e12 / HBM_TBS:.0f} % of the "
                        f"{HBM_TBS:.0f} TB/s HBM rate" if sel > 0 else ""))
        for line in block:
            print(line, flush=True)
        lines += block
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "bands_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
