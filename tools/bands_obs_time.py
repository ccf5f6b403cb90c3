#!/usr/bin/env python3
"""What the observations of the ensemble bands (rh_bands_observations; k_bands_obs and k_bands_obs_row in roger_amd/csrc/rh_bands.h) cost
per COUNTED step: fused steps (rh_run_steps) of the benchmark's columns under a forcing without precipitation, where every step is a day
and closes a daily interval.  Two items (q_ss summed, theta_rz at the interval's end), three probabilities.  Per shape:
    (n)  nothing configured,
    (a)  the parent commit's library, plain bands with one mask over every column (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped
         if unset),
    (p)  this tree's library, the same plain bands, no observations: no launch is added,
    (o)  this tree's library, the same plain bands with an observation on every interval for both items,
    (w)  this tree's library, weighted bands (seeded weights 1 ... 65535 on every column), no observations,
    (v)  this tree's library, the same weighted bands with the observations.
Shapes: 80 x 53 columns (launch-bound) and 1000 x 1000 columns.

Every figure is one child process (create, 60 warm-up steps, three timed calls of `steps` steps that end in a synchronise, the fastest
taken); the variants alternate `repeats` times, and the median and the range over the repeats are printed.

    python3 tools/bands_obs_time.py [steps [repeats]]        # writes profiles/bands_obs_cost.txt as well"""
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
            ("o", "(o) this commit, plain bands with observations"), ("w", "(w) this commit, weighted bands"),
            ("v", "(v) this commit, weighted bands with observations")]


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
    if variant in "po":
        ctx.bands_configure(ITEMS, KINDS, PROBS, 86400, 0, np.ones(n, dtype=np.uint8), 4096)
    elif variant in "wv":
        ctx.bands_configure(ITEMS, KINDS, PROBS, 86400, 0, None, 4096, weights=np.random.default_rng(1).integers(1, 65536, n).astype(np.uint16))
    if variant in "ov":   # an observation inside the ensemble's range on every interval: the pass runs on every step
        ctx.bands_observations(np.stack([np.full(3 * steps + 100, 0.01), np.full(3 * steps + 100, 0.25)]))
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
    if variant in "ov":
        pairs = ctx.bands_obs_read(ctx.bands_count() - steps, steps)
        assert (pairs >= 0).all(), "an interval without a pair"
    ctx.close()
    print(json.dumps(best))


def run_child(nx, ny, steps, variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), variant],
                         env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


def spread(v):
    return 1e3 * (max(v) - min(v))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    lines = [f"python3 tools/bands_obs_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
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
        if "a" in med:
            diff, own = 1e3 * (med["p"] - med["a"]), spread(got["a"])
            block.append(f"    (a) plain bands without observations, this commit against the parent: (p) - (a) = {diff:+.1f} us; the parent's own repeats "
                         f"spread over {own:.1f} us (max - min): the difference lies {'WITHIN' if abs(diff) <= own else 'OUTSIDE'} that spread")
        add_o, add_v = 1e3 * (med["o"] - med["p"]), 1e3 * (med["v"] - med["w"])
        sel_p, sel_w = 1e3 * (med["p"] - med["n"]), 1e3 * (med["w"] - med["n"])
        block.append(f"    (b) a counted step with observations, 2 launches more: plain (o) - (p) = {add_o:+.1f} us on top of the bands' {sel_p:.1f} us "
                     f"({100 * add_o / sel_p:+.1f} %); weighted (v) - (w) = {add_v:+.1f} us on top of {sel_w:.1f} us ({100 * add_v / sel_w:+.1f} %)   "
                     f"(spreads: (p) {spread(got['p']):.1f}, (o) {spread(got['o']):.1f}, (w) {spread(got['w']):.1f}, (v) {spread(got['v']):.1f} us)")
        keys_mb, obs_mb, obs_w_mb = PASSES * 8 * n * len(ITEMS) / 1e6, 8 * n * len(ITEMS) / 1e6, 10 * n * len(ITEMS) / 1e6
        block.append(f"    the cost model's expectation: one more pass of 8 B x {n} keys x {len(ITEMS)} items = {obs_mb:.2f} MB (weighted: + 2 B of weights, "
                     f"{obs_w_mb:.2f} MB) on top of the selection's {PASSES} passes = {keys_mb:.2f} MB of keys, about one sixth more traffic (+16.7 %), plus two "
                     f"launches; at the measured {add_o:.1f} us / {add_v:.1f} us the added bytes alone would move at "
                     f"{obs_mb / max(add_o, 1e-3):.3f} / {obs_w_mb / max(add_v, 1e-3):.3f} TB/s")
        for line in block:
            print(line, flush=True)
        lines += block
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "bands_obs_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
