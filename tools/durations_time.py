#!/usr/bin/env python3
"""What the duration curves' observer (rh_durations_*, k_durations) costs per step: 200 fused steps (rh_run_steps) of the benchmark's
columns at 1000 x 1000 and at 80 x 53, for

    (a)  the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset),
    (b)  this tree's library with nothing configured,
    (c)  this tree's library with four SUM items of 32 edges each at a daily interval (two of them with a spell),
    (d)  this tree's library with rh_diag_configure of the same four planes as rate accumulators: the same bytes per non-closing step.

Every figure is one child process (create, 120 warm-up steps, three timed calls of `steps` steps, the fastest taken); the variants
alternate `repeats` times, and the median and the range over the repeats are printed.  The condition for (b) is not a time: every
kernel of the parent commit has the same ISA in this tree (tools/isa_diff.py), and a context without durations launches nothing new;
whether the median of (b) lies inside (a)'s min ... max range of the same run is written down as it comes out.  (c) has no cap: it is
reported next to (d), with the configured bytes per column and the share of closing steps among the timed ones.

    python3 tools/durations_time.py [steps [repeats]]        # writes profiles/durations_cost.txt as well"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ["prec", "aet", "q_ss", "inf_mat_rz"]   # aet, q_ss: pure outputs (the KEEP variant runs)
GRIDS = [(1000, 1000), (80, 53)]
EDGES = 32
BYTES_PER_COLUMN = len(NAMES) * ((EDGES + 2) * 4 + 3 * 8 + 3 * 4)   # counters, {acc, min, max}, {run, longest, n_spells}
VARIANTS = [("a", "(a) parent commit, no observers"), ("b", "(b) this commit, nothing configured"),
            ("c", "(c) this commit, durations: four SUM items of 32 edges, daily interval"), ("d", "(d) this commit, accumulators: four rate planes")]


def child(nx, ny, steps, variant):
    import numpy as np

    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(nx, ny)
    ctx.set_forcing_series(combo_forcing(ndays=400))
    if variant == "c":
        e = np.concatenate([[0.0], np.geomspace(1e-3, 50.0, EDGES - 1)])
        ctx.durations_configure(NAMES, [0] * len(NAMES), [e] * len(NAMES), [(1, 1.0), None, (0, 0.1), None], None, 86400, 0)
    elif variant == "d":
        ctx.diag_configure(rate=NAMES, n_slots=1)
    ctx.run_steps(120)
    ctx.sync()
    before = int(ctx.durations_read()[0][0][:, 0].sum()) if variant == "c" else 0
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    closing = 0
    if variant == "c":
        closing = int(ctx.durations_read()[0][0][:, 0].sum()) - before
        assert closing > 0
    ctx.close()
    print(json.dumps([best, closing]))


CLOSING = []   # counted intervals of column 0 over the three timed calls of every (c) child


def run_child(nx, ny, steps, variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), variant],
                         env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    best, closing = json.loads(out.strip().splitlines()[-1])
    if variant == "c":
        CLOSING.append(int(closing))
    return float(best)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    lines = [f"python3 tools/durations_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
                                                                  "   (ROGER_HIP_PARENT unset: (a) NOT measured)")]
    print(lines[0], flush=True)
    for nx, ny in GRIDS:
        got = {key: [] for key, _ in VARIANTS}
        for _ in range(repeats):
            for key, _ in VARIANTS:
                if key == "a":
                    if parent:
                        got[key].append(run_child(nx, ny, steps, "b", parent))
                else:
                    got[key].append(run_child(nx, ny, steps, key))
        block = [f"{nx} x {ny}, {steps} fused steps per call, {len(NAMES)} planes, ms per step, median [min ... max] of {repeats} alternating repeats"]
        for key, label in VARIANTS:
            if got[key]:
                v = got[key]
                block.append(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
        med = {key: statistics.median(v) for key, v in got.items() if v}
        block.append(f"    over (b), us per step: (c) {1e3 * (med['c'] - med['b']):+.1f}, (d) {1e3 * (med['d'] - med['b']):+.1f}")
        share = statistics.median(CLOSING[-repeats:]) / (3.0 * steps)
        block.append(f"    (c): {BYTES_PER_COLUMN} bytes per column configured ({len(NAMES)} items x ({EDGES} + 2 counters, 3 float64, 3 uint32)); "
                     f"{100.0 * share:.1f} % of the timed steps close a day ({1e3 * (med['c'] - med['b']) / max(share, 1e-9):+.1f} us per closing step "
                     "if all of the difference is theirs)")
        if "a" in med:
            ok = min(got["a"]) <= med["b"] <= max(got["a"])
            block.append(f"    (b) - (a): {1e3 * (med['b'] - med['a']):+.1f} us; median of (b) inside (a)'s range: {'yes' if ok else 'no'} "
                         "(the condition is the ISA identity, not this time)")
        for line in block:
            print(line, flush=True)
        lines += block
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "durations_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
