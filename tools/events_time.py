#!/usr/bin/env python3
"""What the event outputs' observer (rh_events_*, k_events) costs per step on the launch-bound 80 x 53 case: 200 fused steps
(rh_run_steps) of the benchmark's columns, for

    (a)  the parent commit's library (ROGER_HIP_PARENT=/path/to/libroger_hip.so; skipped if unset),
    (b)  this tree's library with nothing configured,
    (c)  this tree's library with four items (two sums, a peak, a first value) and 64 slots: most steps of the combo forcing belong to
         no event, where the launch exits on a scalar.

Every figure is one child process (create, 120 warm-up steps, three timed calls of `steps` steps, the fastest taken); the variants
alternate `repeats` times, and the median and the range over the repeats are printed.  No gate rests on the numbers.

    python3 tools/events_time.py [steps [repeats]]        # writes profiles/events_cost.txt as well"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ITEMS = [("prec", 0), ("q_ss", 0), ("q_sur", 1), ("theta_rz", 2)]
NX, NY = 80, 53
VARIANTS = [("a", "(a) parent commit, no observers"), ("b", "(b) this commit, nothing configured"),
            ("c", "(c) this commit, events: two sums, a peak, a first value")]


def child(steps, variant):
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(NX, NY)
    ctx.set_forcing_series(combo_forcing(ndays=400))
    if variant == "c":
        ctx.events_configure([v for v, _ in ITEMS], [k for _, k in ITEMS], 64)
    ctx.run_steps(120)
    ctx.sync()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        best = ms if best is None else min(best, ms)
    if variant == "c":
        hdr, _, lost = ctx.events_read(slots=())
        assert (hdr[:, 0] > 0).sum() >= 3 and not lost
    ctx.close()
    print(json.dumps(best))


def run_child(steps, variant, lib=None):
    env = dict(os.environ)
    if lib:
        env.update(ROGER_HIP_LIB=lib, RH_OLD_VARIANT="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(steps), variant],
                         env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return float(json.loads(out.strip().splitlines()[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(int(sys.argv[2]), sys.argv[3])
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = os.environ.get("ROGER_HIP_PARENT")
    lines = [f"python3 tools/events_time.py {steps} {repeats}" + ("   (ROGER_HIP_PARENT set: the parent commit's library)" if parent else
                                                                  "   (ROGER_HIP_PARENT unset: (a) NOT measured)")]
    got = {key: [] for key, _ in VARIANTS}
    for _ in range(repeats):
        for key, _ in VARIANTS:
            if key == "a":
                if parent:
                    got[key].append(run_child(steps, "b", parent))
            else:
                got[key].append(run_child(steps, key))
    lines.append(f"{NX} x {NY}, {steps} fused steps per call, ms per step, median [min ... max] of {repeats} alternating repeats")
    for key, label in VARIANTS:
        if got[key]:
            v = got[key]
            lines.append(f"    {label}: {statistics.median(v):.4f} [{min(v):.4f} ... {max(v):.4f}]   {[f'{x:.4f}' for x in v]}")
    med = {key: statistics.median(v) for key, v in got.items() if v}
    lines.append(f"    (c) - (b): {1e3 * (med['c'] - med['b']):+.1f} us per step" + (f"; (b) - (a): {1e3 * (med['b'] - med['a']):+.1f} us" if "a" in med else ""))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "events_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
