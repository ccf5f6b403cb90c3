#!/usr/bin/env python3
"""What the points recorder (rh_points_*, k_points) costs per step: the benchmark's fused steps (rh_run_steps) with 16 points x 8
variables against the same run with no observers, at 80 x 53 and at 10^6 columns -- once with an observed set that holds no pure
output (the plain sparse kernel + k_points) and once with one that does (the KEEP variant of the sparse kernel + k_points; the KEEP
share is the sparse kernel's, DESIGN.md section 9.9, not the recorder's).  Medians of five alternating pairs in one process.

    python3 tools/points_time.py [steps]                     this tree's library, with and without points
    ROGER_HIP_PARENT=/path/to/parent/libroger_hip.so ...     the baseline runs on the parent's library in child processes
                                                             (RH_OLD_VARIANT: an older ABI is accepted)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STATE = ["S_rz", "S_ss", "swe", "S_fp_rz", "S_lp_rz", "S_fp_ss", "S_lp_ss", "theta_rz"]         # no pure output among them
MIXED = ["S_rz", "S_ss", "swe", "S_fp_rz", "S_lp_rz", "S_fp_ss", "S_lp_ss", "q_ss"]             # q_ss: a pure output (KEEP variant)
GRIDS = [(80, 53), (1000, 1000)]


def measure(nx, ny, names, steps, pairs):
    """ms per step, `pairs` times: [(without points, with points)] on two contexts of one process stepped alternately."""
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctxs = []
    for with_points in (False, True):
        ctx = create_svat(nx, ny)
        ctx.set_forcing_series(combo_forcing(ndays=400))
        if with_points and names:
            n = nx * ny
            ctx.points_configure([(k * (n - 1)) // 15 for k in range(16)], names, capacity=4096)
        ctx.run_steps(120)
        ctx.sync()
        ctxs.append(ctx)
    out = []
    for _ in range(pairs):
        row = []
        for ctx in ctxs:
            t0 = time.perf_counter()
            ctx.run_steps(steps)
            ctx.sync()
            row.append((time.perf_counter() - t0) / steps * 1e3)
        out.append(row)
    pure = [v for v in (names or []) if v in ctxs[1].pure_output_planes()]
    for ctx in ctxs:
        ctx.close()
    return out, pure


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:      # the baseline on another library: prints the ms per step without observers
        nx, ny, steps, pairs = (int(v) for v in sys.argv[2:6])
        rows, _ = measure(nx, ny, None, steps, pairs)
        print(json.dumps([r[0] for r in rows]))
        sys.exit(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    parent = os.environ.get("ROGER_HIP_PARENT")
    for nx, ny in GRIDS:
        for label, names in (("state planes only (plain sparse kernel + k_points)", STATE), ("one pure output (KEEP variant + k_points)", MIXED)):
            rows, pure = measure(nx, ny, names, steps, 5)
            assert bool(pure) == (names is MIXED), pure
            base, pts = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
            line = (f"{nx} x {ny}, 16 points x 8 variables, {label}; pure outputs observed: {pure}\n"
                    f"    this tree, no observers {base:.4f} ms per step, with points {pts:.4f} ms per step: {1e3 * (pts - base):+.1f} us "
                    f"(medians of 5 alternating pairs of {steps} steps; pairs {[f'{a:.4f}/{b:.4f}' for a, b in rows]})")
            if parent:
                env = dict(os.environ, ROGER_HIP_LIB=parent, RH_OLD_VARIANT="1")
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nx), str(ny), str(steps), "5"], env=env,
                                     check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
                pbase = statistics.median(json.loads(got))
                line += f"\n    parent library, no observers {pbase:.4f} ms per step (median of 5): with points {1e3 * (pts - pbase):+.1f} us against the parent"
            print(line, flush=True)
