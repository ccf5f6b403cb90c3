#!/usr/bin/env python3
"""What the native host code enqueues, compared between two builds of the library (for refactors of the host side):

    rocprofv3 --kernel-trace --output-format csv -d OLD_DIR -- python tools/launch_trace.py   # with ROGER_HIP_LIB=<the other library>
    rocprofv3 --kernel-trace --output-format csv -d NEW_DIR -- python tools/launch_trace.py
    python tools/launch_trace.py cmp OLD_DIR NEW_DIR     # exit status 1 at the first difference
    python tools/launch_trace.py cmp OLD_DIR NEW_DIR --own   # ... leaving out the runtime's own copy and fill kernels (__amd_rocclr_*)

Without arguments: a scenario of a few seconds that takes every stepping path for two to six steps each and prints its sections in
order.  In front of section k the scenario waits for the device and runs the rh_pow selftest on 256 (k + 1) pairs, a kernel no
stepping path launches: `cmp` cuts the ordered list of (kernel name, grid size, workgroup size) at those launches and prints the
first difference of every section.  The runtime performs hipMemcpyAsync / hipMemsetAsync on device memory with kernels of its own, which
the trace lists too: a change that only reorders copies and clears (inside a configure call, say) differs without --own and is equal with it."""
import csv
import glob
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
MARK = "k_selftest_rh_pow"
SECTIONS = []


def section(name, native):
    native.selftest_pow(np.ones(256 * (len(SECTIONS) + 1)), np.ones(256 * (len(SECTIONS) + 1)))
    SECTIONS.append(name)
    print(f"section {len(SECTIONS) - 1}: {name}", flush=True)


class switch:
    """An environment switch of rh_create, set while a context is created."""

    def __init__(self, name=None, value="1"):
        self.name, self.value = name, value

    def __enter__(self):
        if self.name:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.name:
            del os.environ[self.name]


def scenario():
    import hip_util as H
    from golden_util import load_case
    from roger_amd import _native as native
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params
    from test_hip_routing import routed_ctx

    native.load()
    forcing = combo_forcing(ndays=12)

    def svat(nx, ny, lateral=False, env=None, value="1"):
        p = hetero_params(nx * ny, seed=5)
        if lateral:
            p.update(slope=0.05, slope_per=5, dmph=50.0)
            p["z_soil"] = np.maximum(p["z_soil"], 800.0)
        with switch(env, value):
            ctx = create_svat(nx, ny, params=p, lateral=lateral)
        ctx.set_forcing_series(forcing)
        return ctx

    def observe(ctx, cells):
        ctx.diag_configure(rate=("aet", "q_ss"), collect=("S_rz_m1",), n_slots=2)   # a pure output, an _m1 plane
        ctx.points_configure(cells, ("theta", "transp"))

    def done(ctx):
        ctx.sync()
        ctx.close()

    section("SVAT 40 x 25: rh_run_steps(6)", native)
    ctx = svat(40, 25)
    ctx.run_steps(6)
    done(ctx)
    section("SVAT 40 x 25: rh_run_steps(6), accumulators and points", native)
    ctx = svat(40, 25)
    observe(ctx, (0, 255, 256, 999))
    ctx.run_steps(6)
    done(ctx)
    section("SVAT 40 x 25: rh_svat_step x 3", native)
    ctx = svat(40, 25)
    drv = H.HipForcingDriver(ctx, forcing)
    for _ in range(3):
        ctx.step(drv.before_step())
    done(ctx)
    section("SVAT 40 x 25: routine by routine x 2, accumulators and points", native)
    ctx = svat(40, 25)
    observe(ctx, (0, 255, 256, 999))
    for _ in range(2):
        for entry in ("rh_hooks_phase", "rh_adaptive_dt", "rh_step_core", "rh_after_timestep"):
            ctx.call(entry)
    done(ctx)
    for env in ("RH_NO_TAIL_CTRL", "RH_NO_LAZY_ROTATION", "RH_NO_SPARSE_STORES"):
        section(f"SVAT 40 x 25: rh_run_steps(4), {env}=1", native)
        ctx = svat(40, 25, env=env)
        ctx.run_steps(4)
        done(ctx)
    rng = np.random.default_rng(3)
    weights = (rng.uniform(0.8, 1.2, 257), rng.uniform(-1.0, 1.0, 257), rng.uniform(0.8, 1.2, 257))
    for env in (None, "RH_PER_CELL_OLD_FRONT", "RH_CELL_AGG_SPLIT_MIN"):
        section(f"SVAT 257 x 1, per-cell weights: rh_run_steps(4), {env or 'the one-launch front'}", native)
        ctx = svat(257, 1, env=env)
        ctx.set_forcing_weights(*weights)
        ctx.run_steps(4)
        done(ctx)
    section("oneD 40 x 25: rh_run_steps(4)", native)
    ctx = svat(40, 25, lateral=True)
    ctx.run_steps(4)
    done(ctx)
    g, names, gforcing = load_case("oned_routing")
    for what, env, obs in (("rh_run_steps(4)", None, False), ("rh_run_steps(4), accumulators and points", None, True),
                           ("rh_run_steps(4), RH_ROUTED_BY_ROUTINE=1", "RH_ROUTED_BY_ROUTINE", False), ("rh_step_routed x 2", None, False)):
        section(f"routing 4 x 6: {what}", native)
        with switch(env):
            ctx = routed_ctx(native, g, names)
        if obs:
            observe(ctx, (0, 5, 23))
        if what.startswith("rh_run_steps"):
            ctx.set_forcing_series(gforcing)
            ctx.run_steps(4)
        else:
            drv = H.HipForcingDriver(ctx, gforcing)
            for _ in range(2):
                ctx.step_routed(drv.before_step())
        done(ctx)
    section("one-rank communicator, SVAT 40 x 25: rh_run_steps_dist(4)", native)
    ctx = svat(40, 25)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.run_steps_dist(4)
    done(ctx)
    section("one-rank communicator, routing 4 x 6: rh_run_steps_dist(4)", native)
    ctx = routed_ctx(native, g, names)
    ctx.set_forcing_series(gforcing)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    ctx.run_steps_dist(4)
    done(ctx)
    from roger_amd import sas as rsas

    section("transport 96 columns x 300 ages, no points: rh_sas_run_days(3), rh_sas_step x 2", native)
    sas = rsas.create_sas(96, 300, 3, 90.0, 260.0, daily=rsas.synthetic_daily_inputs(96, 8, seed=42), age_statistics=True)
    sas.run_days(0, 3)
    sas.step(3)
    sas.step(4)
    done(sas)
    section("end", native)


def launches(directory, own=False):
    """[[(kernel name, grid, workgroup), ...] per section] of the one kernel trace below `directory`."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{directory}: expected one *kernel_trace.csv, found {len(files)}")
    rows = list(csv.DictReader(open(files[0], newline="")))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dims = lambda r, what: tuple(int(r[k]) for k in sorted(r) if k.startswith(what))   # noqa: E731
    out = []
    for r in rows:
        if MARK in r["Kernel_Name"]:
            out.append([])
        elif out and not (own and r["Kernel_Name"].startswith("__amd_rocclr_")):
            out[-1].append((r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size")))
    return out


def compare(old, new, own=False):
    a, b = launches(old, own), launches(new, own)
    bad = len(a) != len(b)
    if bad:
        print(f"{len(a)} sections before, {len(b)} after")
    for k, (x, y) in enumerate(zip(a, b)):
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
        print(f"section {k}: {len(x)} launches before, {len(y)} after, " + ("equal" if first is None else f"first difference at launch {first}:"))
        if first is not None:
            bad = True
            print("  before:", x[first] if first < len(x) else "(none)")
            print("  after: ", y[first] if first < len(y) else "(none)")
            print("  the section holds", "the same launches in another order" if sorted(x) == sorted(y) else "other launches")
    return bad


if __name__ == "__main__":
    if sys.argv[1:2] == ["cmp"]:
        sys.exit(compare(*sys.argv[2:4], own="--own" in sys.argv[4:]))
    scenario()
