"""Child process of tests/test_hip_grid_ranks.py: ranks on a (px, py) process grid as threads of this process on one GPU, each with its
own context, joined by the loopback communicator (tests/loopback_nccl.cpp through RH_RCCL_LIB).  Every rank holds the block
`get_chunk_slices(nx, ny, (px, py), rank)` of a golden domain and is told the grid with rh_comm_set_grid; the routing's halo then
reaches the neighbours in x and y and the corners.

    python tests/grid_ranks_child.py routing | unchanged | routing_by_routine | allreduce | errors
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hip_util as H  # noqa: E402
from golden_util import ROUTING_CASES, compare, load_case  # noqa: E402
from loopback_ranks_child import loopback_counts, run_ranks  # noqa: E402
from roger_amd import _native as native  # noqa: E402
from roger_amd.distributed import get_chunk_slices, get_process_neighbors  # noqa: E402

RH_ERR_ARG, RH_ERR_STATE = -1, -3

# (case, grids); the first grid of a case is also stepped without a communicator (the non-vacuous check)
GRIDS = (
    ("oned_routing", ((2, 2), (1, 2), (2, 3))),           # 4 x 6: (2, 2) has diagonal flow across the corner of the blocks
    ("oned_routing_combo", ((1, 2), (1, 4))),             # 5 x 4: (1, 4) gives one-row blocks
    ("oned_routing_tutorial", ((1, 2), (1, 4))),          # 1 x 20, every cell drains along +y
)


def block(g, key, grid, rank):
    """The rank's block of a golden snapshot (planes, nx * ny) as (planes, nxl * nyl), and its global cell indices."""
    nx, ny = (int(v) for v in g["nx_ny"])
    (gx, gy), _ = get_chunk_slices(nx, ny, grid, rank)
    snap = np.asarray(g[key])
    return snap.reshape(snap.shape[0], nx, ny)[:, gx, gy].reshape(snap.shape[0], -1), np.arange(nx * ny).reshape(nx, ny)[gx, gy].ravel()


def local_shape(g, grid):
    nx, ny = (int(v) for v in g["nx_ny"])
    return nx // grid[0], ny // grid[1]


def routed_ctx(g, names, grid=(1, 1), rank=0, key="state0", scal_key="scal0"):
    nxl, nyl = local_shape(g, grid)
    dx, dy = (float(v) for v in g["routing_dx_dy"])
    ctx = native.Context(nxl, nyl, enable_lateral_flow=1, enable_routing_1D=1, dx=dx, dy=dy)
    H.upload_snapshot(ctx, block(g, key, grid, rank)[0], names)
    ctx.set_scalars(H.scalars_from_row(g[scal_key]))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    ctx.set_lut_mlms(g["lut_mlms"])
    return ctx


def stitch(g, names, grid, snaps):
    """The ranks' downloaded snapshots as one global (planes, nx * ny) array."""
    nx, ny = (int(v) for v in g["nx_ny"])
    got = np.full((len(names), nx * ny), np.nan)
    for r, snap in enumerate(snaps):
        got[:, block(g, "state0", grid, r)[1]] = np.asarray(snap).reshape(len(names), -1)
    return got


def neighbour_count(grid):
    """Present neighbours summed over the ranks: one send per neighbour, rank and quantity in every exchange."""
    return sum(v is not None for r in range(grid[0] * grid[1]) for v in get_process_neighbors(r, grid).values())


def differing(names, got, ref):
    return [names[p] for p in np.unique(np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:, 0])][:8]


def single_domain(g, names, forcing):
    nsteps = int(g["nsteps"])
    whole = routed_ctx(g, names)
    whole.set_forcing_series(forcing)
    whole.run_steps(nsteps)
    row = H.scalars_to_row(whole.get_scalars())
    np.testing.assert_array_equal(row, g["scal"][nsteps - 1])
    ref = H.download_snapshot(whole, names).reshape(len(names), -1)
    whole.close()
    return row, ref


def run_grid(g, names, forcing, grid, set_grid=True):
    """rh_run_steps on every block of `grid` with a communicator; (scalar rows, stitched planes, sends through the loopback)."""
    nr = grid[0] * grid[1]
    nsteps = int(g["nsteps"])
    uid = native.comm_unique_id()
    s0, _, _ = loopback_counts()

    def rank(r):
        ctx = routed_ctx(g, names, grid, r)
        ctx.set_forcing_series(forcing)
        ctx.comm_init(uid, nr, r)
        if set_grid:
            ctx.comm_set_grid(*grid)
        ctx.run_steps(nsteps)
        row = H.scalars_to_row(ctx.get_scalars())
        snap = H.download_snapshot(ctx, names)
        ctx.close()
        return row, snap

    res = run_ranks(rank, nr)
    s1, _, _ = loopback_counts()
    return [x[0] for x in res], stitch(g, names, grid, [x[1] for x in res]), s1 - s0


def scenario_routing():
    """Device-driven routed steps on (px, py) grids: the blocks together equal the single domain bit for bit and, for the reference's
    routing cases, its golden trajectory; exactly one send per present neighbour, rank and routing in every step (+ flow direction and
    mask once); the same blocks without a communicator do not equal the single domain (water crosses the y-cuts)."""
    for case, grids in GRIDS:
        g, names, forcing = load_case(case)
        nsteps = int(g["nsteps"])
        want, ref = single_domain(g, names, forcing)
        for k, grid in enumerate(grids):
            rows, got, sends = run_grid(g, names, forcing, grid)
            for r, row in enumerate(rows):
                np.testing.assert_array_equal(row, want, err_msg=f"{case} {grid} rank {r}: scalars")
            assert np.array_equal(got, ref, equal_nan=True), f"{case} on {grid}: planes differ: {differing(names, got, ref)}"
            if case in ROUTING_CASES:
                compare(got, g[f"s{nsteps:05d}"], names, what=f"{case}: {grid} grid, routed run_steps")
            n = neighbour_count(grid)
            assert sends == (2 * nsteps + 2) * n, (case, grid, sends, n)
            print(f"routing {case}: grid {grid} == single domain{' == golden' if case in ROUTING_CASES else ''} over {nsteps} steps; "
                  f"{sends} sends = (2 x {nsteps} + 2) x {n} neighbours")
            if k == 0:   # without a communicator every block routes on its own
                snaps = []
                for r in range(grid[0] * grid[1]):
                    ctx = routed_ctx(g, names, grid, r)
                    ctx.set_forcing_series(forcing)
                    ctx.run_steps(nsteps)
                    snaps.append(H.download_snapshot(ctx, names))
                    ctx.close()
                alone = stitch(g, names, grid, snaps)
                assert not np.array_equal(alone, ref, equal_nan=True), f"{case} on {grid}: the blocks alone equal the single domain"
                print(f"routing {case}: grid {grid} without a communicator differs from the single domain in {differing(names, alone, ref)}")


def scenario_unchanged():
    """A grid set explicitly as (N, 1) is the default: the same bits and the same sends as without rh_comm_set_grid."""
    g, names, forcing = load_case("oned_routing")
    _, ref = single_domain(g, names, forcing)
    for grid in ((2, 1), (4, 1)):
        rows0, got0, sends0 = run_grid(g, names, forcing, grid, set_grid=False)
        rows1, got1, sends1 = run_grid(g, names, forcing, grid, set_grid=True)
        assert np.array_equal(got0, ref, equal_nan=True) and np.array_equal(got1, got0, equal_nan=True), grid
        np.testing.assert_array_equal(np.array(rows1), np.array(rows0))
        assert sends1 == sends0 == (2 * int(g["nsteps"]) + 2) * neighbour_count(grid), (grid, sends0, sends1)
        print(f"unchanged: grid {grid} set explicitly == default, {sends1} sends each")


def scenario_routing_by_routine():
    """rh_surface_routing, rh_subsurface_runoff and rh_subsurface_routing on the four blocks of a (2, 2) grid equal the single domain at
    the stored steps of the golden run (the exchange inside route_all)."""
    case, grid = "oned_routing", (2, 2)
    g, names, _ = load_case(case)
    steps = sorted({int(k[1:6]) for k in g.files if k.startswith("r") and k.endswith("_calculate_surface_runoff")})[:6]
    nr = grid[0] * grid[1]
    uids = {step: native.comm_unique_id() for step in steps}
    entries = ("rh_surface_routing", "rh_subsurface_runoff", "rh_subsurface_routing")

    def rank(r):
        out = []
        for step in steps:
            kp = f"r{step:05d}_calculate_infiltration"
            ctx = routed_ctx(g, names, grid, r, key=kp, scal_key=kp + "_scal")
            ctx.comm_init(uids[step], nr, r)
            ctx.comm_set_grid(*grid)
            for e in entries:
                ctx.call(e)
            out.append(H.download_snapshot(ctx, names))
            ctx.close()
        return out

    res = run_ranks(rank, nr)
    for k, step in enumerate(steps):
        kp = f"r{step:05d}_calculate_infiltration"
        whole = routed_ctx(g, names, key=kp, scal_key=kp + "_scal")
        for e in entries:
            whole.call(e)
        ref = H.download_snapshot(whole, names).reshape(len(names), -1)
        whole.close()
        got = stitch(g, names, grid, [res[r][k] for r in range(nr)])
        assert np.array_equal(got, ref, equal_nan=True), f"step {step}: planes differ: {differing(names, got, ref)}"
    print(f"routing by routine {case}: grid {grid} == single domain at {len(steps)} golden steps")


def scenario_allreduce():
    """rh_run_steps_dist (the SVAT step, no halo) on the four blocks of a (2, 2) grid: every rank holds the golden run's scalars and the
    blocks together its state."""
    g, names, forcing = load_case("svat_hetero_combo")
    grid, nsteps = (2, 2), 240
    nr = grid[0] * grid[1]
    nxl, nyl = local_shape(g, grid)
    uid = native.comm_unique_id()

    def rank(r):
        ctx = native.Context(nxl, nyl)
        H.upload_snapshot(ctx, block(g, "state0", grid, r)[0], names)
        ctx.set_scalars(H.scalars_from_row(g["scal0"]))
        ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
        ctx.set_forcing_series(forcing)
        ctx.comm_init(uid, nr, r)
        ctx.comm_set_grid(*grid)
        ctx.run_steps_dist(nsteps)
        row = H.scalars_to_row(ctx.get_scalars())
        snap = H.download_snapshot(ctx, names)
        ctx.close()
        return row, snap

    res = run_ranks(rank, nr)
    for r in range(nr):
        np.testing.assert_array_equal(res[r][0], g["scal"][nsteps - 1], err_msg=f"rank {r}: scalars")
    compare(stitch(g, names, grid, [x[1] for x in res]), g[f"s{nsteps:05d}"], names, what=f"svat_hetero_combo on {grid}, step {nsteps}")
    print(f"allreduce: grid {grid} == golden over {nsteps} steps")


def scenario_errors():
    """rh_comm_set_grid: RH_ERR_STATE without a communicator; RH_ERR_ARG when px * py is not the number of ranks or a value is below 1."""
    g, names, _ = load_case("oned_routing")
    ctx = routed_ctx(g, names, (2, 2), 0)
    lib = ctx._lib
    assert lib.rh_comm_set_grid(ctx._h, 1, 1) == RH_ERR_STATE
    ctx.close()
    uid = native.comm_unique_id()

    def rank(r):
        c = routed_ctx(g, names, (2, 2), r)
        c.comm_init(uid, 4, r)
        got = [lib.rh_comm_set_grid(c._h, px, py) for px, py in ((3, 1), (1, 2), (0, 4), (4, 0), (-2, -2), (2, 2), (4, 1), (1, 4))]
        c.close()
        return got

    for r, got in enumerate(run_ranks(rank, 4)):
        assert got == [RH_ERR_ARG] * 5 + [0] * 3, (r, got)
    print("errors: RH_ERR_STATE without a communicator, RH_ERR_ARG for a grid that is not the communicator's")


if __name__ == "__main__":
    {"routing": scenario_routing, "unchanged": scenario_unchanged, "routing_by_routine": scenario_routing_by_routine,
     "allreduce": scenario_allreduce, "errors": scenario_errors}[sys.argv[1]]()
