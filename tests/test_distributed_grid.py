"""The grid split along y too (num_proc = (px, py > 1)) on CPU: `gloo` ranks, each holding the block `get_chunk_slices(nx, ny, num_proc,
rank)`, the oracle standing in for the device (OracleContext test double).  SVAT runs only: their columns never read their neighbours,
the ranks exchange the predicate words, which do not depend on the block shape.  (The routing's halo in y is device code; its tests run on
the GPU, tests/test_hip_grid_ranks.py: the oracle double's routing exchange knows the x-neighbours only.)"""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _init(rank, world, port, num_proc):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from roger_amd import runtime_settings

    runtime_settings.update(num_proc=num_proc)     # before the core is imported (locked afterwards, as in the reference)
    import oracle_binding as ob
    import oracle_context
    from roger_amd import _native

    _native.Context = oracle_context.OracleContext
    _native.plane_table = lambda: list(zip(ob.plane_names(), ob.plane_is_int()))


def _block(nx, ny, num_proc, rank):
    from roger_amd.distributed import get_chunk_slices

    (gx, gy), _ = get_chunk_slices(nx, ny, num_proc, rank)
    return gx, gy, np.arange(nx * ny).reshape(nx, ny)[gx, gy].ravel()


def _setup_worker(rank, world, port, num_proc, case, ndays, out_dir, device_hooks):
    _init(rank, world, port, num_proc)
    import svat_scripts as S
    from golden_util import load_case

    g, names, forcing = load_case(case)
    nx, ny = (int(v) for v in g["nx_ny"])
    gx, gy, sel = _block(nx, ny, num_proc, rank)
    p = {k: v[gx, gy] for k, v in S.params_from_golden(g, names).items()}
    model = S.make_model(p, forcing, ndays, global_shape=(nx, ny))
    model.setup()
    vs = model.state.variables
    assert np.asarray(vs.lu_id).shape == (nx // num_proc[0] + 4, ny // num_proc[1] + 4)
    if device_hooks:
        model.run_device(int(np.sum(g["scal"][:, 1] <= ndays * 86400)))
    else:
        model.run()
    np.savez(os.path.join(out_dir, f"setup{rank}.npz"), snap=S.snapshot_from_vs(vs, names), sel=sel,
             scal=np.array([int(vs.itt), int(vs.time), int(vs.dt_secs), int(vs.itt_day), int(vs.event_id_counter)]))
    dist.destroy_process_group()


@pytest.mark.parametrize("device_hooks", [False, True])
def test_roger_setup_on_a_2x2_grid(tmp_path, oracle, device_hooks):
    """`RogerSetup.run()` and `run_device()` with num_proc = (2, 2): the four blocks together reproduce the single-domain reference run,
    and every rank derives the same dt, event ids and forcing window."""
    from golden_util import compare, load_case

    case, ndays, num_proc = "svat_hetero_combo", 24, (2, 2)
    port = 29500 + (os.getpid() % 2000) + 41 + int(device_hooks)
    mp.spawn(_setup_worker, args=(4, port, num_proc, case, ndays, str(tmp_path), device_hooks), nprocs=4, join=True)
    g, names, _ = load_case(case)
    nsteps = int(np.sum(g["scal"][:, 1] <= ndays * 86400))
    key = f"s{nsteps:05d}"
    assert key in g.files
    gs = g["scal"][nsteps - 1]
    got = np.full_like(g[key], np.nan)
    for r in range(4):
        d = np.load(tmp_path / f"setup{r}.npz")
        np.testing.assert_array_equal(d["scal"], [gs[0], gs[1], gs[2], gs[3], gs[6]], err_msg=f"rank {r}")
        got[:, d["sel"]] = d["snap"]
    compare(got, g[key], names, what=f"RogerSetup on a {num_proc} grid, step {nsteps}")


def _per_cell_worker(rank, world, port, num_proc, case, nsteps, out_dir):
    _init(rank, world, port, num_proc)
    import svat_scripts as S
    from golden_util import load_case, load_stations, load_weights

    g, names, forcing = load_case(case)
    nx, ny = (int(v) for v in g["nx_ny"])
    gx, gy, sel = _block(nx, ny, num_proc, rank)
    p = {k: v[gx, gy] for k, v in S.params_from_golden(g, names).items()}
    w = load_weights(g)
    weights = {k: v.reshape(nx, ny)[gx, gy] for k, v in w.items()} if w else None
    stations = None
    if load_stations(g) is not None:
        stations = dict(station_ids=g["station_station_ids"], station_id=np.asarray(g["station_station_id"]).reshape(nx, ny)[gx, gy],
                        PREC=g["station_PREC"], TA=g["station_TA"], PET=g["station_PET"])
    model = S.make_model(p, forcing, len(forcing["PREC"]) // 144, global_shape=(nx, ny), weights=weights, stations=stations)
    model.setup()
    model.run_device(nsteps)
    assert model._per_cell_forcing
    vs = model.state.variables
    np.savez(os.path.join(out_dir, f"percell{rank}.npz"), snap=S.snapshot_from_vs(vs, names), sel=sel,
             scal=np.array([int(vs.itt), int(vs.time), int(vs.dt_secs), int(vs.itt_day)]))
    dist.destroy_process_group()


@pytest.mark.parametrize("case,nsteps", [("svat_eberbaechle_weights", 100), ("svat_stations", 120)])
def test_per_cell_forcing_on_a_y_split(tmp_path, oracle, case, nsteps):
    """Station weights / several stations (4 x 3) with num_proc = (1, 3): every rank holds one row of cells along y, the step length
    is decided by the columns of all three (the three-phase protocol of run_device); the blocks reproduce the reference's run."""
    from golden_util import compare, load_case

    num_proc = (1, 3)
    port = 29500 + (os.getpid() % 2000) + 43 + (case == "svat_stations")
    mp.spawn(_per_cell_worker, args=(3, port, num_proc, case, nsteps, str(tmp_path)), nprocs=3, join=True)
    g, names, _ = load_case(case)
    gs = g["scal"][nsteps - 1]
    got = np.full_like(g[f"s{nsteps:05d}"], np.nan)
    for r in range(3):
        d = np.load(tmp_path / f"percell{r}.npz")
        np.testing.assert_array_equal(d["scal"], [gs[0], gs[1], gs[2], gs[3]], err_msg=f"rank {r}")
        got[:, d["sel"]] = d["snap"]
    compare(got, g[f"s{nsteps:05d}"], names, what=f"{case} on a {num_proc} grid, step {nsteps}")


def _restart_model(case, ndays, template, global_shape=None, block=None):
    import svat_scripts as S
    from golden_util import load_case

    g, names, forcing = load_case(case)
    p = S.params_from_golden(g, names)
    if block is not None:
        p = {k: v[block] for k, v in p.items()}
    model = S.make_model(p, forcing, ndays, global_shape=global_shape)
    model.override_settings = dict(write_restart=True, restart_output_filename=template)
    return model


def _restart_worker(rank, world, port, num_proc, case, ndays, template):
    _init(rank, world, port, num_proc)
    from golden_util import load_case

    g, _, _ = load_case(case)
    nx, ny = (int(v) for v in g["nx_ny"])
    gx, gy, _ = _block(nx, ny, num_proc, rank)
    model = _restart_model(case, ndays, template, global_shape=(nx, ny), block=(gx, gy))
    model.setup()
    model.run()       # the restart file is written at the end of run(), by rank 0 with the gathered global arrays
    dist.destroy_process_group()


def test_restart_of_a_2x2_run(tmp_path, monkeypatch, oracle):
    """The restart file rank 0 writes for a num_proc = (2, 2) run holds the same global arrays (ghost frame included) as the file of
    the one-rank run at the same step.  (The 1-d coordinates x and y are not gathered on any multi-rank run -- restart.collect gathers
    the (x, y, ...) variables --, so they are rank 0's own here as with num_proc = (N, 1).)"""
    import oracle_context as OC
    from roger_amd import _native, h5lite

    case, ndays = "svat_hetero_combo", 2
    port = 29500 + (os.getpid() % 2000) + 47
    mp.spawn(_restart_worker, args=(4, port, (2, 2), case, ndays, str(tmp_path / "grid_{itt:0>4d}.restart.h5")), nprocs=4, join=True)
    monkeypatch.setattr(_native, "Context", OC.OracleContext)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    one = _restart_model(case, ndays, str(tmp_path / "one_{itt:0>4d}.restart.h5"))
    one.setup()
    one.run()
    n = int(one.state.variables.itt)
    a = h5lite.read(tmp_path / f"grid_{n:0>4d}.restart.h5")
    b = h5lite.read(tmp_path / f"one_{n:0>4d}.restart.h5")
    assert set(a) == set(b) and len(a["core"]) > 100
    for grp in b:
        assert set(a[grp]) == set(b[grp]), grp
        for k in b[grp]:
            if grp == "core" and k in ("x", "y"):
                continue
            x, y = np.asarray(a[grp][k]), np.asarray(b[grp][k])
            assert x.shape == y.shape and x.dtype == y.dtype, (grp, k, x.shape, y.shape)
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (grp, k)
