"""Checkpoint / restart of the offline transport model (roger_amd/restart.py, transport branch) through the host package, the oracle
standing in for the device: a run interrupted half-way -- `write_restart`, a fresh model with `restart_input_filename`, the other half --
equals the uninterrupted run bit for bit, variables and output records; `restart_frequency` writes at the start of the due days; two
gloo ranks write the single-rank file; a file of another model is refused; h5lite's block-wise writer round-trips."""
import os
import sys

import numpy as np
import pytest

import sas_binding as sb
from oracle_sas_context import OracleSasContext
from sas_scripts import make_transport_model

HERE = os.path.dirname(os.path.abspath(__file__))
DAY = 86400
OUTPUTS = ["C_q_ss", "C_rz", "tt_q_ss", "sa_s"]


class CellOracleSasContext(OracleSasContext):
    """The oracle stand-in with the row-block transfers of the C ABI (rh_sas_upload_cells / rh_sas_download_cells)."""

    def download_cells(self, name, first_cell, n_cells):
        return self._arrays()[name][first_cell:first_cell + n_cells].copy()

    def upload_cells(self, name, first_cell, host):
        host = np.asarray(host)
        self._arrays()[name][first_cell:first_cell + host.shape[0]] = host


@pytest.fixture
def oracle_sas(monkeypatch):
    from roger_amd import _native

    monkeypatch.setattr(_native, "SasContext", CellOracleSasContext)


@pytest.fixture
def on_disk():
    from roger_amd import runtime_settings as rs

    prev = rs.diskless_mode
    object.__setattr__(rs, "diskless_mode", False)   # (runtime settings are locked once the core modules are imported)
    yield
    object.__setattr__(rs, "diskless_mode", prev)


def golden_model(case, warmup_days=0, slices=None, global_shape=None):
    """The setup class of the SAS golden vectors for `case` (isotope or anion); `slices` = (gx, gy): this rank's block of the grid."""
    g = sb.SasGolden(case)
    svat = {k[3:]: g.z[k] for k in g.z.files if k.startswith("in_")}
    sas = {f: g.z[f"sas_{f}"].reshape(g.nx, g.ny, 8) for f in sb.FLUXES}
    extra = None
    if g.tracer != "oxygen18" and g.tracer != "deuterium":
        shape = (g.nx, g.ny)
        C_IN = np.zeros(shape + (g.ndays + 1,))
        for d in range(1, g.ndays + 1):
            C_IN[:, :, d] = g.day(d, "C_in").reshape(shape)
        extra = {k: g.z[k].reshape(shape) for k in ("alpha_transp", "alpha_q", "lu_id")}
        extra["C_IN"] = C_IN
    if slices is not None:
        gx, gy = slices
        svat = {k: (v[gx, gy] if np.ndim(v) >= 2 else v) for k, v in svat.items()}
        sas = {k: v[gx, gy] for k, v in sas.items()}
        if extra is not None:
            extra = {k: v[gx, gy] for k, v in extra.items()}
    model = make_transport_model("roger_amd", svat, sas, g.ages, g.substeps, g.ndays, bool(g.stats), warmup_days=warmup_days,
                                 tracer=g.tracer, extra=extra, solver=g.solver)
    if global_shape is None:
        return g, model
    from roger_amd import roger_routine
    from roger_amd.core.operators import at, update
    from roger_amd.distributed import get_chunk_slices
    from roger_amd import runtime_settings as rs, runtime_state as rst

    class Block(type(model)):
        @roger_routine
        def set_settings(self, state):
            super().set_settings(state)
            state.settings.nx, state.settings.ny = global_shape

        @roger_routine
        def set_grid(self, state):
            super().set_grid(state)
            vs = state.variables
            nx, ny = global_shape
            g_, l_ = get_chunk_slices(nx, ny, rs.num_proc, rst.proc_rank, include_overlap=True)
            for k, n, gsl, lsl in (("x", nx, g_[0], l_[0]), ("y", ny, g_[1], l_[1])):
                full = np.zeros(n + 4)
                full[3:-2] = np.cumsum(np.ones(n - 1))
                setattr(vs, k, update(getattr(vs, k), at[lsl], full[gsl]))

    return g, Block()


def with_outputs(model, path):
    from roger_amd import roger_routine

    class WithOutput(type(model)):
        @roger_routine
        def set_diagnostics(self, state):
            d = state.diagnostics["collect"]
            d.output_variables = list(OUTPUTS)
            d.output_frequency = DAY
            d.sampling_frequency = 1
            d.base_output_path = str(path)

    os.makedirs(path, exist_ok=True)
    out = WithOutput()
    out.override_settings = dict(model.override_settings)
    return out


def read_records(path, ident):
    from nc_util import netcdf_file

    with netcdf_file(os.path.join(str(path), f"{ident}.collect.nc"), "r", mmap=False) as f:
        return {k: np.array(f.variables[k][:]) for k in ["Time"] + OUTPUTS}


def assert_same_state(a, b):
    va, vb = a.state.variables, b.state.variables
    assert int(va.itt) == int(vb.itt) and int(va.time) == int(vb.time)
    for key in a.state.var_meta:
        np.testing.assert_array_equal(np.asarray(getattr(va, key)), np.asarray(getattr(vb, key)), err_msg=key)


def split_run(tmp_path, factory, ndays, warmup, at_warmup=False):
    """(uninterrupted model, restarted model, restart file): `ndays` days after `warmup` warm-up runs, interrupted after half of them
    (or, with `at_warmup`, right after the warm-up and its rescale_SA) with a restart file in between; output records of both runs."""
    half = 0 if at_warmup else ndays // 2
    a = factory()
    a.override_settings = dict(runlen=ndays * DAY)
    a = with_outputs(a, tmp_path / "a")
    a.setup()
    a.warmup(repeat=warmup)
    a.run()
    b = factory()
    b.override_settings = dict(runlen=half * DAY, write_restart=True, restart_output_filename=str(tmp_path / "b_{itt:0>4d}.h5"))
    b = with_outputs(b, tmp_path / "b")
    b.setup()
    b.warmup(repeat=warmup)
    if not at_warmup:
        b.run()
    fname = tmp_path / f"b_{half:0>4d}.h5"
    assert fname.is_file()
    c = factory()
    c.override_settings = dict(runlen=(ndays - half) * DAY, restart_input_filename=str(fname))
    c = with_outputs(c, tmp_path / "c")
    c.setup()
    assert int(c.state.variables.itt) == half and int(c.state.variables.time) == half * DAY and c.state.settings.warmup_done
    c.run()
    return a, c, fname


def assert_records_continue(tmp_path, ident):
    ra, rb, rc = (read_records(tmp_path / t, ident) for t in "abc")
    for k in ["Time"] + OUTPUTS:
        np.testing.assert_array_equal(ra[k], np.concatenate([rb[k], rc[k]]), err_msg=k)


@pytest.mark.parametrize("case,warmup", [("sas_stats_a30", 0), ("sas_bromide_rk4_a30", 1)])
def test_interrupted_run_equals_uninterrupted(oracle_sas, on_disk, tmp_path, case, warmup):
    ndays = sb.SasGolden(case).ndays

    def factory():
        return golden_model(case, warmup_days=ndays if warmup else 0)[1]

    a, c, fname = split_run(tmp_path, factory, ndays, warmup)
    assert_same_state(a, c)
    assert_records_continue(tmp_path, a.state.settings.identifier)
    from roger_amd import h5lite

    small, stream = h5lite.open_blocks(str(fname), streamed=("sa_rz",))
    with stream:
        more = small["hip_core"]
        assert stream.shape("hip_core", "sa_rz") == (a.state.settings.nx, a.state.settings.ny, a.state.settings.ages)
        assert {"sa_ss", "msa_rz", "msa_ss", "sa_s", "msa_s"} <= set(more) and "sa_rz" not in more
        assert int(more["warmup_done"]) == 1 and "itt" in small["core"] and "time" in small["core"]
        assert not any(k in more or k in small["core"] for k in ("PREC_DIST_DAILY", "INF_MAT_RZ", "C_IN", "C_ISO_IN", "tt_q_ss", "SA_rz"))


def test_restart_right_after_the_warmup(oracle_sas, on_disk, tmp_path):
    case = "sas_warmup_a30"
    ndays = sb.SasGolden(case).ndays
    a, c, fname = split_run(tmp_path, lambda: golden_model(case, warmup_days=ndays)[1], ndays, 1, at_warmup=True)
    assert_same_state(a, c)
    assert_records_continue(tmp_path, a.state.settings.identifier)


def test_restart_frequency_writes_the_due_days(oracle_sas, on_disk, tmp_path):
    g, m = golden_model("sas_stats_a30")
    m.override_settings = dict(restart_frequency=3 * DAY, restart_output_filename=str(tmp_path / "f_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    got = sorted(p.name for p in tmp_path.glob("f_*.h5"))
    assert got == [f"f_{d:0>4d}.h5" for d in range(3, g.ndays, 3)]   # at the start of the steps of days 4, 7, 10


def test_write_restart_without_frequency_writes_nothing_else(oracle_sas, on_disk, tmp_path):
    g, m = golden_model("sas_stats_a30")
    m.override_settings = dict(write_restart=True, restart_output_filename=str(tmp_path / "w_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    assert sorted(p.name for p in tmp_path.glob("w_*.h5")) == ["w_0000.h5", f"w_{g.ndays:0>4d}.h5"]   # after warm-up, end of run()


def test_no_frequency_files_during_the_warmup(oracle_sas, on_disk, tmp_path):
    """restart_frequency writes in the run proper only: a warm-up twice as long as the run writes no file of its own."""
    g, m = golden_model("sas_warmup_a30", warmup_days=10)
    m.override_settings = dict(runlen=5 * DAY, restart_frequency=3 * DAY, restart_output_filename=str(tmp_path / "f_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=1)
    m.run()
    assert sorted(p.name for p in tmp_path.glob("f_*.h5")) == ["f_0003.h5"]
    from roger_amd import h5lite

    assert int(h5lite.read(str(tmp_path / "f_0003.h5"))["hip_core"]["warmup_done"]) == 1


def test_write_reads_no_age_resolved_variable(oracle_sas, on_disk, tmp_path, monkeypatch):
    """After day steps every age-resolved variable is newer on the device; a restart write streams them from the context and never
    fills their host mirrors (`vs.<name>` would download the whole array), the restart_frequency write included."""
    from roger_amd import restart
    from roger_amd.state import RogerVariables

    g, m = golden_model("sas_stats_a30")
    m.override_settings = dict(runlen=3 * DAY, restart_frequency=2 * DAY, write_restart=True,
                               restart_output_filename=str(tmp_path / "s_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=0)
    aged = {k for k, v in m.state.var_meta.items() if v.dims and ("ages" in v.dims or "nages" in v.dims)}
    downloads = []
    real = RogerVariables._download

    def spy(self, key):
        downloads.append(key)
        return real(self, key)

    monkeypatch.setattr(RogerVariables, "_download", spy)
    m.run()                                                  # the frequency write at the start of day 3, the final write
    restart.write_restart(m.state, filename=str(tmp_path / "again.h5"))
    assert sorted(p.name for p in tmp_path.glob("s_*.h5")) == ["s_0000.h5", "s_0002.h5", "s_0003.h5"]   # (s_0000: after warmup())
    assert not aged & set(downloads), sorted(aged & set(downloads))
    monkeypatch.setattr(RogerVariables, "_download", real)
    from roger_amd import h5lite

    small, stream = h5lite.open_blocks(str(tmp_path / "again.h5"), streamed=restart.AGE_STATE)
    with stream:
        vs = m.state.variables
        for k in restart.AGE_STATE:
            want = np.asarray(getattr(vs, k))[2:-2, 2:-2, 1]
            got = stream.get("hip_core", k, 0, want.size).reshape(want.shape)
            np.testing.assert_array_equal(got, want, err_msg=k)


def _refuse(tmp_path, override):
    g, m = golden_model("sas_stats_a30")
    m.override_settings = dict(write_restart=True, restart_output_filename=str(tmp_path / "r.h5"))
    m.setup()
    m.warmup(repeat=0)
    g, other = golden_model("sas_stats_a30")
    other.override_settings = dict(restart_input_filename=str(tmp_path / "r.h5"), **override)
    return other


def test_mismatched_files_are_refused(oracle_sas, on_disk, tmp_path):
    with pytest.raises(RuntimeError, match="age classes"):
        _refuse(tmp_path, dict(ages=20, nages=21)).setup()
    with pytest.raises(RuntimeError, match="sas_solver"):
        _refuse(tmp_path, dict(sas_solver="Euler", h=1 / 3)).setup()
    with pytest.raises(RuntimeError, match="sas_tracer"):
        _refuse(tmp_path, dict(enable_oxygen18=False, enable_bromide=True)).setup()


def test_svat_file_is_not_a_transport_file(oracle_sas, on_disk, tmp_path):
    from roger_amd import h5lite

    h5lite.write(str(tmp_path / "svat.h5"), {"core": {"itt": np.int64(3)}, "hip_core": {"prec": np.zeros((6, 6))}})
    g, m = golden_model("sas_stats_a30")
    m.override_settings = dict(restart_input_filename=str(tmp_path / "svat.h5"))
    with pytest.raises(RuntimeError, match="offline transport"):
        m.setup()


# ---- several ranks ---------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, num_proc, case, half, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from roger_amd import runtime_settings

    runtime_settings.update(num_proc=num_proc, diskless_mode=False)
    from roger_amd import _native
    from roger_amd.distributed import get_chunk_slices

    _native.SasContext = CellOracleSasContext
    g = sb.SasGolden(case)
    (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, rank)
    _, m = golden_model(case, slices=(gx, gy), global_shape=(g.nx, g.ny))
    m.override_settings = dict(runlen=half * DAY, write_restart=True, restart_output_filename=os.path.join(out, "ranks_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    # ... and read back on the same grid: every rank continues from its own cells
    _, r = golden_model(case, slices=(gx, gy), global_shape=(g.nx, g.ny))
    r.override_settings = dict(runlen=(g.ndays - half) * DAY, restart_input_filename=os.path.join(out, f"ranks_{half:0>4d}.h5"))
    r.setup()
    r.run()
    vs = r.state.variables
    np.savez(os.path.join(out, f"rank{rank}.npz"), **{k: np.asarray(getattr(vs, k))[2:-2, 2:-2] for k in ("sa_rz", "msa_ss", "C_q_ss")})
    dist.destroy_process_group()


@pytest.mark.parametrize("num_proc", [(2, 1), (1, 2)])
def test_two_ranks_write_the_single_rank_file(oracle_sas, on_disk, tmp_path, num_proc):
    import torch.multiprocessing as mp

    from roger_amd import h5lite
    from roger_amd.distributed import get_chunk_slices

    case = "sas_stats_a30"
    g = sb.SasGolden(case)
    half = g.ndays // 2
    _, m = golden_model(case)
    m.override_settings = dict(runlen=half * DAY, write_restart=True, restart_output_filename=str(tmp_path / "one_{itt:0>4d}.h5"))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    _, full = golden_model(case)
    full.setup()
    full.warmup(repeat=0)
    full.run()
    port = 29500 + (os.getpid() % 2000) + 61 + num_proc[1]
    mp.spawn(_rank_worker, args=(2, port, num_proc, case, half, str(tmp_path)), nprocs=2, join=True)
    one, two = (h5lite.read(str(tmp_path / f"{p}_{half:0>4d}.h5")) for p in ("one", "ranks"))
    assert set(one) == set(two)
    for gname in one:
        assert set(one[gname]) == set(two[gname]), gname
        for k, v in one[gname].items():
            np.testing.assert_array_equal(two[gname][k], v, err_msg=f"{gname}/{k}")
    vs = full.state.variables
    for r in range(2):   # the ranks, restarted from that file, finish the run like the single domain
        (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, r)
        d = np.load(tmp_path / f"rank{r}.npz")
        for k in d.files:
            np.testing.assert_array_equal(d[k], np.asarray(getattr(vs, k))[2:-2, 2:-2][gx, gy], err_msg=f"rank {r} {k}")


# ---- h5lite's block-wise writer --------------------------------------------------------------------------------------------------
def test_h5lite_blockwise_round_trip(tmp_path):
    from roger_amd import h5lite

    rng = np.random.default_rng(3)
    big = rng.normal(size=(9, 7, 1001))
    small = {"core": {"itt": np.int64(5), "S_rz": rng.normal(size=(13, 11, 2))}, "hip_core": {"flag": np.int64(1)}}
    groups = {"core": dict(small["core"]), "hip_core": dict(small["hip_core"], sa_rz=h5lite.Deferred(big.shape, np.float64),
                                                          msa_rz=h5lite.Deferred(big.shape, np.float64))}
    block = 17 * 1001   # elements per block: the dataset is larger than a block, and the last block is a partial one
    flat = big.reshape(-1)
    with h5lite.create(str(tmp_path / "s.h5"), groups) as f:
        for name, src in (("sa_rz", flat), ("msa_rz", -flat)):
            for first in range(0, flat.size, block):
                f.put("hip_core", name, first, src[first:first + block])
        with pytest.raises(IndexError):
            f.put("hip_core", "sa_rz", flat.size - 3, np.zeros(4))
    whole = h5lite.read(str(tmp_path / "s.h5"))   # the whole-file reader sees ordinary contiguous datasets
    np.testing.assert_array_equal(whole["hip_core"]["sa_rz"], big)
    np.testing.assert_array_equal(whole["hip_core"]["msa_rz"], -big)
    np.testing.assert_array_equal(whole["core"]["S_rz"], small["core"]["S_rz"])
    got_small, stream = h5lite.open_blocks(str(tmp_path / "s.h5"), streamed=("sa_rz",))
    with stream:
        assert stream.shape("hip_core", "sa_rz") == big.shape and "sa_rz" not in got_small["hip_core"]
        back = np.concatenate([stream.get("hip_core", "sa_rz", first, min(block, flat.size - first))
                               for first in range(0, flat.size, block)])
    np.testing.assert_array_equal(back, flat)
    assert int(got_small["core"]["itt"]) == 5 and int(got_small["hip_core"]["flag"]) == 1
    # a file without deferred datasets is what `write` makes, byte for byte
    h5lite.write(str(tmp_path / "w.h5"), small)
    h5lite.create(str(tmp_path / "c.h5"), small).close()
    assert (tmp_path / "w.h5").read_bytes() == (tmp_path / "c.h5").read_bytes()
