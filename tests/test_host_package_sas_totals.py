"""CPU: the host package's TransportTotals (roger_amd/sas_totals.py) on the oracle double with totals: a transport setup script ends
with a `.transport_totals.nc` whose records are the restatement (tests/sas_totals_reference.py) of what `state.variables.<name>` held
after every step, bit for bit; validation, file naming, `combine`."""
import os
import sys

import numpy as np
import pytest

import sas_binding as sb
import sas_totals_reference as T
import test_host_package_sas_restart as R
from sas_points_reference import PointsOracleSasContext

DAY = 86400
ITEMS = [("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s", "C_rz", ("TT_transp", "transp"), "q_ss"]
on_disk = R.on_disk


class TotalsOracleSasContext(PointsOracleSasContext):
    """The double with the four totals_* methods of `_native.SasContext`."""

    _tot = None

    def totals_configure(self, items, mask=None, capacity=4096):
        items = [(it, None) if isinstance(it, str) else tuple(it) for it in items]
        self._tot = None
        if items:
            m = None if mask is None else np.asarray(mask).reshape(-1) != 0
            self._tot = dict(items=items, mask=m, cap=int(capacity), rows=[], tags=[], ncells=self.n if m is None else int(m.sum()))

    def totals_record(self, tag=0, day=-1):
        from roger_amd._native import DAILY_INPUTS

        t, held = self._tot, self._arrays()
        row = {}
        for v, w in t["items"]:
            live = day >= 0 or (w is None and v not in DAILY_INPUTS)
            row[v if w is None else f"{v}_by_{w}"] = T.item_block(held[v], None if w is None else held[w], t["mask"], live)
        t["rows"].append(row)
        t["tags"].append(int(tag))

    def totals_count(self):
        return len(self._tot["rows"]), self._tot["ncells"]

    def totals_read(self, first, n):
        t = self._tot
        assert first >= len(t["rows"]) - t["cap"] and first + n <= len(t["rows"]), "rows overwritten or not recorded"
        out = {}
        for key in t["rows"][0] if t["rows"] else ():
            blocks = np.array([r[key] for r in t["rows"][first:first + n]]).reshape(n, -1)
            d = {"wsum": blocks[:, 0].copy(), "count": blocks[:, 1].copy()}
            if blocks.shape[1] == 5:
                d.update(sum=blocks[:, 2].copy(), min=blocks[:, 3].copy(), max=blocks[:, 4].copy())
            else:
                d["sum"] = blocks[:, 2:].copy()
            out[key] = d
        return np.array(t["tags"][first:first + n], dtype=np.int64), out

    def step(self, day):
        super().step(day)
        if self._tot is not None:
            self.totals_record(day, day)


@pytest.fixture
def made(monkeypatch):
    from roger_amd import _native

    out = []

    def make(*a, **k):
        out.append(TotalsOracleSasContext(*a, **k))
        return out[-1]

    monkeypatch.setattr(_native, "SasContext", make)
    return out


def totals_model(case, path, items=ITEMS, mask=None, capacity=4096, warmup_days=0, diagnose=False, **kw):
    """The golden setup of `case` with transport totals; `diagnose`: state.diagnostics writes the items' fields in the same run."""
    from roger_amd import roger_routine

    g, base = R.golden_model(case, warmup_days=warmup_days, **kw)

    class WithTotals(type(base)):
        @roger_routine
        def set_diagnostics(self, state):
            t = state.transport_totals
            t.mask, t.output_variables, t.base_output_path, t.capacity = mask, list(items), str(path), capacity
            if diagnose:
                d = state.diagnostics["collect"]
                d.output_variables = sorted({v for it in items for v in ((it,) if isinstance(it, str) else it)})
                d.output_frequency, d.sampling_frequency, d.base_output_path = DAY, 1, str(path)

    return g, WithTotals()


def field(state, name):
    """What `vs.<name>` holds over the interior, time level tau: (n,) or (n, width)."""
    a = np.asarray(getattr(state.variables, name))[2:-2, 2:-2]
    if "timesteps" in state.var_meta[name].dims:
        a = a[:, :, 1]
    return a.reshape(a.shape[0] * a.shape[1], *a.shape[2:])


def blocks_of(state, items, mask, live_day):
    out = {}
    for it in items:
        v, w = (it, None) if isinstance(it, str) else it
        live = live_day or (w is None and v not in T.DAILY and v != "q_ss")
        out[v if w is None else f"{v}_by_{w}"] = T.item_block(field(state, v), None if w is None else field(state, w),
                                                               None if mask is None else np.asarray(mask).reshape(-1), live)
    return out


def read_nc(path):
    from nc_util import netcdf_file

    with netcdf_file(str(path), "r", mmap=False) as f:
        return {k: np.array(v[...]) for k, v in f.variables.items()}, {k: v.dimensions for k, v in f.variables.items()}


def file_block(data, key, k):
    """Row k of item `key` of a file as the row block."""
    tail = [data[f"{key}_min"][k], data[f"{key}_max"][k]] if f"{key}_min" in data else []
    wsum = data[f"{key}_wsum"][k] if f"{key}_wsum" in data else data[f"{key}_count"][k]
    return np.concatenate([[wsum, data[f"{key}_count"][k]], np.atleast_1d(data[f"{key}_sum"][k]), tail])


def run_and_note(model, items, mask):
    notes, step = [], model.step

    def noting(state):
        step(state)
        notes.append((int(state.variables.itt), int(state.variables.time), blocks_of(state, items, mask, True)))

    model.step = noting
    model.run()
    return notes


def test_state_has_transport_totals():
    from roger_amd.sas_totals import TransportTotals
    from roger_amd.state import RogerState

    t = RogerState().transport_totals
    assert isinstance(t, TransportTotals) and not t.active and t.output_path == "{identifier}.transport_totals.nc"
    assert t.mask is None and t.capacity == 4096 and t.base_output_path is None and t.output_variables == []


@pytest.mark.parametrize("masked", [False, True])
def test_script_writes_the_restated_totals(made, on_disk, tmp_path, masked):
    g, _ = totals_model("sas_stats_a30", tmp_path)
    mask = None
    if masked:
        mask = np.ones((g.nx, g.ny), dtype=bool)
        mask[0, 0] = False
    g, model = totals_model("sas_stats_a30", tmp_path, mask=mask, capacity=2)      # (a ring shorter than the run: drained on the way)
    model.setup()
    model.warmup(repeat=0)
    first = (0, 0, blocks_of(model.state, ITEMS, mask, False))
    notes = [first] + run_and_note(model, ITEMS, mask)
    assert len(notes) == g.ndays + 1
    data, dims = read_nc(tmp_path / "GoldenSAS.transport_totals.nc")
    np.testing.assert_array_equal(data["itt"], [n[0] for n in notes])
    np.testing.assert_array_equal(data["Time"], np.array([n[1] for n in notes]) / float(DAY))
    assert int(data["ncells"].reshape(-1)[0]) == g.n - int(masked)
    for k, (_, _, blocks) in enumerate(notes):
        for key, want in blocks.items():
            assert T.same_bits(file_block(data, key, k), want), (key, k)
    assert dims["tt_q_ss_by_q_ss_sum"] == ("Time", "ages") and dims["TT_transp_by_transp_mean"] == ("Time", "nages")
    assert dims["tt_q_ss_by_q_ss_wsum"] == ("Time",) and dims["C_rz_sum"] == ("Time",) and dims["sa_s_count"] == ("Time",)
    assert "C_rz_wsum" not in data and "sa_s_min" not in data and "C_iso_q_ss_by_q_ss_max" in data
    # record 0: no day's flux yet; later days carry percolation
    assert data["C_iso_q_ss_by_q_ss_count"][0] == 0 and data["q_ss_count"][0] == 0 and data["C_rz_count"][0] == g.n - int(masked)
    assert data["C_iso_q_ss_by_q_ss_count"][1:].any() and data["tt_q_ss_by_q_ss_sum"][1:].any()
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(data["C_iso_q_ss_by_q_ss_mean"], data["C_iso_q_ss_by_q_ss_sum"] / data["C_iso_q_ss_by_q_ss_wsum"])
        np.testing.assert_array_equal(data["sa_s_mean"], data["sa_s_sum"] / data["sa_s_count"][:, None])
    # the catchment's travel time distribution sums to 1 where anything percolated
    k = int(np.flatnonzero(data["tt_q_ss_by_q_ss_wsum"] > 0)[0])
    assert abs(data["tt_q_ss_by_q_ss_mean"][k].sum() - 1.0) < 1e-12


def test_warmup_records_nothing(made, on_disk, tmp_path):
    g, model = totals_model("sas_stats_a30", tmp_path, warmup_days=2)
    model.setup()
    assert made[-1]._tot is None
    model.warmup(repeat=1)
    assert made[-1].totals_count()[0] == 1 and made[-1]._tot["tags"] == [0]
    data, _ = read_nc(tmp_path / "GoldenSAS.transport_totals.nc")
    assert list(data["itt"]) == [0]


BAD = (
    (dict(items=["sa_rz"]), NotImplementedError, "'sa_rz' would be reduced after the ageing"),
    (dict(items=[("msa_ss", "q_ss")]), NotImplementedError, "'msa_ss' would be reduced after the ageing"),
    (dict(items=["no_such_variable"]), NotImplementedError, "'no_such_variable' is not a float64 per-cell variable"),
    (dict(items=["maskCatch"]), NotImplementedError, "'maskCatch' is not a float64 per-cell variable"),
    (dict(items=[("C_rz", "C_in")]), NotImplementedError, "the weight 'C_in' of 'C_rz' is not a daily flux input"),
    (dict(items=[("C_rz", "C_ss")]), NotImplementedError, "the weight 'C_ss' of 'C_rz' is not a daily flux input"),
    (dict(items=[("C_rz", "q_ss", "transp")]), ValueError, "neither a variable's name nor a pair"),
    (dict(items=["C_rz", ("C_rz", "q_ss"), "C_rz"]), ValueError, "an item is given twice"),
    (dict(items=["C_rz"] * 33), ValueError, "33 items (at most 32)"),
    (dict(mask=np.zeros((2, 2), dtype=bool)), ValueError, "the mask holds no column"),
    (dict(mask=np.ones((3, 5), dtype=bool)), ValueError, "the mask has shape (3, 5)"),
    (dict(capacity=0), ValueError, "capacity"),
)


@pytest.mark.parametrize("kw,exc,text", BAD)
def test_refusals(made, tmp_path, kw, exc, text):
    g, model = totals_model("sas_stats_a30", tmp_path, **kw)
    with pytest.raises(exc) as e:
        model.setup()
    assert text in str(e.value), str(e.value)


def test_outside_the_transport_model_it_is_refused_and_state_totals_still_raises(made, tmp_path):
    from roger_amd import roger_routine, sas_totals
    from roger_amd.state import RogerState

    g, model = totals_model("sas_stats_a30", tmp_path, items=[])

    class AlsoTotals(type(model)):
        @roger_routine
        def set_diagnostics(self, state):
            state.totals.output_variables = ["q_ss"]

    with pytest.raises(NotImplementedError, match="totals: the offline transport model steps by the day.*state.transport_totals"):
        AlsoTotals().setup()
    state = RogerState()
    state.transport_totals.output_variables = ["C_rz"]
    with pytest.raises(NotImplementedError, match="transport_totals: the totals of the offline transport model"):
        sas_totals.initialize(state)


def hand_made(path, scale, ncells, itt=(0, 1, 2)):
    from roger_amd import sas_totals

    n = len(itt)
    k = np.arange(n, dtype=np.float64)
    items = [("C_by_q", True, {"sum": scale * (k + 0.1), "count": scale * (k + 1), "wsum": scale * (k + 0.5), "min": -scale * (k + 1), "max": scale * k}),
             ("tt_by_q", True, {"sum": scale * np.outer(k + 1, [0.1, 0.2, 0.7]), "count": scale * (k + 1), "wsum": scale * (k + 1)}),
             ("S", False, {"sum": scale * k, "count": np.full(n, float(ncells)), "min": scale + k, "max": 2 * scale + k})]
    dims, variables = sas_totals._file_variables(np.array(itt), np.array(itt, dtype=np.float64), items, ncells, "1900-01-01 00:00:00", 3)
    sas_totals._write_file(str(path), dims, variables, "hand")
    return items


def test_combine(tmp_path):
    from roger_amd import sas_totals

    paths = [tmp_path / f"hand.transport_totals.{r:04d}.nc" for r in range(3)]
    parts = [hand_made(p, s, c) for p, s, c in zip(paths, (1.0, 0.3, 7.0), (4, 2, 5))]
    out = tmp_path / "hand.transport_totals.nc"
    sas_totals.combine(paths, out)
    data, dims = read_nc(out)
    assert int(data["ncells"].reshape(-1)[0]) == 11 and list(data["itt"]) == [0, 1, 2]
    for j, name in enumerate(("C_by_q", "tt_by_q", "S")):
        for s in ("sum", "count", "wsum"):
            if s in parts[0][j][2]:
                want = (parts[0][j][2][s] + parts[1][j][2][s]) + parts[2][j][2][s]          # in rank order
                assert T.same_bits(data[f"{name}_{s}"], want), (name, s)
    assert T.same_bits(data["C_by_q_min"], -7.0 * (np.arange(3) + 1.0)) and T.same_bits(data["S_max"], 14.0 + np.arange(3))
    assert T.same_bits(data["C_by_q_mean"], data["C_by_q_sum"] / data["C_by_q_wsum"])
    assert T.same_bits(data["tt_by_q_mean"], data["tt_by_q_sum"] / data["tt_by_q_wsum"][:, None])
    assert T.same_bits(data["S_mean"], data["S_sum"] / data["S_count"])
    assert dims["tt_by_q_sum"] == ("Time", "ages") and "S_wsum" not in data and "tt_by_q_min" not in data
    hand_made(tmp_path / "other.transport_totals.0001.nc", 1.0, 2, itt=(0, 1, 3))
    with pytest.raises(ValueError, match="itt of .*other.transport_totals.0001.nc differs"):
        sas_totals.combine([paths[0], tmp_path / "other.transport_totals.0001.nc"], tmp_path / "x.nc")
    with pytest.raises(ValueError, match="no files"):
        sas_totals.combine([], tmp_path / "x.nc")


# ---- the diagnostics of the same run -------------------------------------------------------------------------------------------
def diagnosed_fields(data, name, k):
    """Record k of `name` in a state.diagnostics file -- (y, x) or (ages, y, x) -- as (n,) or (n, width) in the context's cell order."""
    a = np.asarray(data[name][k], dtype=np.float64)
    return a.T.reshape(-1) if a.ndim == 2 else a.transpose(2, 1, 0).reshape(a.shape[2] * a.shape[1], a.shape[0])


def assert_totals_restate_the_diagnostics(path, items, mask, ndays, ident="GoldenSAS"):
    """Every row of `.transport_totals.nc` is the restatement of the fields `.collect.nc` holds for that record."""
    tot, _ = read_nc(path / f"{ident}.transport_totals.nc")
    diag, _ = read_nc(path / f"{ident}.collect.nc")
    assert len(tot["itt"]) == len(diag["Time"]) == ndays + 1
    np.testing.assert_array_equal(tot["Time"], diag["Time"])
    m = None if mask is None else np.asarray(mask).reshape(-1)
    for k in range(ndays + 1):
        for it in items:
            v, w = (it, None) if isinstance(it, str) else it
            live = k > 0 or (w is None and v not in T.DAILY and v != "q_ss")          # record 0: no day's flux yet
            want = T.item_block(diagnosed_fields(diag, v, k), None if w is None else diagnosed_fields(diag, w, k), m, live)
            key = v if w is None else f"{v}_by_{w}"
            assert T.same_bits(file_block(tot, key, k), want), (key, k)
    return tot, diag


def test_totals_restate_the_diagnostics_of_the_same_run(made, on_disk, tmp_path):
    g, _ = totals_model("sas_stats_a30", tmp_path)
    mask = np.ones((g.nx, g.ny), dtype=bool)
    mask[0, 0] = False
    g, model = totals_model("sas_stats_a30", tmp_path, mask=mask, capacity=2, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    tot, _ = assert_totals_restate_the_diagnostics(tmp_path, ITEMS, mask, g.ndays)
    assert tot["tt_q_ss_by_q_ss_sum"][1:].any()


# ---- several ranks ---------------------------------------------------------------------------------------------------------------
def slab_mask(g):
    mask = np.ones((g.nx, g.ny), dtype=bool)
    mask[g.nx - 1, g.ny - 1] = False
    return mask


def _rank_worker(rank, world, port, num_proc, case, out, double):
    """One rank of a two-rank run of the golden setup with totals: its block of the grid, its own `.NNNN.nc`."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from roger_amd import runtime_settings

    runtime_settings.update(num_proc=num_proc, diskless_mode=False)
    from roger_amd import _native
    from roger_amd.distributed import get_chunk_slices

    if double:
        _native.SasContext = TotalsOracleSasContext
    g = sb.SasGolden(case)
    (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, rank)
    _, m = totals_model(case, out, mask=slab_mask(g), diagnose=False, slices=(gx, gy), global_shape=(g.nx, g.ny))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    m.state.sas_context.close()
    dist.destroy_process_group()


def two_ranks_against_the_single_domain(tmp_path, num_proc, double, offset):
    """The single domain (this process, diagnostics beside the totals) and two ranks (child processes); the ranks' files merged by
    `combine` equal the single domain's within n * 2^-52 * sum|t| per sum, counts, minima and maxima exactly."""
    import math

    import torch.multiprocessing as mp

    from roger_amd import sas_totals

    case = "sas_stats_a30"
    g = sb.SasGolden(case)
    mask = slab_mask(g)
    _, model = totals_model(case, tmp_path, mask=mask, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    model.state.sas_context.close()
    one, diag = assert_totals_restate_the_diagnostics(tmp_path, ITEMS, mask, g.ndays)
    port = 29500 + (os.getpid() % 2000) + offset + num_proc[1]
    mp.spawn(_rank_worker, args=(2, port, num_proc, case, str(tmp_path), double), nprocs=2, join=True)
    paths = [tmp_path / f"GoldenSAS.transport_totals.{r:04d}.nc" for r in range(2)]
    assert all(p.is_file() for p in paths)
    sas_totals.combine(paths, tmp_path / "combined.nc")
    two, _ = read_nc(tmp_path / "combined.nc")
    assert int(two["ncells"].reshape(-1)[0]) == int(one["ncells"].reshape(-1)[0]) == g.n - 1
    np.testing.assert_array_equal(two["itt"], one["itt"])
    m = mask.reshape(-1)
    for it in ITEMS:
        v, w = (it, None) if isinstance(it, str) else it
        key = v if w is None else f"{v}_by_{w}"
        for s in ("count", "min", "max"):
            if f"{key}_{s}" in one:
                np.testing.assert_array_equal(two[f"{key}_{s}"], one[f"{key}_{s}"], err_msg=f"{key}_{s}")
        for k in range(1, g.ndays + 1):
            val = diagnosed_fields(diag, v, k)
            wt = None if w is None else diagnosed_fields(diag, w, k)
            e = T.eligible(g.n, wt, m)
            with np.errstate(invalid="ignore"):
                t = val if wt is None else (val * wt if val.ndim == 1 else val * wt[:, None])
            t = np.where((e if val.ndim == 1 else e[:, None]) & ~np.isnan(val), t, 0.0).reshape(g.n, -1)
            a, b = np.atleast_1d(two[f"{key}_sum"][k]), np.atleast_1d(one[f"{key}_sum"][k])
            for c in range(t.shape[1]):
                assert abs(a[c] - b[c]) <= g.n * 2.0 ** -52 * math.fsum(np.abs(t[:, c])), (key, k, c)
            if wt is not None:
                assert abs(two[f"{key}_wsum"][k] - one[f"{key}_wsum"][k]) <= g.n * 2.0 ** -52 * math.fsum(np.abs(wt[e]))
    return one, two


@pytest.mark.parametrize("num_proc", [(2, 1), (1, 2)])
def test_two_ranks_write_their_files_and_combine_to_the_single_domain(made, on_disk, tmp_path, num_proc):
    two_ranks_against_the_single_domain(tmp_path, num_proc, True, 83)


def test_a_rank_without_a_masked_column_writes_nothing(made, on_disk, tmp_path, monkeypatch):
    """Ranks (2, 1), the mask inside the block of rank 0: rank 1 configures nothing and writes no file."""
    from roger_amd import runtime_settings as rs, runtime_state as rst, sas_totals

    g, _ = totals_model("sas_stats_a30", tmp_path)
    assert g.nx >= 2
    mask = np.zeros((g.nx, g.ny), dtype=bool)
    mask[0, :] = True
    g, model = totals_model("sas_stats_a30", tmp_path, mask=mask)
    model.setup()
    prev = rs.num_proc
    object.__setattr__(rs, "num_proc", (2, 1))
    try:
        monkeypatch.setattr(type(rst), "proc_rank", 1, raising=False)
        sas_totals.start(model.state)
        assert not model.state.transport_totals._on and made[-1]._tot is None and not list(tmp_path.iterdir())
    finally:
        object.__setattr__(rs, "num_proc", prev)
