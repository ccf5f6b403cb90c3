"""CPU: the host package's TransportZonalTotals (roger_amd/sas_zonal_totals.py) on the oracle double with the zonal_* methods
(tests/sas_zonal_reference.py): a transport setup script ends with a `.transport_zonal_totals.nc` whose block (record, zone z, item) is
the totals' rule (tests/sas_totals_reference.py) with mask = (zones == z) of what `state.variables.<name>` held after every step, bit
for bit; validation, file naming, `combine`."""
import os
import sys

import numpy as np
import pytest

import sas_binding as sb
import sas_totals_reference as T
import sas_zonal_reference as Z
import test_host_package_sas_totals as HP

DAY = 86400
FILL = 9.969209968386869e36
ITEMS = HP.ITEMS
on_disk = HP.on_disk


@pytest.fixture
def made(monkeypatch):
    from roger_amd import _native

    out = []

    def make(*a, **k):
        out.append(Z.ZonalOracleSasContext(*a, **k))
        return out[-1]

    monkeypatch.setattr(_native, "SasContext", make)
    return out


def zone_map(g):
    """Ids 7, 3 and 12 as a script gives them (so the file's zone list is 3, 7, 12), 0 and -4 outside."""
    zones = np.array([7, 3, 12])[np.arange(g.nx * g.ny) % 3].reshape(g.nx, g.ny)
    zones[0, 0] = 0
    if g.nx * g.ny > 4:
        zones[-1, -1] = -4
    return zones


def zonal_model(case, path, items=ITEMS, zones=None, capacity=None, warmup_days=0, diagnose=False, totals_too=False, **kw):
    """The golden setup of `case` with transport zonal totals; `diagnose`: state.diagnostics writes the items' fields in the same run."""
    from roger_amd import roger_routine

    g, base = HP.R.golden_model(case, warmup_days=warmup_days, **kw)

    class WithZonal(type(base)):
        @roger_routine
        def set_diagnostics(self, state):
            t = state.transport_zonal_totals
            t.zones, t.output_variables, t.base_output_path, t.capacity = zones, list(items), str(path), capacity
            if totals_too:
                o = state.transport_totals
                o.output_variables, o.base_output_path, o.capacity = list(items), str(path), 3
            if diagnose:
                d = state.diagnostics["collect"]
                d.output_variables = sorted({v for it in items for v in ((it,) if isinstance(it, str) else it)})
                d.output_frequency, d.sampling_frequency, d.base_output_path = DAY, 1, str(path)

    return g, WithZonal()


def file_block(data, key, k, z):
    """Record k, zone z of item `key` of a file as the row block, `_FillValue` taken back where nothing was counted."""
    count = data[f"{key}_count"][k, z]
    tail = []
    if f"{key}_min" in data:
        tail = [data[f"{key}_min"][k, z], data[f"{key}_max"][k, z]]
        if count == 0:
            assert tail == [FILL, FILL], (key, k, z)
            tail = [np.inf, -np.inf]
    if count == 0:
        assert (np.atleast_1d(data[f"{key}_mean"][k, z]) == FILL).all(), (key, k, z)
    wsum = data[f"{key}_wsum"][k, z] if f"{key}_wsum" in data else count
    return np.concatenate([[wsum, count], np.atleast_1d(data[f"{key}_sum"][k, z]), tail])


def blocks_of(state, items, zones, live_day):
    """{item: {zone id: block}} of what the state holds, by the totals' rule with mask = (zones == id)."""
    ids = np.unique(zones[zones > 0])
    return {key: {int(i): blk[key] for i, blk in ((i, HP.blocks_of(state, items, zones == i, live_day)) for i in ids)}
            for key in (it if isinstance(it, str) else f"{it[0]}_by_{it[1]}" for it in items)}


def test_state_has_transport_zonal_totals():
    from roger_amd.sas_zonal_totals import TransportZonalTotals
    from roger_amd.state import RogerState

    t = RogerState().transport_zonal_totals
    assert isinstance(t, TransportZonalTotals) and not t.active and t.output_path == "{identifier}.transport_zonal_totals.nc"
    assert t.zones is None and t.capacity is None and t.base_output_path is None and t.output_variables == []


def test_script_writes_the_restated_zonal_totals(made, on_disk, tmp_path):
    g, _ = zonal_model("sas_stats_a30", tmp_path)
    zones = zone_map(g)
    g, model = zonal_model("sas_stats_a30", tmp_path, zones=zones, capacity=2, totals_too=True)   # (a ring shorter than the run)
    model.setup()
    model.warmup(repeat=0)
    notes, step = [(0, 0, blocks_of(model.state, ITEMS, zones, False))], model.step

    def noting(state):
        step(state)
        notes.append((int(state.variables.itt), int(state.variables.time), blocks_of(state, ITEMS, zones, True)))

    model.step = noting
    model.run()
    assert len(notes) == g.ndays + 1
    data, dims = HP.read_nc(tmp_path / "GoldenSAS.transport_zonal_totals.nc")
    np.testing.assert_array_equal(data["itt"], [n[0] for n in notes])
    np.testing.assert_array_equal(data["Time"], np.array([n[1] for n in notes]) / float(DAY))
    ids = [3, 7, 12]
    assert list(data["zone"]) == ids and list(data["ncells"]) == [int((zones == i).sum()) for i in ids]
    for k, (_, _, blocks) in enumerate(notes):
        for key, per_zone in blocks.items():
            for z, i in enumerate(ids):
                assert T.same_bits(file_block(data, key, k, z), per_zone[i]), (key, k, i)
    assert dims["tt_q_ss_by_q_ss_sum"] == ("Time", "zone", "ages") and dims["TT_transp_by_transp_mean"] == ("Time", "zone", "nages")
    assert dims["tt_q_ss_by_q_ss_wsum"] == ("Time", "zone") and dims["C_rz_sum"] == ("Time", "zone") and dims["sa_s_count"] == ("Time", "zone")
    assert dims["ncells"] == ("zone",) and dims["C_iso_q_ss_by_q_ss_min"] == ("Time", "zone")
    assert "C_rz_wsum" not in data and "sa_s_min" not in data
    # record 0: no day's flux yet; later days carry percolation
    assert not data["C_iso_q_ss_by_q_ss_count"][0].any() and not data["q_ss_count"][0].any() and list(data["C_rz_count"][0]) == list(data["ncells"])
    assert data["C_iso_q_ss_by_q_ss_count"][1:].any() and data["tt_q_ss_by_q_ss_sum"][1:].any()
    some = data["C_iso_q_ss_by_q_ss_count"] > 0
    np.testing.assert_array_equal(data["C_iso_q_ss_by_q_ss_mean"][some], (data["C_iso_q_ss_by_q_ss_sum"] / data["C_iso_q_ss_by_q_ss_wsum"])[some])
    np.testing.assert_array_equal(data["sa_s_mean"], data["sa_s_sum"] / data["sa_s_count"][:, :, None])
    # a zone's travel time distribution sums to 1 where anything percolated
    k, z = np.argwhere(data["tt_q_ss_by_q_ss_wsum"] > 0)[0]
    assert abs(data["tt_q_ss_by_q_ss_mean"][k, z].sum() - 1.0) < 1e-12
    # beside the one-mask recorder: both files of the same run, the zones' counts add up to the unmasked count of the inside cells
    tot, _ = HP.read_nc(tmp_path / "GoldenSAS.transport_totals.nc")
    assert len(tot["itt"]) == len(data["itt"]) and (data["sa_s_count"].sum(axis=1) == tot["sa_s_count"] - int((zones <= 0).sum())).all()


def test_default_capacity_and_the_zone_ids(made, on_disk, tmp_path):
    from roger_amd import sas_zonal_totals

    g, _ = zonal_model("sas_stats_a30", tmp_path)
    g, model = zonal_model("sas_stats_a30", tmp_path, zones=zone_map(g))
    model.setup()
    t = model.state.transport_zonal_totals
    elems = 5 + (2 + g.ages) + (2 + g.ages) + 5 + (2 + g.ages + 1) + 5
    assert t.capacity == min(4096, (64 << 20) // (3 * elems * 8)) and list(t._ids) == [3, 7, 12]
    assert sas_zonal_totals.default_capacity(1024, 32 * 1003) == 1 and sas_zonal_totals.default_capacity(1, 5) == 4096


def test_warmup_records_nothing(made, on_disk, tmp_path):
    g, _ = zonal_model("sas_stats_a30", tmp_path)
    g, model = zonal_model("sas_stats_a30", tmp_path, zones=zone_map(g), warmup_days=2)
    model.setup()
    assert made[-1]._zon is None
    model.warmup(repeat=1)
    assert made[-1].zonal_count()[0] == 1 and made[-1]._zon["tags"] == [0]
    data, _ = HP.read_nc(tmp_path / "GoldenSAS.transport_zonal_totals.nc")
    assert list(data["itt"]) == [0]


BAD = (
    (dict(items=["sa_rz"]), NotImplementedError, "transport_zonal_totals: 'sa_rz' would be reduced after the ageing"),
    (dict(items=["no_such_variable"]), NotImplementedError, "'no_such_variable' is not a float64 per-cell variable"),
    (dict(items=["maskCatch"]), NotImplementedError, "'maskCatch' is not a float64 per-cell variable"),
    (dict(items=[("C_rz", "C_in")]), NotImplementedError, "the weight 'C_in' of 'C_rz' is not a daily flux input"),
    (dict(items=[("C_rz", "q_ss", "transp")]), ValueError, "neither a variable's name nor a pair"),
    (dict(items=["C_rz", ("C_rz", "q_ss"), "C_rz"]), ValueError, "transport_zonal_totals: an item is given twice"),
    (dict(items=["C_rz"] * 33), ValueError, "33 items (at most 32)"),
    (dict(zones=np.zeros((2, 2), dtype=int)), ValueError, "the zone map holds no column in any zone"),
    (dict(zones=np.ones((3, 5), dtype=int)), ValueError, "the zone map has shape (3, 5)"),
    (dict(zones=np.ones((2, 2))), ValueError, "the zone map holds float64 values"),
    (dict(capacity=0), ValueError, "capacity"),
)


@pytest.mark.parametrize("kw,exc,text", BAD)
def test_refusals(made, tmp_path, kw, exc, text):
    g, _ = zonal_model("sas_stats_a30", tmp_path)
    assert (g.nx, g.ny) == (2, 2)
    args = dict(zones=zone_map(g))
    args.update(kw)
    g, model = zonal_model("sas_stats_a30", tmp_path, **args)
    with pytest.raises(exc) as e:
        model.setup()
    assert text in str(e.value), str(e.value)


def test_too_many_zones_are_refused(made, tmp_path):
    from roger_amd import sas_zonal_totals

    g, model = zonal_model("sas_stats_a30", tmp_path, items=[])
    model.setup()
    state = model.state
    with state.settings.unlock():
        state.settings.nx, state.settings.ny = 41, 25
    t = state.transport_zonal_totals
    t.output_variables, t.zones = ["C_rz"], np.arange(1, 1026).reshape(41, 25)
    with pytest.raises(ValueError, match=r"1025 zones \(at most 1024\)"):
        sas_zonal_totals.initialize(state)


def test_outside_the_transport_model_it_is_refused_and_state_zonal_totals_still_raises(made, tmp_path):
    from roger_amd import roger_routine, sas_zonal_totals
    from roger_amd.state import RogerState

    g, model = zonal_model("sas_stats_a30", tmp_path, items=[])

    class AlsoZonal(type(model)):
        @roger_routine
        def set_diagnostics(self, state):
            state.zonal_totals.output_variables, state.zonal_totals.zones = ["q_ss"], np.ones((g.nx, g.ny), dtype=int)

    with pytest.raises(NotImplementedError, match="offline transport.*transport_totals") as e:
        AlsoZonal().setup()
    assert "state.transport_zonal_totals" in str(e.value)
    state = RogerState()
    state.transport_zonal_totals.output_variables, state.transport_zonal_totals.zones = ["C_rz"], np.ones((2, 2), dtype=int)
    with pytest.raises(NotImplementedError, match="transport_zonal_totals: the zonal totals of the offline transport model.*state.zonal_totals"):
        sas_zonal_totals.initialize(state)


def hand_made(path, scale, ncells, itt=(0, 1, 2), ids=(3, 7)):
    """A file of two zones; with scale < 0 the rank counted nothing in zone 7."""
    from roger_amd import sas_totals, sas_zonal_totals

    n = len(itt)
    k = np.arange(n, dtype=np.float64)[:, None] + np.array([0.0, 0.25])[None, :]
    a = abs(scale)
    on = np.array([1.0, 0.0 if scale < 0 else 1.0])[None, :]
    items = [("C_by_q", True, {"sum": a * (k + 0.1) * on, "count": a * (k + 1) * on, "wsum": a * (k + 0.5) * on,
                               "min": np.where(on > 0, -a * (k + 1), np.inf), "max": np.where(on > 0, a * k, -np.inf)}),
             ("tt_by_q", True, {"sum": (a * (k + 1) * on)[:, :, None] * np.array([0.1, 0.2, 0.7]), "count": a * (k + 1) * on, "wsum": a * (k + 1) * on}),
             ("S", False, {"sum": a * k * on, "count": np.broadcast_to(np.asarray(ncells, dtype=np.float64) * on, k.shape).copy(),
                           "min": np.where(on > 0, a + k, np.inf), "max": np.where(on > 0, 2 * a + k, -np.inf)})]
    dims, variables = sas_zonal_totals._file_variables(np.array(itt), np.array(itt, dtype=np.float64), items, ids, np.asarray(ncells) * on[0].astype(int),
                                                       "1900-01-01 00:00:00", 3)
    sas_totals._write_file(str(path), dims, variables, "hand")
    return items


def test_combine(tmp_path):
    from roger_amd import sas_zonal_totals

    paths = [tmp_path / f"hand.transport_zonal_totals.{r:04d}.nc" for r in range(3)]
    parts = [hand_made(p, s, c) for p, s, c in zip(paths, (1.0, -0.3, 7.0), ((4, 1), (2, 3), (5, 2)))]
    raw, _ = HP.read_nc(paths[1])
    assert (raw["C_by_q_min"][:, 1] == FILL).all() and (raw["S_mean"][:, 1] == FILL).all() and (raw["C_by_q_min"][:, 0] != FILL).all()
    out = tmp_path / "hand.transport_zonal_totals.nc"
    sas_zonal_totals.combine(paths, out)
    data, dims = HP.read_nc(out)
    assert list(data["ncells"]) == [11, 3] and list(data["itt"]) == [0, 1, 2] and list(data["zone"]) == [3, 7]
    for j, name in enumerate(("C_by_q", "tt_by_q", "S")):
        for s in ("sum", "count", "wsum"):
            if s in parts[0][j][2]:
                want = (parts[0][j][2][s] + parts[1][j][2][s]) + parts[2][j][2][s]          # in rank order
                assert T.same_bits(data[f"{name}_{s}"], want), (name, s)
    k = np.arange(3, dtype=np.float64)
    assert T.same_bits(data["C_by_q_min"][:, 0], -7.0 * (k + 1.0)) and T.same_bits(data["S_max"][:, 1], 14.0 + k + 0.25)
    assert T.same_bits(data["C_by_q_min"][:, 1], -7.0 * (k + 1.25))                     # (rank 1 counted nothing in zone 7)
    assert T.same_bits(data["C_by_q_mean"], data["C_by_q_sum"] / data["C_by_q_wsum"])
    assert T.same_bits(data["tt_by_q_mean"], data["tt_by_q_sum"] / data["tt_by_q_wsum"][:, :, None])
    assert dims["tt_by_q_sum"] == ("Time", "zone", "ages") and "S_wsum" not in data and "tt_by_q_min" not in data
    hand_made(tmp_path / "other.0001.nc", 1.0, (2, 2), itt=(0, 1, 3))
    with pytest.raises(ValueError, match="itt of .*other.0001.nc differs"):
        sas_zonal_totals.combine([paths[0], tmp_path / "other.0001.nc"], tmp_path / "x.nc")
    hand_made(tmp_path / "zones.0001.nc", 1.0, (2, 2), ids=(3, 8))
    with pytest.raises(ValueError, match="zone of .*zones.0001.nc differs"):
        sas_zonal_totals.combine([paths[0], tmp_path / "zones.0001.nc"], tmp_path / "x.nc")
    with pytest.raises(ValueError, match="no files"):
        sas_zonal_totals.combine([], tmp_path / "x.nc")


# ---- the diagnostics of the same run -------------------------------------------------------------------------------------------
def assert_zonal_restate_the_diagnostics(path, items, zones, ndays, ident="GoldenSAS"):
    """Every block of `.transport_zonal_totals.nc` is the totals' rule with mask = (zones == id) applied to the fields `.collect.nc`
    holds for that record (after HP.assert_totals_restate_the_diagnostics)."""
    zon, _ = HP.read_nc(path / f"{ident}.transport_zonal_totals.nc")
    diag, _ = HP.read_nc(path / f"{ident}.collect.nc")
    assert len(zon["itt"]) == len(diag["Time"]) == ndays + 1
    np.testing.assert_array_equal(zon["Time"], diag["Time"])
    ids = np.unique(zones[zones > 0])
    assert list(zon["zone"]) == list(ids)
    for k in range(ndays + 1):
        for it in items:
            v, w = (it, None) if isinstance(it, str) else it
            live = k > 0 or (w is None and v not in T.DAILY and v != "q_ss")          # record 0: no day's flux yet
            key = v if w is None else f"{v}_by_{w}"
            for z, i in enumerate(ids):
                want = T.item_block(HP.diagnosed_fields(diag, v, k), None if w is None else HP.diagnosed_fields(diag, w, k),
                                    (zones == i).reshape(-1), live)
                assert T.same_bits(file_block(zon, key, k, z), want), (key, k, i)
    return zon, diag


def test_zonal_totals_restate_the_diagnostics_of_the_same_run(made, on_disk, tmp_path):
    g, _ = zonal_model("sas_stats_a30", tmp_path)
    zones = zone_map(g)
    g, model = zonal_model("sas_stats_a30", tmp_path, zones=zones, capacity=2, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    zon, _ = assert_zonal_restate_the_diagnostics(tmp_path, ITEMS, zones, g.ndays)
    assert zon["tt_q_ss_by_q_ss_sum"][1:].any()


# ---- several ranks ---------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, num_proc, case, out, double):
    """One rank of a two-rank run of the golden setup with zonal totals: its block of the grid, its own `.NNNN.nc`."""
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
        _native.SasContext = Z.ZonalOracleSasContext
    g = sb.SasGolden(case)
    (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, rank)
    _, m = zonal_model(case, out, zones=zone_map(g), slices=(gx, gy), global_shape=(g.nx, g.ny))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    m.state.sas_context.close()
    dist.destroy_process_group()


def two_ranks_against_the_single_domain(tmp_path, num_proc, double, offset):
    """The single domain (this process, diagnostics beside the recorder) and two ranks (child processes); the ranks' files merged by
    `combine` equal the single domain's within n * 2^-52 * sum|t| per sum -- the bound of the two orders -- counts, minima and maxima
    exactly."""
    import math

    import torch.multiprocessing as mp

    from roger_amd import sas_zonal_totals

    case = "sas_stats_a30"
    g = sb.SasGolden(case)
    zones = zone_map(g)
    _, model = zonal_model(case, tmp_path, zones=zones, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    model.state.sas_context.close()
    one, diag = assert_zonal_restate_the_diagnostics(tmp_path, ITEMS, zones, g.ndays)
    port = 29500 + (os.getpid() % 2000) + offset + num_proc[1]
    mp.spawn(_rank_worker, args=(2, port, num_proc, case, str(tmp_path), double), nprocs=2, join=True)
    paths = [tmp_path / f"GoldenSAS.transport_zonal_totals.{r:04d}.nc" for r in range(2)]
    assert all(p.is_file() for p in paths)
    sas_zonal_totals.combine(paths, tmp_path / "combined.nc")
    two, _ = HP.read_nc(tmp_path / "combined.nc")
    np.testing.assert_array_equal(two["ncells"], one["ncells"])
    np.testing.assert_array_equal(two["itt"], one["itt"])
    np.testing.assert_array_equal(two["zone"], one["zone"])
    for it in ITEMS:
        v, w = (it, None) if isinstance(it, str) else it
        key = v if w is None else f"{v}_by_{w}"
        for s in ("count", "min", "max"):
            if f"{key}_{s}" in one:
                np.testing.assert_array_equal(two[f"{key}_{s}"], one[f"{key}_{s}"], err_msg=f"{key}_{s}")
        for k in range(1, g.ndays + 1):
            val = HP.diagnosed_fields(diag, v, k)
            wt = None if w is None else HP.diagnosed_fields(diag, w, k)
            for z, i in enumerate(one["zone"]):
                e = T.eligible(g.n, wt, (zones == i).reshape(-1))
                with np.errstate(invalid="ignore"):
                    t = val if wt is None else (val * wt if val.ndim == 1 else val * wt[:, None])
                t = np.where((e if val.ndim == 1 else e[:, None]) & ~np.isnan(val), t, 0.0).reshape(g.n, -1)
                a, b = np.atleast_1d(two[f"{key}_sum"][k, z]), np.atleast_1d(one[f"{key}_sum"][k, z])
                for c in range(t.shape[1]):
                    assert abs(a[c] - b[c]) <= g.n * 2.0 ** -52 * math.fsum(np.abs(t[:, c])), (key, k, i, c)
                if wt is not None:
                    assert abs(two[f"{key}_wsum"][k, z] - one[f"{key}_wsum"][k, z]) <= g.n * 2.0 ** -52 * math.fsum(np.abs(wt[e]))
    return one, two


@pytest.mark.parametrize("num_proc", [(2, 1), (1, 2)])
def test_two_ranks_write_their_files_and_combine_to_the_single_domain(made, on_disk, tmp_path, num_proc):
    two_ranks_against_the_single_domain(tmp_path, num_proc, True, 61)


def test_a_rank_without_a_zone_column_writes_nothing(made, on_disk, tmp_path, monkeypatch):
    """Ranks (2, 1), every zone inside the block of rank 0: rank 1 configures nothing and writes no file."""
    from roger_amd import runtime_settings as rs, runtime_state as rst, sas_zonal_totals

    g, _ = zonal_model("sas_stats_a30", tmp_path)
    assert g.nx >= 2
    zones = np.zeros((g.nx, g.ny), dtype=int)
    zones[0, :] = 5
    g, model = zonal_model("sas_stats_a30", tmp_path, zones=zones)
    model.setup()
    prev = rs.num_proc
    object.__setattr__(rs, "num_proc", (2, 1))
    try:
        monkeypatch.setattr(type(rst), "proc_rank", 1, raising=False)
        sas_zonal_totals.start(model.state)
        assert not model.state.transport_zonal_totals._on and made[-1]._zon is None and not list(tmp_path.iterdir())
    finally:
        object.__setattr__(rs, "num_proc", prev)
