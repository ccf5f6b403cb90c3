"""CPU: the host package's TransportScores (roger_amd/sas_scores.py) on the oracle double with the scores_* methods
(tests/sas_scores_reference.py): a transport setup script ends with a `.transport_scores.nc` whose moments are the restatement applied
to the per-day fields that `state.diagnostics` wrote in the same run, bit for bit; the warm-up, a restart in mid-window, a series map
with columns that are not scored, two ranks, validation."""
import os
import sys

import numpy as np
import pytest

import sas_binding as sb
import sas_scores_reference as S
import test_host_package_sas_totals as HP

DAY = 86400
FILL = 9.969209968386869e36
on_disk = HP.on_disk
ITEMS = [("C_iso_q_ss", "q_ss", "bulk"), ("C_iso_rz", None, "last"), ("C_rz", None, "mean")]
WINDOWS = (np.array([1, 2, 6, 10, 12]), np.array([1, 4, 8, 11, 14]))     # model days; the last one closes beyond the 12 days of the run
FILE_MOMENTS = (("sum_sim", 3), ("sum_sim2", 4), ("sum_simobs", 5), ("sse", 6), ("sum_obs", 7), ("sum_obs2", 8))


@pytest.fixture
def made(monkeypatch):
    from roger_amd import _native

    out = []

    def make(*a, **k):
        out.append(S.ScoresOracleSasContext(*a, **k))
        return out[-1]

    monkeypatch.setattr(_native, "SasContext", make)
    return out


def observations(n_series=1, K=len(WINDOWS[0])):
    rng = np.random.default_rng(17 + n_series)
    obs = {("C_iso_q_ss", "q_ss"): -9.5 + 2.0 * rng.random((n_series, K)), "C_iso_rz": -9.0 + 2.0 * rng.random((n_series, K)),
           "C_rz": 0.0019 + 0.0002 * rng.random((n_series, K))}
    obs["C_iso_rz"][0, 1] = np.nan
    return {k: (o[0] if n_series == 1 else o) for k, o in obs.items()}


def scores_model(case, path, obs=None, windows=WINDOWS, series=None, aggregation=None, warmup_days=0, diagnose=False, **kw):
    """The golden setup of `case` with transport scores; `diagnose`: state.diagnostics writes the items' fields in the same run."""
    from roger_amd import roger_routine

    g, base = HP.R.golden_model(case, warmup_days=warmup_days, **kw)
    obs = observations() if obs is None else obs

    class WithScores(type(base)):
        @roger_routine
        def set_diagnostics(self, state):
            t = state.transport_scores
            t.observations, t.windows, t.series, t.base_output_path = dict(obs), windows, series, str(path)
            t.aggregation = ({"C_iso_rz": "last"} if "C_iso_rz" in obs else {}) if aggregation is None else aggregation
            if diagnose:
                d = state.diagnostics["collect"]
                d.output_variables = ["C_iso_q_ss", "C_iso_rz", "C_rz", "q_ss"]
                d.output_frequency, d.sampling_frequency, d.base_output_path = DAY, 1, str(path)

    return g, WithScores()


def read_attributes(path):
    from nc_util import netcdf_file

    with netcdf_file(str(path), "r", mmap=False) as f:
        return {k: getattr(f, k) for k in ("observations_dropped", "first_scored_model_day")}


def file_map(data, key):
    """A (y, x) map of the file in the context's cell order."""
    return np.asarray(data[key]).T.reshape(-1)


def assert_scores_restate_the_diagnostics(path, g, obs=None, windows=WINDOWS, series=None, day0=1, ident="GoldenSAS"):
    """The moments of `.transport_scores.nc` are the restatement applied to the fields `.collect.nc` holds for the days from model day
    `day0` on; the windows that began before it are not in the file; the metrics are `derive` of the moments."""
    from roger_amd.sas_scores import derive

    data, dims = HP.read_nc(path / f"{ident}.transport_scores.nc")
    diag, _ = HP.read_nc(path / f"{ident}.collect.nc")
    obs = observations() if obs is None else obs
    keep = windows[0] >= day0
    first, last = windows[0][keep], windows[1][keep]
    assert list(data["window_first"]) == list(first) and list(data["window_last"]) == list(last)
    o3 = np.stack([np.atleast_2d(o)[:, keep] for o in obs.values()])
    flat = None if series is None else np.asarray(series).reshape(-1)
    want = S.HostSasScores([(v, w, S.KINDS[k]) for v, w, k in ITEMS], o3, (first - day0, last - day0), g.n, flat)
    days = np.rint(np.asarray(diag["Time"])).astype(int)
    for k in np.flatnonzero(days >= day0):
        want.add({v: HP.diagnosed_fields(diag, v, k) for v in ("C_iso_q_ss", "C_iso_rz", "C_rz", "q_ss")})
    assert want.win.days == int(days.max()) - day0 + 1
    assert list(data["closed"]) == list(want.closed)
    scored = np.ones(g.n, dtype=bool) if flat is None else flat >= 0
    for j, (v, w, _) in enumerate(ITEMS):
        name = v if w is None else f"{v}_by_{w}"
        for key, m in FILE_MOMENTS:
            assert S.same_bits(file_map(data, f"{name}_{key}"), np.where(scored, want.moments[j, m], FILL)), (name, key)
            assert dims[f"{name}_{key}"] == ("y", "x")
        assert list(file_map(data, f"{name}_n")) == list(np.where(scored, want.moments[j, 2], 0).astype(int)), name
        maps = derive(want.moments[j], flat)
        for key in ("bias", "rmse", "r", "nse", "kge"):
            assert S.same_bits(file_map(data, f"{name}_{key}"), maps[key]), (name, key)
    return data


def test_state_has_transport_scores():
    from roger_amd.sas_scores import TransportScores
    from roger_amd.state import RogerState

    t = RogerState().transport_scores
    assert isinstance(t, TransportScores) and not t.active and t.output_path == "{identifier}.transport_scores.nc"
    assert t.observations == {} and t.aggregation == {} and t.windows is None and t.series is None and t.read() is None


def test_script_writes_the_restated_scores(made, on_disk, tmp_path):
    g, model = scores_model("sas_stats_a30", tmp_path, diagnose=True)
    model.setup()
    assert made[-1]._sc is None                      # nothing is configured before the run proper
    model.warmup(repeat=0)
    assert made[-1].scores_read()[2] == 0
    model.run()
    assert made[-1].scores_read()[2] == g.ndays == 12
    data = assert_scores_restate_the_diagnostics(tmp_path, g)
    assert list(data["closed"]) == [1, 1, 1, 1, 0]
    assert read_attributes(tmp_path / "GoldenSAS.transport_scores.nc") == {"observations_dropped": 0, "first_scored_model_day": 1}
    # the bulk item counts samples, and not the same number in every column or for every item: days without percolation, a missing observation
    n_bulk, n_last = data["C_iso_q_ss_by_q_ss_n"], data["C_iso_rz_n"]
    assert n_bulk.any() and n_last.max() == 3 and data["C_rz_n"].max() == 4
    assert (data["C_iso_q_ss_by_q_ss_sum_sim"][n_bulk > 0] < 0).all()      # delta values: negative sums
    got = model.state.transport_scores.read()
    assert S.same_bits(got["C_rz_sse"].T, data["C_rz_sse"]) and list(got["closed"]) == [1, 1, 1, 1, 0]


def test_a_warmup_before_the_first_window(made, on_disk, tmp_path):
    """The warm-up runs score nothing; the day count starts with the run proper."""
    g, model = scores_model("sas_stats_a30", tmp_path, warmup_days=2, diagnose=True)
    model.setup()
    model.warmup(repeat=1)
    assert made[-1].scores_read()[2] == 0 and not made[-1].scores_read()[0].any()
    model.run()
    assert made[-1].scores_read()[2] == g.ndays
    assert_scores_restate_the_diagnostics(tmp_path, g)


def test_a_restart_in_mid_window_drops_that_window(made, on_disk, tmp_path):
    """Interrupted after day 6, inside the window [6, 8]: the continued run scores from model day 7, drops the three windows that
    began before it and says so; the moments are not in the restart file."""
    g, b = scores_model("sas_stats_a30", tmp_path / "b")
    b.override_settings = dict(runlen=6 * DAY, write_restart=True, restart_output_filename=str(tmp_path / "b_{itt:0>4d}.h5"))
    b.setup()
    b.warmup(repeat=0)
    b.run()
    first, _ = HP.read_nc(tmp_path / "b" / "GoldenSAS.transport_scores.nc")
    assert list(first["closed"]) == [1, 1, 0, 0, 0]
    g, c = scores_model("sas_stats_a30", tmp_path / "c", diagnose=True)
    c.override_settings = dict(runlen=6 * DAY, restart_input_filename=str(tmp_path / "b_0006.h5"))
    c.setup()
    assert int(c.state.variables.itt) == 6 and made[-1].scores_read()[2] == 0
    c.run()
    data = assert_scores_restate_the_diagnostics(tmp_path / "c", g, day0=7)
    assert list(data["window_first"]) == [10, 12] and list(data["closed"]) == [1, 0]
    assert read_attributes(tmp_path / "c" / "GoldenSAS.transport_scores.nc") == {"observations_dropped": 3, "first_scored_model_day": 7}
    assert data["C_rz_n"].max() == 1


def test_a_series_map_with_columns_that_are_not_scored(made, on_disk, tmp_path):
    series = np.array([[1, -1], [0, 1]])
    obs = observations(2)
    g, model = scores_model("sas_stats_a30", tmp_path, obs=obs, series=series, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    data = assert_scores_restate_the_diagnostics(tmp_path, g, obs=obs, series=series)
    np.testing.assert_array_equal(data["series"], series.T)
    assert data["C_rz_n"].T[0, 1] == 0 and data["C_rz_sse"].T[0, 1] == FILL and data["C_rz_kge"].T[0, 1] == FILL
    assert data["C_rz_sse"].T[0, 0] != data["C_rz_sse"].T[1, 0]


BAD = (
    (dict(obs={"sa_rz": np.zeros(5)}), NotImplementedError, "transport_scores: 'sa_rz' is age-resolved"),
    (dict(obs={"tt_q_ss": np.zeros(5)}), NotImplementedError, "'tt_q_ss' is age-resolved"),
    (dict(obs={"no_such_variable": np.zeros(5)}), NotImplementedError, "'no_such_variable' is not a float64 per-cell variable"),
    (dict(obs={"maskCatch": np.zeros(5)}), NotImplementedError, "'maskCatch' is not a float64 per-cell variable"),
    (dict(obs={"q_ss": np.zeros(5)}), NotImplementedError, "'q_ss' is a daily input of the transport step"),
    (dict(obs={("C_rz", "C_in"): np.zeros(5)}), NotImplementedError, "the weight 'C_in' of 'C_rz' is not a daily flux input"),
    (dict(obs={("C_rz", "q_ss", "transp"): np.zeros(5)}), ValueError, "neither a variable's name nor a pair"),
    (dict(obs={"C_rz": np.zeros(5)}, aggregation={"C_rz": "bulk"}), ValueError, '\'C_rz\' is aggregated as "bulk" and has no weight'),
    (dict(obs={("C_rz", "q_ss"): np.zeros(5)}, aggregation={("C_rz", "q_ss"): "last"}), ValueError, 'aggregated as "last" and has a weight'),
    (dict(obs={"C_rz": np.zeros(5)}, aggregation={"C_rz": "sum"}), ValueError, '("bulk", "mean" or "last")'),
    (dict(obs={"C_rz": np.zeros(5)}, aggregation={"C_ss": "last"}), ValueError, "aggregation names 'C_ss', which has no observations"),
    (dict(obs={"C_rz": np.zeros(5), "C_ss": np.zeros(4)}, aggregation={}), ValueError, "the observations have shapes (1, 5), (1, 4)"),
    (dict(obs={"C_rz": np.zeros((1025, 5))}, aggregation={}), ValueError, "1025 series (at most 1024)"),
    (dict(obs={"C_rz": np.zeros(4)}, aggregation={}), ValueError, "as the observations hold 4 samples"),
    (dict(windows=None), ValueError, "windows = (first, last)"),
    (dict(windows=(np.array([1.0, 2, 6, 10, 12]), WINDOWS[1])), ValueError, "two integer arrays (5,)"),
    (dict(windows=(np.array([1, 2, 4, 10, 12]), WINDOWS[1])), ValueError, "window 2 starts on day 4, window 1 ends on day 4"),
    (dict(windows=(np.array([1, 2, 9, 10, 12]), WINDOWS[1])), ValueError, "window 2 is [9, 8]: its last day lies before its first"),
    (dict(series=np.zeros((3, 5), dtype=int)), ValueError, "the series map has shape (3, 5)"),
    (dict(series=np.zeros((2, 2))), ValueError, "the series map holds float64 values"),
    (dict(series=np.ones((2, 2), dtype=int)), ValueError, "the series map names series 1, the observations hold 1"),
    (dict(series=np.full((2, 2), -1)), ValueError, "the series map scores no column"),
)


@pytest.mark.parametrize("kw,exc,text", BAD)
def test_refusals(made, tmp_path, kw, exc, text):
    g, model = scores_model("sas_stats_a30", tmp_path, **kw)
    assert (g.nx, g.ny) == (2, 2)
    with pytest.raises(exc) as e:
        model.setup()
    assert text in str(e.value), str(e.value)


def test_too_many_items_are_refused(made, tmp_path):
    names = ["C_rz", "C_ss", "C_s", "C_iso_rz", "C_iso_ss", "C_iso_s"] + [f"C_{f}" for f in sb.FLUXES] + [f"C_iso_{f}" for f in sb.FLUXES] + ["C_inf_mat_rz"]
    g, model = scores_model("sas_stats_a30", tmp_path, obs={v: np.zeros(5) for v in names}, aggregation={})
    with pytest.raises(ValueError, match=r"transport_scores: 17 items \(at most 16\)"):
        model.setup()


def test_outside_the_transport_model_it_is_refused_and_state_scores_names_it(made, tmp_path):
    from roger_amd import roger_routine, sas_scores
    from roger_amd.state import RogerState

    g, model = scores_model("sas_stats_a30", tmp_path, obs={})

    class AlsoScores(type(model)):
        @roger_routine
        def set_diagnostics(self, state):
            state.scores.observations = {"q_ss": np.zeros(3)}

    with pytest.raises(NotImplementedError, match="scores: the offline transport model") as e:
        AlsoScores().setup()
    assert "state.transport_scores" in str(e.value)
    state = RogerState()
    state.transport_scores.observations = {"C_rz": np.zeros(3)}
    with pytest.raises(NotImplementedError, match="transport_scores: the scores of the offline transport model.*state.scores"):
        sas_scores.initialize(state)


# ---- several ranks ---------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, num_proc, case, out, series):
    """One rank of a two-rank run of the golden setup with transport scores on the double: its block, its own `.NNNN.nc`."""
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

    _native.SasContext = S.ScoresOracleSasContext
    g = sb.SasGolden(case)
    (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, rank)
    _, m = scores_model(case, out, obs=observations(2), series=series, slices=(gx, gy), global_shape=(g.nx, g.ny))
    m.setup()
    m.warmup(repeat=0)
    m.run()
    dist.destroy_process_group()


@pytest.mark.parametrize("num_proc", [(2, 1), (1, 2)])
def test_two_ranks_write_their_blocks_of_the_single_domain(made, on_disk, tmp_path, num_proc):
    """Columns do not talk to each other: each rank's file holds, bit for bit, its block of the single domain's maps."""
    import torch.multiprocessing as mp

    from roger_amd.distributed import get_chunk_slices

    case = "sas_stats_a30"
    g = sb.SasGolden(case)
    series = np.array([[1, -1], [0, 1]])
    _, model = scores_model(case, tmp_path, obs=observations(2), series=series)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    one, _ = HP.read_nc(tmp_path / "GoldenSAS.transport_scores.nc")
    port = 29500 + (os.getpid() % 2000) + 83 + num_proc[1]
    mp.spawn(_rank_worker, args=(2, port, num_proc, case, str(tmp_path), series), nprocs=2, join=True)
    for rank in range(2):
        two, _ = HP.read_nc(tmp_path / f"GoldenSAS.transport_scores.{rank:04d}.nc")
        (gx, gy), _ = get_chunk_slices(g.nx, g.ny, num_proc, rank)
        assert list(two["closed"]) == list(one["closed"])
        for key, a in one.items():
            if a.ndim == 2:
                assert two[key].dtype == a.dtype and S.same_bits(two[key].astype(np.float64), a[gy, gx].astype(np.float64)), (rank, key)
