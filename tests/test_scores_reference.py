"""CPU: the scores' device rule restated (tests/scores_reference.py) on hand-worked step sequences, the order of its operations pinned by
values that another order or a fused multiply-add sums differently, the host package's derivation (roger_amd/scores.py: derive) against a
two-pass numpy computation of the same interval series, the twin, and the host package's Scores on the oracle double: a RogerSetup
script ends with a `.scores.nc` whose maps are `derive` of the restatement over the double's own planes."""
import types
from fractions import Fraction

import numpy as np
import pytest

from golden_util import load_case
from scores_reference import LAST, SUM, HostScores, ScoresOracleContext, clock, interval_series

EPS = np.finfo(np.float64).eps
B = 2.0 ** 60      # B + 1 == B in float64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def mixed_steps(ncol=1):
    """Day 0: six 10-minute steps and 23 hourly ones; day 1: one daily step; day 2: 24 hourly steps.  Step idx holds (idx + 1) * (c + 1)
    in column c."""
    lengths = [600] * 6 + [3600] * 23 + [86400] + [3600] * 24
    steps, t = [], 0
    for idx, dt in enumerate(lengths):
        steps.append((t, t + dt, (idx + 1.0) * (np.arange(ncol) + 1.0)))
        t += dt
    assert t == 3 * 86400 and len(steps) == 54
    return steps


def run(steps, kinds, obs, n, **kw):
    h = HostScores(kinds, obs, n, **kw)
    for t0, t1, v in steps:
        h.add(t0, t1, [v] * len(kinds))
    return h


def test_clock():
    assert clock(0, 600, 3600, 0, 5) == (True, False, -1, False)
    assert clock(3000, 3600, 3600, 0, 5) == (False, True, 0, True)
    assert clock(3600, 7200, 3600, 0, 1) == (True, True, 1, False)           # k at n_intervals
    assert clock(3600, 7200, 3600, 7200, 5) == (True, True, -1, False)       # k below 0
    assert clock(86400, 172800, 3600, 0, 100)[1:] == (False, 47, False)      # a daily step closes no hour
    assert clock(86400, 172800, 86400, 86400, 3) == (True, True, 0, True)


def test_daily_interval_over_mixed_steps_sum_against_last():
    steps = mixed_steps()
    obs = np.array([[[400.0, np.nan, 1000.0]], [[20.0, np.nan, 50.0]]])      # (items: SUM, LAST; one series; three days), day 1 missing
    h = run(steps, [SUM, LAST], obs, 1)
    assert list(h.closed) == [1, 1, 1]                                       # (a missing observation does not unclose the interval)
    # SUM: day 0 = 1 + ... + 29 = 435, day 1 = 30 (not scored: NaN), day 2 = 31 + ... + 54 = 1020
    assert list(h.moments[0, :, 0]) == [1020.0, 435.0 + 1020.0, 435.0 ** 2 + 1020.0 ** 2, 435.0 * 400 + 1020.0 * 1000, 35.0 ** 2 + 20.0 ** 2]
    # LAST: day 0 = 29, day 2 = 54; its acc plane stays +0.0
    assert list(h.moments[1, :, 0]) == [0.0, 29.0 + 54.0, 29.0 ** 2 + 54.0 ** 2, 29.0 * 20 + 54.0 * 50, 9.0 ** 2 + 4.0 ** 2]
    assert not np.signbit(h.moments[1, 0, 0])


def test_hourly_interval_the_hours_under_a_daily_step_stay_unclosed():
    steps = mixed_steps()
    h = run(steps, [SUM, LAST], np.zeros((2, 1, 72)), 1, interval=3600)
    assert list(h.closed) == [1] * 24 + [0] * 24 + [1] * 24
    # hour 0 = 1 + ... + 6 = 21, hours 1 ... 23 = 7 ... 29, hours 48 ... 71 = 31 ... 54
    assert h.moments[0, 1, 0] == 21 + 414 + 1020 and h.moments[0, 2, 0] == 21 ** 2 + sum(v * v for v in range(7, 30)) + sum(v * v for v in range(31, 55))
    assert h.moments[0, 3, 0] == 0 and h.moments[0, 4, 0] == h.moments[0, 2, 0]
    assert h.moments[1, 1, 0] == 6 + 414 + 1020                              # LAST: hour 0 ends with step 6
    assert h.moments[0, 0, 0] == 54.0


def test_a_start_in_mid_run_and_intervals_beyond_the_observations():
    steps = mixed_steps()
    h = run(steps, [SUM], np.array([[[25.0]]]), 1, t_first=86400)            # one observation: day 1 only (k = -1, 0, 1)
    assert list(h.closed) == [1]
    assert list(h.moments[0, :, 0]) == [1020.0, 30.0, 900.0, 750.0, 25.0]
    h = run(steps, [SUM], np.full((1, 1, 2), 1.0), 1, interval=3600, t_first=86400 + 23 * 3600)   # hours 47 (never closed) and 48
    assert list(h.closed) == [0, 1] and h.moments[0, 1, 0] == 31.0


def test_three_series_and_a_hole():
    steps = mixed_steps(4)
    series = np.array([0, 2, -1, 1])
    obs = np.array([[[1.0, 2.0, 3.0], [10.0, np.nan, 30.0], [np.nan, np.nan, np.nan]]])
    h = run(steps, [SUM], obs, 4, series=series)
    day = np.array([435.0, 30.0, 1020.0])
    assert list(h.moments[0, :, 0]) == [1020.0, day.sum(), (day ** 2).sum(), (day * [1, 2, 3]).sum(), ((day - [1, 2, 3]) ** 2).sum()]
    assert list(h.moments[0, :, 1]) == [2040.0, 0.0, 0.0, 0.0, 0.0]          # series 2: every observation missing; acc still runs
    assert (h.moments[0, :, 2] == 0).all() and not np.signbit(h.moments[0, :, 2]).any()   # the hole: nothing loaded, nothing stored
    d4 = day * 4
    assert list(h.moments[0, 1:, 3]) == [d4[0] + d4[2], d4[0] ** 2 + d4[2] ** 2, d4[0] * 10 + d4[2] * 30, (d4[0] - 10) ** 2 + (d4[2] - 30) ** 2]
    assert list(h.closed) == [1, 1, 1]


def daily(values):
    """One daily step per value: [(t0, t1, (n,))]."""
    return [(k * 86400, (k + 1) * 86400, np.atleast_1d(np.asarray(v, dtype=np.float64))) for k, v in enumerate(values)]


def test_order_pinned():
    """m1 is added in increasing k: B, 1, -B gives 0 (B + 1 == B), any order that adds the 1 last gives 1.  m2 and m3 take the ROUNDED
    product: after two intervals of 1 the third holds a = 2^27 + 1, a * a = 2^54 + 2^28 + 1 rounds to 2^54 + 2^28, and 2 + that is a tie
    that goes to even, 2^54 + 2^28; a fused multiply-add rounds 2^54 + 2^28 + 3 once, to 2^54 + 2^28 + 4.  m4 squares the rounded
    difference: with a = B and o = B - 256, d = 256 and d * d = 65536, where a * a - 2 a o + o * o in doubles is 0."""
    assert B + 1.0 == B
    h = run(daily([B, 1.0, -B]), [SUM], np.zeros((1, 1, 3)), 1)
    assert same_bits(h.moments[0, 1, 0], 0.0) and (B + -B) + 1.0 == 1.0
    a = 2.0 ** 27 + 1.0
    h = run(daily([1.0, 1.0, a]), [SUM], np.array([[[1.0, 1.0, a]]]), 1)
    separate, fused = 2.0 ** 54 + 2.0 ** 28, float(Fraction(2) + Fraction(a) * Fraction(a))
    assert fused == 2.0 ** 54 + 2.0 ** 28 + 4.0 and fused != separate
    assert same_bits(h.moments[0, 2, 0], separate) and same_bits(h.moments[0, 3, 0], separate)
    assert same_bits(h.moments[0, 4, 0], 0.0)
    o = B - 256.0
    h = run(daily([B]), [SUM], np.array([[[o]]]), 1)
    assert same_bits(h.moments[0, 4, 0], 65536.0) and (B * B - 2.0 * B * o) + o * o != 65536.0


def two_pass(sim, obs):
    """bias, rmse, r, nse, kge of two equally long series, means first and centred sums second."""
    mu_s, mu_o = sim.mean(), obs.mean()
    var_s, var_o = ((sim - mu_s) ** 2).mean(), ((obs - mu_o) ** 2).mean()
    cov = ((sim - mu_s) * (obs - mu_o)).mean()
    r, alpha, beta = cov / np.sqrt(var_s * var_o), np.sqrt(var_s / var_o), mu_s / mu_o
    sse = ((sim - obs) ** 2).sum()
    return dict(bias=mu_s - mu_o, rmse=np.sqrt(sse / sim.size), r=r, nse=1.0 - sse / (sim.size * var_o),
                kge=1.0 - np.sqrt((r - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2))


def cancellation_bound(x):
    """8 n eps (mu^2 + var) / var: the relative error bound of the raw-moment variance sum x^2 / n - mu^2."""
    return 8.0 * x.size * EPS * (x.mean() ** 2 + x.var()) / x.var()


def study(seed=3, ndays=40, ncol=6):
    rng = np.random.default_rng(seed)
    truth = 2.0 + rng.gamma(2.0, 1.5, size=ndays)
    sims = truth[:, None] * rng.uniform(0.6, 1.4, size=ncol)[None, :] + rng.normal(0.0, 0.4, size=(ndays, ncol))
    obs = truth + rng.normal(0.0, 0.3, size=ndays)
    # every day in three steps (10 minutes, the rest of the first hour's class, the rest): the SUM of the three parts is the day's value
    steps = []
    for k in range(ndays):
        parts = sims[k] * np.array([[0.2], [0.3], [0.5]])
        for (a, b), p in zip(((0, 600), (600, 3600), (3600, 86400)), parts):
            steps.append((k * 86400 + a, k * 86400 + b, p))
    return steps, obs


def test_derived_metrics_against_two_pass():
    """The tolerance is the cancellation bound of the raw-moment variance, 8 n eps (mu^2 + var) / var, the larger of the two series',
    relative (for nse and kge, which are differences from 1, relative to 1; for the bias relative to the two means)."""
    from roger_amd.scores import FILL, derive

    steps, obs = study()
    obs = obs.copy()
    obs[7] = np.nan
    K = obs.size + 2                                       # two intervals nobody closes
    o3 = np.concatenate([obs, [5.0, 6.0]])[None, None, :]
    h = run(steps, [SUM], o3, 6)
    assert list(h.closed) == [1] * obs.size + [0, 0]
    got = derive(h.moments[0], h.closed, o3[0])
    series = interval_series(steps, SUM, 86400, 0, K)
    keep = ~np.isnan(obs)
    assert (got["n"] == keep.sum()).all()
    for c in range(6):
        sim = series[:obs.size, c][keep]
        tol = max(cancellation_bound(sim), cancellation_bound(obs[keep]))
        assert tol < 1e-6
        want = two_pass(sim, obs[keep])
        for key, w in want.items():
            g = got[key][c]
            assert g != FILL and abs(g - w) <= tol * max(abs(w), 1.0 if key in ("nse", "kge") else 0.0) + (tol * (abs(sim.mean()) + abs(obs[keep].mean())) if key == "bias" else 0.0), (key, c, g, w, tol)
        assert same_bits(got["sse"][c], np.add.accumulate(np.concatenate([[0.0], (sim - obs[keep]) ** 2]))[-1])


def test_twin():
    """Observations equal to column 2's own aggregated series: sse, rmse and bias are exactly zero there, nse and kge are 1 within the
    cancellation bound, and every other column has sse > 0."""
    from roger_amd.scores import derive

    steps, _ = study(seed=11)
    series = interval_series(steps, SUM, 86400, 0, 40)
    o3 = np.ascontiguousarray(series[:, 2])[None, None, :]
    h = run(steps, [SUM], o3, 6)
    got = derive(h.moments[0], h.closed, o3[0])
    assert got["sse"][2] == 0.0 and got["rmse"][2] == 0.0 and got["bias"][2] == 0.0
    tol = cancellation_bound(series[:, 2])
    assert tol < 1e-6 and abs(got["nse"][2] - 1.0) <= tol and abs(got["kge"][2] - 1.0) <= tol and abs(got["r"][2] - 1.0) <= tol
    others = [c for c in range(6) if c != 2]
    assert (got["sse"][others] > 0).all() and (got["nse"][others] < 1).all()


def test_fill_values_of_the_derivation():
    from roger_amd.scores import FILL, derive

    m = np.zeros((5, 4))
    m[1:, :] = [[3.0], [5.0], [3.0], [2.0]]                                  # two intervals: 1 and 2 against constant observations 1, 1
    obs = np.array([[1.0, 1.0, np.nan], [1.0, np.nan, np.nan], [1.0, 2.0, 3.0]])
    got = derive(m, np.array([1, 1, 0]), obs, np.array([0, 1, -1, 2]))
    assert list(got["n"]) == [2, 1, 0, 2]
    assert got["bias"][0] == 0.5 and got["rmse"][0] == 1.0 and got["nse"][0] == FILL and got["r"][0] == FILL and got["kge"][0] == FILL   # var_o == 0
    assert all(got[k][1] == FILL for k in ("bias", "rmse", "r", "nse", "kge")) and got["sum_sim"][1] == 3.0                              # n < 2
    assert all(got[k][2] == FILL for k in ("sum_sim", "sse", "bias", "kge"))                                                             # not scored
    assert all(got[k][3] != FILL for k in ("bias", "rmse", "r", "nse", "kge"))


# ---- the host package on the oracle double ----
@pytest.fixture
def scores_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []

    def make(*a, **k):
        made.append(ScoresOracleContext(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


SERIES = np.array([[0, 0, 1, 1], [2, -1, 1, 0], [2, 2, -3, 1], [0, 1, 2, 2]])
K = 8


def script_obs():
    rng = np.random.default_rng(2)
    q = rng.uniform(0.0, 3.0, size=(3, K))
    q[1, 2] = np.nan
    theta = rng.uniform(0.2, 0.4, size=(3, K))
    theta[2, :] = np.nan                                    # series 2 has no soil-moisture record
    return {"q_ss": q, "theta_rz": theta}


def make_model(tmp_path, ndays=6, script_hooks=None, **settings):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks=script_hooks)
    cfg = dict(observations=script_obs(), series=SERIES, base_output_path=str(tmp_path))
    cfg.update(settings)

    def set_diagnostics(self, state):
        for k, v in cfg.items():
            setattr(state.scores, k, v)

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model


@pytest.mark.parametrize("script_hooks,by_routine", [(None, False), ("plain", True)])
def test_script_writes_the_maps_of_the_doubles_planes(scores_backend, tmp_path, monkeypatch, script_hooks, by_routine):
    from nc_util import netcdf_file

    from roger_amd.scores import FILL, derive

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    model = make_model(tmp_path, script_hooks=script_hooks)
    model.setup()
    ctx = scores_backend[-1]
    steps = []
    accumulate = ctx._accumulate
    ctx._accumulate = lambda: (accumulate(), steps.append((int(ctx.st.scal.time) - int(ctx.st.scal.dt_secs), int(ctx.st.scal.time),
                                                           {v: ctx.download(v).copy() for v in ("q_ss", "theta_rz")})))[0]
    model.run()
    assert {t1 - t0 for t0, t1, _ in steps} == {600, 3600, 86400}
    live = model.state.scores.read()
    obs = script_obs()
    f = netcdf_file(str(tmp_path / "GoldenSVAT.scores.nc"))
    assert list(f.variables["closed"][:]) == [1] * 6 + [0] * 2 and f.variables["closed"].dimensions == ("interval",)
    np.testing.assert_array_equal(f.variables["interval"][:], np.arange(1, K + 1))
    np.testing.assert_array_equal(f.variables["series"][:], SERIES.T)
    for j, (v, kind) in enumerate((("q_ss", SUM), ("theta_rz", LAST))):       # the defaults: a flux is summed, a state taken at the end
        h = HostScores([kind], obs[v][None], 16, SERIES.reshape(-1))
        for t0, t1, p in steps:
            h.add(t0, t1, [p[v]])
        want = derive(h.moments[0], h.closed, obs[v], SERIES.reshape(-1))
        assert np.any(h.moments[0, 1] != 0), v
        for key, w in want.items():
            var = f.variables[f"{v}_{key}"]
            a = np.asarray(var[:])
            assert var.dimensions == ("y", "x") and a.shape == (4, 4)
            if key == "n":
                np.testing.assert_array_equal(a, w.reshape(4, 4).T)
                continue
            assert var._FillValue == FILL
            assert same_bits(a, w.reshape(4, 4).T), (v, key)
            assert same_bits(live[f"{v}_{key}"], w.reshape(4, 4)), (v, key)
            assert (a[SERIES.T < 0] == FILL).all(), (v, key, "a column that is not scored")
        n = np.asarray(f.variables[f"{v}_n"][:])
        assert (n[SERIES.T < 0] == 0).all()
    assert (np.asarray(f.variables["q_ss_n"][:])[SERIES.T == 1] == 5).all() and (np.asarray(f.variables["q_ss_n"][:])[SERIES.T == 0] == 6).all()
    assert (np.asarray(f.variables["theta_rz_kge"][:])[SERIES.T == 2] == FILL).all(), "a series without a single observation"
    assert (np.asarray(f.variables["q_ss_kge"][:])[SERIES.T >= 0] != FILL).all()


def test_hourly_frequency_and_a_start_in_mid_run(scores_backend, tmp_path):
    """frequency 3600, start two days in: 96 observations cover days 2 and 3; the hours of a day the model takes in one step stay open."""
    model = make_model(tmp_path, ndays=5, observations={"q_ss": np.ones(96)}, series=None, frequency=3600, start=2 * 86400,
                       aggregation={"q_ss": "sum"})
    model.setup()
    ctx = scores_backend[-1]
    ends = []
    accumulate = ctx._accumulate
    ctx._accumulate = lambda: (accumulate(), ends.append((int(ctx.st.scal.time), int(ctx.st.scal.dt_secs))))[0]
    model.run()
    got = model.state.scores.read()
    want = np.zeros(96, dtype=np.uint8)
    for t1, dt in ends:
        k = t1 // 3600 - 1 - 48
        if t1 % 3600 == 0 and dt <= 3600 and 0 <= k < 96:
            want[k] = 1
    np.testing.assert_array_equal(got["closed"], want)
    assert 0 < want.sum() and (got["q_ss_n"] == want.sum()).all()


def test_refusals(scores_backend, tmp_path):
    q = np.ones(K)
    for kw, exc, text in ((dict(observations={"q_ss": np.ones((2, 3, 4))}), ValueError, r"observations of 'q_ss' have shape \(2, 3, 4\)"),
                          (dict(observations={"q_ss": np.float64(1.0)}), ValueError, r"observations of 'q_ss' have shape \(\)"),
                          (dict(observations={"q_ss": np.ones((3, K)), "theta_rz": q}), ValueError, "one .n_series, n_intervals. for all"),
                          (dict(series=np.zeros((4, 5), dtype=int)), ValueError, r"series map has shape \(4, 5\)"),
                          (dict(series=np.zeros(16, dtype=int)), ValueError, r"series map has shape \(16,\)"),
                          (dict(series=np.zeros((4, 4))), ValueError, "float64 values"),
                          (dict(series=np.full((4, 4), 3)), ValueError, r"names series 3, the observations hold 3"),
                          (dict(frequency=7200), ValueError, "frequency = 7200"),
                          (dict(start=600), ValueError, "start = 600 s is not a multiple"),
                          (dict(aggregation={"q_ss": "mean"}), ValueError, "'mean'"),
                          (dict(aggregation={"aet": "sum"}), ValueError, "'aet', which has no observations"),
                          (dict(observations={"lu_id": q}, series=None), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(observations={"no_such_variable": q}, series=None), NotImplementedError, "no_such_variable"),
                          (dict(observations={f"v{k}": q for k in range(17)}, series=None), ValueError, r"17 variables \(at most 16\)"),
                          (dict(observations={"q_ss": np.ones((1025, 2))}, series=None), ValueError, r"1025 series \(at most 1024\)")):
        model = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model = make_model(tmp_path, ndays=1, observations={})
    model.setup()
    model.run()
    assert scores_backend[-1]._scores is None and model.state.scores.read() is None and not list(tmp_path.iterdir())


def test_the_offline_transport_is_refused():
    from roger_amd import scores
    from roger_amd.state import RogerState

    st = RogerState()
    assert not st.scores.active
    scores.initialize(st)
    st.scores.observations = {"q_ss": np.ones(3)}
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    with pytest.raises(NotImplementedError, match="offline transport"):
        scores.initialize(st)


def test_two_rank_block_cut_of_the_series_map_and_a_continued_run(monkeypatch, tmp_path):
    """num_proc = (2, 1), rank 1: the device gets the rank's half of the map, the file carries the rank in its name; a clock past
    `start` moves interval 0 to the next boundary and drops the observations before it."""
    from roger_amd import runtime_state, scores

    calls = []
    series = np.arange(24).reshape(6, 4) % 3 - 1      # -1, 0, 1: two series
    ctx = types.SimpleNamespace(scores_configure=lambda *a: calls.append(a))
    meta = types.SimpleNamespace(plane=7, dtype=None)
    state = types.SimpleNamespace(
        settings=types.SimpleNamespace(nx=6, ny=4, enable_offline_transport=False, identifier="run"), var_meta={"q_ss": meta},
        variables=types.SimpleNamespace(time=3 * 86400 + 600, flush_to_device=lambda: None), backend_context=ctx, scores=scores.Scores())
    s = state.scores
    s.observations, s.series, s.base_output_path = {"q_ss": np.arange(20.0).reshape(2, 10)}, series, str(tmp_path)
    monkeypatch.setattr(scores, "rs", types.SimpleNamespace(num_proc=(2, 1)))
    monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self: 1))
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
    scores.initialize(state)
    scores.start(state)
    (names, kinds, obs, local, f, t_first), = calls
    assert names == ["q_ss"] and kinds == [0] and f == 86400 and t_first == 4 * 86400
    np.testing.assert_array_equal(local, series[3:].reshape(-1))
    assert local.dtype == np.int32
    np.testing.assert_array_equal(obs, np.arange(20.0).reshape(1, 2, 10)[:, :, 4:])
    assert s._on and s._dropped == 4 and s._path.endswith("run.scores.0001.nc")
    # a rank whose block holds no scored column configures nothing
    calls.clear()
    state.scores = s2 = scores.Scores()
    s2.observations, s2.base_output_path = {"q_ss": np.arange(10.0)}, str(tmp_path)
    s2.series = np.where(np.arange(24).reshape(6, 4) < 12, 0, -1)
    scores.initialize(state)
    scores.start(state)
    assert not calls and not s2._on and s2.read() is None
