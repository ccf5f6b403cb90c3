"""CPU: the duration curves' device rule restated (tests/durations_reference.py) on hand-worked step sequences of all three step classes,
the host package's derivation (roger_amd/durations.py: derive) against the raw interval values, and the host package's Durations on the
oracle double: a RogerSetup script ends with a `.durations.nc` whose maps are `derive` of the restatement over the double's own planes."""
import types

import numpy as np
import pytest

from diag_reference import HostAccumulator
from durations_reference import AT_OR_ABOVE, BELOW, LAST, LONGEST, NSPELLS, RUN, SUM, HostDurations, clock, interval_series, oracle_double
from golden_util import load_case

DAY = 86400


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
    assert t == 3 * DAY and len(steps) == 54 and {b - a for a, b, _ in steps} == {600, 3600, 86400}
    return steps


def run(steps, kinds, edges, n, **kw):
    h = HostDurations(kinds, edges, n, **kw)
    for t0, t1, v in steps:
        h.add(t0, t1, [v] * len(kinds))
    return h


def daily(values):
    """One daily step per value (a scalar or an (n,) array)."""
    return [(k * DAY, (k + 1) * DAY, np.atleast_1d(np.asarray(v, dtype=np.float64))) for k, v in enumerate(values)]


def test_clock_has_no_upper_bound():
    assert clock(0, 600, 3600, 0) == (True, False, -1, False)
    assert clock(3000, 3600, 3600, 0) == (False, True, 0, True)
    assert clock(3600, 7200, 3600, 7200) == (True, True, -1, False)           # k below 0
    assert clock(86400, 172800, 3600, 0)[1:] == (False, 47, False)            # a daily step closes no hour
    assert clock(10 ** 9 * DAY - DAY, 10 ** 9 * DAY, DAY, 0)[1:] == (True, 10 ** 9 - 1, True)


def test_bins_edges_zeros_infinities_and_nan():
    """A value on an edge goes up, -0.0 on the edge 0.0 goes up, -inf to bin 0, +inf to bin m, NaN to bin m + 1; no edges: one finite bin."""
    values = [0.0, -0.0, 1.0, np.nextafter(1.0, 0.0), -np.inf, np.inf, np.nan, 0.5, 2.0, -1.0]
    h = run(daily(values), [LAST, LAST], [[0.0, 1.0, 2.0], []], 1)
    # bins of [0, 1, 2]: (-inf, 0) [0, 1) [1, 2) [2, inf] NaN
    assert list(h.counts[0][:, 0]) == [2, 4, 1, 2, 1]
    assert list(h.counts[1][:, 0]) == [9, 1]
    assert h.vals[0, 1, 0] == -np.inf and h.vals[0, 2, 0] == np.inf
    assert h.vals[0, 0, 0] == 0.0 and not np.signbit(h.vals[0, 0, 0])         # LAST: the acc plane stays +0.0
    for v, b in ((0.0, 1), (-0.0, 1), (1.0, 2), (np.nextafter(1.0, 0.0), 1), (2.0, 3)):
        one = run(daily([v]), [LAST], [[0.0, 1.0, 2.0]], 1)
        assert one.counts[0][b, 0] == 1 and one.counts[0].sum() == 1, (v, b)


def test_extremes_keep_the_first_of_equal_zeros_and_skip_nan():
    h = run(daily([np.nan, 0.0, -0.0, np.nan]), [LAST], [[]], 1)
    assert same_bits(h.vals[0, 1, 0], 0.0) and same_bits(h.vals[0, 2, 0], 0.0)
    h = run(daily([-0.0, 0.0]), [LAST], [[]], 1)
    assert same_bits(h.vals[0, 1, 0], -0.0) and same_bits(h.vals[0, 2, 0], -0.0)
    h = run(daily([np.nan]), [LAST], [[]], 1)
    assert h.vals[0, 1, 0] == np.inf and h.vals[0, 2, 0] == -np.inf and list(h.counts[0][:, 0]) == [0, 1]


def test_daily_interval_over_mixed_steps_sum_against_last():
    steps = mixed_steps()
    h = run(steps, [SUM, LAST], [[100.0, 500.0], [30.0]], 1)
    # SUM: day 0 = 1 + ... + 29 = 435, day 1 = 30, day 2 = 31 + ... + 54 = 1020;  LAST: 29, 30, 54
    assert list(h.counts[0][:, 0]) == [1, 1, 1, 0] and list(h.vals[0, :, 0]) == [1020.0, 30.0, 1020.0]
    assert list(h.counts[1][:, 0]) == [1, 2, 0] and list(h.vals[1, :, 0]) == [0.0, 29.0, 54.0]


def test_sum_order_is_the_accumulators():
    """Values whose sum depends on the order: the SUM of a day equals HostAccumulator's rate slot bit for bit."""
    rng = np.random.default_rng(1)
    steps = [(t0, t1, rng.uniform(0, 1, 5) * 10.0 ** rng.integers(-8, 8, 5)) for t0, t1, _ in mixed_steps()]
    acc = HostAccumulator(("v",), (), 3, 5)
    h = HostDurations([SUM], [[]], 5)
    per_day = []
    for t0, t1, v in steps:
        acc.add(t1, t1 - t0, {"v": v})
        h.add(t0, t1, [v])
        if t1 % DAY == 0:
            per_day.append(h.vals[0, 0].copy())
    for d in range(3):
        assert same_bits(per_day[d], acc.data["v"][d])
    assert same_bits(h.vals[0, 1], np.minimum.reduce(per_day)) and same_bits(h.vals[0, 2], np.maximum.reduce(per_day))


def test_hours_under_a_daily_step_are_neither_counted_nor_break_a_run():
    steps = mixed_steps()
    # hourly values: hour 0 = 21 (SUM) / 6 (LAST), hours 1 ... 23 = 7 ... 29, [day 1: no hour], hours 48 ... 71 = 31 ... 54
    h = run(steps, [SUM, LAST], [[], []], 1, interval=3600, spells=[(AT_OR_ABOVE, 25.0), (BELOW, 8.0)])
    assert h.counts[0][0, 0] == 48 and h.counts[1][0, 0] == 48                # 24 + 24: the 24 hours of day 1 were never started
    # SUM >= 25: hours 19 ... 23 (25 ... 29) of day 0 and all 24 of day 2 -- ONE run of 29 across the daily step
    assert list(h.spells[0, :, 0]) == [29, 29, 1]
    # LAST < 8: hours 0 and 1 (6, 7), then never again
    assert h.spells[1, RUN, 0] == 0 and h.spells[1, LONGEST, 0] == 2 and h.spells[1, NSPELLS, 0] == 1
    assert h.vals[0, 1, 0] == 7.0 and h.vals[0, 2, 0] == 54.0 and h.vals[1, 1, 0] == 6.0


def test_spells_of_each_side():
    values = [1, 5, 5, 1, np.nan, 5, 1, 1, 1, 5]
    h = run(daily(values), [LAST, LAST, LAST], [[], [], []], 1, spells=[(BELOW, 5.0), (AT_OR_ABOVE, 5.0), None])
    assert list(h.spells[0, :, 0]) == [0, 3, 3]          # below: 1 | 1 (the NaN is not below and ends the run) | 1 1 1
    assert list(h.spells[1, :, 0]) == [1, 2, 3]          # at or above (a value on the threshold is inside): 5 5 | 5 | 5 under way
    assert not h.spells[2].any()


def test_a_start_in_the_future_and_in_the_past():
    steps = mixed_steps()
    h = run(steps, [SUM], [[]], 1, t_first=DAY)          # the future: day 0 closes with k = -1 and is not counted
    assert h.counts[0][0, 0] == 2 and list(h.vals[0, :, 0]) == [1020.0, 30.0, 1020.0]
    # the past: configured in the middle of day 0 (after 10 steps) with t_first = 0 -- the interval under way is counted with what was
    # seen from then on, the rule of an accumulator slot first touched inside its interval
    h = HostDurations([SUM, LAST], [[], []], 1, t_first=0)
    for t0, t1, v in steps[10:]:
        h.add(t0, t1, [v, v])
    assert list(h.counts[0][:, 0]) == [3, 0] and h.vals[0, 1, 0] == 30.0 and h.vals[0, 2, 0] == 1020.0
    assert sum(range(11, 30)) == 380 and interval_series(steps[10:], SUM, DAY, 0)[0, 0] == 380.0


def test_mask_leaves_a_column_untouched():
    h = run(mixed_steps(3), [SUM], [[100.0]], 3, mask=[1, 0, 1], spells=[(BELOW, 1e9)])
    assert not h.counts[0][:, 1].any() and list(h.vals[0, :, 1]) == [0.0, np.inf, -np.inf] and not h.spells[0, :, 1].any()
    assert h.counts[0][:, 0].sum() == 3 and h.counts[0][:, 2].sum() == 3


# ---- derive ----
def raw_case(seed=0, ncol=7, nk=200):
    rng = np.random.default_rng(seed)
    raw = rng.gamma(1.5, 2.0, size=(nk, ncol)) * rng.uniform(0.2, 3.0, size=ncol)[None, :]
    raw[rng.random(raw.shape) < 0.2] = 0.0               # days without flow
    raw[3, 1] = np.nan
    raw[:, 6] = np.nan                                   # a column without a single number
    edges = np.concatenate([[0.0], np.geomspace(0.05, 20.0, 30)])
    return raw, edges


def test_derive_quantiles_exceedance_and_extremes():
    """Every quantile lies in the bin (its closed interval) that holds the empirical quantile sorted[ceil(p n) - 1] of the raw values;
    p = 0 and p = 1 are the extremes exactly; exceed is the direct count of s >= e_q divided by v_n, exactly."""
    from roger_amd.durations import FILL, derive

    raw, edges = raw_case()
    h = run(daily(raw), [LAST], [edges], raw.shape[1], spells=[(BELOW, 0.5)])
    ps = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 0.999, 1.0)
    got = derive(h.counts[0], h.vals[0], edges, ps, h.spells[0])
    m = edges.size
    for c in range(raw.shape[1]):
        x = np.sort(raw[:, c][~np.isnan(raw[:, c])])
        assert got["n"][c] == x.size and got["nan"][c] == raw.shape[0] - x.size
        if not x.size:
            assert got["min"][c] == FILL and got["max"][c] == FILL and (got["q"][:, c] == FILL).all() and (got["exceed"][:, c] == FILL).all()
            continue
        assert got["min"][c] == x[0] and got["max"][c] == x[-1] and got["q"][0, c] == x[0] and got["q"][-1, c] == x[-1]
        for iq, p in enumerate(ps[1:-1], start=1):
            emp = x[int(np.ceil(p * x.size)) - 1]
            b = int((edges <= emp).sum())
            lo, hi = (edges[b - 1] if b else -np.inf), (edges[b] if b < m else np.inf)
            q = got["q"][iq, c]
            assert lo <= q <= hi and x[0] <= q <= x[-1], (c, p, q, lo, hi)
        for k in range(m):
            assert got["exceed"][k, c] == (x >= edges[k]).sum() / x.size, (c, k)
        assert got["exceed"][0, c] == 1.0                                   # every value is >= 0
    assert (np.diff(got["q"][:, :6], axis=0) >= 0).all(), "quantiles ascend with p"
    assert (got["longest"] >= 1)[:6].all() and (got["spells"][:6] >= got["longest"][:6].clip(max=1)).all()


def test_derive_interpolates_by_the_fraction_of_the_bins_count():
    from roger_amd.durations import derive

    # ten values in one bin [0, 10), min 1 and max 8: the median needs 5 of the bin's 10 -> half way from lo = max(0, 1) to hi = min(10, 8)
    counts = np.array([[0], [10], [0], [0]])
    vals = np.array([[0.0], [1.0], [8.0]])
    got = derive(counts, vals, [0.0, 10.0], (0.5, 0.1))
    assert got["q"][0, 0] == 1.0 + 0.5 * 7.0 and got["q"][1, 0] == 1.0 + 0.1 * 7.0
    # no edges: one finite bin from min to max
    got = derive(np.array([[4], [0]]), np.array([[0.0], [2.0], [6.0]]), [], (0.25,))
    assert got["q"][0, 0] == 3.0 and got["exceed"].shape == (0, 1)


# ---- the host package on the oracle double ----
@pytest.fixture
def durations_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []
    double = oracle_double()

    def make(*a, **k):
        made.append(double(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


MASK = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1]])
Q_EDGES = np.concatenate([[0.0], np.geomspace(1e-3, 10.0, 12)])
T_EDGES = np.linspace(0.1, 0.5, 9)


def make_model(tmp_path, ndays=6, script_hooks=None, **settings):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks=script_hooks)
    cfg = dict(variables={"q_ss": Q_EDGES, "theta_rz": T_EDGES}, spells={"theta_rz": ("below", 0.3)}, mask=MASK, base_output_path=str(tmp_path))
    cfg.update(settings)

    def set_diagnostics(self, state):
        for k, v in cfg.items():
            setattr(state.durations, k, v)

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model


@pytest.mark.parametrize("script_hooks,by_routine,frequency", [(None, False, DAY), ("plain", True, DAY), (None, False, 3600)])
def test_script_writes_the_maps_of_the_doubles_planes(durations_backend, tmp_path, monkeypatch, script_hooks, by_routine, frequency):
    from roger_amd import h5lite
    from roger_amd.durations import FILL, derive

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    quantiles = (0.0, 0.05, 0.5, 0.95, 1.0)
    model = make_model(tmp_path, script_hooks=script_hooks, frequency=frequency, quantiles=quantiles)
    model.setup()
    ctx = durations_backend[-1]
    steps = []
    accumulate = ctx._accumulate
    ctx._accumulate = lambda: (accumulate(), steps.append((int(ctx.st.scal.time) - int(ctx.st.scal.dt_secs), int(ctx.st.scal.time),
                                                           {v: ctx.download(v).copy() for v in ("q_ss", "theta_rz")})))[0]
    model.run()
    assert {t1 - t0 for t0, t1, _ in steps} == {600, 3600, 86400}
    live = model.state.durations.read()
    f = h5lite.read_root(str(tmp_path / "GoldenSVAT.durations.nc"))
    np.testing.assert_array_equal(f["quantile"], quantiles)
    np.testing.assert_array_equal(f["mask"], MASK.T)
    np.testing.assert_array_equal(f["q_ss_edges"], Q_EDGES)
    np.testing.assert_array_equal(f["theta_rz_edges"], T_EDGES)
    for v, kind, edges, spell in (("q_ss", SUM, Q_EDGES, None), ("theta_rz", LAST, T_EDGES, (BELOW, 0.3))):   # the defaults of the aggregation
        h = HostDurations([kind], [edges], 16, spells=[spell], mask=MASK.reshape(-1), interval=frequency)
        for t0, t1, p in steps:
            h.add(t0, t1, [p[v]])
        want = derive(h.counts[0], h.vals[0], edges, quantiles, h.spells[0] if spell else None)
        assert (want["n"][MASK.reshape(-1) != 0] > 0).all() and (np.count_nonzero(h.counts[0][:-1].sum(axis=1)) >= 2), v
        for key, w in want.items():
            a = np.asarray(f[f"{v}_{key}" if key != "edges" else f"{v}_edges"])
            w = np.swapaxes(w.reshape(w.shape[:-1] + (4, 4)), -1, -2)
            assert a.shape == w.shape, (v, key, a.shape, w.shape)
            if w.dtype.kind == "f":
                assert same_bits(a, w), (v, key)
                assert same_bits(np.swapaxes(live[f"{v}_{key}"], -1, -2), w), (v, key)
            else:
                np.testing.assert_array_equal(a, w, err_msg=f"{v}_{key}")
        assert (np.asarray(f[f"{v}_n"])[MASK.T == 0] == 0).all() and (np.asarray(f[f"{v}_min"])[MASK.T == 0] == FILL).all()
    assert "q_ss_longest" not in f and "theta_rz_longest" in f and "theta_rz_spells" in f and "theta_rz_run" in f
    n_days = np.asarray(f["q_ss_n"])[MASK.T != 0]
    assert (n_days == 6).all() if frequency == DAY else (0 < n_days).all() and (n_days < 6 * 24).all()


def test_a_clock_past_the_start_counts_from_the_next_boundary_and_the_rank_gets_its_block(monkeypatch, tmp_path):
    from roger_amd import durations, runtime_state

    calls = []
    mask = (np.arange(24).reshape(6, 4) % 3 != 0)
    ctx = types.SimpleNamespace(durations_configure=lambda *a: calls.append(a))
    meta = types.SimpleNamespace(plane=7, dtype=None)
    state = types.SimpleNamespace(
        settings=types.SimpleNamespace(nx=6, ny=4, enable_offline_transport=False, identifier="run"), var_meta={"q_ss": meta},
        variables=types.SimpleNamespace(time=3 * DAY + 600, flush_to_device=lambda: None), backend_context=ctx, durations=durations.Durations())
    d = state.durations
    d.variables, d.mask, d.base_output_path, d.spells = {"q_ss": [0.0, 1.0]}, mask, str(tmp_path), {"q_ss": ("at_or_above", 1.0)}
    monkeypatch.setattr(durations, "rs", types.SimpleNamespace(num_proc=(2, 1), diskless_mode=False))
    monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self: 1))
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
    durations.initialize(state)
    durations.start(state)
    (names, kinds, edges, spells, local, f, t_first), = calls
    assert names == ["q_ss"] and kinds == [0] and f == DAY and t_first == 4 * DAY and spells == [(1, 1.0)]
    np.testing.assert_array_equal(edges[0], [0.0, 1.0])
    np.testing.assert_array_equal(local, mask[3:].reshape(-1))
    assert local.dtype == np.uint8 and d._on and d._path.endswith("run.durations.0001.nc")
    # a start in the future stays; a rank whose block holds no counted column configures nothing
    calls.clear()
    state.durations = d2 = durations.Durations()
    d2.variables, d2.start, d2.base_output_path = {"q_ss": []}, 10 * DAY, str(tmp_path)
    durations.initialize(state)
    durations.start(state)
    assert calls[0][6] == 10 * DAY and calls[0][4] is None
    calls.clear()
    state.durations = d3 = durations.Durations()
    d3.variables, d3.mask = {"q_ss": []}, np.arange(24).reshape(6, 4) < 12
    durations.initialize(state)
    durations.start(state)
    assert not calls and not d3._on and d3.read() is None


def test_refusals(durations_backend, tmp_path):
    e = Q_EDGES
    for kw, exc, text in ((dict(variables={f"v{k}": e for k in range(17)}), ValueError, r"17 variables \(at most 16\)"),
                          (dict(variables={"q_ss": np.arange(64.0)}), ValueError, r"64 edges for 'q_ss' \(at most 63\)"),
                          (dict(variables={"q_ss": [0.0, np.inf]}), ValueError, "edges of 'q_ss' are not all finite"),
                          (dict(variables={"q_ss": [0.0, np.nan]}), ValueError, "edges of 'q_ss' are not all finite"),
                          (dict(variables={"q_ss": [0.0, 1.0, 1.0]}), ValueError, "edges of 'q_ss' are not strictly ascending"),
                          (dict(variables={"q_ss": np.zeros((2, 2))}), ValueError, r"edges of 'q_ss' have shape \(2, 2\)"),
                          (dict(variables={"lu_id": e}, spells={}), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(variables={"no_such_variable": e}, spells={}), NotImplementedError, "no_such_variable"),
                          (dict(frequency=7200), ValueError, "frequency = 7200"),
                          (dict(start=600), ValueError, "start = 600 s is not a multiple"),
                          (dict(aggregation={"q_ss": "mean"}), ValueError, "'mean'"),
                          (dict(aggregation={"aet": "sum"}), ValueError, "aggregation names 'aet', which has no edges"),
                          (dict(spells={"aet": ("below", 1.0)}), ValueError, "spells names 'aet', which has no edges"),
                          (dict(spells={"q_ss": ("above", 1.0)}), ValueError, "the spell of 'q_ss' is"),
                          (dict(spells={"q_ss": ("below", np.nan)}), ValueError, "the threshold of 'q_ss' is"),
                          (dict(mask=np.ones((4, 5))), ValueError, r"mask has shape \(4, 5\)"),
                          (dict(mask=np.zeros((4, 4))), ValueError, "the mask holds no column"),
                          (dict(quantiles=(0.5, 1.5)), ValueError, "quantiles")):
        if "variables" in kw:
            kw.setdefault("spells", {})                  # (the default spell names theta_rz)
        model = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model = make_model(tmp_path, ndays=1, variables={}, spells={})
    model.setup()
    model.run()
    assert durations_backend[-1]._durations is None and model.state.durations.read() is None and not list(tmp_path.iterdir())


def test_the_offline_transport_is_refused():
    from roger_amd import durations
    from roger_amd.state import RogerState

    st = RogerState()
    assert not st.durations.active
    durations.initialize(st)
    st.durations.variables = {"q_ss": [0.0, 1.0]}
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    with pytest.raises(NotImplementedError, match="offline transport"):
        durations.initialize(st)


def test_log_edges():
    from roger_amd.durations import log_edges

    e = log_edges(0.01, 100.0, 5)
    assert e.shape == (5,) and np.allclose(e, [0.01, 0.1, 1.0, 10.0, 100.0]) and (np.diff(e) > 0).all()
    with pytest.raises(ValueError, match="log_edges"):
        log_edges(0.0, 1.0, 5)
