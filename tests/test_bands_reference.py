"""CPU: the ensemble bands' rule restated (tests/bands_reference.py) against numpy's own "inverted_cdf" quantile, the rank formula on
hand-worked cases, the key map of the device's radix selection, and the host package's Bands on the oracle double: a RogerSetup script
ends with a `.bands.nc` whose rows are the restatement over the double's own planes."""
import numpy as np
import pytest

from bands_reference import KEY_MASKED, KEY_NAN, LAST, SUM, HostBands, key_of, oracle_double, quantiles_of, rank_of, value_of
from golden_util import load_case

DAY = 86400


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def test_the_restatement_is_numpys_inverted_cdf():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 64, 257, 1000):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        x[rng.random(n) < 0.2] = 0.0
        probs = [float(p) for p in rng.uniform(0.001, 0.999, 6)] + [0.05, 0.5]
        got, m, n_nan = quantiles_of(x, probs)
        assert m == n and n_nan == 0
        assert same_bits(got, np.quantile(x, probs, method="inverted_cdf")), n
        ends, _, _ = quantiles_of(x, [0.0, 1.0])
        assert same_bits(ends, [x.min(), x.max()])
    # NaN are counted and left out, infinities are values, -0.0 comes back as +0.0
    got, m, n_nan = quantiles_of([np.nan, -0.0, np.inf, -np.inf, np.nan, 1.0], [0.0, 0.5, 1.0])
    assert (m, n_nan) == (4, 2) and same_bits(got, [-np.inf, 0.0, np.inf])
    got, m, n_nan = quantiles_of([np.nan, np.nan], [0.0, 0.5])
    assert (m, n_nan) == (0, 2) and np.isnan(got).all()


def test_rank_formula():
    assert [rank_of(p, 1) for p in (0.0, 0.3, 1.0)] == [0, 0, 0]
    assert [rank_of(p, 2) for p in (0.0, 0.25, 0.5, 0.5000001, 1.0)] == [0, 0, 0, 1, 1]
    assert [rank_of(p, 3) for p in (0.0, 1 / 3, 0.34, 2 / 3, 0.67, 1.0)] == [0, 0, 1, 1, 2, 2]
    # p * m exactly integral: the value AT the boundary belongs to the lower rank
    assert rank_of(0.5, 4) == 1 and rank_of(0.25, 8) == 1 and rank_of(0.75, 8) == 5 and rank_of(0.5, 10 ** 6) == 499999
    assert rank_of(0.05, 20) == 0 and rank_of(0.95, 20) == 18 and rank_of(1.0, 20) == 19


def test_key_map_is_monotone_and_invertible():
    tiny = np.finfo(np.float64).tiny
    sub = np.nextafter(0.0, 1.0)
    x = np.array([-np.inf, -np.finfo(np.float64).max, -1.5, -1.0, -np.nextafter(1.0, 0.0), -tiny, -tiny / 2, -sub, 0.0, sub, tiny / 2, tiny,
                  np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 1.5, np.finfo(np.float64).max, np.inf])
    assert (np.diff(x) > 0).all()
    k = key_of(x)
    assert k.dtype == np.uint64 and (k[1:] > k[:-1]).all()
    assert same_bits(value_of(k), x)
    assert key_of(np.array([-0.0]))[0] == key_of(np.array([0.0]))[0] == np.uint64(1 << 63)
    assert k.max() == np.uint64(0xFFF0000000000000) < KEY_NAN < KEY_MASKED                    # no value's key is a flag
    assert np.isnan(value_of(np.array([KEY_NAN, KEY_MASKED]))).all()
    rng = np.random.default_rng(0)
    y = rng.normal(size=4096) * 10.0 ** rng.integers(-300, 300, 4096)
    order = np.argsort(key_of(y), kind="stable")
    assert same_bits(y[order], np.sort(y)) and same_bits(value_of(key_of(y)), y)


def test_sum_and_last_over_mixed_steps():
    """Day 0 in six 10-minute and 23 hourly steps, day 1 in one step, day 2 in 24 hourly steps; column c holds (idx + 1) * (c + 1)."""
    lengths = [600] * 6 + [3600] * 23 + [86400] + [3600] * 24
    h = HostBands([SUM, LAST], [0.0, 0.5, 1.0], 4, mask=[1, 1, 0, 1])
    t = 0
    for idx, dt in enumerate(lengths):
        v = (idx + 1.0) * (np.arange(4) + 1.0)
        h.add(t, t + dt, [v, v])
        t += dt
    hdr, values = h.rows()
    assert hdr.tolist() == [[0, DAY, 3, 0, 3, 0], [1, 2 * DAY, 3, 0, 3, 0], [2, 3 * DAY, 3, 0, 3, 0]]
    # columns 0, 1, 3 (factors 1, 2, 4): p = 0.5 of three values is rank 1
    assert values[:, 0].tolist() == [[435.0, 870.0, 1740.0], [30.0, 60.0, 120.0], [1020.0, 2040.0, 4080.0]]
    assert values[:, 1].tolist() == [[29.0, 58.0, 116.0], [30.0, 60.0, 120.0], [54.0, 108.0, 216.0]]
    hourly = HostBands([LAST], [1.0], 4, interval=3600, t_first=2 * DAY)
    t = 0
    for idx, dt in enumerate(lengths):
        hourly.add(t, t + dt, [np.full(4, idx + 1.0)])
        t += dt
    hdr, values = hourly.rows()
    assert len(hdr) == 24 and hdr[0].tolist() == [0, 2 * DAY + 3600, 4, 0] and values[-1, 0, 0] == 54.0   # the hours of day 1 have no row


# ---- the host package on the oracle double ----
@pytest.fixture
def bands_backend(monkeypatch, oracle):
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
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)


def make_model(tmp_path, ndays=6, script_hooks=None, **settings):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks=script_hooks)
    cfg = dict(variables=["q_ss", "theta_rz"], mask=MASK, base_output_path=str(tmp_path))
    cfg.update(settings)

    def set_diagnostics(self, state):
        for k, v in cfg.items():
            setattr(state.bands, k, v)

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model


@pytest.mark.parametrize("script_hooks,by_routine,frequency,capacity", [(None, False, DAY, 4096), ("plain", True, DAY, 2), (None, False, 3600, 8)])
def test_script_writes_the_rows_of_the_doubles_planes(bands_backend, tmp_path, monkeypatch, script_hooks, by_routine, frequency, capacity):
    from nc_util import netcdf_file
    from roger_amd.bands import FILL

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    model = make_model(tmp_path, script_hooks=script_hooks, frequency=frequency, probabilities=PROBS, capacity=capacity)
    model.setup()
    ctx = bands_backend[-1]
    steps = []
    accumulate = ctx._accumulate
    ctx._accumulate = lambda: (accumulate(), steps.append((int(ctx.st.scal.time) - int(ctx.st.scal.dt_secs), int(ctx.st.scal.time),
                                                           {v: ctx.download(v).copy() for v in ("q_ss", "theta_rz")})))[0]
    model.run()
    assert {t1 - t0 for t0, t1, _ in steps} == {600, 3600, 86400}
    h = HostBands([SUM, LAST], PROBS, 16, MASK.reshape(-1), frequency)           # the defaults of the aggregation
    for t0, t1, p in steps:
        h.add(t0, t1, [p["q_ss"], p["theta_rz"]])
    hdr, values = h.rows()
    assert (len(hdr) == 6) if frequency == DAY else (6 < len(hdr) < 6 * 24)
    assert (hdr[:, 2] == 14).all() and (hdr[:, 3] == 0).all() and np.isfinite(values).all()
    assert (np.diff(values, axis=2) >= 0).all() and (values[:, :, 0] < values[:, :, -1]).any()
    live = model.state.bands.read()
    f = netcdf_file(str(tmp_path / "GoldenSVAT.bands.nc"))
    assert f.columns == b"this rank's block" and int(f.frequency_seconds) == frequency
    np.testing.assert_array_equal(f.variables["probability"][:], PROBS)
    np.testing.assert_array_equal(f.variables["interval"][:], hdr[:, 0])
    np.testing.assert_array_equal(live["interval"], hdr[:, 0])
    np.testing.assert_array_equal(live["time"], hdr[:, 1])
    assert same_bits(f.variables["Time"][:], hdr[:, 1] / float(DAY))
    for j, v in enumerate(("q_ss", "theta_rz")):
        assert f.variables[v].dimensions == ("Time", "probability") and f.variables[v]._FillValue == FILL
        assert same_bits(f.variables[v][:], values[:, j]) and same_bits(live[v], values[:, j]), v
        for key, col in (("n", 2 + 2 * j), ("nan", 3 + 2 * j)):
            np.testing.assert_array_equal(f.variables[f"{v}_{key}"][:], hdr[:, col])
            np.testing.assert_array_equal(live[f"{v}_{key}"], hdr[:, col])


def test_a_row_without_a_column_holds_the_fill_value(tmp_path):
    """m == 0: NaN on the device and from read(), _FillValue in the file."""
    import types

    from nc_util import netcdf_file
    from roger_amd import bands

    rows = (np.array([[0, DAY, 0, 3], [1, 2 * DAY, 3, 0]], dtype=np.int64), np.array([[[np.nan, np.nan]], [[1.0, 2.0]]]))
    ctx = types.SimpleNamespace(bands_count=lambda: 2, bands_read=lambda first, n: (rows[0][first:first + n], rows[1][first:first + n]))
    b = bands.Bands()
    b._on, b._names, b._kinds, b._probs, b._path = True, ["q_ss"], [0], (0.1, 0.9), str(tmp_path / "run.bands.nc")
    state = types.SimpleNamespace(bands=b, backend_context=ctx, settings=types.SimpleNamespace(time_origin="1900-01-01", identifier="run"))
    b._state = state
    live = b.read()
    assert np.isnan(live["q_ss"][0]).all() and live["q_ss"][1].tolist() == [1.0, 2.0] and live["q_ss_nan"].tolist() == [3, 0]
    bands.close(state)
    f = netcdf_file(b._path)
    assert (f.variables["q_ss"][:][0] == bands.FILL).all() and f.variables["q_ss"][:][1].tolist() == [1.0, 2.0]
    assert f.variables["q_ss_n"][:].tolist() == [0, 3]


def test_a_clock_past_the_start_counts_from_the_next_boundary_and_the_rank_gets_its_block(monkeypatch, tmp_path):
    import types

    from roger_amd import bands, runtime_state

    calls = []
    mask = (np.arange(24).reshape(6, 4) % 3 != 0)
    ctx = types.SimpleNamespace(bands_configure=lambda *a: calls.append(a))
    meta = types.SimpleNamespace(plane=7, dtype=None)
    state = types.SimpleNamespace(
        settings=types.SimpleNamespace(nx=6, ny=4, enable_offline_transport=False, identifier="run"), var_meta={"q_ss": meta},
        variables=types.SimpleNamespace(time=3 * DAY + 600, flush_to_device=lambda: None), backend_context=ctx, bands=bands.Bands())
    b = state.bands
    b.variables, b.mask, b.base_output_path, b.capacity = ["q_ss"], mask, str(tmp_path), 16
    monkeypatch.setattr(bands, "rs", types.SimpleNamespace(num_proc=(2, 1), diskless_mode=False))
    monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self: 1))
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
    bands.initialize(state)
    bands.start(state)
    (names, kinds, probs, f, t_first, local, capacity), = calls
    assert names == ["q_ss"] and kinds == [0] and probs == (0.05, 0.5, 0.95) and f == DAY and t_first == 4 * DAY and capacity == 16
    np.testing.assert_array_equal(local, mask[3:].reshape(-1))
    assert local.dtype == np.uint8 and b._on and b._path.endswith("run.bands.0001.nc")
    calls.clear()
    state.bands = b2 = bands.Bands()
    b2.variables, b2.mask = ["q_ss"], np.arange(24).reshape(6, 4) < 12
    bands.initialize(state)
    bands.start(state)
    assert not calls and not b2._on and b2.read() is None


def test_refusals(bands_backend, tmp_path):
    for kw, exc, text in ((dict(variables=[f"v{k}" for k in range(9)]), ValueError, r"9 variables \(at most 8\)"),
                          (dict(probabilities=tuple(np.linspace(0.1, 0.9, 9))), ValueError, r"9 probabilities \(1 \.\.\. 8\)"),
                          (dict(probabilities=()), ValueError, r"0 probabilities"),
                          (dict(probabilities=(0.5, 1.5)), ValueError, r"probabilities = \(0\.5, 1\.5\) \(each within \[0, 1\]\)"),
                          (dict(probabilities=(-0.1,)), ValueError, "each within"),
                          (dict(probabilities=(np.nan,)), ValueError, "each within"),
                          (dict(start=600), ValueError, "start = 600 s is not a multiple of the frequency"),
                          (dict(frequency=7200), ValueError, "frequency = 7200"),
                          (dict(variables=["lu_id"]), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(variables=["no_such_variable"]), NotImplementedError, "no_such_variable"),
                          (dict(variables=["q_ss", "q_ss"]), ValueError, "named twice"),
                          (dict(aggregation={"q_ss": "mean"}), ValueError, "'mean'"),
                          (dict(aggregation={"aet": "sum"}), ValueError, "aggregation names 'aet'"),
                          (dict(capacity=0), ValueError, "capacity = 0"),
                          (dict(mask=np.ones((4, 5))), ValueError, r"mask has shape \(4, 5\)"),
                          (dict(mask=np.zeros((4, 4))), ValueError, "the mask holds no column")):
        model = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model = make_model(tmp_path, ndays=1, variables=[])
    model.setup()
    model.run()
    assert bands_backend[-1]._bands is None and model.state.bands.read() is None and not list(tmp_path.iterdir())


def test_the_offline_transport_is_refused():
    from roger_amd import bands
    from roger_amd.state import RogerState

    st = RogerState()
    assert not st.bands.active and st.bands.probabilities == (0.05, 0.5, 0.95)
    bands.initialize(st)
    st.bands.variables = ["q_ss"]
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    with pytest.raises(NotImplementedError, match="offline transport"):
        bands.initialize(st)
