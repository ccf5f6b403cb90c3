"""CPU: `state.bands.weights` (roger_amd/bands.py) -- the quantisation, the refusals, the mask folded in, `read()` and the file, the ranks
and resuming -- through fake contexts over tests/bands_weighted_reference.py (as tests/test_bands_zonal_host.py does for the zones), and
once through a setup script on the oracle double."""
import types

import numpy as np
import pytest

from bands_reference import LAST, SUM
from bands_weighted_reference import HostWeightedBands, oracle_double, weighted_quantiles_of
from test_bands_zonal_host import fake_state, on_rank

DAY = 86400
PROBS = (0.0, 0.5, 1.0)
ATTRIBUTE = "integer 0 ... 65535: rint(w / max(w) * 65535)"


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)).all()


def initialized(weights, nx=4, ny=3, **kw):
    from roger_amd import bands

    state = fake_state(nx, ny, types.SimpleNamespace())
    b = state.bands
    b.variables, b.weights = ["q_ss"], weights
    for k, v in kw.items():
        setattr(b, k, v)
    bands.initialize(state)
    return b


# ---- the quantisation and the refusals ----
def test_floats_become_the_stated_integers_and_integers_are_taken_as_they_are():
    w = np.array([[0.0, 1e-9, 0.25], [0.5, 1.0, 2.0], [1.0 / 3.0, 1.9999, 1.5e-5], [1.6e-5, 0.1, 0.7]])
    b = initialized(w)
    want = np.rint(w / 2.0 * 65535.0).astype(np.uint16)
    assert b._weights.dtype == np.uint16 and b._weights.shape == (4, 3) and (b._weights == want).all()
    assert b._weights[0].tolist() == [0, 0, 8192] and b._weights[1].tolist() == [16384, 32768, 65535]     # 8191.875 and 16383.75 round up
    assert b._weights[2, 2] == 0 and b._weights[3, 0] == 1                                            # 0.49 rounds to 0: takes no part
    assert (initialized(w.astype(np.float32))._weights == np.rint(w.astype(np.float32).astype(np.float64) / 2.0 * 65535.0).astype(np.uint16)).all()
    ints = np.array([[0, 1, 2], [65535, 7, 0], [3, 3, 3], [1, 0, 65534]])
    for dtype in (np.int64, np.int32, np.uint16, np.uint8):
        a = ints.astype(dtype) if dtype != np.uint8 else (ints % 256).astype(dtype)
        b = initialized(a)
        assert b._weights.dtype == np.uint16 and (b._weights == a).all()                                 # not rescaled
    assert initialized(None)._weights is None


@pytest.mark.parametrize("weights,kw,text", [
    (np.array([[1.0, 2.0, 3.0]] * 3 + [[1.0, -0.5, -2.0]]), {}, r"bands: weight -0\.5 at cell \(3, 1\) \(weights are finite and >= 0\)"),
    (np.array([[1.0, np.nan, 3.0]] + [[1.0, 2.0, 3.0]] * 3), {}, r"bands: weight nan at cell \(0, 1\) \(weights are finite and >= 0\)"),
    (np.array([[1.0, 2.0, 3.0]] * 2 + [[np.inf, 2.0, 3.0]] * 2), {}, r"bands: weight inf at cell \(2, 0\) \(weights are finite and >= 0\)"),
    (np.zeros((4, 3)), {}, r"bands: every weight is 0 \(the largest weight must be positive\)"),
    (np.zeros((4, 3), dtype=np.int64), {}, r"bands: no column takes part \(a column takes part iff its integer weight is > 0\)"),
    (np.array([[1, 2, 3]] * 3 + [[1, 65536, 70000]]), {}, r"bands: weight 65536 at cell \(3, 1\) \(integer weights lie within 0 \.\.\. 65535\)"),
    (np.array([[1, 2, 3]] * 3 + [[1, 2, -1]]), {}, r"bands: weight -1 at cell \(3, 2\) \(integer weights lie within 0 \.\.\. 65535\)"),
    (np.ones((3, 4)), {}, r"bands: the weights map has shape \(3, 4\), the grid 4 x 3 columns"),
    (np.ones((4, 3)), dict(zones=np.ones((4, 3), dtype=int)), r"bands: weights with zones is not built"),
    (np.eye(4, 3), dict(mask=1 - np.eye(4, 3)), r"bands: no column takes part \(a column takes part iff its integer weight is > 0 and mask != 0\)"),
    (np.ones((4, 3), dtype=complex), {}, r"bands: the weights have dtype complex128"),
])
def test_every_refusal_with_its_message(weights, kw, text):
    with pytest.raises(ValueError, match=text):
        initialized(weights, **kw)


# ---- through a fake context ----
class FakeWeightedContext:
    """bands_configure / bands_count / bands_read / bands_weight_sums / bands_state / bands_restore of `_native.Context` over
    tests/bands_weighted_reference.py; `feed` is a step."""

    def __init__(self, n):
        self.n, self.calls, self.h, self.row0 = n, [], None, 0

    def bands_configure(self, names, kinds, probs, interval, t_first, mask, capacity, weights=None):
        self.calls.append(dict(names=names, kinds=kinds, probs=probs, interval=interval, t_first=t_first, mask=mask, capacity=capacity, weights=weights))
        assert mask is None and weights.dtype == np.uint16 and weights.shape == (self.n,)
        self.h, self.row0 = HostWeightedBands(kinds, probs, self.n, weights, interval, t_first), 0

    def feed(self, t0, t1, planes):
        self.h.add(t0, t1, planes)

    def bands_count(self):
        return self.row0 + len(self.h.rows()[0])

    def bands_read(self, first, n):
        return tuple(a[first - self.row0:first - self.row0 + n].copy() for a in self.h.rows()[:2])

    def bands_weight_sums(self, first, n):
        return self.h.rows()[2][first - self.row0:first - self.row0 + n].copy()

    def bands_state(self):
        return self.h.acc.copy()

    def bands_restore(self, acc, rows):
        self.h.acc[:], self.row0 = acc, int(rows)


W43 = np.array([[0.9, 0.0, 0.2], [0.45, 0.1, 0.0], [0.3, 0.3, 1e-7], [0.05, 0.6, 0.15]])
M43 = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])


def days_of(rng, n, ndays):
    days = [[rng.normal(size=n), rng.normal(size=n)] for _ in range(ndays)]
    days[1][1][[0, 6]] = np.nan
    return days


def test_read_and_the_file_carry_the_weight_sums_and_a_mask_is_folded_in(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    nx, ny = 4, 3
    ctx = FakeWeightedContext(nx * ny)
    state = fake_state(nx, ny, ctx)
    on_rank(monkeypatch, 0, (1, 1), diskless=False)
    b = state.bands
    b.variables, b.aggregation, b.probabilities, b.weights, b.mask, b.base_output_path = ["q_ss", "theta_rz"], {"theta_rz": "last"}, PROBS, W43, M43, str(tmp_path)
    bands.initialize(state)
    bands.start(state)
    (call,) = ctx.calls
    q = np.rint(W43 / 0.9 * 65535.0).astype(np.uint16)
    folded = np.where(M43 != 0, q, 0).reshape(-1)
    assert call["weights"].tolist() == folded.tolist() and call["mask"] is None and call["kinds"] == [SUM, LAST]
    assert folded[4] == 0 and q[1, 1] > 0 and folded[9] == 0 and q[2, 2] == 0                        # masked out; rounded to 0
    days = days_of(np.random.default_rng(3), nx * ny, 3)
    for k, planes in enumerate(days):
        ctx.feed(k * DAY, (k + 1) * DAY, planes)
    live = b.read()
    assert list(live) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan", "q_ss_w", "theta_rz", "theta_rz_n", "theta_rz_nan", "theta_rz_w"]
    for k, planes in enumerate(days):
        for v, x in zip(("q_ss", "theta_rz"), planes):
            want, m, n_nan, W = weighted_quantiles_of(x, folded, PROBS)
            assert same_bits(live[v][k], want) and (live[f"{v}_n"][k], live[f"{v}_nan"][k], live[f"{v}_w"][k]) == (m, n_nan, W)
    assert live["q_ss_w"].dtype == np.int64 and live["q_ss_w"].shape == (3,) and live["q_ss_w"][0] == int(folded.astype(np.int64).sum())
    assert live["theta_rz_nan"].tolist() == [0, 2, 0] and live["theta_rz_w"][1] == int(folded.astype(np.int64).sum()) - int(folded[0]) - int(folded[6])
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert list(rec["variables"]) == ["Time", "interval", "probability", "q_ss", "q_ss_n", "q_ss_nan", "q_ss_w", "theta_rz", "theta_rz_n", "theta_rz_nan", "theta_rz_w"]
    assert rec["attributes"]["weights"] == ATTRIBUTE and rec["attributes"]["columns"] == "this rank's block"
    for v in ("q_ss", "theta_rz"):
        dims, data, attrs = rec["variables"][f"{v}_w"][:3]
        assert dims == ("Time",) and np.asarray(data).tolist() == live[f"{v}_w"].tolist()
        assert attrs["long_name"] == f"{v}: sum of the integer weights of the columns that took part"
        assert same_bits(np.asarray(rec["variables"][v][1]), live[v])


def test_the_global_maximum_is_used_on_a_split_grid(monkeypatch):
    """2 x 1 ranks on 4 x 2: the maximum sits in rank 0's block, and rank 1 forms its integers from it all the same; with rank 1's
    columns weighted 0 it configures nothing."""
    from roger_amd import bands

    w = np.array([[4.0, 1.0], [0.5, 2.0], [1.0, 0.0], [3.0, 0.25]])
    q = np.rint(w / 4.0 * 65535.0).astype(np.uint16)
    for weights, want_on in ((w, {0: True, 1: True}), (np.where(np.arange(4)[:, None] < 2, w, 0.0), {0: True, 1: False})):
        for rank in (0, 1):
            ctx = FakeWeightedContext(4)
            state = fake_state(4, 2, ctx)
            on_rank(monkeypatch, rank, (2, 1), diskless=True)
            b = state.bands
            b.variables, b.weights, b.probabilities = ["q_ss"], weights, PROBS
            bands.initialize(state)
            bands.start(state)
            assert b._on == want_on[rank] and len(ctx.calls) == int(want_on[rank]) and (b._weights[:2] == q[:2]).all()
            if not b._on:
                assert b.read() is None and b._path is None
                continue
            assert ctx.calls[0]["weights"].tolist() == q[2 * rank:2 * rank + 2].reshape(-1).tolist()
            ctx.feed(0, DAY, [np.arange(4.0)])
            assert b.read()["q_ss_w"].tolist() == [int(q[2 * rank:2 * rank + 2].astype(np.int64).sum())]


def test_without_weights_the_call_read_and_the_file_are_todays(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    rows = (np.array([[0, DAY, 0, 3], [1, 2 * DAY, 3, 0]], dtype=np.int64), np.array([[[np.nan, np.nan]], [[1.0, 2.0]]]))
    calls = []
    ctx = types.SimpleNamespace(bands_configure=lambda *a, **kw: calls.append((a, kw)), bands_count=lambda: 2,
                                bands_read=lambda first, n: (rows[0][first:first + n], rows[1][first:first + n]))
    state = fake_state(4, 2, ctx)
    on_rank(monkeypatch, 0, (1, 1), diskless=False)
    b = state.bands
    assert b.weights is None
    b.variables, b.probabilities, b.base_output_path = ["q_ss"], (0.1, 0.9), str(tmp_path)
    bands.initialize(state)
    bands.start(state)
    assert calls == [((["q_ss"], [SUM], (0.1, 0.9), DAY, 0, None, 4096), {})]                 # no `weights` keyword, no other call
    assert list(b.read()) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan"]
    assert list(b._request(state)) == ["variables", "kinds", "probabilities", "frequency", "start", "mask", "zones", "grid"]
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert list(rec["variables"]) == ["Time", "interval", "probability", "q_ss", "q_ss_n", "q_ss_nan"]
    assert list(rec["attributes"]) == ["date_created", "roger_version", "comment", "columns", "setup_identifier", "frequency_seconds",
                                       "first_interval_starts_seconds"]


# ---- resuming ----
def weighted_run(monkeypatch, weights, time=0, resume=True, carried=None, restart_file=None, mask=None):
    from roger_amd import bands

    ctx = FakeWeightedContext(12) if weights is not None else types.SimpleNamespace(bands_configure=lambda *a, **kw: None, bands_restore=lambda *a: None)
    state = fake_state(4, 3, ctx, time=time)
    on_rank(monkeypatch, 0, (1, 1), diskless=True)
    b = state.bands
    b.variables, b.aggregation, b.probabilities, b.weights, b.mask, b.resume = ["q_ss", "theta_rz"], {"theta_rz": "last"}, PROBS, weights, mask, resume
    b._restart_file, b._carried = restart_file, carried
    bands.initialize(state)
    bands.start(state)
    return state, ctx, b


def halves(days):
    """Two steps a day: [(t0, t1, planes)]."""
    return [(k * DAY + h * DAY // 2, k * DAY + (h + 1) * DAY // 2, [days[k][0] * (h + 1), days[k][1] + h]) for k in range(len(days)) for h in (0, 1)]


def test_a_continued_weighted_run_ends_with_the_uninterrupted_runs_rows(monkeypatch):
    steps = halves(days_of(np.random.default_rng(9), 12, 4))
    _, ctx_a, a = weighted_run(monkeypatch, W43, resume=False)
    for t0, t1, planes in steps:
        ctx_a.feed(t0, t1, planes)
    whole = a.read()
    assert whole["interval"].tolist() == [0, 1, 2, 3]
    stop = 5                                                                # the restart file is written in the middle of day 2
    state_b, ctx_b, b = weighted_run(monkeypatch, W43)
    for t0, t1, planes in steps[:stop]:
        ctx_b.feed(t0, t1, planes)
    group = b.restart_state(state_b)
    assert sorted(group) == sorted(["acc", "scalars"] + [f"request_{k}" for k in ("variables", "kinds", "probabilities", "frequency", "start", "mask", "zones", "grid", "weights")])
    assert group["request_weights"].dtype == np.int64 and (group["request_weights"] == np.rint(W43 / 0.9 * 65535.0)).all() and group["scalars"].tolist() == [0, 2]
    first = b.read()
    _, ctx_c, c = weighted_run(monkeypatch, W43, time=steps[stop - 1][1], carried=group, restart_file="run.restart.h5")
    assert ctx_c.calls[0]["t_first"] == 0 and ctx_c.row0 == 2 and same_bits(ctx_c.h.acc, ctx_b.h.acc)
    for t0, t1, planes in steps[stop:]:
        ctx_c.feed(t0, t1, planes)
    rest = c.read()
    assert rest["interval"].tolist() == [2, 3]
    for key in whole:
        joined = np.concatenate([first[key], rest[key]])
        assert same_bits(joined, whole[key]) if joined.dtype.kind == "f" else joined.tolist() == whole[key].tolist(), key
    assert (whole["q_ss_w"] > 0).all()


def test_the_two_mismatch_errors_name_the_weights(monkeypatch):
    state_b, ctx_b, b = weighted_run(monkeypatch, W43)
    with_weights = b.restart_state(state_b)
    state_p, _, p = weighted_run(monkeypatch, None)
    p._on = False
    without = dict({f"request_{k}": v for k, v in p._request(state_p).items()}, acc=np.zeros((2, 12)), scalars=np.array([0, 0]))
    assert "request_weights" not in without
    with pytest.raises(RuntimeError, match=r"bands: resume = True, but the restart file old\.h5 was written with weights = an array of shape \(4, 3\) and "
                                           r"this run asks for weights = None: a resumed observer takes the same request"):
        weighted_run(monkeypatch, None, carried=with_weights, restart_file="old.h5")
    with pytest.raises(RuntimeError, match=r"bands: resume = True, but the restart file old\.h5 was written with weights = nothing and this run asks for "
                                           r"weights = an array of shape \(4, 3\)"):
        weighted_run(monkeypatch, W43, carried=without, restart_file="old.h5")
    other = W43.copy()
    other[2, 1] = 0.31
    with pytest.raises(RuntimeError, match=r"was written with weights = an array of shape \(4, 3\) and this run asks for weights = an array of shape \(4, 3\), "
                                           r"first difference at flat index 7"):
        weighted_run(monkeypatch, other, carried=with_weights, restart_file="old.h5")
    weighted_run(monkeypatch, None, carried=without, restart_file="old.h5")                  # files of runs without weights resume as before


# ---- a setup script on the oracle double ----
@pytest.fixture
def weighted_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []
    double = oracle_double()

    def make(*a, **k):
        made.append(double(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


def test_a_script_with_weights_writes_the_rows_of_the_doubles_planes(weighted_backend, tmp_path):
    import test_bands_reference as plain
    from nc_util import netcdf_file

    rng = np.random.default_rng(21)
    weights = rng.random((4, 4)) ** 3
    weights[1, 2] = 0.0
    model = plain.make_model(tmp_path, probabilities=plain.PROBS, weights=weights)             # (its mask on top)
    model.setup()
    ctx = weighted_backend[-1]
    steps = []
    accumulate = ctx._accumulate
    ctx._accumulate = lambda: (accumulate(), steps.append((int(ctx.st.scal.time) - int(ctx.st.scal.dt_secs), int(ctx.st.scal.time),
                                                           {v: ctx.download(v).copy() for v in ("q_ss", "theta_rz")})))[0]
    model.run()
    folded = np.where(plain.MASK != 0, np.rint(weights / weights.max() * 65535.0), 0).astype(np.uint16).reshape(-1)
    h = HostWeightedBands([SUM, LAST], plain.PROBS, 16, folded, DAY)
    for t0, t1, p in steps:
        h.add(t0, t1, [p["q_ss"], p["theta_rz"]])
    hdr, values, wsum = h.rows()
    assert len(hdr) == 6 and (hdr[:, 2] == int((folded != 0).sum())).all() and (wsum == int(folded.astype(np.int64).sum())).all()
    live = model.state.bands.read()
    f = netcdf_file(str(tmp_path / "GoldenSVAT.bands.nc"))
    assert f.weights == ATTRIBUTE.encode()
    for j, v in enumerate(("q_ss", "theta_rz")):
        assert same_bits(f.variables[v][:], values[:, j]) and same_bits(live[v], values[:, j]), v
        np.testing.assert_array_equal(f.variables[f"{v}_w"][:], wsum[:, j])
        np.testing.assert_array_equal(live[f"{v}_w"], wsum[:, j])
        np.testing.assert_array_equal(f.variables[f"{v}_n"][:], hdr[:, 2 + 2 * j])
