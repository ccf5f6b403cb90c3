"""CPU: `state.bands.observations` (roger_amd/bands.py) -- the refusals, `read()` and the file, plain, per zone and weighted, the index of
a run that starts past `start`, resuming, and the two pure functions -- through a fake context over tests/bands_obs_reference.py, in the
manner of tests/test_bands_weighted_host.py."""
import types

import numpy as np
import pytest

from bands_obs_reference import HostObsBands, HostObsWeightedBands, HostObsZonalBands, pair_of
from bands_reference import LAST, SUM
from test_bands_zonal_host import fake_state, on_rank

DAY = 86400
PROBS = (0.05, 0.5, 0.95)
FILL = 9.969209968386869e+36                # roger_amd.scores.FILL: the files' _FillValue


class FakeObsContext:
    """The bands_* methods of `_native.Context` over tests/bands_obs_reference.py, whichever configuration; `feed` is a step."""

    def __init__(self, n):
        self.n, self.calls, self.obs_calls, self.h, self.row0 = n, [], [], None, 0

    def bands_configure(self, names, kinds, probs, interval, t_first, mask, capacity, zones=None, n_zones=None, weights=None):
        self.calls.append(dict(names=names, kinds=kinds, probs=probs, interval=interval, t_first=t_first, mask=mask, capacity=capacity, zones=zones,
                               n_zones=n_zones, weights=weights))
        self.row0 = 0
        if zones is not None:
            self.h = HostObsZonalBands(kinds, probs, self.n, zones, n_zones, interval, t_first)
        elif weights is not None:
            self.h = HostObsWeightedBands(kinds, probs, self.n, weights, interval, t_first)
        else:
            self.h = HostObsBands(kinds, probs, self.n, mask, interval, t_first)

    def bands_observations(self, obs, first_index=0):
        assert len(self.calls) > len(self.obs_calls), "bands_observations comes behind the configure call"
        self.obs_calls.append(dict(obs=np.array(obs), first_index=first_index))
        self.h.observe(obs, first_index)

    def feed(self, t0, t1, planes):
        self.h.add(t0, t1, planes)

    def bands_count(self):
        return self.row0 + len(self.h.rows()[0])

    def _cut(self, arrays, first, n):
        return tuple(a[first - self.row0:first - self.row0 + n].copy() for a in arrays)

    def bands_read(self, first, n):
        return self._cut(self.h.rows()[:2], first, n)

    def bands_zonal_read(self, first, n):
        return self._cut(self.h.rows(), first, n)

    def bands_weight_sums(self, first, n):
        return self._cut(self.h.rows()[2:], first, n)[0]

    def bands_obs_read(self, first, n):
        assert self.obs_calls, "no observations are set"
        return self._cut((self.h.pair_rows(),), first, n)[0]

    def bands_state(self):
        return self.h.acc.copy()

    def bands_restore(self, acc, rows):
        self.h.acc[:], self.row0 = acc, int(rows)


def initialized(observations, nx=4, ny=3, **kw):
    from roger_amd import bands

    state = fake_state(nx, ny, types.SimpleNamespace())
    b = state.bands
    b.variables, b.observations = ["q_ss", "theta_rz"], observations
    for k, v in kw.items():
        setattr(b, k, v)
    bands.initialize(state)
    return b


ZONES = np.array([[7, 3, 9], [0, 7, -5], [3, 3, 9], [7, 0, 7]])


# ---- validation ----
@pytest.mark.parametrize("observations,kw,text", [
    ({"q_sub": np.ones(3)}, {}, r"bands: observations names 'q_sub', which is not among the variables"),
    ({"q_ss": np.arange(3)}, {}, r"bands: the observations of 'q_ss' have dtype int64 \(a float array, NaN: missing\)"),
    ({"q_ss": np.ones((2, 3))}, {}, r"bands: the observations of 'q_ss' have shape \(2, 3\) \(\(n_intervals,\)\)"),
    ({"q_ss": np.ones((2, 3))}, dict(zones=ZONES), r"bands: the observations of 'q_ss' have shape \(2, 3\) \(\(n_intervals,\) or \(3, n_intervals\): a series per zone"),
    ({"q_ss": np.ones((1, 3, 3))}, dict(zones=ZONES), r"bands: the observations of 'q_ss' have shape \(1, 3, 3\)"),
    ({"theta_rz": np.ones(0)}, {}, r"bands: the observations of 'theta_rz' are empty \(at least one interval\)"),
    ({"theta_rz": np.ones((3, 0))}, dict(zones=ZONES), r"bands: the observations of 'theta_rz' are empty"),
])
def test_every_refusal_with_its_message(observations, kw, text):
    with pytest.raises(ValueError, match=text):
        initialized(observations, **kw)


def test_the_array_handed_to_the_device():
    assert initialized({})._obs is None
    b = initialized({"theta_rz": np.array([1.0, np.nan, 3.0], dtype=np.float32)})
    assert b._obs.dtype == np.float64 and b._obs.shape == (2, 3) and np.isnan(b._obs[0]).all() and b._obs[1].tolist()[::2] == [1.0, 3.0]
    b = initialized({"q_ss": np.arange(4.0), "theta_rz": np.ones(2)})                 # the shorter series is missing behind its end
    assert b._obs[0].tolist() == [0.0, 1.0, 2.0, 3.0] and b._obs[1].tolist()[:2] == [1.0, 1.0] and np.isnan(b._obs[1, 2:]).all()
    b = initialized({"q_ss": np.arange(2.0), "theta_rz": np.arange(6.0).reshape(3, 2)}, zones=ZONES)
    assert b._ids.tolist() == [3, 7, 9] and b._obs.shape == (2, 3, 2)
    assert (b._obs[0] == np.arange(2.0)).all() and (b._obs[1] == np.arange(6.0).reshape(3, 2)).all()    # one series for every zone; a series per zone


# ---- read() and the file ----
def run(monkeypatch, tmp_path, n_days=4, time=0, feed_from=0, **kw):
    from roger_amd import bands

    nx, ny = 4, 3
    ctx = FakeObsContext(nx * ny)
    state = fake_state(nx, ny, ctx, time=time)
    on_rank(monkeypatch, 0, (1, 1), diskless=tmp_path is None)
    b = state.bands
    b.variables, b.aggregation, b.probabilities = ["q_ss", "theta_rz"], {"theta_rz": "last"}, PROBS
    if tmp_path is not None:
        b.base_output_path = str(tmp_path)
    for k, v in kw.items():
        setattr(b, k, v)
    bands.initialize(state)
    bands.start(state)
    rng = np.random.default_rng(3)
    days = [[np.round(rng.normal(size=nx * ny)), np.round(rng.normal(size=nx * ny) * 2) / 2] for _ in range(n_days)]
    days[1][1][[0, 6]] = np.nan
    for k in range(feed_from, n_days):
        ctx.feed(k * DAY, (k + 1) * DAY, days[k])
    return state, ctx, b, days


OBS_Q = np.array([0.0, np.nan, 1.0])                                                    # shorter than the run; missing on day 1
OBS_T = np.array([0.5, -0.5, 0.0, 9.0])


def test_plain_read_and_file(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    mask = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
    state, ctx, b, days = run(monkeypatch, tmp_path, observations={"q_ss": OBS_Q, "theta_rz": OBS_T}, mask=mask)
    assert len(ctx.calls) == 1 and len(ctx.obs_calls) == 1 and ctx.obs_calls[0]["first_index"] == 0 and ctx.obs_calls[0]["obs"].shape == (2, 4)
    live = b.read()
    assert list(live) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan",
                          "q_ss_obs", "q_ss_below", "q_ss_equal", "theta_rz_obs", "theta_rz_below", "theta_rz_equal"]
    on = mask.reshape(-1) != 0
    for j, (v, series) in enumerate((("q_ss", OBS_Q), ("theta_rz", OBS_T))):
        assert live[f"{v}_obs"].dtype == np.float64 and live[f"{v}_below"].dtype == np.int64 and live[f"{v}_equal"].dtype == np.int64
        for k in range(4):
            o = series[k] if k < len(series) else np.nan
            assert (live[f"{v}_below"][k], live[f"{v}_equal"][k]) == pair_of(days[k][j][on], o), (v, k)
            assert np.isnan(live[f"{v}_obs"][k]) if o != o else live[f"{v}_obs"][k] == o
    assert live["q_ss_below"].tolist()[1] == -1 and live["q_ss_equal"].tolist()[3] == -1 and (live["q_ss_equal"][[0, 2]] > 0).all()
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert sorted(rec["variables"]) == sorted(["Time", "interval", "probability", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan",
                                               "q_ss_obs", "q_ss_below", "q_ss_equal", "q_ss_pit", "theta_rz_obs", "theta_rz_below", "theta_rz_equal", "theta_rz_pit"])
    assert rec["attributes"]["observations"] == bands.OBSERVATIONS_ATTRIBUTE and "below + equal >= T(p_lo) and below < T(p_hi)" in bands.OBSERVATIONS_ATTRIBUTE
    assert list(rec["attributes"])[-1] == "observations"
    for v in ("q_ss", "theta_rz"):
        for tail in ("obs", "below", "equal", "pit"):
            assert rec["variables"][f"{v}_{tail}"][0] == ("Time",)
        below, equal, total = live[f"{v}_below"], live[f"{v}_equal"], live[f"{v}_n"]
        assert np.asarray(rec["variables"][f"{v}_below"][1]).tolist() == below.tolist() and np.asarray(rec["variables"][f"{v}_equal"][1]).tolist() == equal.tolist()
        want = np.where(below >= 0, (below + equal / 2.0) / total, FILL)
        assert np.asarray(rec["variables"][f"{v}_pit"][1]).tolist() == want.tolist() and rec["variables"][f"{v}_pit"][2]["_FillValue"] == FILL
        assert np.asarray(rec["variables"][f"{v}_obs"][1]).tolist() == np.where(np.isnan(live[f"{v}_obs"]), FILL, live[f"{v}_obs"]).tolist()
        assert rec["variables"][f"{v}_obs"][2]["_FillValue"] == FILL
    assert np.asarray(rec["variables"]["q_ss_pit"][1])[[1, 3]].tolist() == [FILL, FILL]


def test_zonal_read_and_file(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    per_zone = np.array([[0.0, 1.0, -1.0, np.nan], [0.5, 0.5, 0.5, 0.5], [2.0, 2.0, 2.0, 2.0]])
    state, ctx, b, days = run(monkeypatch, tmp_path, observations={"theta_rz": per_zone}, zones=ZONES, mask=ZONES != 9)   # zone 9: emptied
    assert ctx.obs_calls[0]["obs"].shape == (2, 3, 4) and np.isnan(ctx.obs_calls[0]["obs"][0]).all()
    live = b.read()
    assert list(live)[-3:] == ["theta_rz_obs", "theta_rz_below", "theta_rz_equal"] and "q_ss_obs" not in live and live["theta_rz_below"].shape == (4, 3)
    index = ctx.calls[0]["zones"]
    for k in range(4):
        for z in range(3):
            assert (live["theta_rz_below"][k, z], live["theta_rz_equal"][k, z]) == pair_of(days[k][1][index == z], per_zone[z, k]), (k, z)
    assert (live["theta_rz_below"][:, 2] == 0).all() and (live["theta_rz_equal"][:, 2] == 0).all() and live["theta_rz_below"][3, 0] == -1
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert sorted(set(rec["variables"]) - {"Time", "interval", "probability", "zone", "ncells", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan"}) == [
        "theta_rz_below", "theta_rz_equal", "theta_rz_obs", "theta_rz_pit"]
    assert rec["variables"]["theta_rz_pit"][0] == ("Time", "zone") and rec["attributes"]["observations"] == bands.OBSERVATIONS_ATTRIBUTE
    pit = np.asarray(rec["variables"]["theta_rz_pit"][1])
    assert (pit[:, 2] == FILL).all() and pit[3, 0] == FILL                              # nothing took part; no observation
    total = live["theta_rz_n"]
    ok = (live["theta_rz_below"] >= 0) & (total > 0)
    assert np.array_equal(pit[ok], ((live["theta_rz_below"] + live["theta_rz_equal"] / 2.0) / np.where(ok, total, 1))[ok]) and ok.sum() >= 6


def test_weighted_read_and_file(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    w = np.array([[3, 0, 1], [65535, 2, 0], [1, 1, 1], [7, 9, 2]])
    state, ctx, b, days = run(monkeypatch, tmp_path, observations={"q_ss": OBS_Q}, weights=w)
    live = b.read()
    assert list(live) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan", "q_ss_w", "theta_rz", "theta_rz_n", "theta_rz_nan", "theta_rz_w",
                          "q_ss_obs", "q_ss_below", "q_ss_equal"]
    for k in range(4):
        o = OBS_Q[k] if k < 3 else np.nan
        assert (live["q_ss_below"][k], live["q_ss_equal"][k]) == pair_of(days[k][0], o, w.reshape(-1)), k
    assert live["q_ss_below"].max() > 12                                               # weights, not columns
    bands.close(state)
    rec = nc4lite.read(b._path)
    pit = np.asarray(rec["variables"]["q_ss_pit"][1])
    assert pit[[1, 3]].tolist() == [FILL, FILL] and pit[0] == (live["q_ss_below"][0] + live["q_ss_equal"][0] / 2.0) / live["q_ss_w"][0]
    assert list(rec["attributes"])[-2:] == ["weights", "observations"]


def test_without_observations_nothing_changes(monkeypatch, tmp_path):
    """The same calls, the same `read()` keys and the same file as before: byte for byte, the creation date aside."""
    from roger_amd import bands, nc4lite

    state, ctx, b, _ = run(monkeypatch, tmp_path)
    assert b.observations == {} and ctx.obs_calls == [] and len(ctx.calls) == 1
    live = b.read()
    assert list(live) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan"]
    assert list(b._request(state)) == ["variables", "kinds", "probabilities", "frequency", "start", "mask", "zones", "grid"]
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert list(rec["variables"]) == ["Time", "interval", "probability", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan"]
    assert list(rec["attributes"]) == ["date_created", "roger_version", "comment", "columns", "setup_identifier", "frequency_seconds",
                                       "first_interval_starts_seconds"]
    # the rows of an observed run are the same rows, and its file holds the same bytes for them
    state_o, _, o, _ = run(monkeypatch, tmp_path / "observed", observations={"q_ss": OBS_Q})
    seen = o.read()
    for key in live:
        assert seen[key].dtype == live[key].dtype and seen[key].tobytes() == live[key].tobytes(), key
    bands.close(state_o)
    rec_o = nc4lite.read(o._path)
    for key in rec["variables"]:
        assert np.asarray(rec_o["variables"][key][1]).tobytes() == np.asarray(rec["variables"][key][1]).tobytes() and rec_o["variables"][key][2] == rec["variables"][key][2], key


# ---- the index of a run that starts past `start` ----
def test_first_index_of_a_run_that_starts_past_start(monkeypatch):
    series = np.arange(10.0) * 0.5 - 1.0
    # start = day 1, the clock at day 3 and a half: the first counted interval is day 4, the fourth element of the series from `start`
    state, ctx, b, days = run(monkeypatch, None, n_days=7, time=3 * DAY + DAY // 2, feed_from=4, observations={"q_ss": series}, start=DAY)
    assert ctx.calls[0]["t_first"] == 4 * DAY and ctx.obs_calls[0]["first_index"] == 3
    live = b.read()
    assert live["interval"].tolist() == [0, 1, 2] and live["q_ss_obs"].tolist() == series[3:6].tolist()
    for row, k in enumerate((4, 5, 6)):
        assert (live["q_ss_below"][row], live["q_ss_equal"][row]) == pair_of(days[k][0], series[k - 1])
    # the clock at `start`: the series from its first element
    _, ctx0, b0, _ = run(monkeypatch, None, n_days=3, time=DAY, feed_from=1, observations={"q_ss": series}, start=DAY)
    assert ctx0.calls[0]["t_first"] == DAY and ctx0.obs_calls[0]["first_index"] == 0 and b0.read()["q_ss_obs"].tolist() == series[:2].tolist()


# ---- resuming ----
def resumed(monkeypatch, observations, time=0, carried=None, restart_file=None, **kw):
    from roger_amd import bands

    ctx = FakeObsContext(12)
    state = fake_state(4, 3, ctx, time=time)
    on_rank(monkeypatch, 0, (1, 1), diskless=True)
    b = state.bands
    b.variables, b.aggregation, b.probabilities, b.observations, b.resume = ["q_ss", "theta_rz"], {"theta_rz": "last"}, PROBS, observations, True
    for k, v in kw.items():
        setattr(b, k, v)
    b._restart_file, b._carried = restart_file, carried
    bands.initialize(state)
    bands.start(state)
    return state, ctx, b


def test_the_resume_request_with_and_without_observations(monkeypatch):
    plain_keys = ["variables", "kinds", "probabilities", "frequency", "start", "mask", "zones", "grid"]
    state_p, _, p = resumed(monkeypatch, {})
    without = p.restart_state(state_p)
    assert sorted(without) == sorted(["acc", "scalars"] + [f"request_{k}" for k in plain_keys])
    state_o, ctx_o, o = resumed(monkeypatch, {"q_ss": OBS_Q})
    rng = np.random.default_rng(2)
    steps = [(h * DAY // 2, (h + 1) * DAY // 2, [np.round(rng.normal(size=12)), rng.normal(size=12)]) for h in range(8)]
    for t0, t1, planes in steps[:3]:
        ctx_o.feed(t0, t1, planes)
    group = o.restart_state(state_o)
    assert sorted(group) == sorted(["acc", "scalars"] + [f"request_{k}" for k in plain_keys + ["observations"]])
    assert group["request_observations"].shape == (2, 3) and group["request_observations"].dtype == np.float64 and group["scalars"].tolist() == [0, 1]
    first = o.read()
    assert first["q_ss_below"].shape == (1,)                                         # drained and written with the rows: nothing new is carried
    # the continued run: the same observations, the stored start, the pairs of the rows that follow
    _, ctx_c, c = resumed(monkeypatch, {"q_ss": OBS_Q}, time=steps[2][1], carried=group, restart_file="run.restart.h5")
    assert ctx_c.calls[0]["t_first"] == 0 and ctx_c.obs_calls[0]["first_index"] == 0 and ctx_c.row0 == 1
    for t0, t1, planes in steps[3:]:
        ctx_c.feed(t0, t1, planes)
    rest = c.read()
    assert rest["interval"].tolist() == [1, 2, 3] and rest["q_ss_below"][0] == -1 and rest["q_ss_below"][2] == -1
    day2 = steps[4][2][0] + steps[5][2][0]
    assert (rest["q_ss_below"][1], rest["q_ss_equal"][1]) == pair_of(day2, OBS_Q[2])
    # with and without, and different ones: the error names the first difference
    with pytest.raises(RuntimeError, match=r"bands: resume = True, but the restart file old\.h5 was written with observations = an array of shape \(2, 3\) and "
                                           r"this run asks for observations = \{\}: a resumed observer takes the same request"):
        resumed(monkeypatch, {}, carried=group, restart_file="old.h5")
    with pytest.raises(RuntimeError, match=r"was written with observations = nothing and this run asks for observations = \[\[0\.0, nan, 1\.0\], \[nan, nan, nan\]\]"):
        resumed(monkeypatch, {"q_ss": OBS_Q}, carried=without, restart_file="old.h5")
    other = OBS_Q.copy()
    other[2] = 1.5
    with pytest.raises(RuntimeError, match=r"was written with observations = \[\[0\.0, nan, 1\.0\], \[nan, nan, nan\]\] and this run asks for observations = "
                                           r"\[\[0\.0, nan, 1\.5\], \[nan, nan, nan\]\]"):
        resumed(monkeypatch, {"q_ss": other}, carried=group, restart_file="old.h5")
    resumed(monkeypatch, {}, carried=without, restart_file="old.h5")                 # files of runs without observations resume as before


# ---- the two pure functions ----
def test_inside_on_hand_made_numbers():
    from roger_amd import bands

    # ten members 1 ... 10, the 5 - 95 band is [1, 10]; T(0.05) = 1, T(0.95) = 10
    below = np.array([0, 0, 4, 9, 10, -1, 0])
    equal = np.array([0, 1, 1, 1, 0, -1, 0])
    total = np.array([10, 10, 10, 10, 10, 10, 0])
    #                 o < 1  o = 1  o = 5  o = 10  o > 10  missing  nothing took part
    assert bands.inside(below, equal, total, 0.05, 0.95).tolist() == [False, True, True, True, False, False, False]
    # the 25 - 75 band of the same members is [3, 8]: T = 3 and 8
    assert bands.targets(0.25, 10) == 3 and bands.targets(0.75, 10) == 8 and bands.targets(0.0, 10) == 1 and bands.targets(1.0, 10) == 10
    got = [bool(bands.inside(o - 1, 1, 10, 0.25, 0.75)) for o in range(1, 11)]
    assert got == [False, False, True, True, True, True, True, True, False, False]
    assert not bands.inside(2, 0, 10, 0.25, 0.75) and bands.inside(3, 0, 10, 0.25, 0.75) and bands.inside(7, 0, 10, 0.25, 0.75) and not bands.inside(8, 0, 10, 0.25, 0.75)
    # weights: three members with W = 2 + 5 + 3, an observation equal to the middle one
    assert bands.inside(2, 5, 10, 0.25, 0.75) and not bands.inside(7, 3, 10, 0.25, 0.5)
    observed = below >= 0
    assert bands.inside(below, equal, total, 0.05, 0.95)[observed & (total > 0)].mean() == 0.6      # the containing ratio
    assert bands.inside(np.zeros((2, 3), dtype=int), np.ones((2, 3), dtype=int), np.full((2, 3), 4), 0.0, 1.0).shape == (2, 3)


def test_pit_and_rank_histogram_on_hand_made_numbers():
    from roger_amd import bands

    pit = bands.pit([0, 4, 9, 10, -1, 0], [0, 1, 1, 0, -1, 0], [10, 10, 10, 10, 10, 0])
    assert pit[:4].tolist() == [0.0, 0.45, 0.95, 1.0] and np.isnan(pit[4:]).all()
    assert bands.pit([3, -1], [2, -1], [8, 8], fill=FILL).tolist() == [0.5, FILL]
    assert bands.rank_histogram(pit, 4).tolist() == [1, 1, 0, 2] and bands.rank_histogram(pit, 4).dtype == np.int64
    assert bands.rank_histogram([0.0, 0.1, 0.1, 0.5, 1.0, FILL, np.nan], 10).tolist() == [1, 2, 0, 0, 0, 1, 0, 0, 0, 1]
    assert bands.rank_histogram([], 3).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match=r"bands.rank_histogram: bins = 0"):
        bands.rank_histogram([0.5], 0)
    with pytest.raises(ValueError, match=r"PIT values lie within \[0, 1\]"):
        bands.rank_histogram([0.5, 1.5], 4)
