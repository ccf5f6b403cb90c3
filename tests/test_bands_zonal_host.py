"""CPU: `state.bands.zones` (roger_amd/bands.py) -- the zone list, the capacity, the file layout and the ranks through fake contexts --
and the per-zone restatement the GPU tests hold the device to (tests/bands_zonal_reference.py: HostBands under mask = (zone == z))."""
import types

import numpy as np
import pytest

from bands_reference import LAST, SUM, HostBands, quantiles_of
from bands_zonal_reference import HostZonalBands, fold, zonal_quantiles_of

DAY = 86400
PROBS = (0.0, 0.5, 1.0)


def fake_state(nx, ny, ctx, time=0):
    from roger_amd import observers

    state = types.SimpleNamespace(
        settings=types.SimpleNamespace(nx=nx, ny=ny, enable_offline_transport=False, identifier="run", time_origin="1900-01-01"),
        var_meta={v: types.SimpleNamespace(plane=7 + k, dtype=None) for k, v in enumerate(("q_ss", "theta_rz"))}, backend_context=ctx,
        variables=types.SimpleNamespace(time=time, itt=0, flush_to_device=lambda: None))
    observers.create(state)
    return state


def on_rank(monkeypatch, rank, num_proc, diskless):
    from roger_amd import bands, observers, runtime_state

    monkeypatch.setattr(bands, "rs", types.SimpleNamespace(num_proc=num_proc))
    monkeypatch.setattr(observers, "rs", types.SimpleNamespace(diskless_mode=diskless, force_overwrite=True))
    monkeypatch.setattr(type(runtime_state), "proc_rank", property(lambda self: rank))
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: num_proc[0] * num_proc[1]))


def test_the_restatement_has_teeth():
    """Crafted planes: the rows of the zones differ from each other and from the whole area's row, a NaN is counted in its own zone, a
    mask folded in takes its column out, and a zone without a column holds m = 0 and NaN."""
    n = 12
    zone = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, -1, 0, 1])
    a = np.array([1.0, 10.0, 100.0, 2.0, 20.0, 200.0, 3.0, 30.0, np.nan, 1e9, 4.0, 40.0])       # SUM: added over the two steps of a day
    b = np.array([-1.0, 5.0, 7.0, -2.0, 6.0, 8.0, -3.0, 4.0, 9.0, -1e9, -0.0, 3.0])             # LAST
    h = HostZonalBands((SUM, LAST), PROBS, n, zone, 4, DAY, 0)
    whole = HostBands((SUM, LAST), PROBS, n, zone >= 0, DAY, 0)
    for t0, t1 in ((0, DAY // 2), (DAY // 2, DAY)):
        h.add(t0, t1, [a, b])
        whole.add(t0, t1, [a, b])
    hdr, counts, values = h.rows()
    assert hdr.tolist() == [[0, DAY]] and counts.shape == (1, 2, 4, 2) and values.shape == (1, 2, 4, 3)
    assert counts[0, 0].tolist() == [[4, 0], [4, 0], [2, 1], [0, 0]] and counts[0, 1].tolist() == [[4, 0], [4, 0], [3, 0], [0, 0]]
    assert values[0, 0, :3].tolist() == [[2.0, 4.0, 8.0], [20.0, 40.0, 80.0], [200.0, 200.0, 400.0]]
    assert values[0, 1, :3].tolist() == [[-3.0, -2.0, 0.0], [3.0, 4.0, 6.0], [7.0, 8.0, 9.0]] and np.isnan(values[0, :, 3]).all()
    assert not np.signbit(values[0, 1, 0, 2])                                                    # the + 0.0 rule
    whdr, wvalues = whole.rows()
    assert whdr[0, 2:].tolist() == [10, 1, 11, 0] and wvalues[0, 0].tolist() == [2.0, 20.0, 400.0]
    assert all((wvalues[0] != values[0, :, z]).any() for z in range(3))
    # the one-step form the crafted GPU tests use, and a mask folded in
    v, c = zonal_quantiles_of(b, fold(zone, np.arange(n) != 6), 3, PROBS)
    assert v[0].tolist() == [-2.0, -1.0, 0.0] and c.tolist() == [[3, 0], [4, 0], [3, 0]]
    assert v[1].tolist() == quantiles_of(b[zone == 1], PROBS)[0].tolist()


def test_initialize_refuses_and_gives_the_sorted_zone_list():
    from roger_amd import bands

    def initialized(zones, **kw):
        state = fake_state(4, 3, types.SimpleNamespace())
        b = state.bands
        b.variables, b.zones = ["q_ss"], zones
        for k, v in kw.items():
            setattr(b, k, v)
        bands.initialize(state)
        return b

    with pytest.raises(ValueError, match=r"bands: the zone map has shape \(3, 4\), the grid 4 x 3 columns"):
        initialized(np.ones((3, 4), dtype=int))
    with pytest.raises(ValueError, match=r"bands: the zone map holds no column in any zone"):
        initialized(np.array([[0, -1, 0]] * 4))
    with pytest.raises(ValueError, match="integer id"):
        initialized(np.ones((4, 3)))
    zones = np.array([[7, 3, 1000000], [0, 7, -5], [3, 3, 1000000], [7, 0, 0]])
    b = initialized(zones)
    assert b._ids.tolist() == [3, 7, 1000000] and b.capacity == 4096
    assert b._index.tolist() == [[1, 0, 2], [-1, 1, -1], [0, 0, 2], [1, -1, -1]] and b._index.dtype == np.int32
    # a mask on top: folded into the index; the zone it empties stays in the list
    b = initialized(zones, mask=zones != 1000000)
    assert b._ids.tolist() == [3, 7, 1000000] and b._index.tolist() == [[1, 0, -1], [-1, 1, -1], [0, 0, -1], [1, -1, -1]]
    # without zones nothing of this is touched
    b = initialized(None, capacity=100000)
    assert b._ids is None and b.capacity == 100000


def test_1025_zones_are_refused_and_the_capacity_follows_the_row_size():
    from roger_amd import bands

    def initialized(n_zones, variables, probabilities, capacity):
        state = fake_state(41, 25, types.SimpleNamespace())
        b = state.bands
        b.variables, b.probabilities, b.capacity = variables, probabilities, capacity
        b.zones = np.minimum(np.arange(1025) + 1, n_zones).reshape(41, 25)
        bands.initialize(state)
        return b

    with pytest.raises(ValueError, match=r"bands: 1025 zones \(at most 1024\)"):
        initialized(1025, ["q_ss"], (0.5,), 4096)
    eight = tuple(np.linspace(0, 1, 8))
    b = initialized(1024, ["q_ss", "theta_rz"], eight, 4096)
    row = 2 * 1024 * 8 * 8 + 2 * 1024 * 16 + 16
    assert len(b._ids) == 1024 and b.capacity == (64 << 20) // row == 409
    assert initialized(3, ["q_ss"], (0.5,), 4096).capacity == 4096                  # small rows: as asked for
    assert initialized(1024, ["q_ss"], (0.5,), 7).capacity == 7                     # never raised
    assert bands.zonal_capacity(4096, 8, 1024, 8) == (64 << 20) // (8 * 1024 * 8 * 8 + 8 * 1024 * 16 + 16) == 102
    assert bands.zonal_capacity(4096, 8, 1024, 8) * (8 * 1024 * 8 * 8 + 8 * 1024 * 16 + 16) <= 64 << 20
    assert bands.zonal_capacity(1, 8, 1024, 8) == 1


class FakeZonalContext:
    """bands_configure / bands_count / bands_zonal_read of `_native.Context` over tests/bands_zonal_reference.py; `feed` is a step."""

    def __init__(self, n):
        self.n, self.calls, self.h = n, [], None

    def bands_configure(self, names, kinds, probs, interval, t_first, mask, capacity, zones=None, n_zones=None):
        self.calls.append(dict(names=names, kinds=kinds, probs=probs, interval=interval, t_first=t_first, mask=mask, capacity=capacity,
                               zones=zones, n_zones=n_zones))
        assert mask is None and zones.dtype == np.int32 and zones.shape == (self.n,)
        self.h = HostZonalBands(kinds, probs, self.n, zones, n_zones, interval, t_first)

    def feed(self, t0, t1, planes):
        self.h.add(t0, t1, planes)

    def bands_count(self):
        return len(self.h.rows()[0])

    def bands_zonal_read(self, first, n):
        return tuple(a[first:first + n].copy() for a in self.h.rows())


def test_file_layout_through_a_fake_context(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    nx, ny = 4, 3
    zones = np.array([[7, 3, 1000000], [0, 7, -5], [3, 3, 1000000], [7, 0, 7]])
    mask = zones != 1000000                                     # zone 1000000 stays in the list, empty
    ctx = FakeZonalContext(nx * ny)
    state = fake_state(nx, ny, ctx)
    on_rank(monkeypatch, 0, (1, 1), diskless=False)
    b = state.bands
    b.variables, b.aggregation, b.probabilities, b.zones, b.mask, b.base_output_path = ["q_ss", "theta_rz"], {"theta_rz": "last"}, PROBS, zones, mask, str(tmp_path)
    bands.initialize(state)
    bands.start(state)
    (call,) = ctx.calls
    assert call["n_zones"] == 3 and call["zones"].tolist() == [1, 0, -1, -1, 1, -1, 0, 0, -1, 1, -1, 1] and call["kinds"] == [SUM, LAST]
    assert b._on and b._ncells.tolist() == [3, 4, 0] and b._path == str(tmp_path / "run.bands.nc")
    rng = np.random.default_rng(3)
    days = [[rng.normal(size=nx * ny), rng.normal(size=nx * ny)] for _ in range(3)]
    days[1][1][[1, 6, 7]] = np.nan                              # day 1: zone 3 of theta_rz has no number
    for k, planes in enumerate(days):
        ctx.feed(k * DAY, (k + 1) * DAY, planes)
    live = b.read()
    assert sorted(live) == ["interval", "q_ss", "q_ss_n", "q_ss_nan", "theta_rz", "theta_rz_n", "theta_rz_nan", "time"]
    assert live["interval"].tolist() == [0, 1, 2] and live["time"].tolist() == [DAY, 2 * DAY, 3 * DAY]
    assert live["q_ss"].shape == (3, 3, 3) and live["q_ss_n"].shape == (3, 3) and live["theta_rz_nan"].shape == (3, 3)
    for k, planes in enumerate(days):
        for v, x in zip(("q_ss", "theta_rz"), planes):
            want, counts = zonal_quantiles_of(x, call["zones"], 3, PROBS)
            assert (live[v][k].view(np.uint64) == want.view(np.uint64)).all() and live[f"{v}_n"][k].tolist() == counts[:, 0].tolist()
            assert live[f"{v}_nan"][k].tolist() == counts[:, 1].tolist()
    assert live["theta_rz_n"][1].tolist() == [0, 4, 0] and live["theta_rz_nan"][1].tolist() == [3, 0, 0] and np.isnan(live["theta_rz"][1, 0]).all()
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert rec["dimensions"] == {"Time": None, "zone": 3, "probability": 3}
    v = rec["variables"]
    assert v["zone"][0] == ("zone",) and np.asarray(v["zone"][1]).tolist() == [3, 7, 1000000]
    assert v["ncells"][0] == ("zone",) and np.asarray(v["ncells"][1]).tolist() == [3, 4, 0]
    assert np.asarray(v["probability"][1]).tolist() == list(PROBS) and np.asarray(v["Time"][1]).tolist() == [1.0, 2.0, 3.0]
    for name in ("q_ss", "theta_rz"):
        assert v[name][0] == ("Time", "zone", "probability") and v[f"{name}_n"][0] == v[f"{name}_nan"][0] == ("Time", "zone")
        q, m = np.asarray(v[name][1]), np.asarray(v[f"{name}_n"][1])
        assert v[name][2]["_FillValue"] == bands.FILL
        assert ((q == bands.FILL).all(axis=2) == (m == 0)).all() and (m[:, 2] == 0).all()      # fill values exactly where v_n == 0
        np.testing.assert_array_equal(m, live[f"{name}_n"])
        np.testing.assert_array_equal(q[m > 0], live[name][m > 0])
    assert (np.asarray(v["theta_rz"][1])[1, 0] == bands.FILL).all()
    assert rec["attributes"]["columns"] == "this rank's block"


def test_two_fake_ranks_on_4_x_2(monkeypatch):
    """Rank 0 holds zones 5 and 9, rank 1 only zone 9 -- zone 5 has v_n = 0 and NaN there; with the zones of rank 1 masked out it
    configures nothing.  Both report the same ring capacity."""
    from roger_amd import bands, observers

    zones = np.array([[5, 9], [9, 5], [0, 9], [9, 0]])
    planes = [np.arange(4.0) + 1.0]
    for mask, want_on in ((None, {0: True, 1: True}), (np.array([[1, 1], [1, 0], [0, 0], [0, 1]]), {0: True, 1: False})):
        capacity = {}
        for rank in (0, 1):
            ctx = FakeZonalContext(4)
            state = fake_state(4, 2, ctx)
            on_rank(monkeypatch, rank, (2, 1), diskless=True)
            b = state.bands
            b.variables, b.zones, b.mask, b.capacity, b.probabilities = ["q_ss"], zones, mask, 12, PROBS
            bands.initialize(state)
            bands.start(state)
            capacity[rank] = observers.ring_capacity(state)
            assert b._on == want_on[rank] and b._ids.tolist() == [5, 9] and len(ctx.calls) == int(want_on[rank])
            if not b._on:
                assert b.read() is None and b._path is None
                continue
            assert ctx.calls[0]["n_zones"] == 2                 # the GLOBAL list on every rank
            ctx.feed(0, DAY, planes)
            live = b.read()
            if rank == 1:
                assert ctx.calls[0]["zones"].tolist() == [-1, 1, 1, -1] and b._ncells.tolist() == [0, 2]
                assert live["q_ss_n"].tolist() == [[0, 2]] and np.isnan(live["q_ss"][0, 0]).all() and live["q_ss"][0, 1].tolist() == [2.0, 2.0, 3.0]
            else:
                want = [[0, 1, 1, 0], [0, 1, 1, -1]][mask is not None]
                assert ctx.calls[0]["zones"].tolist() == want and live["q_ss_n"].tolist() == [[2 - (mask is not None), 2]]
        assert capacity == {0: 12, 1: 12}


def test_without_zones_read_and_the_file_are_todays(monkeypatch, tmp_path):
    from roger_amd import bands, nc4lite

    rows = (np.array([[0, DAY, 0, 3], [1, 2 * DAY, 3, 0]], dtype=np.int64), np.array([[[np.nan, np.nan]], [[1.0, 2.0]]]))
    calls = []
    ctx = types.SimpleNamespace(bands_configure=lambda *a, **kw: calls.append((a, kw)), bands_count=lambda: 2,
                                bands_read=lambda first, n: (rows[0][first:first + n], rows[1][first:first + n]))
    state = fake_state(4, 2, ctx)
    on_rank(monkeypatch, 0, (1, 1), diskless=False)
    b = state.bands
    b.variables, b.probabilities, b.base_output_path, b.capacity = ["q_ss"], (0.1, 0.9), str(tmp_path), 100000
    bands.initialize(state)
    bands.start(state)
    assert calls == [((["q_ss"], [SUM], (0.1, 0.9), DAY, 0, None, 100000), {})]          # positional, no keyword, the capacity as asked for
    live = b.read()
    assert list(live) == ["interval", "time", "q_ss", "q_ss_n", "q_ss_nan"]
    assert live["q_ss"].shape == (2, 2) and live["q_ss_n"].tolist() == [0, 3] and live["q_ss_nan"].tolist() == [3, 0]
    bands.close(state)
    rec = nc4lite.read(b._path)
    assert rec["dimensions"] == {"Time": None, "probability": 2}
    assert list(rec["variables"]) == ["Time", "interval", "probability", "q_ss", "q_ss_n", "q_ss_nan"]
    assert rec["variables"]["q_ss"][0] == ("Time", "probability") and rec["variables"]["q_ss_n"][0] == ("Time",)
    assert (np.asarray(rec["variables"]["q_ss"][1])[0] == bands.FILL).all()
