"""CPU: the host package's TransportPointSeries (roger_amd/sas_points.py) on the oracle double with points
(tests/sas_points_reference.py): a transport setup script ends with a `.transport_points.nc` whose records are what
`state.variables.<name>` held after every step, bit for bit."""
import numpy as np
import pytest

import sas_binding as sb
import test_host_package_sas_restart as R
from sas_points_reference import PointsOracleSasContext, TagRing

DAY = 86400
SCALARS = ["C_iso_q_ss", "C_iso_rz", "C_rz", "tt50_q_ss"]
VARS = SCALARS + ["tt_q_ss", "TT_transp", "sa_s"]
NO_STATS = [v for v in VARS if v != "tt50_q_ss"]     # (a golden case without age statistics)
on_disk = R.on_disk


@pytest.fixture
def made(monkeypatch):
    from roger_amd import _native

    out = []

    def make(*a, **k):
        out.append(PointsOracleSasContext(*a, **k))
        return out[-1]

    monkeypatch.setattr(_native, "SasContext", make)
    return out


def points_model(case, path, cells, variables=VARS, capacity=4096, warmup_days=0, **override):
    """The golden setup of `case` with transport points (cells None: without them)."""
    from roger_amd import roger_routine

    g, base = R.golden_model(case, warmup_days=warmup_days)

    class WithPoints(type(base)):
        @roger_routine
        def set_diagnostics(self, state):
            if cells is None:
                return
            p = state.transport_points
            p.cells, p.output_variables, p.base_output_path, p.capacity = list(cells), list(variables), str(path), capacity

    model = WithPoints()
    model.override_settings = dict(override)
    return g, model


def corners(g):
    return [(0, 0), (0, g.ny - 1), (g.nx - 1, g.ny - 1)]


def held(state, name, cells):
    """What `vs.<name>` holds at the cells: (K,) or (K, width), time level tau."""
    a = np.asarray(getattr(state.variables, name))[2:-2, 2:-2]
    if "timesteps" in state.var_meta[name].dims:
        a = a[:, :, 1]
    return np.stack([a[ix, iy] for ix, iy in cells])


def run_and_note(model, cells, variables):
    """run() with what the variables held after every step: [(itt, time, {name: values})]"""
    notes, step = [], model.step

    def noting(state):
        step(state)
        vs = state.variables
        notes.append((int(vs.itt), int(vs.time), {v: held(state, v, cells) for v in variables}))

    model.step = noting
    model.run()
    return notes


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def read_file(path, ident="GoldenSAS"):
    from nc_util import netcdf_file

    with netcdf_file(str(path / f"{ident}.transport_points.nc"), "r", mmap=False) as f:
        return ({k: np.array(v[:]) for k, v in f.variables.items()}, {k: v.dimensions for k, v in f.variables.items()}, dict(f.dimensions),
                {"time_origin": f.variables["Time"].time_origin, "fill": f.variables["sa_s"]._FillValue if "sa_s" in f.variables else None})


def assert_file_holds(path, first, notes, variables):
    """Record 0 = `first`, then one record per noted step; Time and itt beside them."""
    data, dims, _, _ = read_file(path)
    itt0, time0, values0 = first
    np.testing.assert_array_equal(data["itt"], [itt0] + [n[0] for n in notes])
    np.testing.assert_array_equal(data["Time"], np.array([time0] + [n[1] for n in notes]) / float(DAY))
    for v in variables:
        want = np.stack([values0[v]] + [n[2][v] for n in notes])
        assert same_bits(data[v], want), v
    return data, dims


def test_ring_with_tags():
    ring = TagRing(3, 4)
    for k in range(8):
        ring.add(10 + k, np.arange(4.0) + 100 * k)
    tags, values = ring.read(5, 3)      # slots 2, 0, 1: across the wrap
    assert list(tags) == [15, 16, 17] and np.array_equal(values, np.arange(4.0) + 100 * np.arange(5, 8)[:, None])
    with pytest.raises(ValueError, match="overwritten"):
        ring.read(4, 2)


def test_script_writes_what_the_variables_held(made, on_disk, tmp_path):
    """1. sas_stats_a30, three cells with the first and the last column, scalars + tt_q_ss + TT_transp + sa_s over g.ndays."""
    g, model = points_model("sas_stats_a30", tmp_path, None)
    cells = corners(g)
    assert cells[0] == (0, 0) and cells[-1] == (g.nx - 1, g.ny - 1) and len(set(cells)) == 3
    g, model = points_model("sas_stats_a30", tmp_path, cells)
    model.setup()
    assert made[-1]._ring is None, "configured before the warm-up is through"
    model.warmup(repeat=0)
    state = model.state
    first = (0, 0, {v: held(state, v, cells) for v in VARS})
    assert made[-1].points_count() == 1
    notes = run_and_note(model, cells, VARS)
    assert len(notes) == g.ndays and made[-1].points_count() == g.ndays + 1
    data, dims = assert_file_holds(tmp_path, first, notes, VARS)
    _, _, fdims, attrs = read_file(tmp_path)
    assert fdims["point"] == 3 and fdims["ages"] == g.ages and fdims["nages"] == g.ages + 1 and fdims["Time"] is None
    assert list(data["Time"]) == [float(k) for k in range(g.ndays + 1)] and list(data["itt"]) == list(range(g.ndays + 1))
    assert data["itt"].dtype.kind == "i" and attrs["time_origin"] == b"01-01-2022" and attrs["fill"] == -9999.0
    np.testing.assert_array_equal(data["ix"], [c[0] for c in cells])
    np.testing.assert_array_equal(data["iy"], [c[1] for c in cells])
    vs = state.variables
    np.testing.assert_array_equal(data["x"], [np.asarray(vs.x)[2 + c[0]] for c in cells])
    np.testing.assert_array_equal(data["y"], [np.asarray(vs.y)[2 + c[1]] for c in cells])
    for v in SCALARS:
        assert dims[v] == ("Time", "point") and data[v].shape == (g.ndays + 1, 3)
    assert dims["tt_q_ss"] == ("Time", "point", "ages") and dims["sa_s"] == ("Time", "point", "ages")
    assert dims["TT_transp"] == ("Time", "point", "nages") and data["TT_transp"].shape == (g.ndays + 1, 3, g.ages + 1)
    for v in VARS:
        assert np.any(np.nan_to_num(data[v][1:]) != 0), f"{v} never held a value"
    # the rows are the double's own: the day of rh_sas_step as the tag, every row recorded once
    assert [t for t, _ in made[-1].trace] == [0] * (g.ndays + 1)


def test_small_ring_loses_no_row(made, on_disk, tmp_path):
    """2. capacity 2: the drain runs before the ring wraps."""
    g, model = points_model("sas_stats_a30", tmp_path, [(0, 0), (1, 1)], capacity=2)
    assert g.ndays >= 5
    cells = [(0, 0), (1, 1)]
    model.setup()
    model.warmup(repeat=0)
    ctx = made[-1]
    first = (0, 0, {v: held(model.state, v, cells) for v in VARS})
    reads, read = [], ctx.points_read
    ctx.points_read = lambda a, n: (reads.append((a, n)), read(a, n))[1]
    notes = run_and_note(model, cells, VARS)
    assert ctx.points_count() == g.ndays + 1 and ctx._ring.capacity == 2
    assert max(n for _, n in reads) <= 2 and sum(n for _, n in reads) == g.ndays
    assert_file_holds(tmp_path, first, notes, VARS)


def test_warmup_records_nothing(made, on_disk, tmp_path):
    """3. sas_warmup_a30, warmup(repeat=1): no row from the warm-up run, record 0 is the rescaled state, Time restarts at 0."""
    case = "sas_warmup_a30"
    ndays = sb.SasGolden(case).ndays
    g, model = points_model(case, tmp_path, [(0, 0), (1, 0)], variables=NO_STATS, warmup_days=ndays)
    cells = [(0, 0), (1, 0)]
    model.setup()
    ctx = made[-1]
    configured = []
    configure = ctx.points_configure
    ctx.points_configure = lambda *a, **k: (configured.append((int(model.state.variables.itt), bool(model.state.settings.warmup_done))),
                                            configure(*a, **k))[1]
    model.warmup(repeat=1)
    assert configured == [(0, True)] and ctx.points_count() == 1
    data, _, _, _ = read_file(tmp_path)
    assert list(data["Time"]) == [0.0] and list(data["itt"]) == [0]
    first = (0, 0, {v: held(model.state, v, cells) for v in NO_STATS})
    assert same_bits(data["C_iso_rz"][0], first[2]["C_iso_rz"])
    flat = [ix * g.ny + iy for ix, iy in cells]
    sb.compare_sas(data["C_iso_rz"][0], g.day(0, "C_iso_rz")[flat], "record 0: the rescaled state")
    notes = run_and_note(model, cells, NO_STATS)
    data, _ = assert_file_holds(tmp_path, first, notes, NO_STATS)
    assert list(data["Time"]) == [float(k) for k in range(ndays + 1)]


@pytest.mark.parametrize("kw,exc,text", [
    (dict(variables=["C_rz", "sa_rz"]), NotImplementedError, "'sa_rz' would be recorded after the ageing"),
    (dict(variables=["C_snow"]), NotImplementedError, "'C_snow' exists on the host only"),
    (dict(variables=["no_such_variable"]), NotImplementedError, "no_such_variable"),
    (dict(cells=[(0, 0), (99, 0)]), ValueError, r"cell \(99, 0\) is outside the grid"),
    (dict(cells=[(1, 1), (0, 0), (1, 1)]), ValueError, r"cell \(1, 1\) is given twice"),
    (dict(variables=["C_rz"] * 33), ValueError, "33 variables"),
    (dict(capacity=0), ValueError, "capacity = 0"),
])
def test_refusals(made, tmp_path, kw, exc, text):
    """4."""
    args = dict(cells=[(0, 0)], variables=["C_rz"], capacity=8)
    args.update(kw)
    _, model = points_model("sas_stats_a30", tmp_path, **args)
    with pytest.raises(exc, match=text):
        model.setup()


def test_more_cells_than_the_recorder_takes():
    """4. ... 257 cells, on a grid that has them."""
    from roger_amd import sas_points
    from roger_amd.state import RogerState

    st = RogerState()
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
        st.settings.nx, st.settings.ny = 20, 20
    st.transport_points.cells, st.transport_points.output_variables = [(k // 20, k % 20) for k in range(257)], ["C_s"]
    with pytest.raises(ValueError, match="257 cells x 1 variables"):
        sas_points.initialize(st)


def test_nothing_asked_for_nothing_written(made, on_disk, tmp_path):
    _, model = points_model("sas_stats_a30", tmp_path, None, runlen=2 * DAY)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    assert made[-1]._ring is None and not list(tmp_path.iterdir())


def test_restart_drains_first_and_starts_a_new_series(made, on_disk, tmp_path, monkeypatch):
    """5. restart_frequency of a day: the ring is drained before every restart file; the resumed run starts a new series; interrupted
    and resumed runs end in the state of the same runs without points."""
    from roger_amd import restart

    case = "sas_stats_a30"
    ndays = sb.SasGolden(case).ndays
    half = ndays // 2
    cells = [(0, 0), (1, 1)]
    pending = []
    write = restart.write_restart

    def spy(state, *a, **k):
        p = state.transport_points
        if p._on:
            pending.append(state.sas_context.points_count() - p._read)
        return write(state, *a, **k)

    monkeypatch.setattr(restart, "write_restart", spy)
    runs = {}
    for tag, pts in (("with", cells), ("without", None)):
        out = tmp_path / tag
        out.mkdir()
        _, b = points_model(case, out / "b", pts, capacity=64, runlen=half * DAY, restart_frequency=DAY, write_restart=True,
                            restart_output_filename=str(out / "b_{itt:0>4d}.h5"))
        b.setup()
        b.warmup(repeat=0)
        first_b = (0, 0, {v: held(b.state, v, cells) for v in VARS})
        notes_b = run_and_note(b, cells, VARS)
        _, c = points_model(case, out / "c", pts, capacity=64, runlen=(ndays - half) * DAY,
                            restart_input_filename=str(out / f"b_{half:0>4d}.h5"))
        c.setup()
        first_c = (half, half * DAY, {v: held(c.state, v, cells) for v in VARS})
        notes_c = run_and_note(c, cells, VARS)
        runs[tag] = (b, c)
        if pts:
            assert len(pending) >= half and not any(pending), pending     # capacity 64: only the restart path drains in between
            assert_file_holds(out / "b", first_b, notes_b, VARS)
            data, _ = assert_file_holds(out / "c", first_c, notes_c, VARS)    # a new series: record 0 is the state at the restart
            assert list(data["itt"]) == list(range(half, ndays + 1)) and made[-1].points_count() == ndays - half + 1
    for k in (0, 1):
        R.assert_same_state(runs["with"][k], runs["without"][k])


@pytest.mark.parametrize("num_proc", [(2, 1), (2, 2)])
def test_block_ownership(num_proc):
    """6. The transport series maps global cells to a rank's block through the function the SVAT points use."""
    from roger_amd import points, sas_points
    from roger_amd.distributed import proc_rank_to_index

    assert sas_points.local_cells is points.local_cells
    nx, ny = 6, 4
    px, py = num_proc
    nxl, nyl = nx // px, ny // py
    cells = [(0, 0), (2, 3), (3, 0), (5, 3), (2, 1), (3, 2)]
    field = np.arange(nx * ny).reshape(nx, ny)
    owners = []
    for r in range(px * py):
        bx, by = proc_rank_to_index(r, num_proc)
        block = field[bx * nxl:(bx + 1) * nxl, by * nyl:(by + 1) * nyl].reshape(-1)
        got = sas_points.local_cells(cells, nx, ny, num_proc, r)
        for k, c in got:
            assert block[c] == field[cells[k]]
            owners.append(k)
    assert sorted(owners) == list(range(len(cells)))     # every point on exactly one rank


def test_a_rank_without_a_point_writes_nothing(made, on_disk, tmp_path, monkeypatch):
    """6. ... and the series of a rank: ranks (2, 1), all points in the block of rank 0 -- rank 1 configures nothing and writes no file."""
    from roger_amd import runtime_settings as rs, runtime_state as rst, sas_points

    g, model = points_model("sas_stats_a30", tmp_path, [(0, 0), (0, 1)])
    assert g.nx >= 2
    model.setup()
    prev = rs.num_proc
    object.__setattr__(rs, "num_proc", (2, 1))
    try:
        monkeypatch.setattr(type(rst), "proc_rank", 1, raising=False)
        sas_points.start(model.state)
        assert not model.state.transport_points._on and made[-1]._ring is None and not list(tmp_path.iterdir())
    finally:
        object.__setattr__(rs, "num_proc", prev)
