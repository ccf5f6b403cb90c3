"""CPU: the points recorder's ring rule, the global -> local cell mapping, and the host package's PointSeries on the oracle double
(tests/points_reference.py): a RogerSetup script ends with a `.points.nc` whose rows are the double's own per-step values."""
import numpy as np
import pytest

from golden_util import load_case
from points_reference import HostRing, PointsOracleContext


@pytest.mark.parametrize("capacity", [1, 2, 16])
def test_ring_arithmetic(capacity):
    ring = HostRing(capacity, 2, 3)
    rows = [((k + 1, 600 * (k + 1), 600), np.arange(6, dtype=np.float64).reshape(2, 3) + 10.0 * k) for k in range(37)]
    assert ring.read(0, 0)[0].shape == (0, 3)
    for k, (hdr, values) in enumerate(rows):
        ring.add(hdr, values)
        assert ring.count == k + 1
        first = max(0, k + 1 - capacity)
        hdr_got, got = ring.read(first, k + 1 - first)         # everything resident: straddles the wrap whenever k + 1 > capacity
        assert [tuple(h) for h in hdr_got] == [r[0] for r in rows[first:k + 1]]
        np.testing.assert_array_equal(got, np.stack([r[1] for r in rows[first:k + 1]]))
        hdr_got, got = ring.read(k, 1)
        assert tuple(hdr_got[0]) == hdr and np.array_equal(got[0], values)
        if first > 0:
            for bad in ((first - 1, 1), (first - 1, 2), (0, k + 1)):
                with pytest.raises(ValueError, match="overwritten"):
                    ring.read(*bad)
        for bad in ((k + 1, 1), (k, 2), (-1, 1)):
            with pytest.raises(ValueError, match="not been recorded"):
                ring.read(*bad)
    with pytest.raises(ValueError):
        HostRing(0, 1, 1)


def test_global_cells_map_to_the_ranks_blocks():
    """6 x 4 columns on (2, 2) ranks: blocks of 3 x 2, ranks x-fastest.  One point inside each block and one on each block edge."""
    from roger_amd.points import local_cells

    nx, ny, num_proc = 6, 4, (2, 2)
    cells = [(1, 0), (4, 1), (0, 3), (5, 2),      # one per block: ranks 0, 1, 2, 3
             (2, 1), (3, 1), (2, 2), (3, 2)]      # the four corners where the blocks meet: the last / first column and row of each
    got = {r: local_cells(cells, nx, ny, num_proc, r) for r in range(4)}
    assert got[0] == [(0, 1 * 2 + 0), (4, 2 * 2 + 1)]
    assert got[1] == [(1, 1 * 2 + 1), (5, 0 * 2 + 1)]
    assert got[2] == [(2, 0 * 2 + 1), (6, 2 * 2 + 0)]
    assert got[3] == [(3, 2 * 2 + 0), (7, 0 * 2 + 0)]
    assert sorted(k for r in range(4) for k, _ in got[r]) == list(range(len(cells)))     # every point on exactly one rank
    # against the decomposition itself: the local cell of a rank's block is where the global array's value sits
    from roger_amd.distributed import proc_rank_to_index

    field = np.arange(nx * ny).reshape(nx, ny)
    for r in range(4):
        bx, by = proc_rank_to_index(r, num_proc)
        block = field[bx * 3:(bx + 1) * 3, by * 2:(by + 1) * 2].reshape(-1)
        for k, c in got[r]:
            assert block[c] == field[cells[k]]
    assert local_cells(cells, nx, ny, (1, 1), 0) == [(k, ix * ny + iy) for k, (ix, iy) in enumerate(cells)]


@pytest.fixture
def points_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []

    def make(*a, **k):
        made.append(PointsOracleContext(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


CELLS = [(0, 0), (2, 1), (1, 3)]
VARS = ["theta_rz", "q_ss", "swe", "S_rz"]


def make_model(tmp_path, cells=CELLS, variables=VARS, capacity=8, ndays=6, **kw):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, **kw)

    def set_diagnostics(self, state):
        state.points.cells = list(cells)
        state.points.output_variables = list(variables)
        state.points.base_output_path = str(tmp_path)
        state.points.capacity = capacity

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model, g


@pytest.mark.parametrize("script_hooks,by_routine", [(None, False), ("plain", False), ("plain", True)])
def test_script_writes_the_doubles_own_rows(points_backend, tmp_path, monkeypatch, script_hooks, by_routine):
    """svat_hetero_combo, three points, four variables, capacity 8: the ring is drained many times (rounds of device steps; the host
    loop's step calls) and the file holds every step."""
    from nc_util import netcdf_file

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    model, g = make_model(tmp_path, script_hooks=script_hooks)
    nx, ny = (int(v) for v in g["nx_ny"])
    assert all(ix < nx and iy < ny for ix, iy in CELLS)
    model.setup()
    ctx = points_backend[-1]
    initial = np.stack([ctx.download(v)[[ix * ny + iy for ix, iy in CELLS]] for v in VARS])
    reads = []
    read = ctx.points_read
    ctx.points_read = lambda first, n: (reads.append((first, n)), read(first, n))[1]
    model.run()
    trace = ctx.trace
    assert len(trace) > 5 * 8 and ctx.points_count() == len(trace)
    assert len(reads) >= len(trace) // 8 and max(n for _, n in reads) <= 8, "the ring was not drained in pieces of at most its capacity"
    f = netcdf_file(str(tmp_path / "GoldenSVAT.points.nc"))
    assert f.dimensions["point"] == 3 and f.variables["Time"].dimensions == ("Time",)
    t = f.variables["Time"][:]
    assert len(t) == len(trace) + 1 and t[0] == 0 and np.all(np.diff(t) > 0) and t[-1] * 86400 == model.state.settings.runlen
    assert f.variables["Time"].time_origin == b"2018-01-01 00:00:00" and f.variables["dt"].units == b"s"
    np.testing.assert_array_equal(f.variables["dt"][:], [0] + [h[2] for h, _ in trace])
    np.testing.assert_array_equal(f.variables["itt"][:], [0] + [h[0] for h, _ in trace])
    np.testing.assert_array_equal(t[1:], np.array([h[1] for h, _ in trace]) / 86400.0)
    np.testing.assert_array_equal(f.variables["ix"][:], [c[0] for c in CELLS])
    np.testing.assert_array_equal(f.variables["iy"][:], [c[1] for c in CELLS])
    assert f.variables["itt"][:].dtype.kind == "i" and f.variables["ix"][:].dtype.kind == "i"
    vs = model.state.variables
    np.testing.assert_array_equal(f.variables["x"][:], [np.asarray(vs.x)[2 + c[0]] for c in CELLS])
    np.testing.assert_array_equal(f.variables["y"][:], [np.asarray(vs.y)[2 + c[1]] for c in CELLS])
    for j, v in enumerate(VARS):
        a = f.variables[v][:]
        assert f.variables[v].dimensions == ("Time", "point") and a.dtype == np.float64
        np.testing.assert_array_equal(a[0], initial[j], err_msg=f"{v}: record 0 holds the initial values")
        np.testing.assert_array_equal(a[1:], np.stack([vals[j] for _, vals in trace]), err_msg=v)
        assert np.any(a != 0), v
    assert f.variables["theta_rz"].units == b"-" and f.variables["q_ss"].units == b"mm/dt"


def test_run_device_called_directly(points_backend, tmp_path):
    """run_device(n) drains before and after; more steps than the ring holds are refused before anything is enqueued."""
    model, _ = make_model(tmp_path)
    model.setup()
    ctx = points_backend[-1]
    model.run_device(8)
    model.run_device(5)
    assert ctx.points_count() == 13 and sum(len(h) for h in model.state.points._hdr) == 14
    itt = int(model.state.variables.itt)
    with pytest.raises(RuntimeError, match="shorter pieces"):
        model.run_device(9)
    assert int(model.state.variables.itt) == itt == 13 and ctx.points_count() == 13


def test_validation(points_backend, tmp_path):
    for kw, exc, text in ((dict(cells=[(0, 0), (4, 1)]), ValueError, r"cell \(4, 1\) is outside the grid"),
                          (dict(cells=[(0, 0), (0, -1)]), ValueError, "outside the grid"),
                          (dict(cells=[(1, 1), (0, 0), (1, 1)]), ValueError, r"cell \(1, 1\) is given twice"),
                          (dict(variables=["theta_rz", "lu_id"]), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(variables=["prec_day"]), NotImplementedError, "'prec_day' is not a float64"),
                          (dict(variables=["no_such_variable"]), NotImplementedError, "no_such_variable"),
                          (dict(capacity=0), ValueError, "capacity = 0")):
        model, g = make_model(tmp_path, **kw)
        assert tuple(int(v) for v in g["nx_ny"]) == (4, 4)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model, _ = make_model(tmp_path, cells=[], ndays=1)
    model.setup()
    model.run()
    assert points_backend[-1]._ring is None and not list(tmp_path.iterdir())


def test_offline_transport_is_refused(tmp_path):
    from roger_amd import points
    from roger_amd.state import RogerState

    st = RogerState()
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    st.points.cells, st.points.output_variables = [(0, 0)], ["C_s"]
    with pytest.raises(NotImplementedError, match="offline transport"):
        points.initialize(st)
