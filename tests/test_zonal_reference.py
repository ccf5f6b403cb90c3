"""CPU: the zonal totals' index and reduction order (tests/zonal_reference.py) against the totals' restatement with mask = zones == z
(tests/totals_reference.py: tree_totals), the host package's copy of it, `combine`, the validation, and the host package's ZonalTotals on
the oracle double: a RogerSetup script ends with a `.zonal_totals.nc` whose rows are tree_totals of the double's own planes per zone."""
import numpy as np
import pytest

from golden_util import load_case
from totals_reference import same_bits, tree_totals
from zonal_reference import TILE, ZonalOracleContext, build_index, walk_index

B = 2.0 ** 60      # B + 1 == B in float64: where a 1 meets B decides the result (tests/test_totals_reference.py)
SIZES = [3, 64, 65, 256, 257, 65537]


def random_map(n, n_zones, seed, outside=0.2):
    rng = np.random.default_rng(seed)
    z = rng.integers(0, n_zones, size=n)
    z[rng.random(n) < outside] = -1
    if not (z >= 0).any():
        z[0] = 0
    return z


@pytest.mark.parametrize("n,n_zones", [(3, 2), (64, 5), (257, 3), (1000, 13), (70001, 40)])
def test_index_lists_every_pair_once_in_tile_order(n, n_zones):
    zone = random_map(n, n_zones, n)
    tile_ptr, tile_zone, acc_ptr, acc_slot = build_index(zone, n_zones)
    ntiles = (n + TILE - 1) // TILE
    pairs = {(i // TILE, int(z)) for i, z in enumerate(zone) if z >= 0}
    assert len(tile_ptr) == ntiles + 1 and tile_ptr[0] == 0 and tile_ptr[-1] == len(tile_zone) == len(acc_slot) == len(pairs)   # S
    listed = [(b, int(tile_zone[s])) for b in range(ntiles) for s in range(tile_ptr[b], tile_ptr[b + 1])]
    assert len(set(listed)) == len(listed) and set(listed) == pairs, "every (tile, zone) pair once"
    for b in range(ntiles):
        here = tile_zone[tile_ptr[b]:tile_ptr[b + 1]]
        assert (np.diff(here) > 0).all(), "ascending zones within a tile"
    tile_of_slot = np.repeat(np.arange(ntiles), np.diff(tile_ptr))
    assert len(acc_ptr) == n_zones * TILE + 1 and acc_ptr[0] == 0 and acc_ptr[-1] == len(pairs)
    assert sorted(acc_slot) == list(range(len(pairs))), "every slot in exactly one accumulator's list"
    for z in range(n_zones):
        for t in range(TILE):
            slots = acc_slot[acc_ptr[z * TILE + t]:acc_ptr[z * TILE + t + 1]]
            assert (tile_zone[slots] == z).all() and (tile_of_slot[slots] % TILE == t).all()
            assert (np.diff(tile_of_slot[slots]) > 0).all(), "increasing tile order"


def placements(n):
    """Values whose tree sum differs from other orders: B, -B and ones placed as tests/test_totals_reference.py's hand-worked cases."""
    v = np.zeros(n)
    at = {3: {0: B, 1: 1.0, 2: -B}, 64: {0: B, 1: -B, 32: 1.0}, 65: {0: B, 1: -B, 32: 1.0, 64: 1.0},
          256: {0: B, 64: 1.0, 128: -B, 192: 1.0}, 257: {0: B, 255: 1.0, 256: -B}, 65537: {0: B, 256: 1.0, 65536: -B}}[n]
    for k, x in at.items():
        v[k] = x
    want = {3: 1.0, 64: 0.0, 65: 1.0, 256: 0.0, 257: 0.0, 65537: 1.0}[n]
    return v, sorted(at), want


@pytest.mark.parametrize("n", SIZES)
def test_walking_the_index_is_the_masked_tree(n):
    """Per zone the walk over the index equals tree_totals(values, zones == z) in every bit, for random values and for the placement
    of B = 2^60 and ones that another order sums differently; the host package's zone_totals likewise."""
    from roger_amd.zonal_totals import zone_totals

    rng = np.random.default_rng(n)
    n_zones = 4
    hand, cols, want = placements(n)
    # zone 1 holds the placed columns and every third other column (zeros there), zone 3 no column at all, some columns are outside
    zone = np.where(np.arange(n) % 3 == 0, 1, np.where(np.arange(n) % 3 == 1, 0, 2))
    zone[np.arange(n) % 7 == 6] = -1
    zone[cols] = 1
    noise = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    for values in (hand, noise, np.where(zone == 1, hand, noise)):
        for f in (walk_index, zone_totals):
            got = f(values, zone, n_zones)
            for z in range(n_zones):
                ref = tree_totals(values, zone == z)
                assert same_bits(got[z, 0], ref[0]), (f.__name__, n, z, got[z, 0], ref[0])
                assert got[z, 1] == ref[1] and got[z, 2] == ref[2], (f.__name__, n, z)
            assert tuple(got[3]) == (0.0, np.inf, -np.inf) and not np.signbit(got[3, 0]), "a zone without a column holds the identities"
    assert B + 1.0 == B
    got = walk_index(hand, zone, n_zones)
    assert same_bits(got[1, 0], want), (n, got[1, 0], want)
    serial = np.add.accumulate(hand[zone == 1])[-1]
    if n not in (3, 257):    # (3: the hand-worked value IS what another order misses; 257: left to right gives 0 as well)
        assert serial != want, "the placement does not tell the orders apart"


@pytest.mark.parametrize("n,n_zones", [(1000, 13), (4099, 200)])
def test_random_maps_against_the_masked_tree(n, n_zones):
    from roger_amd.zonal_totals import zone_totals

    zone = random_map(n, n_zones, 17 + n)
    v = np.random.default_rng(n).normal(size=n)
    for f in (walk_index, zone_totals):
        got = f(v, zone, n_zones)
        for z in range(n_zones):
            ref = tree_totals(v, zone == z) if (zone == z).any() else (0.0, np.inf, -np.inf)
            assert same_bits(got[z], ref), (f.__name__, z)


def test_zone_ids_map_positive_values_in_ascending_order():
    from roger_amd.zonal_totals import default_capacity, zone_ids

    ids, index = zone_ids(np.array([[7, 0, 3], [-2, 7, 100]]))
    assert list(ids) == [3, 7, 100] and index.dtype == np.int32
    np.testing.assert_array_equal(index, [[1, -1, 0], [-1, 1, 2]])
    with pytest.raises(ValueError, match="float64"):
        zone_ids(np.ones((2, 2)))
    assert default_capacity(1, 1) == 4096 and default_capacity(1024, 32) * 1024 * 32 * 24 <= 64 << 20 and default_capacity(1024, 32) >= 1


def test_combine_two_half_domain_files(tmp_path):
    from nc_util import netcdf_file

    from roger_amd import zonal_totals as zt

    rng = np.random.default_rng(3)
    nrec, names, ids = 7, ["prec", "S_rz"], np.array([2, 5, 9, 11])
    hdr = np.stack([np.arange(nrec), np.arange(nrec) * 600, np.full(nrec, 600)], axis=1).astype(np.int64)
    hdr[0, 2] = 0
    planes = rng.normal(size=(nrec, len(names), 600))
    # zone index 2 lies in the second half only, zone index 3 nowhere
    zones = [rng.integers(-1, 2, size=300), rng.integers(-1, 3, size=300)]
    paths, per_rank, cells = [], [], []
    for r, (h, z) in enumerate(zip((slice(0, 300), slice(300, 600)), zones)):
        values = np.stack([np.stack([walk_index(planes[k, j, h], z, 4) for j in range(len(names))], axis=1) for k in range(nrec)])
        per_rank.append(values)
        cells.append(np.bincount(z[z >= 0], minlength=4))
        paths.append(str(tmp_path / f"run.zonal_totals.{r:04d}.nc"))
        zt._write_file(paths[-1], zt._file_variables(hdr, values, names, ids, cells[-1], "2018-01-01 00:00:00"), "run")
    f = netcdf_file(paths[0])
    assert f.variables["prec_min"].dimensions == ("Time", "zone") and f.variables["prec_min"]._FillValue == zt.FILL
    a = np.asarray(f.variables["prec_min"][:])
    assert (a[:, 2:] == zt.FILL).all() and (np.asarray(f.variables["prec_mean"][:])[:, 2:] == zt.FILL).all()
    assert (np.asarray(f.variables["prec_sum"][:])[:, 2:] == 0).all()
    out = str(tmp_path / "run.zonal_totals.nc")
    zt.combine(paths, out)
    f = netcdf_file(out)
    ncells = cells[0] + cells[1]
    np.testing.assert_array_equal(f.variables["zone"][:], ids)
    np.testing.assert_array_equal(f.variables["ncells"][:], ncells)
    np.testing.assert_array_equal(f.variables["itt"][:], hdr[:, 0])
    np.testing.assert_array_equal(f.variables["dt"][:], hdr[:, 2])
    np.testing.assert_array_equal(f.variables["Time"][:], hdr[:, 1] / 86400.0)
    for j, v in enumerate(names):
        a, b = per_rank[0][:, :, j], per_rank[1][:, :, j]
        assert same_bits(f.variables[f"{v}_sum"][:], a[:, :, 0] + b[:, :, 0])
        np.testing.assert_array_equal(np.asarray(f.variables[f"{v}_min"][:])[:, :3], np.minimum(a[:, :, 1], b[:, :, 1])[:, :3])
        np.testing.assert_array_equal(np.asarray(f.variables[f"{v}_max"][:])[:, :3], np.maximum(a[:, :, 2], b[:, :, 2])[:, :3])
        assert same_bits(np.asarray(f.variables[f"{v}_mean"][:])[:, :3], (a[:, :, 0] + b[:, :, 0])[:, :3] / ncells[:3])
        for key in ("min", "max", "mean"):
            assert (np.asarray(f.variables[f"{v}_{key}"][:])[:, 3] == zt.FILL).all(), "a zone without a column on any rank"
        np.testing.assert_array_equal(np.asarray(f.variables[f"{v}_min"][:])[:, 2], b[:, 2, 1])   # (only rank 1 holds zone index 2)
    for key, col in (("itt", 0), ("Time", 1)):
        hdr2 = hdr.copy()
        hdr2[3, col] += 600
        other = str(tmp_path / "other.zonal_totals.0001.nc")
        zt._write_file(other, zt._file_variables(hdr2, per_rank[1], names, ids, cells[1], "2018-01-01 00:00:00"), "run")
        with pytest.raises(ValueError, match=f"{key} of .*other.zonal_totals.0001.nc differs"):
            zt.combine([paths[0], other], str(tmp_path / "refused.nc"))
    zt._write_file(other, zt._file_variables(hdr, per_rank[1], names, ids + 1, cells[1], "2018-01-01 00:00:00"), "run")
    with pytest.raises(ValueError, match="zone of .*other.zonal_totals.0001.nc differs"):
        zt.combine([paths[0], other], str(tmp_path / "refused.nc"))


@pytest.fixture
def zonal_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []

    def make(*a, **k):
        made.append(ZonalOracleContext(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


VARS = ["theta_rz", "q_ss", "swe", "S_rz", "prec"]
ZONES = np.array([[30, 30, 10, 10], [30, 0, 10, -4], [20, 20, 20, 10], [0, 20, 30, 30]])    # ids 10, 20, 30; three columns outside


def make_model(tmp_path, zones=ZONES, variables=VARS, capacity=8, ndays=6, **kw):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, **kw)

    def set_diagnostics(self, state):
        state.zonal_totals.zones = zones
        state.zonal_totals.output_variables = list(variables)
        state.zonal_totals.base_output_path = str(tmp_path)
        state.zonal_totals.capacity = capacity

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model, g


@pytest.mark.parametrize("script_hooks,by_routine", [(None, False), ("plain", False), ("plain", True)])
def test_script_writes_tree_totals_of_the_doubles_planes_per_zone(zonal_backend, tmp_path, monkeypatch, script_hooks, by_routine):
    """svat_hetero_combo, capacity 8: the ring is drained many times and the file holds every step, every zone equal to the totals'
    rule with mask = zones == id."""
    from nc_util import netcdf_file

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    model, g = make_model(tmp_path, script_hooks=script_hooks)
    assert tuple(int(v) for v in g["nx_ny"]) == ZONES.shape
    model.setup()
    ctx = zonal_backend[-1]
    ids = [10, 20, 30]
    initial = np.array([[tree_totals(ctx.download(v), ZONES == i) for v in VARS] for i in ids])
    planes, reads = [], []
    accumulate, read = ctx._accumulate, ctx.zonal_read
    ctx._accumulate = lambda: (accumulate(), planes.append({v: ctx.download(v).copy() for v in VARS}))[0]
    ctx.zonal_read = lambda first, n: (reads.append((first, n)), read(first, n))[1]
    model.run()
    trace = ctx.zonal_trace
    rows, cells = ctx.zonal_count()
    assert len(trace) > 5 * 8 and rows == len(trace) == len(planes) and list(cells) == [4, 4, 5]
    assert len(reads) >= len(trace) // 8 and max(n for _, n in reads) <= 8, "the ring was not drained in pieces of at most its capacity"
    f = netcdf_file(str(tmp_path / "GoldenSVAT.zonal_totals.nc"))
    t = f.variables["Time"][:]
    assert len(t) == len(trace) + 1 and t[0] == 0 and np.all(np.diff(t) > 0) and t[-1] * 86400 == model.state.settings.runlen
    assert f.variables["Time"].time_origin == b"2018-01-01 00:00:00" and f.variables["dt"].units == b"s"
    np.testing.assert_array_equal(f.variables["dt"][:], [0] + [h[2] for h, _ in trace])
    np.testing.assert_array_equal(f.variables["itt"][:], [0] + [h[0] for h, _ in trace])
    np.testing.assert_array_equal(f.variables["zone"][:], ids)
    assert f.variables["ncells"].dimensions == ("zone",) and list(f.variables["ncells"][:]) == [4, 4, 5]
    for j, v in enumerate(VARS):
        for k, stat in enumerate(("sum", "min", "max")):
            a = np.asarray(f.variables[f"{v}_{stat}"][:])
            assert f.variables[f"{v}_{stat}"].dimensions == ("Time", "zone") and a.dtype == np.float64
            assert same_bits(a[0], initial[:, j, k]), f"{v}_{stat}: record 0 holds the initial values"
            want = np.array([[tree_totals(p[v], ZONES == i)[k] for i in ids] for p in planes])
            assert same_bits(a[1:], want), f"{v}_{stat}"
        assert same_bits(f.variables[f"{v}_mean"][:], np.asarray(f.variables[f"{v}_sum"][:]) / np.array([4.0, 4.0, 5.0]))
        assert np.any(np.asarray(f.variables[f"{v}_sum"][:]) != 0), v


def test_run_device_called_directly(zonal_backend, tmp_path):
    """run_device(n) drains before and after; more steps than the ring holds are refused before anything is enqueued."""
    model, _ = make_model(tmp_path)
    model.setup()
    ctx = zonal_backend[-1]
    model.run_device(8)
    model.run_device(5)
    assert ctx.zonal_count()[0] == 13 and sum(len(h) for h in model.state.zonal_totals._hdr) == 14
    with pytest.raises(RuntimeError, match="shorter pieces"):
        model.run_device(9)
    assert int(model.state.variables.itt) == 13 and ctx.zonal_count()[0] == 13


def test_validation(zonal_backend, tmp_path):
    for kw, exc, text in ((dict(zones=np.ones((4, 5), dtype=int)), ValueError, r"zone map has shape \(4, 5\)"),
                          (dict(zones=np.ones(16, dtype=int)), ValueError, r"zone map has shape \(16,\)"),
                          (dict(zones=np.zeros((4, 4), dtype=int)), ValueError, "holds no column in any zone"),
                          (dict(zones=np.ones((4, 4))), ValueError, "float64 values"),
                          (dict(variables=["theta_rz", "lu_id"]), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(variables=["no_such_variable"]), NotImplementedError, "no_such_variable"),
                          (dict(variables=["prec"] * 33), ValueError, "33 variables"),
                          (dict(capacity=0), ValueError, "capacity = 0")):
        model, g = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model, _ = make_model(tmp_path, variables=[], ndays=1)
    model.setup()
    model.run()
    assert zonal_backend[-1]._zring is None and not list(tmp_path.iterdir())


def test_more_than_1024_zones_and_the_offline_transport_are_refused():
    from roger_amd import zonal_totals
    from roger_amd.state import RogerState

    st = RogerState()
    with st.settings.unlock():
        st.settings.nx, st.settings.ny = 41, 25
    st.zonal_totals.zones = np.arange(1, 1026).reshape(41, 25)
    st.zonal_totals.output_variables = []
    zonal_totals.initialize(st)   # (no variables: inactive)
    st.zonal_totals.output_variables = ["prec"]
    with pytest.raises(ValueError, match=r"1025 zones \(at most 1024\)"):
        zonal_totals.initialize(st)
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    with pytest.raises(NotImplementedError, match="offline transport.*transport_totals"):
        zonal_totals.initialize(st)
