"""GPU: zonal totals (rh_zonal_*, k_zonal_tiles / k_zonal_finish in roger_amd/csrc/rh_zonal.h) against the totals' host restatement applied
per zone (tests/totals_reference.py: tree_totals(plane, zones == z)).

The reference is tests/test_hip_points.py's: a context WITHOUT observers that steps one step at a time and downloads the observed planes
after every step.  Rows come from one rh_run_steps call.  Comparison rule: sums as bits, minimum and maximum by value, headers exactly.

Grids: 3 x 2 (one partial wavefront), 257 x 1 (two tiles, a stripe across the tile edge), 40 x 25 (four tiles), each for SVAT and oneD, and
65 537 x 1 (257 tiles: accumulator 0 takes tiles 0 and 256).  Maps: one zone everywhere; stripes of 5 columns (13 zones in a wavefront);
a checkerboard of two zones; `mixed`: a zone of one column, zone ids without a column, and columns outside every zone that make an empty
wavefront and (40 x 25) an empty tile; 1000 random ids over 65 537 columns.

The reference costs 0.26 ms per (row, zone, variable) at 1000 columns and 5 ms at 65 537, so the stripes (200 zones on 40 x 25) are compared
over the first 24 steps and three variables; on 65 537 columns every (row, zone, variable) is compared with the host package's zone_totals
(which tests/test_zonal_reference.py pins to tree_totals bit for bit) and the last row of one variable with tree_totals itself."""
import functools

import numpy as np
import pytest

from diag_reference import HostAccumulator
from test_hip_points import CASES, M1, NSTEPS, VARS, make_ctx, reference, same_bits
from totals_reference import tree_totals

pytestmark = pytest.mark.gpu

KINDS = ("one", "stripes", "checker", "mixed")
FEW = ("aet", "S_rz", "swe")         # the stripes' variables (a pure output among them)
STRIPE_STEPS = 24


def zones_of(nx, ny, kind):
    """(zone index per column int32, -1 outside; number of zones)"""
    n = nx * ny
    i = np.arange(n)
    if kind == "one":
        return np.zeros(n, dtype=np.int32), 1
    if kind == "stripes":
        return (i // 5).astype(np.int32), (n + 4) // 5
    if kind == "checker":
        return ((i // ny + i % ny) % 2).astype(np.int32), 2
    if kind == "half":      # tests/test_hip_totals.py's mask as one zone
        from test_hip_totals import mask_of

        return np.where(mask_of(nx, ny, "half"), 0, -1).astype(np.int32), 1
    assert kind == "mixed"
    if n == 6:
        return np.array([0, -1, 1, 0, 0, -1], dtype=np.int32), 4         # zone 1: one column; zones 2, 3: none
    z = np.random.default_rng(7 + n).integers(0, 3, size=n).astype(np.int32)
    z[64:128] = -1                                                        # an empty wavefront
    if n == 257:
        z[256] = 3                                                        # the second tile's only column, a zone of its own
        return z, 5                                                       # zone 4: none
    z[256:512] = -1                                                       # an empty tile
    z[700] = 4                                                            # a zone of one single column
    return z, 7                                                           # zones 5, 6: none


def setup_of(kind):
    return (FEW, STRIPE_STEPS) if kind == "stripes" else (VARS, NSTEPS)


@functools.lru_cache(maxsize=None)
def want_rows(nx, ny, lateral, kind, names, nrows):
    """(nrows, Z, V, 3): tree_totals of the reference's planes after every step, per zone."""
    ref = reference(nx, ny, lateral)
    zone, nz = zones_of(nx, ny, kind)
    out = np.array([[[tree_totals(ref.planes[v][k], zone == z) for v in names] for z in range(nz)] for k in range(nrows)])
    out.setflags(write=False)
    return out


def assert_zonal(got_hdr, got, want_hdr, want, names, what):
    np.testing.assert_array_equal(got_hdr, want_hdr, err_msg=f"{what}: headers")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for j, v in enumerate(names):
        ok = np.ascontiguousarray(got[:, :, j, 0]).view(np.uint64) == np.ascontiguousarray(want[:, :, j, 0]).view(np.uint64)
        assert ok.all(), (what, v, "sum, (row, zone)", np.argwhere(~ok)[:5], got[:, :, j, 0][~ok][:3], want[:, :, j, 0][~ok][:3])
        for k, stat in ((1, "min"), (2, "max")):
            ok = got[:, :, j, k] == want[:, :, j, k]
            assert ok.all(), (what, v, stat, "(row, zone)", np.argwhere(~ok)[:5], got[:, :, j, k][~ok][:3], want[:, :, j, k][~ok][:3])


def assert_rows(ctx, nx, ny, lateral, kind, names, first, n, what, upto=NSTEPS):
    hdr, vals = ctx.zonal_read(first, n)
    ref = reference(nx, ny, lateral)
    assert_zonal(hdr, vals, ref.hdr[first:first + n], want_rows(nx, ny, lateral, kind, tuple(names), upto)[first:first + n], names, what)


def configured(nx, ny, lateral, kind, names=VARS, **kw):
    ctx, _ = make_ctx(nx, ny, lateral)
    zone, nz = zones_of(nx, ny, kind)
    ctx.zonal_configure(names, zone, nz, **kw)
    rows, cells = ctx.zonal_count()
    assert rows == 0 and list(cells) == list(np.bincount(zone[zone >= 0], minlength=nz))
    return ctx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_one_call_records_every_step(nx, ny, lateral, kind):
    """1. One rh_run_steps call, every map; the zonal recorder is the only observer and pure outputs are among its planes, so the sparse
    KEEP kernel ran.  On 40 x 25, one zone and checkerboard: the guard against a test that pins nothing -- somewhere the tree's sum is
    not the left-to-right sum."""
    names, nsteps = setup_of(kind)
    ctx = configured(nx, ny, lateral, kind, names)
    assert {"aet"} <= set(ctx.pure_output_planes())
    ctx.run_steps(nsteps)
    assert ctx.zonal_count()[0] == nsteps
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, nx, ny, lateral, kind, names, 0, nsteps, f"{nx} x {ny} lateral={lateral} map={kind}", upto=nsteps)
    ctx.close()
    if (nx, ny) == (40, 25) and kind in ("one", "checker"):
        ref, want = reference(nx, ny, lateral), want_rows(nx, ny, lateral, kind, tuple(names), nsteps)
        zone, nz = zones_of(nx, ny, kind)
        serial = np.array([[[np.add.accumulate(ref.planes[v][k][zone == z])[-1] for v in names] for z in range(nz)] for k in range(nsteps)])
        differ = serial.view(np.uint64) != np.ascontiguousarray(want[:, :, :, 0]).view(np.uint64)
        print(f"tree sum != left-to-right sum in {int(differ.sum())} of {differ.size} (row, zone, variable) triples")
        assert differ.any(), "the order of the sum is not what this test compares"
        assert all(np.any(want[:, :, j, 0] != 0) for j in range(len(names)))


@pytest.mark.parametrize("lateral", [False, True])
def test_totals_and_zonal_rings_hold_the_same_sums(lateral):
    """2. One context with rh_totals_configure(mask) and rh_zonal_configure of the single zone `mask`: the sums of the two rings are equal
    bit for bit in every row (minimum and maximum by value)."""
    from test_hip_totals import mask_of

    nx, ny = 40, 25
    ctx, _ = make_ctx(nx, ny, lateral)
    mask = mask_of(nx, ny, "half")
    zone, nz = zones_of(nx, ny, "half")
    ctx.totals_configure(VARS, mask)
    ctx.zonal_configure(VARS, zone, nz)
    ctx.run_steps(NSTEPS)
    th, tv = ctx.totals_read(0, NSTEPS)
    zh, zv = ctx.zonal_read(0, NSTEPS)
    assert zv.shape == (NSTEPS, 1, len(VARS), 3)
    assert_zonal(zh, zv, th, tv[:, None], VARS, "the totals' ring against the zonal ring")
    assert ctx.zonal_count()[1][0] == ctx.totals_count()[1] == int(mask.sum())
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_calls_in_pieces_record_the_same_rows(nx, ny, lateral):
    """3. Pieces of 1, 2, 37 steps and the rest."""
    ctx = configured(nx, ny, lateral, "mixed")
    done = 0
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
        done += n
        assert ctx.zonal_count()[0] == done
    assert_rows(ctx, nx, ny, lateral, "mixed", VARS, 0, NSTEPS, f"{nx} x {ny} lateral={lateral} in pieces")
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_launches_behind_the_time_limit_record_nothing(nx, ny, lateral):
    """4. 500 steps enqueued under a limit of three days: as many rows as the reference needs steps, none beyond the limit."""
    ref = reference(nx, ny, lateral)
    limit = 3 * 86400
    want = int(np.searchsorted(ref.hdr[:, 1], limit)) + 1
    assert ref.hdr[want - 1, 1] == limit and 3 < want < NSTEPS
    ctx = configured(nx, ny, lateral, "mixed")
    ctx.set_time_limit(limit)
    ctx.run_steps(500)
    assert ctx.zonal_count()[0] == want
    assert_rows(ctx, nx, ny, lateral, "mixed", VARS, 0, want, f"{nx} x {ny} lateral={lateral} under the limit")
    ctx.run_steps(5)
    assert ctx.zonal_count()[0] == want
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_ring_keeps_the_last_rows_and_refuses_the_overwritten_ones(nx, ny, lateral):
    """5. capacity 16 over 150 steps."""
    from roger_amd._native import NativeError

    ctx = configured(nx, ny, lateral, "checker", capacity=16)
    ctx.run_steps(NSTEPS)
    assert ctx.zonal_count()[0] == NSTEPS
    assert_rows(ctx, nx, ny, lateral, "checker", VARS, NSTEPS - 16, 16, "the resident rows")     # straddles the wrap: 134 = 8 * 16 + 6
    assert_rows(ctx, nx, ny, lateral, "checker", VARS, NSTEPS - 5, 5, "the last rows")
    for first, n in ((NSTEPS - 17, 1), (NSTEPS - 17, 17), (0, 1)):
        with pytest.raises(NativeError, match=r"rh_zonal_read failed \(-1\).*overwritten"):
            ctx.zonal_read(first, n)
    with pytest.raises(NativeError, match=r"rh_zonal_read failed \(-1\).*not been recorded"):
        ctx.zonal_read(NSTEPS - 1, 2)
    ctx.close()


@pytest.mark.parametrize("order", ["first", "last", "again"])
@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_four_observers_keep_each_others_planes(nx, ny, lateral, order):
    """6. Zonal totals configured first, last, and configured a second time while accumulators, points and totals are active, on disjoint
    pure outputs: all four equal their references.  Fails if one configure call drops another's keep bits."""
    from test_hip_points import POINTS, assert_rows as assert_point_rows
    from test_hip_totals import assert_rows as assert_total_rows, mask_of

    ref, cells = reference(nx, ny, lateral), POINTS[(nx, ny)]
    rate, collect = ("q_ss",), ("S_rz",)
    p_names, t_names, z_names = ("transp", "theta"), ("q_rz", "evap_soil"), ("aet", "inf_mat_rz", "swe")
    ctx, _ = make_ctx(nx, ny, lateral)
    assert {"q_ss", "transp", "theta", "q_rz", "evap_soil", "aet"} <= set(ctx.pure_output_planes())
    zone, nz = zones_of(nx, ny, "mixed")

    def zonal():
        ctx.zonal_configure(z_names, zone, nz)

    def others():
        ctx.totals_configure(t_names, mask_of(nx, ny, "half"))
        ctx.points_configure(cells, p_names)
        ctx.diag_configure(rate=rate, collect=collect, n_slots=3)

    if order == "first":
        zonal(), others()
    elif order == "last":
        others(), zonal()
    else:
        ctx.zonal_configure(("theta", "q_rz"), np.zeros(ctx.n, dtype=np.int32), 1, capacity=3)
        others(), zonal()
    acc = HostAccumulator(rate, collect, 3, ctx.n)
    for k in range(NSTEPS):
        acc.add(ref.hdr[k, 1], ref.hdr[k, 2], {v: ref.planes[v][k] for v in rate + collect})
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_rows(ctx, nx, ny, lateral, "mixed", z_names, 0, NSTEPS, f"zonal, configured {order}")
    assert_total_rows(ctx, nx, ny, lateral, "half", t_names, 0, NSTEPS, f"totals, zonal configured {order}")
    assert_point_rows(ctx, ref, p_names, cells, 0, NSTEPS, f"points, zonal configured {order}")
    for slot in range(3):
        for v in rate + collect:
            assert same_bits(ctx.diag_download(v, slot), acc.data[v][slot]), (v, slot, order)
    ctx.zonal_configure(())   # releasing the zonal totals leaves the others' planes kept
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES)
def test_an_observed_m1_plane_switches_the_lazy_rotation_off(nx, ny, lateral):
    """7. S_rz_m1 among the variables: the rows equal the reference and the run ends in the reference's state, bit for bit."""
    import hip_util as H

    ref = reference(nx, ny, lateral)
    names = ("q_ss", M1, "S_rz", "aet")
    ctx = configured(nx, ny, lateral, "checker", names)
    ctx.run_steps(NSTEPS)
    assert not ctx.step_mode()[0], "the lazy rotation stayed on"
    assert_rows(ctx, nx, ny, lateral, "checker", names, 0, NSTEPS, "with an X_m1 plane")
    assert np.any(want_rows(nx, ny, lateral, "checker", names, NSTEPS)[:, :, 1, 0] != 0)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), ref.final_scalars)
    for nm, want in ref.final.items():
        got = ctx.download(nm)
        assert got.dtype == want.dtype and (same_bits(got, want) if got.dtype.kind == "f" else (got == want).all()), nm
    ctx.close()


def assert_last_row_is_the_state(ctx, names, zone, nz, k, what):
    """Row k - 1 (the k-th step's) against tree_totals of the context's own planes per zone, and its scalars, after that step."""
    assert ctx.zonal_count()[0] == k, what
    hdr, vals = ctx.zonal_read(k - 1, 1)
    s = ctx.get_scalars()
    planes = {v: ctx.download(v) for v in names}
    want = np.array([[[tree_totals(planes[v], zone == z) for v in names] for z in range(nz)]])
    assert_zonal(hdr, vals, np.array([[s.itt, s.time, s.dt_secs]]), want, names, f"{what} step {k}")


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("path", ["routines", "svat_step"])
def test_single_step_paths_record_one_row_per_step(path, lateral):
    """8. rh_adaptive_dt / rh_step_core / rh_after_timestep and rh_svat_step: one row per step, equal to tree_totals of the downloads
    after that step (observed are planes rh_after_timestep does not assign)."""
    from test_hip_points import host_hooks

    nx, ny = 257, 1
    names = ("prec", "aet", "q_ss", "inf_mat_rz", "S_rz", "theta", "swe")
    zone, nz = zones_of(nx, ny, "mixed")
    ctx, forcing = make_ctx(nx, ny, lateral)
    ctx.zonal_configure(names, zone, nz)
    classes = set()
    for k in range(1, 61):
        monthly = host_hooks(ctx, forcing)
        if path == "routines":
            ctx.call("rh_adaptive_dt")
            if monthly:
                ctx.call("rh_params_surface")
            ctx.call("rh_step_core")
            ctx.call("rh_after_timestep")
        else:
            ctx.step(monthly)
        assert_last_row_is_the_state(ctx, names, zone, nz, k, f"{path} lateral={lateral}")
        classes.add(ctx.get_scalars().dt_secs)
    assert len(classes) >= 2, classes
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", CASES[2:])
def test_one_rank_communicator_records_like_run_steps(nx, ny, lateral):
    """9. rh_run_steps_dist with a one-rank RCCL communicator."""
    from roger_amd import _native as native

    ctx, _ = make_ctx(nx, ny, lateral)
    ctx.comm_init(native.comm_unique_id(), 1, 0)
    zone, nz = zones_of(nx, ny, "mixed")
    ctx.zonal_configure(VARS, zone, nz)
    ctx.run_steps_dist(NSTEPS)
    assert ctx.zonal_count()[0] == NSTEPS
    assert_rows(ctx, nx, ny, lateral, "mixed", VARS, 0, NSTEPS, "rh_run_steps_dist, one rank")
    ctx.close()


def test_routed_steps_record_one_row_per_step(monkeypatch):
    """10. The routed step on the smallest routing golden: rh_step_routed step by step against the downloads after each step, then the
    device-driven routed steps of rh_run_steps (and RH_ROUTED_BY_ROUTINE=1) against those rows."""
    import hip_util as H
    from golden_util import ROUTING_CASES, load_case
    from test_hip_routing import routed_ctx

    from roger_amd import _native as native

    g, names_all, forcing = load_case(ROUTING_CASES[0])
    names = ("q_sur_out", "q_sub_in", "aet", "prec", "S", "z0", "q_ss")
    nsteps = 40
    ctx = routed_ctx(native, g, names_all)
    zone, nz = (np.arange(ctx.n) % 4 - 1).astype(np.int32), 3      # every fourth column outside
    ctx.zonal_configure(names, zone, nz)
    drv = H.HipForcingDriver(ctx, forcing)
    for k in range(1, nsteps + 1):
        ctx.step_routed(drv.before_step())
        assert_last_row_is_the_state(ctx, names, zone, nz, k, "rh_step_routed")
    want_hdr, want = ctx.zonal_read(0, nsteps)
    assert all(np.any(want[:, :, j, 0] != 0) for j in range(len(names)) if names[j] != "q_sub_in"), "a routed variable never held a value"
    ctx.close()
    for by_routine in (False, True):
        if by_routine:
            monkeypatch.setenv("RH_ROUTED_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_ROUTED_BY_ROUTINE", raising=False)
        ctx = routed_ctx(native, g, names_all)
        ctx.set_forcing_series(forcing)
        ctx.zonal_configure(names, zone, nz)
        ctx.run_steps(nsteps)
        assert ctx.zonal_count()[0] == nsteps
        hdr, vals = ctx.zonal_read(0, nsteps)
        assert_zonal(hdr, vals, want_hdr, want, names, f"rh_run_steps on a routing context, by_routine={by_routine}")
        ctx.close()


@functools.lru_cache(maxsize=None)
def big_reference():
    """65 537 x 1, SVAT, 20 steps, as tests/test_hip_totals.py forms it (without the assertion on the water-balance flag)."""
    import hip_util as H

    nx, nsteps, names = 65537, 20, ("S_rz", "theta", "aet", "swe")
    ctx, forcing = make_ctx(nx, 1, False)
    drv = H.HipForcingDriver(ctx, forcing)
    hdr, planes = [], {v: [] for v in names}
    for _ in range(nsteps):
        ctx.step(drv.before_step())
        s = ctx.get_scalars()
        hdr.append((s.itt, s.time, s.dt_secs))
        for v in names:
            planes[v].append(ctx.download(v))
    ctx.close()
    return np.array(hdr, dtype=np.int64), planes, names


@pytest.mark.parametrize("kind", ["one", "random1000"])
def test_the_strided_pass_over_more_than_256_tiles(kind):
    """11. 257 tiles.  One zone: accumulator 0 adds the partial of tile 256 to that of tile 0, compared with tree_totals in every row; the
    reference differs from the sum of the first 256 tiles.  1000 random ids: zones that skip most tiles, accumulators with lists of
    different lengths; the zone of the last column also lies in tile 0."""
    from roger_amd.zonal_totals import zone_totals

    nx, nsteps = 65537, 20 if kind == "one" else 4      # (zone_totals over 58 000 (tile, zone) pairs takes 0.6 s per (row, variable))
    ref_hdr, planes, names = big_reference()
    ref_hdr = ref_hdr[:nsteps]
    if kind == "one":
        zone, nz = np.zeros(nx, dtype=np.int32), 1
    else:
        zone, nz = np.random.default_rng(1000).integers(0, 1000, size=nx).astype(np.int32), 1000
        zone[3] = zone[65536]
        assert len(np.unique(zone)) == 1000
    ctx, _ = make_ctx(nx, 1, False)
    ctx.zonal_configure(names, zone, nz)
    ctx.run_steps(nsteps)
    rows, cells = ctx.zonal_count()
    assert rows == nsteps and list(cells) == list(np.bincount(zone, minlength=nz))
    hdr, vals = ctx.zonal_read(0, nsteps)
    ctx.close()
    if kind == "one":
        want = np.array([[[tree_totals(planes[v][k]) for v in names]] for k in range(nsteps)])
        first256 = np.array([[tree_totals(planes[v][k][:65536])[0] for v in names[:2]] for k in range(nsteps)])
        assert (first256 != want[:, 0, :2, 0]).all(), "the last tile's column does not show in the sum"
    else:
        want = np.stack([np.stack([zone_totals(planes[v][k], zone, nz) for v in names], axis=1) for k in range(nsteps)])
        last = np.array([tree_totals(planes["S_rz"][nsteps - 1], zone == z) for z in range(nz)])
        assert same_bits(want[-1, :, 0, 0], last[:, 0]) and np.array_equal(want[-1, :, 0, 1:], last[:, 1:])
    assert_zonal(hdr, vals, ref_hdr, want, names, f"257 tiles, {kind}")


def test_refusals_and_release():
    """12. RH_ERR_ARG with the offending value in the text, RH_ERR_STATE before the configuration and after the release; a new series
    starts from row 0."""
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx, _ = make_ctx(3, 2, False)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    for call in (ctx.zonal_count, lambda: ctx.zonal_read(0, 0)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    zone = np.array([0, -1, 1, 0, 0, -1], dtype=np.int32)
    ok = dict(zones=zone, n_zones=3)
    ctx.zonal_configure(("theta", "swe"), capacity=4, **ok)
    ctx.run_steps(3)
    bad = ((dict(names=(ints[0],), **ok), f"plane {ints[0]} is int32"), (dict(names=(not_held[0],), **ok), f"plane id {ctx.index[not_held[0]]} "),
           (dict(names=floats[:33], **ok), "n_planes = 33"), (dict(names=("theta",), capacity=0, **ok), "capacity = 0"),
           (dict(names=("theta",), capacity=-3, **ok), "capacity = -3"),
           (dict(names=("theta",), zones=zone, n_zones=0), "n_zones = 0"), (dict(names=("theta",), zones=zone, n_zones=1025), "n_zones = 1025"),
           (dict(names=("theta",), zones=zone, n_zones=1), "zone id 1 of column 2"),
           (dict(names=("theta",), zones=np.array([0, 0, -2, 0, 0, 0]), n_zones=1), "zone id -2 of column 2"),
           (dict(names=("theta",), zones=np.full(6, -1), n_zones=2), "0 of 6 "))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_zonal_configure failed \(-1\)") as e:
            ctx.zonal_configure(**kw)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="the zone map has 5 values"):
        ctx.zonal_configure(("theta",), np.zeros(5, dtype=np.int32), 1)
    # every refusal left the configuration working
    ctx.run_steps(2)
    rows, cells = ctx.zonal_count()
    assert rows == 5 and list(cells) == [3, 1, 0]
    hdr, vals = ctx.zonal_read(1, 4)
    assert list(hdr[:, 0]) == [2, 3, 4, 5] and vals.shape == (4, 3, 2, 3)
    assert same_bits(vals[-1, 0, 0, 0], tree_totals(ctx.download("theta"), zone == 0)[0])
    assert vals[-1, 1, 1, 0] == vals[-1, 1, 1, 1] == vals[-1, 1, 1, 2] == ctx.download("swe")[2], "a zone of one column"
    assert (vals[:, 2, :, 0] == 0).all() and not np.signbit(vals[:, 2, :, 0]).any() and (vals[:, 2, :, 1] == np.inf).all() and (vals[:, 2, :, 2] == -np.inf).all()
    # 32 planes and 1024 zones are accepted, and the release
    ctx.zonal_configure(floats[:32], zone, 1024, capacity=2)
    ctx.run_steps(3)
    hdr, vals = ctx.zonal_read(1, 2)
    assert vals.shape == (2, 1024, 32, 3) and same_bits(vals[-1, 0, 5, 0], tree_totals(ctx.download(floats[5]), zone == 0)[0])
    ctx.zonal_configure(())
    ctx.run_steps(2)
    for call in (ctx.zonal_count, lambda: ctx.zonal_read(0, 1)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.zonal_configure(("theta",), np.zeros(6, dtype=np.int32), 1, capacity=1)   # a new series starts at row 0
    assert ctx.zonal_count()[0] == 0
    ctx.run_steps(2)
    hdr, vals = ctx.zonal_read(1, 1)
    assert hdr[0, 0] == 12 and vals[0, 0, 0, 1] == ctx.download("theta").min() and vals[0, 0, 0, 2] == ctx.download("theta").max()
    ctx.close()


def test_script_on_the_device_writes_what_the_routine_by_routine_step_writes(tmp_path, monkeypatch):
    """13. End to end: a RogerSetup script with the reference's hook bodies and zonal totals with capacity 8 writes the same
    `.zonal_totals.nc` values as the same script stepped routine by routine."""
    import svat_scripts as S
    from golden_util import load_case
    from nc_util import netcdf_file

    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    variables, ndays = ["theta_rz", "q_ss", "swe", "S_rz", "aet", "prec"], 6
    nx, ny = (int(v) for v in g["nx_ny"])
    zones = np.random.default_rng(4).integers(-1, 4, size=(nx, ny)) * 10      # ids 10, 20, 30; -10 and 0 outside
    ids = [10, 20, 30]
    assert all((zones == i).any() for i in ids) and (zones <= 0).any()
    keys = ["Time", "dt", "itt", "ncells", "zone"] + [f"{v}_{s}" for v in variables for s in ("sum", "min", "max", "mean")]
    out = {}
    for mode in ("device", "routine"):
        if mode == "routine":
            monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
        else:
            monkeypatch.delenv("RH_STEP_BY_ROUTINE", raising=False)
        model = S.make_model(S.params_from_golden(g, names), forcing, ndays, script_hooks="plain")
        path = tmp_path / mode

        def set_diagnostics(self, state, path=path):
            state.zonal_totals.zones = zones
            state.zonal_totals.output_variables = list(variables)
            state.zonal_totals.base_output_path = str(path)
            state.zonal_totals.capacity = 8

        type(model).set_diagnostics = roger_routine(set_diagnostics)
        model.setup()
        assert model.device_run_possible() == (mode == "device")
        rounds = []
        inner = model.run_device
        model.run_device = lambda n, final=True, inner=inner, rounds=rounds: (rounds.append(n), inner(n, final=final))[1]
        model.run()
        assert (mode == "device") == bool(rounds) and all(n <= 8 for n in rounds), rounds
        f = netcdf_file(str(path / "GoldenSVAT.zonal_totals.nc"))
        out[mode] = {k: np.asarray(f.variables[k][:]) for k in keys}
        model.state.backend_context.close()
    nsteps = int(np.sum(g["scal"][:, 1] <= ndays * 86400))
    d = out["device"]
    for k, a in d.items():
        b = out["routine"][k]
        if a.dtype.kind == "f" and not k.endswith(("_min", "_max")):
            assert same_bits(a, b), k
        else:
            assert a.shape == b.shape and np.array_equal(a, b), k
    assert list(d["zone"]) == ids and list(d["ncells"]) == [int((zones == i).sum()) for i in ids]
    assert len(d["Time"]) == nsteps + 1 and d["Time"][-1] == ndays and d["dt"][0] == 0 and list(d["itt"]) == list(range(nsteps + 1))
    for v in variables:
        assert d[f"{v}_sum"].shape == (nsteps + 1, 3) and np.any(d[f"{v}_sum"][1:] != 0), v
        assert same_bits(d[f"{v}_mean"], d[f"{v}_sum"] / d["ncells"].astype(np.float64))
