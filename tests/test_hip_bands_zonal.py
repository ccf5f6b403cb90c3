"""GPU: ensemble bands per zone (rh_bands_configure_zonal; k_bands_zonal and k_bands_zonal_row in roger_amd/csrc/rh_bands.h) against the ONE
rule they promise -- block z of a row is the row of the plain bands under mask = (zone == z) -- restated on the host
(tests/bands_zonal_reference.py over tests/bands_reference.py) and, directly, against rh_bands_configure itself: every value by bits,
every integer exactly, no tolerance.

The helpers are tests/test_hip_bands.py's: the crafted values go into theta_irr under dry days (dry_ctx; every step closes a daily
interval), the trajectory is the cached observer-free Reference of the two GRIDS over all three step classes."""
import numpy as np
import pytest

from bands_reference import LAST, SUM, rank_of
from bands_zonal_reference import HostZonalBands, fold, zonal_quantiles_of
from test_hip_bands import DAY, GRIDS, KINDS, NAMES, PLANE, PROBS, assert_rows, assert_state, dry_ctx, mask_of, middle_probs, reference
from test_hip_points import NDAYS, NSTEPS, float_planes, make_ctx

pytestmark = pytest.mark.gpu

TRIP = 256 * 8     # roger_amd/csrc/rh_bands.h: the columns a workgroup of k_bands_zonal reads in one trip of its loop (RH_BLOCK x U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def zonal_day(ctx, values, zone, n_zones, probs, what):
    """Upload `values`, step one (dry) day, and compare the row it closed with the restatement; (values (Z, P), counts (Z, 2))."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    rows = ctx.bands_count()
    ctx.upload(PLANE, values)
    ctx.run_steps(1)
    assert ctx.bands_count() == rows + 1, (what, "the step did not close a day")
    back = ctx.download(PLANE)
    assert same_bits(back, values), (what, "the step wrote the parameter plane")
    hdr, counts, got = ctx.bands_zonal_read(rows, 1)
    assert hdr.shape == (1, 2) and hdr[0, 1] == (hdr[0, 0] + 1) * DAY, (what, hdr)
    want, wcounts = zonal_quantiles_of(values, zone, n_zones, probs)
    assert counts.shape == (1, 1, n_zones, 2) and got.shape == (1, 1, n_zones, len(probs)), (what, counts.shape, got.shape)
    np.testing.assert_array_equal(counts[0, 0], wcounts, err_msg=f"{what}: (zone, {{m, n_nan}})")
    ok = got[0, 0].view(np.uint64) == want.view(np.uint64)
    assert ok.all(), (what, "(zone, probability)", np.argwhere(~ok)[:5], got[0, 0][~ok][:4], want[~ok][:4])
    return want, wcounts


def zonal_expected(ref, iv, zone, n_zones, first=0, nsteps=NSTEPS, probs=PROBS):
    h = HostZonalBands(KINDS, probs, ref.planes[NAMES[0]].shape[1], zone, n_zones, iv, 0)
    for k in range(first, nsteps):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in NAMES])
    return h.rows()


def assert_zonal_rows(got, want, what):
    (hdr, counts, values), (whdr, wcounts, wvalues) = got, want
    np.testing.assert_array_equal(hdr, whdr, err_msg=f"{what}: headers {{k, t1}}")
    np.testing.assert_array_equal(counts, wcounts, err_msg=f"{what}: counts (row, item, zone, {{m, n_nan}})")
    assert values.shape == wvalues.shape, (what, values.shape, wvalues.shape)
    ok = values.view(np.uint64) == wvalues.view(np.uint64)
    assert ok.all(), (what, "(row, item, zone, probability)", np.argwhere(~ok)[:5], values[~ok][:4], wvalues[~ok][:4])


def read_all(ctx):
    return ctx.bands_zonal_read(0, ctx.bands_count())


def three_zones(n):
    """Three interleaved zones with holes: every seventh column, and a whole wavefront."""
    i = np.arange(n)
    zone = (i % 3).astype(np.int32)
    zone[i % 7 == 3] = -1
    zone[64:128] = -1
    return zone


# ---- 1. zone list lengths ----
@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 255, 256, 257, TRIP + 1, 65537])
def test_zone_list_lengths(L, layout):
    """Zone 0 holds L columns -- a wavefront, a workgroup and one trip of the loop, each less one, exact and plus one; a single column; a
    list of many trips -- beside a second zone with the rest; the extreme sits in the last position of zone 0's list."""
    if layout == "contiguous":
        n = L + 37
        zone = (np.arange(n) >= L).astype(np.int32)
    else:
        n = 2 * L
        zone = (np.arange(n) % 2).astype(np.int32)
    last = int(np.flatnonzero(zone == 0)[-1])
    assert int((zone == 0).sum()) == L and last == (L - 1 if layout == "contiguous" else n - 2)
    rng = np.random.default_rng(L)
    probs = (0.0, 1.0 / L, 0.25, 0.5, 0.75, 1.0 - 1.0 / L, 1.0)
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, zones=zone, n_zones=2)
    for day in range(2):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-4, 5, n)
        x[rng.random(n) < 0.1] = 0.0
        if day == 1:
            x[last] = -1e300
        want, counts = zonal_day(ctx, x, zone, 2, probs, f"L = {L} {layout}, day {day}")
        assert counts.tolist() == [[L, 0], [n - L, 0]]
        assert day != 1 or (want[0, 0] == -1e300 and want[1, 0] > -1e300)
    ctx.close()


# ---- 2. zone counts ----
def test_zone_counts():
    rng = np.random.default_rng(2)
    probs = (0.0, 0.3, 0.5, 1.0)
    # one zone: the whole area, as the plain bands have it
    n = 300
    ctx = dry_ctx(n)
    zone = np.zeros(n, dtype=np.int32)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone)
    x = rng.normal(size=n)
    want, _ = zonal_day(ctx, x, zone, 1, probs, "Z = 1")
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2)
    ctx.upload(PLANE, x)
    ctx.run_steps(1)
    assert same_bits(ctx.bands_read(0, 1)[1][0, 0], want[0])
    # n_zones names zones that no column has (those of another rank): m = 0 and NaN there, the others untouched
    zone = np.where(np.arange(n) % 2 == 0, 0, 2).astype(np.int32)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone, n_zones=4)
    want, counts = zonal_day(ctx, x, zone, 4, probs, "zones 1 and 3 of 4 without a column")
    assert counts.tolist() == [[150, 0], [0, 0], [150, 0], [0, 0]] and np.isnan(want[[1, 3]]).all() and not np.isnan(want[[0, 2]]).any()
    ctx.close()
    # 1024 zones on 1024 + 37 columns: zones of two columns and of one
    n = 1024 + 37
    zone = (np.arange(n) % 1024).astype(np.int32)
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone)
    want, counts = zonal_day(ctx, rng.normal(size=n), zone, 1024, probs, "Z = 1024")
    assert (counts[:37, 0] == 2).all() and (counts[37:, 0] == 1).all() and (want[:37, 0] < want[:37, -1]).all() and (want[37:, 0] == want[37:, -1]).all()
    ctx.close()


# ---- 3. adversarial keys, each in one zone beside a zone of ordinary values ----
def test_adversarial_keys_per_zone():
    m0 = 300
    n = 2 * m0
    rng = np.random.default_rng(11)
    zone = (np.arange(n) % 2).astype(np.int32)
    at = np.flatnonzero(zone == 0)
    tiny, sub = np.finfo(np.float64).tiny, np.nextafter(0.0, 1.0)
    a = 0.3
    b = np.nextafter(a, 1.0)
    last_digit = (np.float64(1.5).view(np.uint64) + rng.integers(0, 512, m0).astype(np.uint64)).view(np.float64)   # equal but for the last 9 bits
    assert np.unique(last_digit.view(np.uint64) >> np.uint64(9)).size == 1 and np.unique(last_digit).size > 100
    zeros = np.zeros(m0)
    zeros[::3] = -0.0
    specials = rng.choice([np.inf, -np.inf, sub, -sub, tiny / 4, -tiny / 4, tiny, 1.0, -1.0, 0.0], m0)
    all_but_one_nan = np.full(m0, np.nan)
    all_but_one_nan[131] = -2.5
    neg_nan = np.full(m0, -np.nan)            # the sign bit of a NaN does not make it a value
    neg_nan[:10] = np.arange(10.0)
    cases = [("all equal", np.full(m0, 0.125)), ("negatives with positives", rng.normal(size=m0)), ("-0.0 among +0.0", zeros),
             ("infinities and subnormals", specials), ("all but one NaN", all_but_one_nan), ("all NaN", np.full(m0, np.nan)),
             ("NaN of either sign", neg_nan), ("every digit shared but the last", last_digit)]
    ctx = dry_ctx(n)

    def day(case, probs, what):
        x = rng.normal(size=n)                # the neighbour zone: ordinary values
        x[at] = case
        want, counts = zonal_day(ctx, x, zone, 2, probs, what)
        assert counts[1].tolist() == [m0, 0] and want[1, 0] < want[1, -1], (what, "the neighbour zone")
        return want, counts

    for what, case in cases:
        m = int((~np.isnan(case)).sum())
        probs = middle_probs(m)
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone)
        want, counts = day(case, probs, what)
        assert counts[0].tolist() == [m, m0 - m]
        if what == "-0.0 among +0.0":
            assert (want[0].view(np.uint64) == 0).all()
        if what == "all NaN":
            assert np.isnan(want[0]).all()
        if what == "all but one NaN":
            assert (want[0] == -2.5).all()
    # two values one unit in the last place apart: for each probability the split that puts the rank on the smaller and on the larger
    probs = (0.0, 0.25, 0.5, 0.75, 1.0)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 8, zones=zone)
    for p in probs[1:-1]:
        r = rank_of(p, m0)
        for small in (r, r + 1):                       # `small` columns hold a: rank r is b, then a
            case = np.full(m0, b)
            case[rng.permutation(m0)[:small]] = a
            want, _ = day(case, probs, f"ulp split {small} / {m0 - small}")
            assert want[0, probs.index(p)] == (a if small == r + 1 else b)
    ctx.close()


# ---- 4. items and probabilities ----
@pytest.mark.parametrize("n_probs", [1, 8])
@pytest.mark.parametrize("n_items", [1, 8])
def test_items_and_probabilities(n_items, n_probs):
    """SUM and LAST items over three dry days beside a context without observers that gives the planes after every step."""
    n = 600
    zone = three_zones(n)
    probs = (0.5,) if n_probs == 1 else tuple(np.linspace(0.0, 1.0, 8))
    ctx, bare = dry_ctx(n), dry_ctx(n)
    names = [v for v in float_planes(ctx) if not v.endswith("_m1")][:n_items]
    kinds = [(SUM, LAST)[j % 2] for j in range(n_items)]
    ctx.bands_configure(names, kinds, probs, DAY, 0, None, 4, zones=zone)
    h = HostZonalBands(kinds, probs, n, zone, 3, DAY, 0)
    for _ in range(3):
        ctx.run_steps(1)
        bare.run_steps(1)
        s = bare.get_scalars()
        assert int(s.dt_secs) == DAY
        h.add(int(s.time) - int(s.dt_secs), int(s.time), [bare.download(v) for v in names])
    got = read_all(ctx)
    assert got[1].shape == (3, n_items, 3, 2) and got[2].shape == (3, n_items, 3, n_probs)
    assert_zonal_rows(got, h.rows(), f"{n_items} items x {n_probs} probabilities")
    ctx.close()
    bare.close()


# ---- 5. through the step ----
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_one_call_against_the_restatement_per_zone(nx, ny, masked):
    ref = reference(nx, ny)
    zone = fold(three_zones(nx * ny), mask_of(nx * ny) if masked else None)
    want = zonal_expected(ref, 3600, zone, 3)
    assert NDAYS < len(want[0]) < NDAYS * 24 and (want[1][:, :, :, 0] == np.bincount(zone[zone >= 0], minlength=3)).all()
    assert (want[2][:, :, 0] != want[2][:, :, 1]).any() and (want[2][:, :, :, 0] < want[2][:, :, :, -1]).any()
    ctx, _ = make_ctx(nx, ny, False)
    ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, mask_of(nx * ny) if masked else None, NSTEPS, zones=three_zones(nx * ny))
    assert ctx.bands_count() == 0
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_zonal_rows(read_all(ctx), want, f"{nx} x {ny} masked={masked}")
    assert_state(ctx, ref, f"{nx} x {ny} masked={masked}")
    ctx.close()


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_pieces_with_the_zones_configured_in_the_middle_of_a_day(nx, ny):
    ref = reference(nx, ny)
    inside = [k for k in range(20, NSTEPS - 20) if ref.hdr[k - 1, 1] % DAY and ref.hdr[k, 1] % DAY]
    n1 = inside[len(inside) // 2]
    zone = fold(three_zones(nx * ny), mask_of(nx * ny))
    ctx, _ = make_ctx(nx, ny, False)
    ctx.run_steps(n1)
    ctx.bands_configure(NAMES, KINDS, PROBS, DAY, 0, None, NSTEPS, zones=zone, n_zones=3)
    for n in (1, 2, 37, NSTEPS - n1 - 40):
        ctx.run_steps(n)
    want = zonal_expected(ref, DAY, zone, 3, first=n1)
    assert len(want[0]) == NDAYS - int(ref.hdr[n1, 1]) // DAY and want[0][0, 0] == int(ref.hdr[n1, 1]) // DAY
    assert_zonal_rows(read_all(ctx), want, f"{nx} x {ny} configured after {n1} steps, in pieces")
    assert_state(ctx, ref, f"{nx} x {ny} in pieces")
    ctx.close()


# ---- 6. the promise, directly ----
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_block_z_is_the_plain_row_under_the_mask_of_zone_z(nx, ny):
    zone, mask = three_zones(nx * ny), mask_of(nx * ny)
    ctx, _ = make_ctx(nx, ny, False)
    ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, mask, NSTEPS, zones=zone)
    ctx.run_steps(NSTEPS)
    hdr, counts, values = read_all(ctx)
    ctx.close()
    assert len(hdr) > NDAYS
    for z in range(3):
        plain, _ = make_ctx(nx, ny, False)
        plain.bands_configure(NAMES, KINDS, PROBS, 3600, 0, (zone == z) & (mask != 0), NSTEPS)
        plain.run_steps(NSTEPS)
        phdr, pvalues = plain.bands_read(0, plain.bands_count())
        plain.close()
        got = (np.concatenate([hdr, counts[:, :, z].reshape(len(hdr), -1)], axis=1), values[:, :, z])
        assert_rows(got, (phdr, pvalues), f"{nx} x {ny}: block {z} against rh_bands_configure with mask = (zone == {z}) & mask")


# ---- 7. ring ----
def test_ring_release_reconfiguration_and_the_wrong_read():
    from roger_amd._native import NativeError

    n = 257
    rng = np.random.default_rng(5)
    zone = (np.arange(n) % 2).astype(np.int32)
    probs = (0.1, 0.9)
    ctx = dry_ctx(n)
    with pytest.raises(NativeError, match=r"rh_bands_zonal_read failed \(-3\)"):
        ctx.bands_zonal_read(0, 0)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone)
    days = [rng.normal(size=n) for _ in range(5)]
    want = np.array([zonal_quantiles_of(x, zone, 2, probs)[0] for x in days])
    for x in days:                                       # capacity 2, five counted days
        ctx.upload(PLANE, x)
        ctx.run_steps(1)
    assert ctx.bands_count() == 5
    with pytest.raises(NativeError, match=r"rh_bands_zonal_read failed \(-1\)") as e:
        ctx.bands_zonal_read(2, 3)
    assert "have been overwritten" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_zonal_read failed \(-1\)") as e:
        ctx.bands_zonal_read(4, 2)
    assert "have not been recorded" in str(e.value)
    hdr, counts, values = ctx.bands_zonal_read(3, 2)      # the ring's wrap
    assert same_bits(values[:, 0], want[3:]) and hdr.tolist() == [[3, 4 * DAY], [4, 5 * DAY]] and (counts[:, 0, :, 1] == 0).all()
    with pytest.raises(NativeError, match=r"rh_bands_read failed \(-3\)") as e:
        ctx.bands_read(3, 2)
    assert "rh_bands_zonal_read" in str(e.value)
    # zonal -> plain -> zonal: each configuration starts a new series
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, zone == 1, 2)
    assert ctx.bands_count() == 0
    ctx.upload(PLANE, days[0])
    ctx.run_steps(1)
    hdr, values = ctx.bands_read(0, 1)
    assert hdr[0].tolist() == [5, 6 * DAY, 128, 0] and same_bits(values[0, 0], want[0, 1])
    with pytest.raises(NativeError, match=r"rh_bands_zonal_read failed \(-3\)") as e:
        ctx.bands_zonal_read(0, 1)
    assert "rh_bands_read" in str(e.value)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, zones=zone)
    assert ctx.bands_count() == 0
    ctx.upload(PLANE, days[1])
    ctx.run_steps(1)
    hdr, counts, values = ctx.bands_zonal_read(0, 1)
    assert hdr.tolist() == [[6, 7 * DAY]] and counts[0, 0].tolist() == [[129, 0], [128, 0]] and same_bits(values[0, 0], want[1])
    # n_items == 0 releases the buffers
    ctx.bands_configure((), zones=zone)
    ctx.run_steps(2)
    for read in (ctx.bands_zonal_read, ctx.bands_read):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            read(0, 0)
    with pytest.raises(NativeError, match=r"rh_bands_count failed \(-3\)"):
        ctx.bands_count()
    ctx.close()


# ---- 8. refusals ----
def test_refusals_leave_the_running_configuration_recording():
    import ctypes as C

    from roger_amd._native import NativeError

    n = 6
    zone = np.array([0, 1, 0, 1, -1, 0], dtype=np.int32)
    ctx = dry_ctx(n)
    ok = dict(names=(PLANE, "q_ss"), kinds=(LAST, SUM), probs=(0.5,), interval=DAY, t_first=0, mask=None, capacity=4, zones=zone, n_zones=2)
    ctx.bands_configure(**ok)
    bad = ((dict(zones=np.array([0, 1, 2, 1, -1, 0])), "zone index 2 of column 2 (n_zones = 2)"), (dict(n_zones=0), "n_zones = 0 (1 ... 1024)"),
           (dict(n_zones=1025), "n_zones = 1025 (1 ... 1024)"), (dict(zones=np.full(n, -1)), "no participating column"),
           (dict(mask=np.array([0, 0, 0, 0, 1, 0])), "no participating column"),
           (dict(probs=(0.5, 1.5)), "probability 1 = 1.5"), (dict(kinds=(LAST, 2)), "kind 2 of item 1"), (dict(capacity=0), "capacity = 0"),
           (dict(interval=7200, t_first=7200), "interval_seconds = 7200"))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_bands_configure_zonal failed \(-1\)") as err:
            ctx.bands_configure(**dict(ok, **kw))
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(ValueError, match="the zone map has 5 values"):
        ctx.bands_configure(**dict(ok, zones=np.zeros(5, dtype=int)))
    ids = (C.c_int * 1)(ctx.index[PLANE])
    kd = (C.c_int * 1)(LAST)
    pr = np.array([0.5])
    rc = ctx._lib.rh_bands_configure_zonal(ctx._h, ids, kd, 1, pr.ctypes.data_as(C.c_void_p), 1, DAY, 0, None, 2, 4)
    assert rc == -1 and "rh_bands_configure_zonal: null pointer" in ctx._lib.rh_last_error(ctx._h).decode()
    x = np.array([3.0, -1.0, 2.0, np.nan, 0.5, 7.0])
    ctx.upload(PLANE, x)
    ctx.run_steps(1)
    hdr, counts, values = ctx.bands_zonal_read(0, 1)      # the configuration from before the refusals recorded the day
    assert hdr.tolist() == [[0, DAY]] and counts[0, 0].tolist() == [[3, 0], [1, 1]] and values[0, 0].tolist() == [[3.0], [-1.0]]
    assert values.shape == (1, 2, 2, 1)
    ctx.close()


# ---- 9. sparse stores ----
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_an_observed_pure_output_is_kept_by_the_sparse_kernel_for_the_zones(nx, ny, monkeypatch):
    """q_ss is a pure output: with the sparse variant on, the KEEP kernel stores it for the zonal observer as for the plain one."""
    zone = three_zones(nx * ny)
    want = zonal_expected(reference(nx, ny), 3600, zone, 3)
    rows = {}
    for sparse in (True, False):
        if not sparse:
            monkeypatch.setenv("RH_NO_SPARSE_STORES", "1")
        ctx, _ = make_ctx(nx, ny, False)
        assert "q_ss" in ctx.pure_output_planes()
        ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, None, NSTEPS, zones=zone)
        ctx.run_steps(NSTEPS)
        assert (ctx.sparse_steps() > 0) == sparse
        rows[sparse] = read_all(ctx)
        ctx.close()
    assert_zonal_rows(rows[True], rows[False], f"{nx} x {ny}: sparse against eager")
    assert_zonal_rows(rows[True], want, f"{nx} x {ny}: sparse against the restatement")
