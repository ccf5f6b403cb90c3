"""GPU: transport bands by age per zone (rh_sas_age_bands_configure_zonal / _zonal_read; k_sas_age_bands_zonal and k_sas_age_bands_small in
roger_amd/csrc/rh_sas_age_bands.h), tolerance zero.

The truth is the ONE rule they promise, tests/sas_age_bands_zonal_reference.py: block (item, zone z, age class a) is what the plain bands by
age record with mask = (zones == z) & mask -- and, for three zones, what the device's own plain configuration records under that mask.  The
pure inputs are the ones tests/test_sas_age_bands_zonal_reference.py shows to have teeth and to meet their conditions.  Without the feature
every test fails at the reference module's import or at the `zones` argument."""
import ctypes as ct

import numpy as np
import pytest

import sas_age_bands_reference as R
import sas_age_bands_zonal_reference as Z
import sas_binding as sb
from test_hip_sas_age_bands import STEP_ITEMS, pure_context
from test_hip_sas_points import daily_inputs, held_names, same_bits
from test_hip_sas_scores import loaded, named, windows_for
from test_hip_sas_scores import step_items as window_items

pytestmark = pytest.mark.gpu


def assert_same_blocks(got, want_rows, want_hdr, where):
    rows, hdr = got[0], got[1]
    assert list(rows) == list(want_rows) == list(hdr), where
    for v in want_rows:
        assert hdr[v].shape == want_hdr[v].shape and (hdr[v] == want_hdr[v]).all(), (where, v, np.argwhere(hdr[v] != want_hdr[v])[:8])
        assert same_bits(rows[v], want_rows[v]), (where, v, np.argwhere(rows[v].view(np.uint64) != np.ascontiguousarray(want_rows[v]).view(np.uint64))[:8])


def record(ctx, values, days):
    for d in range(days):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.age_bands_record(d)
    return ctx.age_bands_read()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_items,n_probs", [(1, 1), (1, 8), (4, 1), (4, 8)])
@pytest.mark.parametrize("ages", [30, 64])
@pytest.mark.parametrize("kind", Z.MAPS)
def test_pure(kind, ages, n_items, n_probs, weighted):
    """1. No day kernel: uploaded arrays and age_bands_record; the windows [0, 0], [1, 2] and one that closes on a day never reached.  The
    maps (sas_age_bands_zonal_reference.zone_map): zones of 0, 1, 63, 64, 65, 255, 256, 257 and 2049 participating columns, contiguous and
    interleaved -- both selections and the boundary between them in one launch set; 1, 3 and 1024 zones over about 2100 columns; short
    zones only and long zones only, where one of the two selections is not launched.  ages 30 / 64 give the widths 31 / 65 of TT_q_ss (the
    one-item case) and 30 / 64 of the others.  With weights: a mask and a weight plane, so that neither the column index nor the plain
    compacted index of a column is its zone-ordered index."""
    want, (n, mask, w, zones, n_zones), values = Z.restate_zonal_pure(kind, ages, weighted)
    items = R.ITEMS4[:n_items]
    ctx = pure_context(n, ages)
    ctx.age_bands_configure(items, R.pure_probs(n_probs), Z.ZONAL_WINDOWS, mask, w, zones=zones, n_zones=n_zones)
    got = record(ctx, [{v: day[v] for v in items} for day in values], Z.ZONAL_DAYS)
    ctx.close()
    wrows, whdr = Z.sliced(want, ages, n_items, n_probs)
    at = [Z.PROBS8.index(p) for p in R.pure_probs(n_probs)]
    if Z.days_of(kind) < Z.ZONAL_DAYS:   # (1024 zones: every zone on the first closing day, the sampled zones on every day)
        for z, (srows, shdr) in Z.restate_sampled(kind, ages, weighted).items():
            for v in items:
                assert same_bits(got[0][v][:, z], srows[v][..., at]) and (got[1][v][:, z] == shdr[v]).all(), (kind, ages, z, v)
        assert got[1][items[0]][1, :, :, 0].any() and got[1][items[0]][1, list(Z.MANY_SAMPLE), :, 0].any()
        got = ({v: got[0][v][[0, 2]] for v in items}, {v: got[1][v][[0, 2]] for v in items}) + got[2:]
        wrows, whdr = {v: wrows[v][[0, 2]] for v in items}, {v: whdr[v][[0, 2]] for v in items}
    assert_same_blocks(got, wrows, whdr, (kind, ages, n_items, n_probs, weighted))
    assert list(got[2]) == [1, 1, 0] and got[3] == Z.ZONAL_DAYS
    assert all(got[0][v].shape[1:] == (n_zones, R.width_of(v, ages), n_probs) for v in items)
    hdr = got[1][items[0]]
    assert hdr[0, :, :, 0].any() and not hdr[0, :, R.NAN_AGE, 0].any() and not hdr[-1].any() and np.isnan(got[0][items[0]][-1]).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_three_zones_are_three_masks_of_the_plain_configuration(weighted):
    """2. The promise on the device itself: a short zone, one of exactly 256 participating columns and a long one, against the context's own
    rh_sas_age_bands_configure run once per zone with mask = (zones == z) & mask."""
    ages, items, probs = 64, R.ITEMS4[:2], R.PROBS8
    (n, mask, w, zones, n_zones), values = Z.make_zonal_pure("three", ages, items, weighted)
    part = (np.ones(n, dtype=bool) if mask is None else mask != 0) & (True if w is None else w > 0)
    sizes = np.bincount(zones[part & (zones >= 0)], minlength=3).tolist()
    assert sizes[0] < Z.SHORT == sizes[1] < sizes[2] and n_zones == 3
    ctx = pure_context(n, ages)
    ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, mask, w, zones=zones)   # (n_zones: the largest index + 1)
    rows, hdr, closed, days = record(ctx, values, Z.ZONAL_DAYS)
    for z in range(3):
        ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, (zones == z) & (True if mask is None else mask != 0), w)
        prows, phdr, pclosed, pdays = record(ctx, values, Z.ZONAL_DAYS)
        for v in items:
            assert same_bits(rows[v][:, z], prows[v]) and (hdr[v][:, z] == phdr[v]).all() and phdr[v][:2, :, 0].any(), (z, v)
        assert list(pclosed) == list(closed) == [1, 1, 0] and pdays == days == Z.ZONAL_DAYS
    ctx.close()


def bound_values(n, ages):
    rng = np.random.default_rng(12)
    A = -12.0 + 9.0 * rng.random((n, ages))
    A[rng.random((n, ages)) < 0.1] = np.nan
    A[:, 0] = -8.5
    A[:, 1] = np.where(np.arange(n) % 2 == 0, -3.0, 4.0)
    return A


def test_the_bound_is_per_zone():
    """3. A uint32 LDS bin holds the weights of ONE zone's age class.  A zone of 65536 participating cells of weight 65535 beside a short zone:
    accepted, W = 4 294 901 760 in one bin; a zone of 65537: refused, the message names the zone and its size, and the configuration that was
    running stays.  Two weighted zones of 40000 cells, 80000 in total: accepted and exact, where the plain call refuses the total.  65537
    unweighted cells in one zone are exact."""
    from roger_amd._native import NativeError

    full, ages = 65536, 30
    n = full + 1 + 40
    A = bound_values(n, ages)
    ctx = pure_context(n, ages)
    ctx.upload("sa_rz", A)
    probs, win = (0.0, 0.25, 0.5, 0.75, 1.0), (np.array([0]), np.array([0]))
    zones = np.ones(n, dtype=np.int32)
    zones[full:] = 0                      # zone 1: 65536 cells; zone 0: the last 41, of which one will move
    w = np.full(n, 65535, dtype=np.uint16)
    ctx.age_bands_configure(["sa_rz"], probs, win, None, w, zones=zones, n_zones=2)
    ctx.age_bands_record(0)
    rows, hdr, closed, _ = ctx.age_bands_read()
    W = full * 65535
    assert W == 4294901760 and hdr["sa_rz"][0, 1, 0].tolist() == [full, 0, W] and hdr["sa_rz"][0, 1, 1].tolist() == [full, 0, W] and list(closed) == [1]
    assert (rows["sa_rz"][0, 1, 0] == -8.5).all() and rows["sa_rz"][0, 1, 1].tolist() == [-3.0, -3.0, -3.0, 4.0, 4.0]
    for z in (0, 1):
        wrows, whdr = R.select_ages(A, zones == z, w, probs)
        assert same_bits(rows["sa_rz"][0, z], wrows) and (hdr["sa_rz"][0, z] == whdr).all(), z
    assert hdr["sa_rz"][0, 0, 0].tolist() == [41, 0, 41 * 65535]
    # one cell more in zone 1: refused by message, and the configuration that was running stays
    zones[full] = 1
    with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure_zonal failed \(-1\)") as e:
        ctx.age_bands_configure(["sa_rz"], probs, win, None, w, zones=zones, n_zones=2)
    assert "zone 1 has 65537 participating cells under a weight plane (at most 65536" in str(e.value) and "uint32 LDS bin" in str(e.value)
    assert ctx.age_bands_read()[1]["sa_rz"][0, 1, 0].tolist() == [full, 0, W]
    # without weights any zone size is exact
    ctx.age_bands_configure(["sa_rz"], probs, win, zones=zones, n_zones=2)
    ctx.age_bands_record(0)
    rows, hdr, _, _ = ctx.age_bands_read()
    for z in (0, 1):
        wrows, whdr = R.select_ages(A, zones == z, np.ones(n, dtype=np.int64), probs)
        assert same_bits(rows["sa_rz"][0, z], wrows) and (hdr["sa_rz"][0, z] == whdr).all(), z
    assert hdr["sa_rz"][0, 1, 0].tolist() == [full + 1, 0, full + 1]
    ctx.close()
    # two weighted zones of 40000: 80000 cells in total, which the plain call refuses
    n, each = 80000, 40000
    A = bound_values(n, ages)
    rng = np.random.default_rng(5)
    w = rng.integers(1, 65536, size=n).astype(np.uint16)
    zones = (np.arange(n) % 2).astype(np.int32)
    ctx = pure_context(n, ages)
    ctx.upload("sa_rz", A)
    with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure failed \(-1\).*80000 participating cells under a weight plane"):
        ctx.age_bands_configure(["sa_rz"], probs, win, None, w)
    ctx.age_bands_configure(["sa_rz"], probs, win, None, w, zones=zones)
    ctx.age_bands_record(0)
    rows, hdr, _, _ = ctx.age_bands_read()
    for z in (0, 1):
        wrows, whdr = R.select_ages(A, zones == z, w, probs)
        assert same_bits(rows["sa_rz"][0, z], wrows) and (hdr["sa_rz"][0, z] == whdr).all() and whdr[0, 0] == each, z
    ctx.close()


def step_zones(n):
    """A zone map over a golden case's columns: three zones in turn, and a -1 among them where there are enough columns."""
    zones = (np.arange(n) % 3).astype(np.int32)
    if n > 2:
        zones[2] = -1
    return zones


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_benchmark_a1000", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """4. The golden cases with which tests/test_hip_sas_totals.py steps tt_q_ss / TT_* / sa_s.  A: bands by age per zone on, run_days(0, N)
    in one call; A2: step(d) day by day.  B: none, step(d) and downloads on the closing days, restated.  A's rows and headers are B's bits
    and A ends in B's state."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    probs, win = (0.05, 0.5, 0.95), windows_for(N)
    mask = np.arange(g.n) % 4 != 1 if g.n > 2 else None
    wts = (np.arange(g.n) % 3 + 1).astype(np.uint16)
    zones = step_zones(g.n)
    ctxB = loaded(st, inputs, N)
    want = Z.HostSasAgeBandsZonal(STEP_ITEMS, probs, win, g.n, zones, 3, mask, wts)
    for d in range(N):
        ctxB.step(d)
        want.add({v: ctxB.download(v) for v in STEP_ITEMS})
    widths = {v: ctxB.shape(v)[1] for v in STEP_ITEMS}
    wrows, whdr = want.result(widths)
    assert want.closed[0] == 1 and all(whdr[v][..., 0].any() for v in STEP_ITEMS)
    for by_step in (False, True):
        A = loaded(st, inputs, N)
        A.age_bands_configure(STEP_ITEMS, probs, win, mask, wts, zones=zones, n_zones=3)
        if by_step:
            for d in range(N):
                A.step(d)
        else:
            A.run_days(0, N)
        got = A.age_bands_read()
        assert_same_blocks(got, wrows, whdr, (case, by_step))
        assert got[3] == want.win.days and list(got[2]) == list(want.closed)
        for name in held_names(A):
            a, b = A.download(name), ctxB.download(name)
            assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
        A.close()
    ctxB.close()


@pytest.mark.parametrize("zonal_bands", [False, True])
def test_beside_points_totals_zonal_totals_scores_and_bands(zonal_bands):
    """5. Bands by age per zone together with points, totals, zonal totals, scores and the plain (or zonal) bands, configured in two
    different orders: each recorder's output is what it records alone, and the bands by age per zone are the restated ones."""
    from test_hip_sas_scores import observations
    from test_hip_sas_totals import step_items as totals_items

    g = sb.SasGolden("sas_stats_a30")
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items, titems = window_items(st), totals_items(st, g.stats)
    win = windows_for(N)
    sobs = observations(len(items), len(win[0]), 6)
    probs = (0.0, 0.5, 1.0)
    zone = (np.arange(g.n) % 2).astype(np.int32)
    wts = (np.arange(g.n) % 3 + 1).astype(np.uint16)
    awin = (np.array([1]), np.array([N - 1]))            # windows of its own: the clocks are independent
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    bkw = dict(zones=zone, n_zones=2) if zonal_bands else {}
    alone_a, alone_r, C, D = (loaded(st, inputs, N) for _ in range(4))
    recorders = {"age": lambda c: c.age_bands_configure(STEP_ITEMS, probs, awin, None, wts, zones=step_zones(g.n), n_zones=3),
                 "bands": lambda c: c.bands_configure(named(items), probs, win, None, wts, **bkw),
                 "scores": lambda c: c.scores_configure(named(items), sobs, win), "points": lambda c: c.points_configure(cells, pnames, capacity=N),
                 "totals": lambda c: c.totals_configure(titems, None, capacity=N), "zonal": lambda c: c.zonal_configure(titems, zone, 2, capacity=N)}
    recorders["age"](alone_a)
    for key in ("bands", "scores", "points", "totals", "zonal"):
        recorders[key](alone_r)
    for ctx, order in ((C, ("age", "bands", "scores", "points", "totals", "zonal")), (D, ("zonal", "totals", "points", "scores", "bands", "age"))):
        for key in order:
            recorders[key](ctx)
    want = Z.HostSasAgeBandsZonal(STEP_ITEMS, probs, awin, g.n, step_zones(g.n), 3, None, wts)
    plain = loaded(st, inputs, N)
    for d in range(N):
        plain.step(d)
        want.add({v: plain.download(v) for v in STEP_ITEMS})
    wrows, whdr = want.result({v: plain.shape(v)[1] for v in STEP_ITEMS})
    plain.close()
    for ctx in (alone_a, alone_r, C, D):
        ctx.run_days(0, N)
    ra = alone_a.age_bands_read()
    assert_same_blocks(ra, wrows, whdr, "alone")
    assert list(ra[2]) == [1] and ra[3] == N and all(ra[1][v][..., 0].any() for v in STEP_ITEMS)
    rb = alone_r.bands_read()
    ms, cs, _ = alone_r.scores_read()
    others = [alone_r.points_read(0, N), alone_r.totals_read(0, N), alone_r.zonal_read(0, N)]
    for ctx in (C, D):
        rows, hdr, closed, days = ctx.age_bands_read()
        assert all(same_bits(rows[v], ra[0][v]) and (hdr[v] == ra[1][v]).all() for v in STEP_ITEMS) and list(closed) == [1] and days == N
        brow, bhdr, bpair, bclosed, bdays = ctx.bands_read()
        assert same_bits(brow, rb[0]) and (bhdr == rb[1]).all() and (bpair == rb[2]).all() and list(bclosed) == list(rb[3]) and bdays == N
        m, c, _ = ctx.scores_read()
        assert same_bits(m, ms) and list(c) == list(cs)
        for (tags, got), (wtags, wvals) in zip((ctx.points_read(0, N), ctx.totals_read(0, N), ctx.zonal_read(0, N)), others):
            assert list(tags) == list(wtags)
            for key, a in got.items():
                for b, wb in zip(*((x.values() if isinstance(x, dict) else [x]) for x in (a, wvals[key]))):
                    assert same_bits(b, wb), key
    C.age_bands_configure([])   # switched off, the others go on
    C.step(N - 1)
    assert C.totals_count()[0] == N + 1 and C.bands_read()[4] == N + 1
    for ctx in (alone_a, alone_r, C, D):
        ctx.close()


def pointer(a):
    return None if a is None else a.ctypes.data_as(ct.c_void_p)


def test_life_cycle():
    """6. plain -> zonal -> plain, reconfigure, release: each configure call replaces the other and starts the count at 0 with an empty
    result; rh_sas_age_bands_read under a zonal configuration and rh_sas_age_bands_zonal_read under a plain one or none are RH_ERR_STATE;
    rh_sas_age_bands_row_elems serves both and counts no zone axis."""
    from roger_amd._native import NativeError

    ages, items = 30, R.ITEMS4[:2]
    (n, mask, w, zones, n_zones), values = Z.make_zonal_pure("short_only", ages, items, True)
    widths = {v: R.width_of(v, ages) for v in items}
    total_w = sum(widths.values())
    ctx = pure_context(n, ages)
    lib, h = ctx._lib, ctx._h
    K = len(Z.ZONAL_WINDOWS[0])
    total = ct.c_int64()

    def raw_reads(nz):
        """(code of rh_sas_age_bands_read, code of rh_sas_age_bands_zonal_read) with buffers sized for nz zones (0: plain)"""
        rows, hdr = np.empty((K, total_w * max(nz, 1), 3)), np.empty((K, total_w * max(nz, 1), 3), dtype=np.int64)
        closed = np.empty(K, dtype=np.uint8)
        args = (pointer(rows), rows.nbytes, pointer(hdr), hdr.nbytes, pointer(closed), closed.nbytes, None)
        return lib.rh_sas_age_bands_read(h, *args), lib.rh_sas_age_bands_zonal_read(h, *args)

    assert raw_reads(0) == (-3, -3) and b"rh_sas_age_bands_zonal_read: rh_sas_age_bands_configure_zonal has not been called" in lib.rh_sas_last_error(h)
    probs = R.pure_probs(8)[:3]
    plain_want = R.HostSasAgeBands(items, probs, Z.ZONAL_WINDOWS, n, mask, w)
    zonal_want = Z.HostSasAgeBandsZonal(items, probs, Z.ZONAL_WINDOWS, n, zones, n_zones, mask, w)
    for d in range(Z.ZONAL_DAYS):
        plain_want.add(values[d])
        zonal_want.add(values[d])
    for turn in ("plain", "zonal", "zonal", "plain"):
        if turn == "plain":
            ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, mask, w)
            assert raw_reads(0) == (0, -3) and b"rh_sas_age_bands_zonal_read: rh_sas_age_bands_configure_zonal has not been called" in lib.rh_sas_last_error(h)
        else:
            ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, mask, w, zones=zones, n_zones=n_zones)
            assert raw_reads(n_zones) == (-3, 0)
            assert lib.rh_sas_age_bands_read(h, None, 0, None, 0, None, 0, None) == -3
            assert b"rh_sas_age_bands_read: the bands by age are configured per zone (read them with rh_sas_age_bands_zonal_read)" in lib.rh_sas_last_error(h)
        assert lib.rh_sas_age_bands_row_elems(h, ct.byref(total)) == 0 and total.value == total_w
        rows, hdr, closed, days = ctx.age_bands_read()   # a fresh configuration: nothing recorded
        assert days == 0 and not closed.any() and all(np.isnan(rows[v]).all() and not hdr[v].any() for v in items)
        got = record(ctx, values, Z.ZONAL_DAYS)
        if turn == "plain":
            assert_same_blocks(got, *plain_want.result(widths), turn)
        else:
            assert_same_blocks(got, *zonal_want.result(widths), turn)
        assert list(got[2]) == [1, 1, 0] and got[3] == Z.ZONAL_DAYS
    ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, mask, w, zones=zones, n_zones=n_zones)
    assert lib.rh_sas_age_bands_configure_zonal(h, None, 0, None, 0, None, 0, None, None, None, None, 0) == 0   # n_items == 0 releases
    assert raw_reads(n_zones) == (-3, -3)
    with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_age_bands_configure has not been called"):
        ctx.age_bands_record()
    ctx.age_bands_configure(items, probs, Z.ZONAL_WINDOWS, mask, w, zones=zones, n_zones=n_zones)
    ctx.age_bands_configure([])   # ... and so does the plain call
    assert raw_reads(n_zones) == (-3, -3)
    ctx.close()


def test_refusals_leave_the_running_configuration():
    """7. Every refusal by code and message -- what the plain call refuses, under the zonal call's name, and the zonal call's own -- and the
    configuration that was running goes on afterwards."""
    from roger_amd._native import NativeError

    ages, items = 30, R.ITEMS4[:2]
    (n, mask, w, zones, n_zones), values = Z.make_zonal_pure("short_only", ages, items, True)
    widths = {v: R.width_of(v, ages) for v in items}
    ctx = pure_context(n, ages)
    probs = R.pure_probs(8)[:3]
    good = dict(items=list(items), probs=probs, windows=Z.ZONAL_WINDOWS, mask=mask, weights=w, zones=zones, n_zones=n_zones)
    ctx.age_bands_configure(**good)
    want = Z.HostSasAgeBandsZonal(items, probs, Z.ZONAL_WINDOWS, n, zones, n_zones, mask, w)
    for v, a in values[0].items():
        ctx.upload(v, a)
    ctx.age_bands_record(0)
    want.add(values[0])
    last = lambda v: [(v, None, "last")]   # noqa: E731
    low, high = zones.copy(), zones.copy()
    low[7], high[9] = -2, n_zones
    nowhere = np.full(n, -1, dtype=np.int32)
    bad = ((dict(items=last("maskCatch")), "array maskCatch is int32"),
           (dict(items=last("q_ss")), "array q_ss is a daily input"),
           (dict(items=last("sas_params_q_ss")), "array sas_params_q_ss is a parameter block"),
           (dict(items=last("C_rz")), "array C_rz has width 1 (it belongs to rh_sas_bands_configure)"),
           (dict(items=[("sa_rz", "q_ss", "bulk")]), "array sa_rz is BULK (only LAST is built"),
           (dict(items=[("sa_rz", None, "mean")]), "array sa_rz is MEAN (only LAST is built"),
           (dict(items=[("sa_rz", "q_ss", "last")]), "array sa_rz has the weight id"),
           (dict(items=[("sa_rz", None, 3)]), "kind 3 of array sa_rz"),
           (dict(items=["sa_rz", "sa_rz"]), "array sa_rz is given twice"),
           (dict(items=["sa_rz", "sa_ss", "msa_rz", "msa_ss", "sa_s"]), "n_items = 5 (0 ... 4)"),
           (dict(probs=tuple(np.linspace(0, 1, 9))), "n_probs = 9 (1 ... 8)"),
           (dict(probs=()), "n_probs = 0 (1 ... 8)"),
           (dict(probs=(0.5, 1.5)), "probability 1 is 1.5"),
           (dict(probs=(np.nan,)), "probability 0 is nan"),
           (dict(mask=np.zeros(n, dtype=np.uint8)), "no cell takes part (0 of %d cells" % n),
           (dict(weights=np.zeros(n, dtype=np.uint16)), "no cell takes part"),
           (dict(zones=nowhere), "no cell takes part"),
           (dict(windows=(np.array([0, 2, 4]), np.array([2, 3, 5]))), "window 1 starts on day 2, window 0 ends on day 2"),
           (dict(windows=(np.array([0, 3, 4]), np.array([0, 2, 5]))), "window 1 is [3, 2]: its last day lies before its first"),
           (dict(n_zones=0), "n_zones = 0 (1 ... 1024)"),
           (dict(n_zones=1025), "n_zones = 1025 (1 ... 1024)"),
           (dict(zones=low), "zone[7] = -2 (-1: outside every zone, else 0 ... %d)" % (n_zones - 1)),
           (dict(zones=high), "zone[9] = %d (-1: outside every zone, else 0 ... %d)" % (n_zones, n_zones - 1)),
           (dict(n_zones=n_zones - 1), "(-1: outside every zone, else 0 ... %d)" % (n_zones - 2)))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure_zonal failed \(-1\)") as e:
            ctx.age_bands_configure(**dict(good, **kw))
        assert "rh_sas_age_bands_configure_zonal: " in str(e.value) and text in str(e.value), (text, str(e.value))
    lib, h = ctx._lib, ctx._h
    item = np.array([[ctx.index("sa_rz"), -1, 2]], dtype=np.int32)
    pr, days, zn = np.array([0.5]), np.array([0, 2], dtype=np.int64), np.ascontiguousarray(zones)
    p = pointer
    for args in ((None, 1, p(pr), 1, p(zn), n_zones, None, None, p(days), p(days), 2), (p(item), 1, None, 1, p(zn), n_zones, None, None, p(days), p(days), 2),
                 (p(item), 1, p(pr), 1, None, n_zones, None, None, p(days), p(days), 2), (p(item), 1, p(pr), 1, p(zn), n_zones, None, None, None, p(days), 2),
                 (p(item), 1, p(pr), 1, p(zn), n_zones, None, None, p(days), None, 2)):
        assert lib.rh_sas_age_bands_configure_zonal(h, *args) == -1 and b"rh_sas_age_bands_configure_zonal: null pointer" in lib.rh_sas_last_error(h)
    assert lib.rh_sas_age_bands_configure_zonal(h, p(item), 1, p(pr), 1, p(zn), n_zones, None, None, p(days), p(days), 0) == -1
    assert b"n_samples = 0" in lib.rh_sas_last_error(h)
    # rows or headers beyond 2 GiB: 30 age classes x 1024 zones x 24 B of header x 2^12 windows is 3 GiB (the plain call takes 2^12 windows)
    assert lib.rh_sas_age_bands_configure_zonal(h, p(item), 1, p(pr), 1, p(zn), 1024, None, None, p(days), p(days), 1 << 12) == -1
    assert (b"n_samples = 4096 (at least one; rows of 1024 zones x 30 age classes x 1 float64 and headers of 3 int64, each within 2 GiB)"
            in lib.rh_sas_last_error(h))
    rows = np.empty((3, sum(widths.values()) * n_zones, 2))
    hdr, closed = np.empty((3, sum(widths.values()) * n_zones, 3), dtype=np.int64), np.empty(3, dtype=np.uint8)
    assert lib.rh_sas_age_bands_zonal_read(h, p(rows), rows.nbytes, p(hdr), hdr.nbytes, p(closed), closed.nbytes, None) == -1
    assert b"rh_sas_age_bands_zonal_read: size mismatch (n_samples x n_zones x ages_total x n_probs float64" in lib.rh_sas_last_error(h)
    with pytest.raises(ValueError, match="age_bands_configure: zones of dtype float64"):
        ctx.age_bands_configure(**dict(good, zones=zones.astype(np.float64)))
    with pytest.raises(ValueError, match="age_bands_configure"):
        ctx.age_bands_configure(**dict(good, zones=zones[:-1]))
    # the configuration that was running goes on
    for d in range(1, Z.ZONAL_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.age_bands_record(d)
        want.add(values[d])
    got = ctx.age_bands_read()
    assert_same_blocks(got, *want.result(widths), "after the refusals")
    assert list(got[2]) == [1, 1, 0] and got[3] == Z.ZONAL_DAYS
    ctx.close()
