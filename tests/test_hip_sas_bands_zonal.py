"""GPU: transport bands per zone (rh_sas_bands_configure_zonal, rh_sas_bands_zonal_read; k_sas_bands_zonal and k_sas_bands_obs_zonal in
roger_amd/csrc/rh_sas_bands_zonal.h), tolerance zero.

The truth is the ONE rule they promise, tests/sas_bands_zonal_reference.py: block (item, zone z) is what tests/sas_bands_reference.py
records with mask = (zone == z) & mask and obs[:, z] -- and, for a 3-zone case, what the device's own plain configuration records when it
is run once per zone with the zone as its mask.  The pure inputs are the ones tests/test_sas_bands_zonal_reference.py shows to have teeth
and to meet their conditions."""
import numpy as np
import pytest

import sas_binding as sb
import sas_bands_reference as B
import sas_bands_zonal_reference as Z
from test_hip_sas_points import daily_inputs, held_names, same_bits
from test_hip_sas_scores import loaded, named, step_items, windows_for

pytestmark = pytest.mark.gpu


def assert_same_result(got, want, where):
    rows, hdr, pairs, closed, days = got
    assert days == want.win.days and list(closed) == list(want.closed), where
    assert hdr.shape == want.hdr.shape and (hdr == want.hdr).all(), (where, np.argwhere(hdr != want.hdr)[:8])
    assert same_bits(rows, want.rows), (where, np.argwhere(rows.view(np.uint64) != np.ascontiguousarray(want.rows).view(np.uint64))[:8])
    assert (pairs == want.pairs).all(), (where, np.argwhere(pairs != want.pairs)[:8])


def record_pure(ctx, values):
    for d in range(B.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
    return ctx.bands_read()


def run_pure(case, n_items, n_probs, weighted, observed=True):
    from roger_amd._native import SasContext

    n, zone, nz = case
    items = B.ITEMS8[:n_items]
    want, (values, weights, mask, w, obs) = Z.restate_zonal(n, zone, nz, items, n_probs, weighted, observed)
    ctx = SasContext(n, 30, forcing_days=3)
    for wn, a in weights.items():
        ctx.upload(wn, a)
    ctx.bands_configure(named(items), B.pure_probs(n_probs), B.PURE_WINDOWS, mask, w, obs, zones=zone, n_zones=nz)
    got = record_pure(ctx, values)
    assert_same_result(got, want, (n, nz, n_items, n_probs, weighted))
    assert got[0].shape == (4, n_items, nz, n_probs) and list(got[3]) == [1, 1, 1, 0] and got[1][:3, :, :, 0].any()
    return ctx, got, (items, values, weights, mask, w, obs)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_items,n_probs", [(1, 1), (1, 8), (8, 1), (8, 8)])
def test_pure_contiguous_zone_sizes(n_items, n_probs, weighted):
    """1. No day kernel: uploaded values, bands_record over the seven pure days.  Nine contiguous zones of 0, 1, 63, 64, 65, 255, 256, 257
    and 2049 participating columns (wavefront and tile boundaries, and one past the 256 x 8 columns of a trip of the in-flight loop),
    columns outside every zone; with weights, columns with mask == 0 and weight 0 inside the zones; observations below, above, on a member
    and missing, per zone."""
    ctx, got, _ = run_pure(Z.contiguous_case(weighted), n_items, n_probs, weighted)
    ctx.close()
    rows, hdr, pairs = got[:3]
    assert np.isnan(rows[:3, :, 0]).all() and not hdr[:3, :, 0].any() and (pairs[:3] == 0).any() and (pairs[:3] == -1).any()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_zones,n_items,n_probs", [(1, 1, 8), (1, 8, 8), (3, 1, 1), (3, 8, 8), (1024, 1, 8), (1024, 8, 1)])
def test_pure_interleaved_zones(n_zones, n_items, n_probs, weighted):
    """2. zone = i % n_zones: the list position of a column is not its index.  One zone of 2049 columns, three of 257, 1024 zones of two
    columns and one (the largest grid)."""
    ctx, _, _ = run_pure(Z.interleaved_case(n_zones), n_items, n_probs, weighted)
    ctx.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_three_zones_are_three_masks_of_the_plain_configuration(weighted):
    """3. The promise on the device itself: 3 interleaved zones, 8 items, 8 probabilities; the plain configuration (k_sas_bands_hist /
    _pick, k_sas_bands_obs) run once per zone with mask = (zone == z) & mask, the same weights and obs[:, z] records block z, bit for
    bit.  Without observations nothing is counted: the pairs stay (-1, -1)."""
    n, zone, nz = case = Z.interleaved_case(3)
    ctx, (rows, hdr, pairs, closed, days), (items, values, weights, mask, w, obs) = run_pure(case, 8, 8, weighted)
    for z in range(nz):
        mz = (zone == z) & (np.ones(n, dtype=bool) if mask is None else mask != 0)
        ctx.bands_configure(named(items), B.pure_probs(8), B.PURE_WINDOWS, mz, w, obs[:, z])
        prow, phdr, ppair, pclosed, pdays = record_pure(ctx, values)
        assert same_bits(rows[:, :, z], prow) and (hdr[:, :, z] == phdr).all() and (pairs[:, :, z] == ppair).all(), z
        assert list(pclosed) == list(closed) and pdays == days
    ctx.close()
    ctx, got, _ = run_pure(case, 8, 8, weighted, observed=False)
    ctx.close()
    assert (got[2] == -1).all() and same_bits(got[0], rows) and (got[1] == hdr).all()


def test_the_bound_of_a_weighted_zone():
    """4. A uint32 LDS bin holds a zone's weights up to 65536 columns x 65535: one weighted zone of exactly 65536 participating columns, all
    of weight 65535 and of one value, fills one bin with 4 294 901 760 < 2^32 -- accepted, W = 65536 x 65535, beyond 2^31.  A second item
    holds two values, so that a cumulative sum passes 2^31 between two bins.  65537 participating columns are refused by name; the same
    zone without weights is accepted."""
    from roger_amd._native import NativeError, SasContext

    n, full = 65537, 65536
    ctx = SasContext(n, 2)
    ctx.upload("C_rz", np.full(n, -8.5))
    ctx.upload("C_s", np.where(np.arange(n) % 2 == 0, -3.0, 4.0))
    items = [("C_rz", None, "last"), ("C_s", None, "last")]
    probs, win, zone = (0.0, 0.25, 0.5, 0.75, 1.0), (np.array([0]), np.array([0])), np.zeros(n, dtype=np.int32)
    w = np.full(n, 65535, dtype=np.uint16)
    w[-1] = 0
    obs = np.array([[[-8.5]], [[4.0]]])
    ctx.bands_configure(items, probs, win, None, w, obs, zones=zone, n_zones=1)
    ctx.bands_record(0)
    rows, hdr, pairs, closed, _ = ctx.bands_read()
    W = full * 65535
    assert W == 4294901760 and hdr[0, :, 0].tolist() == [[full, 0, W]] * 2 and list(closed) == [1]
    assert (rows[0, 0, 0] == -8.5).all() and rows[0, 1, 0].tolist() == [-3.0, -3.0, -3.0, 4.0, 4.0]
    assert pairs[0, :, 0].tolist() == [[0, W], [W // 2, W // 2]]
    # one column more: refused, and the configuration that was running stays
    w[-1] = 65535
    with pytest.raises(NativeError, match=r"rh_sas_bands_configure_zonal failed \(-1\)") as e:
        ctx.bands_configure(items, probs, win, None, w, obs, zones=zone, n_zones=1)
    assert "zone 0 has 65537 participating cells" in str(e.value) and "at most 65536" in str(e.value) and "mask of rh_sas_bands_configure" in str(e.value)
    assert ctx.bands_read()[1][0, 0, 0].tolist() == [full, 0, W]
    # ... but a mask takes it back to the bound, and without weights any size goes
    ctx.bands_configure(items, probs, win, np.arange(n) != 7, w, obs, zones=zone, n_zones=1)
    ctx.bands_configure(items, probs, win, None, None, obs, zones=zone, n_zones=1)
    ctx.bands_record(0)
    rows, hdr, pairs, _, _ = ctx.bands_read()
    assert hdr[0, :, 0].tolist() == [[n, 0, n]] * 2 and rows[0, 1, 0].tolist() == [-3.0, -3.0, -3.0, 4.0, 4.0] and pairs[0, 1, 0].tolist() == [n // 2 + 1, n // 2]
    ctx.close()


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """5. A: zonal bands on (zone = i % 2), run_days(0, N) in one call; A2: step(d) day by day.  B: no bands, step(d) and downloads per
    day, restated per zone.  A's rows, headers and pairs are B's bits and A ends in B's state."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items, probs, win = step_items(st), (0.05, 0.5, 0.95), windows_for(N)
    zone = (np.arange(g.n) % 2).astype(np.int32)
    obs = -9.0 + 3.0 * np.random.default_rng(5).random((len(items), 2, len(win[0])))
    obs[1, 0, 0] = np.nan
    ctxB = loaded(st, inputs, N)
    want = Z.HostSasBandsZonal(items, probs, win, g.n, zone, 2, None, None, obs)
    for d in range(N):
        ctxB.step(d)
        want.add({v: ctxB.download(v) for v in {it[0] for it in items}}, {"q_ss": inputs["q_ss"][d]})
    assert want.closed[0] == 1 and all(want.hdr[:, j, z, 0].any() for j in range(3) for z in range(2))   # not vacuous
    assert not same_bits(want.rows[:, :, 0], want.rows[:, :, 1])                                            # the zones differ
    for by_step in (False, True):
        A = loaded(st, inputs, N)
        A.bands_configure(named(items), probs, win, obs=obs, zones=zone)
        if by_step:
            for d in range(N):
                A.step(d)
        else:
            A.run_days(0, N)
        assert_same_result(A.bands_read(), want, (case, by_step))
        for name in held_names(A):
            a, b = A.download(name), ctxB.download(name)
            assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
        A.close()
    ctxB.close()


def test_beside_points_totals_zonal_totals_and_scores():
    """6. Zonal bands together with points, totals, zonal totals and scores, configured in two different orders: each recorder's output
    is what it records alone."""
    from test_hip_sas_scores import observations
    from test_hip_sas_totals import step_items as totals_items

    g = sb.SasGolden("sas_stats_a30")
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items, titems = step_items(st), totals_items(st, g.stats)
    win = windows_for(N)
    sobs = observations(len(items), len(win[0]), 6)
    probs, bobs = (0.0, 0.5, 1.0), np.repeat(sobs[:, 0:1, :], 3, axis=1) + np.array([0.0, 0.5, -0.5])[None, :, None]
    zone = (np.arange(g.n) % 2).astype(np.int32)
    bzone = (np.arange(g.n) % 4 - 1).astype(np.int32)      # three zones and columns outside them
    wts = (np.arange(g.n) % 3 + 1).astype(np.uint16)
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    alone_b, alone_r, C, D = (loaded(st, inputs, N) for _ in range(4))
    recorders = {"bands": lambda c: c.bands_configure(named(items), probs, win, None, wts, bobs, zones=bzone, n_zones=3),
                 "scores": lambda c: c.scores_configure(named(items), sobs, win), "points": lambda c: c.points_configure(cells, pnames, capacity=N),
                 "totals": lambda c: c.totals_configure(titems, None, capacity=N), "zonal": lambda c: c.zonal_configure(titems, zone, 2, capacity=N)}
    recorders["bands"](alone_b)
    for key in ("scores", "points", "totals", "zonal"):
        recorders[key](alone_r)
    for ctx, order in ((C, ("bands", "scores", "points", "totals", "zonal")), (D, ("zonal", "totals", "points", "scores", "bands"))):
        for key in order:
            recorders[key](ctx)
    for ctx in (alone_b, alone_r, C, D):
        ctx.run_days(0, N)
    rb = alone_b.bands_read()
    assert rb[0].shape == (len(win[0]), len(items), 3, 3) and rb[1][..., 0].any() and (rb[1][..., 2] != rb[1][..., 0]).any() and (rb[2] >= 0).any()
    ms, cs, _ = alone_r.scores_read()
    want = [alone_r.points_read(0, N), alone_r.totals_read(0, N), alone_r.zonal_read(0, N)]
    for ctx in (C, D):
        rows, hdr, pairs, closed, days = ctx.bands_read()
        assert same_bits(rows, rb[0]) and (hdr == rb[1]).all() and (pairs == rb[2]).all() and list(closed) == list(rb[3]) and days == N
        m, c, _ = ctx.scores_read()
        assert same_bits(m, ms) and list(c) == list(cs)
        for (tags, got), (wtags, wrows) in zip((ctx.points_read(0, N), ctx.totals_read(0, N), ctx.zonal_read(0, N)), want):
            assert list(tags) == list(wtags)
            for key, a in got.items():
                for b, wb in zip(*((x.values() if isinstance(x, dict) else [x]) for x in (a, wrows[key]))):
                    assert same_bits(b, wb), key
    # switched off, the others go on
    C.bands_configure([])
    C.step(N - 1)
    assert C.totals_count()[0] == N + 1
    for ctx in (alone_b, alone_r, C, D):
        ctx.close()


def test_reconfigure_release_and_refusals():
    """7. Plain -> zonal -> plain on one context: each configure starts anew, and the plain rows afterwards are a fresh context's.  The
    plain read is RH_ERR_STATE under a zonal configuration and the zonal read under a plain one or none; no items release everything;
    the argument errors name the offender and leave the configuration that was running."""
    import ctypes as ct

    from roger_amd._native import NativeError, SasContext

    n, zone, nz = Z.interleaved_case(3)
    items = B.ITEMS8[:3]
    values, weights, obs = B.make_pure(n, items)
    zobs = Z.zonal_obs(items, values, zone, nz, zone >= 0)
    plain = dict(items=named(items), probs=(0.05, 0.5, 0.95), windows=B.PURE_WINDOWS, obs=obs)
    zonal = dict(plain, obs=zobs, zones=zone, n_zones=nz)

    def fresh():
        c = SasContext(n, 30, forcing_days=3)
        for wn, a in weights.items():
            c.upload(wn, a)
        return c

    def zonal_read_raw(c, shape):
        rows, hdr, pairs, closed = np.empty(shape + (3,)), np.empty(shape + (3,), dtype=np.int64), np.empty(shape + (2,), dtype=np.int64), np.empty(shape[0], dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(ct.c_void_p)   # noqa: E731
        rc = c._lib.rh_sas_bands_zonal_read(c._h, p(rows), rows.nbytes, p(hdr), hdr.nbytes, p(pairs), pairs.nbytes, p(closed), closed.nbytes, None)
        return rc, c._lib.rh_sas_last_error(c._h).decode()

    ref = fresh()
    ref.bands_configure(**plain)
    want_plain = record_pure(ref, values)
    ref.close()
    ctx = fresh()
    assert zonal_read_raw(ctx, (4, 3, 3)) == (-3, "rh_sas_bands_zonal_read: rh_sas_bands_configure_zonal has not been called")
    ctx.bands_configure(**plain)
    got = record_pure(ctx, values)
    assert all(same_bits(a, b) if a.dtype.kind == "f" else (a == b).all() for a, b in zip(got[:4], want_plain[:4]))
    rc, text = zonal_read_raw(ctx, (4, 3, 3))          # a plain configuration is on: the zonal read refuses
    assert rc == -3 and "rh_sas_bands_configure_zonal has not been called" in text
    ctx.bands_configure(**zonal)
    want = Z.HostSasBandsZonal(items, zonal["probs"], B.PURE_WINDOWS, n, zone, nz, None, None, zobs)
    rows, hdr, pairs, closed, days = ctx.bands_read()   # anew: nothing recorded
    assert rows.shape == (4, 3, 3, 3) and np.isnan(rows).all() and not hdr.any() and (pairs == -1).all() and not closed.any() and days == 0
    plain_read = np.empty((4, 3, 3)), np.empty((4, 3, 3), dtype=np.int64), np.empty((4, 3, 2), dtype=np.int64), np.empty(4, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ct.c_void_p)   # noqa: E731
    rc = ctx._lib.rh_sas_bands_read(ctx._h, *(x for a in plain_read for x in (p(a), a.nbytes)), None)
    assert rc == -3 and "rh_sas_bands_read: the bands are configured per zone (read them with rh_sas_bands_zonal_read)" == ctx._lib.rh_sas_last_error(ctx._h).decode()
    for d in range(3):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
        want.add(values[d], {wn: a[d % 3] for wn, a in weights.items()})
    bad_zone, low_zone = zone.copy(), zone.copy()
    bad_zone[5], low_zone[9] = nz, -2
    bad = ((dict(zones=bad_zone), "zone[5] = 3 (-1: outside every zone, else 0 ... 2)"),
           (dict(zones=low_zone), "zone[9] = -2 (-1: outside every zone, else 0 ... 2)"),
           (dict(n_zones=0, obs=None), "n_zones = 0 (1 ... 1024)"),
           (dict(n_zones=1025, obs=None), "n_zones = 1025 (1 ... 1024)"),
           (dict(zones=np.full(n, -1, dtype=np.int32)), "no cell takes part"),
           (dict(probs=(0.5, 1.5)), "probability 1 is 1.5"),
           (dict(windows=(np.array([0, 3, 4, 6]), np.array([0, 2, 5, 9]))), "window 1 is [3, 2]: its last day lies before its first"))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_sas_bands_configure_zonal failed \(-1\)") as e:
            ctx.bands_configure(**dict(zonal, **kw))
        assert "rh_sas_bands_configure_zonal: " + text in str(e.value), (text, str(e.value))
    item = np.array([[ctx.index("C_rz"), -1, 2]], dtype=np.int32)
    pr, days2 = np.array([0.5]), np.array([0, 2], dtype=np.int64)
    assert ctx._lib.rh_sas_bands_configure_zonal(ctx._h, p(item), 1, p(pr), 1, None, 3, None, None, None, p(days2), p(days2), 2) == -1
    assert b"rh_sas_bands_configure_zonal: null pointer" in ctx._lib.rh_sas_last_error(ctx._h)
    assert ctx._lib.rh_sas_bands_configure_zonal(ctx._h, p(item), 1, p(pr), 1, p(zone), 1024, None, None, None, p(days2), p(days2), 1 << 19) == -1
    assert b"n_samples = 524288 (at least one; rows of 1 x 1024 x 1 float64 within 2 GiB)" in ctx._lib.rh_sas_last_error(ctx._h)
    # the zonal configuration that was running goes on
    for d in range(3, B.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
        want.add(values[d], {wn: a[d % 3] for wn, a in weights.items()})
    assert_same_result(ctx.bands_read(), want, "after the refusals")
    # back to plain: a fresh context's bits
    ctx.bands_configure(**plain)
    got = record_pure(ctx, values)
    assert got[0].shape == (4, 3, 3) and got[4] == want_plain[4]
    assert all(same_bits(a, b) if a.dtype.kind == "f" else (a == b).all() for a, b in zip(got[:4], want_plain[:4]))
    # release through either entry point
    ctx.bands_configure(**zonal)
    ctx.bands_configure([])
    for call in (ctx.bands_read, ctx.bands_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_bands_configure has not been called"):
            call()
    assert zonal_read_raw(ctx, (4, 3, 3))[0] == -3
    ctx.bands_configure(**zonal)
    assert ctx._lib.rh_sas_bands_configure_zonal(ctx._h, None, 0, None, 0, None, 0, None, None, None, None, None, 0) == 0
    with pytest.raises(NativeError, match=r"failed \(-3\)"):
        ctx.bands_record()
    ctx.close()
