"""GPU: transport bands by age (rh_sas_age_bands_*; k_sas_age_keys and k_sas_age_bands in roger_amd/csrc/rh_sas_age_bands.h,
select_walk_run and select_lds_block in rh_select.h), tolerance zero.

The truth is the ONE rule they promise, tests/sas_age_bands_reference.py: block (item, age class a) is what tests/sas_bands_reference.py
selects from the width-1 values A[:, a] with kind LAST -- and, for three age classes, what the device's own plain bands record for a copy
of A[:, a].  The pure inputs are the ones tests/test_sas_age_bands_reference.py shows to have teeth and to meet their conditions.  Without
the feature every test fails at age_bands_configure."""
import ctypes as ct

import numpy as np
import pytest

import sas_age_bands_reference as R
import sas_binding as sb
from test_hip_sas_points import daily_inputs, held_names, same_bits
from test_hip_sas_scores import loaded, named, windows_for
from test_hip_sas_scores import step_items as window_items

pytestmark = pytest.mark.gpu


def assert_same_result(got, want, widths, where):
    rows, hdr, closed, days = got
    wrows, whdr = want.result(widths)
    assert days == want.win.days and list(closed) == list(want.closed), where
    assert list(rows) == list(want.items) == list(hdr), where
    for v in want.items:
        assert hdr[v].shape == whdr[v].shape and (hdr[v] == whdr[v]).all(), (where, v, np.argwhere(hdr[v] != whdr[v])[:8])
        assert same_bits(rows[v], wrows[v]), (where, v, np.argwhere(rows[v].view(np.uint64) != np.ascontiguousarray(wrows[v]).view(np.uint64))[:8])


def pure_context(n, ages):
    from roger_amd._native import SasContext

    return SasContext(n, ages, keep_distributions=True)


def record_pure(ctx, values):
    for d in range(R.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.age_bands_record(d)
    return ctx.age_bands_read()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_items,n_probs", [(1, 1), (1, 8), (4, 1), (4, 8)])
@pytest.mark.parametrize("ages", [30, 63, 64])
@pytest.mark.parametrize("n_part", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_pure(n_part, ages, n_items, n_probs, weighted):
    """1. No day kernel: uploaded arrays and age_bands_record over the seven pure days; the windows [0, 0], [1, 2], a gap day, [4, 5] and
    one that closes on a day never reached.  n_part: wavefront and tile boundaries of the walk, the edge of the transpose's 64-column
    tile, and 2049 = one past the 256 x 8 keys of a trip of the in-flight loop.  ages 30 / 63 / 64 (rh_sas_create accepts all three) give
    the widths 31, 64 and 65 of TT_q_ss (the one-item case) and 30, 63 and 64 of sa_rz, tt_q_ss and sa_s: below, at and one past the
    tile's age edge.  With weights: a mask and a weight plane, so the compacted index of a column is not its index."""
    items = R.ITEMS4[:n_items]
    want, (n, mask, w, values) = R.restate_age_pure(n_part, ages, items, n_probs, weighted)
    ctx = pure_context(n, ages)
    ctx.age_bands_configure(items, R.pure_probs(n_probs), R.PURE_WINDOWS, mask, w)
    got = record_pure(ctx, values)
    ctx.close()
    widths = {v: R.width_of(v, ages) for v in items}
    assert_same_result(got, want, widths, (n_part, ages, n_items, n_probs, weighted))
    assert list(got[2]) == [1, 1, 1, 0] and all(got[0][v].shape == (4, widths[v], n_probs) for v in items)
    hdr = got[1][items[0]]
    assert hdr[:3, :, 0].any() and not hdr[:3, R.NAN_AGE, 0].any() and (hdr[:3, R.NAN_AGE, 1] == n_part).all()


def test_the_bound_of_a_weight_plane():
    """2. A uint32 LDS bin holds an age class's weights up to 65536 cells x 65535.  ages = 30: 65536 participating cells, all of weight
    65535 -- accepted; age class 0 holds one value, so one bin takes W = 4 294 901 760 < 2^32; age class 1 two values, so a cumulative sum
    passes 2^31 between two bins; the other age classes random values with NaN.  65537 weighted cells are refused by message and the
    configuration that was running stays; 65537 unweighted cells are accepted and exact."""
    from roger_amd._native import NativeError

    n, full, ages = 65537, 65536, 30
    rng = np.random.default_rng(12)
    A = -12.0 + 9.0 * rng.random((n, ages))
    A[rng.random((n, ages)) < 0.1] = np.nan
    A[:, 0] = -8.5
    A[:, 1] = np.where(np.arange(n) % 2 == 0, -3.0, 4.0)
    ctx = pure_context(n, ages)
    ctx.upload("sa_rz", A)
    probs, win = (0.0, 0.25, 0.5, 0.75, 1.0), (np.array([0]), np.array([0]))
    w = np.full(n, 65535, dtype=np.uint16)
    w[-1] = 0
    ctx.age_bands_configure(["sa_rz"], probs, win, None, w)
    ctx.age_bands_record(0)
    rows, hdr, closed, _ = ctx.age_bands_read()
    W = full * 65535
    assert W == 4294901760 and hdr["sa_rz"][0, 0].tolist() == [full, 0, W] and hdr["sa_rz"][0, 1].tolist() == [full, 0, W] and list(closed) == [1]
    assert (rows["sa_rz"][0, 0] == -8.5).all() and rows["sa_rz"][0, 1].tolist() == [-3.0, -3.0, -3.0, 4.0, 4.0]
    wrows, whdr = R.select_ages(A, w > 0, w, probs)
    assert same_bits(rows["sa_rz"][0], wrows) and (hdr["sa_rz"][0] == whdr).all() and whdr[2:, 1].all()
    # one cell more: refused, and the configuration that was running stays
    w[-1] = 65535
    with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure failed \(-1\)") as e:
        ctx.age_bands_configure(["sa_rz"], probs, win, None, w)
    assert "65537 participating cells under a weight plane (at most 65536" in str(e.value) and "uint32 LDS bin" in str(e.value)
    assert ctx.age_bands_read()[1]["sa_rz"][0, 0].tolist() == [full, 0, W]
    # ... but a mask takes it back to the bound, and without weights any size goes
    ctx.age_bands_configure(["sa_rz"], probs, win, np.arange(n) != 7, w)
    ctx.age_bands_configure(["sa_rz"], probs, win)
    ctx.age_bands_record(0)
    rows, hdr, _, _ = ctx.age_bands_read()
    wrows, whdr = R.select_ages(A, np.ones(n, dtype=bool), np.ones(n, dtype=np.int64), probs)
    assert hdr["sa_rz"][0, 0].tolist() == [n, 0, n] and same_bits(rows["sa_rz"][0], wrows) and (hdr["sa_rz"][0] == whdr).all()
    ctx.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_three_age_classes_are_three_width_one_arrays_of_the_plain_bands(weighted):
    """3. The promise on the device itself: for the first, the tie and the last age class of TT_q_ss (width 65), A[:, a] copied into C_rz
    and recorded by rh_sas_bands_configure with kind LAST under the same mask, weights, probabilities and windows gives the same bits."""
    n_part, ages, name = 257, 64, "TT_q_ss"
    want, (n, mask, w, values) = R.restate_age_pure(n_part, ages, (name,), 8, weighted)
    ctx = pure_context(n, ages)
    ctx.age_bands_configure([name], R.PROBS8, R.PURE_WINDOWS, mask, w)
    rows, hdr, closed, days = record_pure(ctx, values)
    for a in (0, R.TIE_AGE, ages):
        ctx.bands_configure([("C_rz", None, "last")], R.PROBS8, R.PURE_WINDOWS, mask, w)
        for d in range(R.PURE_DAYS):
            ctx.upload("C_rz", np.ascontiguousarray(values[d][name][:, a]))
            ctx.bands_record(d)
        prow, phdr, _, pclosed, pdays = ctx.bands_read()
        assert same_bits(rows[name][:, a], prow[:, 0]) and (hdr[name][:, a] == phdr[:, 0]).all() and phdr[:3, 0, 0].all(), a
        assert list(pclosed) == list(closed) and pdays == days
    ctx.close()


STEP_ITEMS = ["tt_q_ss", "TT_transp", "sa_s", "sa_rz"]


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_benchmark_a1000", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """4. The golden cases with which tests/test_hip_sas_totals.py steps tt_q_ss / TT_* / sa_s.  A: bands by age on, run_days(0, N) in one
    call; A2: step(d) day by day.  B: none, step(d) and downloads on the closing days, restated.  A's rows and headers are B's bits and
    A ends in B's state.  Not vacuous: every item has an age class with m > 0 under the mask and the weights.  The golden days leave no
    NaN in these four age-resolved arrays, so n_nan is 0 in every block (asserted, so that the statement stays true) and the NaN rules
    are the pure tests'."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    probs, win = (0.05, 0.5, 0.95), windows_for(N)
    mask = np.arange(g.n) % 4 != 1 if g.n > 2 else None
    wts = (np.arange(g.n) % 3 + 1).astype(np.uint16)
    ctxB = loaded(st, inputs, N)
    want = R.HostSasAgeBands(STEP_ITEMS, probs, win, g.n, mask, wts)
    for d in range(N):
        ctxB.step(d)
        want.add({v: ctxB.download(v) for v in STEP_ITEMS})
    widths = {v: ctxB.shape(v)[1] for v in STEP_ITEMS}
    assert want.closed[0] == 1 and all(want.hdr[v][..., 0].any() and not want.hdr[v][..., 1].any() for v in STEP_ITEMS)
    for by_step in (False, True):
        A = loaded(st, inputs, N)
        A.age_bands_configure(STEP_ITEMS, probs, win, mask, wts)
        if by_step:
            for d in range(N):
                A.step(d)
        else:
            A.run_days(0, N)
        assert_same_result(A.age_bands_read(), want, widths, (case, by_step))
        for name in held_names(A):
            a, b = A.download(name), ctxB.download(name)
            assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
        A.close()
    ctxB.close()


@pytest.mark.parametrize("zonal_bands", [False, True])
def test_beside_points_totals_zonal_totals_scores_and_bands(zonal_bands):
    """5. Bands by age together with points, totals, zonal totals, scores and the plain (or zonal) bands, configured in two different
    orders: each recorder's output is what it records alone."""
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
    recorders = {"age": lambda c: c.age_bands_configure(STEP_ITEMS, probs, awin, None, wts),
                 "bands": lambda c: c.bands_configure(named(items), probs, win, None, wts, **bkw),
                 "scores": lambda c: c.scores_configure(named(items), sobs, win), "points": lambda c: c.points_configure(cells, pnames, capacity=N),
                 "totals": lambda c: c.totals_configure(titems, None, capacity=N), "zonal": lambda c: c.zonal_configure(titems, zone, 2, capacity=N)}
    recorders["age"](alone_a)
    for key in ("bands", "scores", "points", "totals", "zonal"):
        recorders[key](alone_r)
    for ctx, order in ((C, ("age", "bands", "scores", "points", "totals", "zonal")), (D, ("zonal", "totals", "points", "scores", "bands", "age"))):
        for key in order:
            recorders[key](ctx)
    for ctx in (alone_a, alone_r, C, D):
        ctx.run_days(0, N)
    ra = alone_a.age_bands_read()
    assert list(ra[2]) == [1] and ra[3] == N and all(ra[1][v][..., 0].any() and (ra[1][v][..., 2] != ra[1][v][..., 0]).any() for v in STEP_ITEMS)
    rb = alone_r.bands_read()
    ms, cs, _ = alone_r.scores_read()
    want = [alone_r.points_read(0, N), alone_r.totals_read(0, N), alone_r.zonal_read(0, N)]
    for ctx in (C, D):
        rows, hdr, closed, days = ctx.age_bands_read()
        assert all(same_bits(rows[v], ra[0][v]) and (hdr[v] == ra[1][v]).all() for v in STEP_ITEMS) and list(closed) == [1] and days == N
        brow, bhdr, bpair, bclosed, bdays = ctx.bands_read()
        assert same_bits(brow, rb[0]) and (bhdr == rb[1]).all() and (bpair == rb[2]).all() and list(bclosed) == list(rb[3]) and bdays == N
        m, c, _ = ctx.scores_read()
        assert same_bits(m, ms) and list(c) == list(cs)
        for (tags, got), (wtags, wrows) in zip((ctx.points_read(0, N), ctx.totals_read(0, N), ctx.zonal_read(0, N)), want):
            assert list(tags) == list(wtags)
            for key, a in got.items():
                for b, wb in zip(*((x.values() if isinstance(x, dict) else [x]) for x in (a, wrows[key]))):
                    assert same_bits(b, wb), key
    # switched off, the others go on
    C.age_bands_configure([])
    C.step(N - 1)
    assert C.totals_count()[0] == N + 1 and C.bands_read()[4] == N + 1
    for ctx in (alone_a, alone_r, C, D):
        ctx.close()


def test_reconfigure_release_and_refusals():
    """6. Before the first configure and after a release, record / read / row_elems are RH_ERR_STATE; a second configure starts the count
    at 0 with an empty result; every refusal names the offender by code and message and leaves the configuration that was running."""
    from roger_amd._native import NativeError, SasContext

    n_part, ages, items = 65, 30, R.ITEMS4[:2]
    want, (n, mask, w, values) = R.restate_age_pure(n_part, ages, items, 3, True)
    widths = {v: R.width_of(v, ages) for v in items}
    ctx = pure_context(n, ages)
    total = ct.c_int64()
    for call in (ctx.age_bands_read, ctx.age_bands_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_age_bands_configure has not been called"):
            call()
    assert ctx._lib.rh_sas_age_bands_row_elems(ctx._h, ct.byref(total)) == -3
    good = dict(items=list(items), probs=R.pure_probs(3), windows=R.PURE_WINDOWS, mask=mask, weights=w)
    ctx.age_bands_configure(**good)
    assert ctx._lib.rh_sas_age_bands_row_elems(ctx._h, ct.byref(total)) == 0 and total.value == sum(widths.values())
    fresh = R.HostSasAgeBands(items, good["probs"], R.PURE_WINDOWS, n, mask, w)
    for d in range(3):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.age_bands_record(d)
        fresh.add(values[d])
    no_diag = SasContext(n, ages)
    with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure failed \(-3\).*array tt_q_ss is not held by this context"):
        no_diag.age_bands_configure(["tt_q_ss"], (0.5,), R.PURE_WINDOWS)
    no_diag.age_bands_configure(["sa_ss", "msa_rz"], (0.5,), R.PURE_WINDOWS)   # always held
    no_diag.close()
    last = lambda v: [(v, None, "last")]   # noqa: E731
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
           (dict(windows=(np.array([0, 2, 4, 6]), np.array([2, 3, 5, 9]))), "window 1 starts on day 2, window 0 ends on day 2"),
           (dict(windows=(np.array([0, 3, 4, 6]), np.array([0, 2, 5, 9]))), "window 1 is [3, 2]: its last day lies before its first"))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_sas_age_bands_configure failed \(-1\)") as e:
            ctx.age_bands_configure(**dict(good, **kw))
        assert "rh_sas_age_bands_configure: " + text in str(e.value), (text, str(e.value))
    item = np.array([[ctx.index("sa_rz"), -1, 2]], dtype=np.int32)
    unknown = np.array([[9999, -1, 2]], dtype=np.int32)
    pr, days = np.array([0.5]), np.array([0, 2], dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ct.c_void_p)   # noqa: E731
    for args in ((None, 1, p(pr), 1, None, None, p(days), p(days), 2), (p(item), 1, None, 1, None, None, p(days), p(days), 2),
                 (p(item), 1, p(pr), 1, None, None, None, p(days), 2), (p(item), 1, p(pr), 1, None, None, p(days), None, 2)):
        assert ctx._lib.rh_sas_age_bands_configure(ctx._h, *args) == -1 and b"rh_sas_age_bands_configure: null pointer" in ctx._lib.rh_sas_last_error(ctx._h)
    assert ctx._lib.rh_sas_age_bands_configure(ctx._h, p(unknown), 1, p(pr), 1, None, None, p(days), p(days), 2) == -1
    assert b"unknown array id 9999" in ctx._lib.rh_sas_last_error(ctx._h)
    assert ctx._lib.rh_sas_age_bands_configure(ctx._h, p(item), 1, p(pr), 1, None, None, p(days), p(days), 0) == -1
    assert b"n_samples = 0" in ctx._lib.rh_sas_last_error(ctx._h)
    # (with one probability the headers, 24 B per age class, are the larger buffer: 30 x 24 B x 2^22 is beyond 2 GiB, the rows are not)
    assert ctx._lib.rh_sas_age_bands_configure(ctx._h, p(item), 1, p(pr), 1, None, None, p(days), p(days), 1 << 22) == -1
    assert b"n_samples = 4194304 (at least one; rows of 30 age classes x 1 float64 and headers of 3 int64, each within 2 GiB)" in ctx._lib.rh_sas_last_error(ctx._h)
    with pytest.raises(NativeError, match=r"rh_sas_age_bands_record failed \(-1\).*day = -1"):
        ctx.age_bands_record(-1)
    rows = np.empty((4, total.value, 2))
    hdr, closed = np.empty((4, total.value, 3), dtype=np.int64), np.empty(4, dtype=np.uint8)
    assert ctx._lib.rh_sas_age_bands_read(ctx._h, p(rows), rows.nbytes, p(hdr), hdr.nbytes, p(closed), closed.nbytes, None) == -1
    assert b"rh_sas_age_bands_read: size mismatch" in ctx._lib.rh_sas_last_error(ctx._h)
    # the configuration that was running goes on
    for d in range(3, R.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.age_bands_record(d)
        fresh.add(values[d])
    assert_same_result(ctx.age_bands_read(), fresh, widths, "after the refusals")
    assert_same_result(ctx.age_bands_read(), want, widths, "the restated pure run")
    # a second configure, with other items: the count is 0 and nothing is recorded
    ctx.age_bands_configure(["sa_s"], (0.5,), R.PURE_WINDOWS)
    rows, hdr, closed, days = ctx.age_bands_read()
    assert list(rows) == ["sa_s"] and rows["sa_s"].shape == (4, ages, 1) and np.isnan(rows["sa_s"]).all() and not hdr["sa_s"].any()
    assert not closed.any() and days == 0
    ctx.age_bands_configure([])
    for call in (ctx.age_bands_read, ctx.age_bands_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_age_bands_configure has not been called"):
            call()
    ctx.age_bands_configure(**good)
    assert ctx._lib.rh_sas_age_bands_configure(ctx._h, None, 0, None, 0, None, None, None, None, 0) == 0
    with pytest.raises(NativeError, match=r"failed \(-3\)"):
        ctx.age_bands_record()
    ctx.close()
