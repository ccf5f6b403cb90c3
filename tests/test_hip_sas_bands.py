"""GPU: transport bands of the SAS context (rh_sas_bands_*; k_sas_bands_day, k_sas_bands_hist, k_sas_bands_pick, k_sas_bands_obs and
k_sas_bands_obs_row in roger_amd/csrc/rh_sas_bands.h), tolerance zero.

The truth is tests/sas_bands_reference.py -- the host's window clock, the day kernel and the selection in numpy -- applied to what was
uploaded where no day kernel runs, and to the downloads of a second context WITHOUT bands that steps day by day where one does.  The pure
inputs are the ones tests/test_sas_bands_reference.py shows to have teeth and to meet their conditions."""
import numpy as np
import pytest

import sas_binding as sb
import sas_bands_reference as B
from test_hip_sas_points import daily_inputs, held_names, same_bits
from test_hip_sas_scores import loaded, named, step_items, windows_for

pytestmark = pytest.mark.gpu


def assert_same_result(got, want, where):
    rows, hdr, pairs, closed, days = got
    assert days == want.win.days and list(closed) == list(want.closed), where
    assert (hdr == want.hdr).all(), (where, hdr, want.hdr)
    assert same_bits(rows, want.rows), (where, rows, want.rows)
    assert (pairs == want.pairs).all(), (where, pairs, want.pairs)


def run_pure(n, n_items, n_probs, weighted, observed):
    from roger_amd._native import SasContext

    items = B.ITEMS8[:n_items]
    values, weights, obs = B.make_pure(n, items)
    mask, w = B.pure_participation(n, weighted)
    want = B.restate_pure(n, items, n_probs, weighted, observed)
    ctx = SasContext(n, 30, forcing_days=3)
    for wn, a in weights.items():
        ctx.upload(wn, a)
    ctx.bands_configure(named(items), B.pure_probs(n_probs), B.PURE_WINDOWS, mask, w, obs if observed else None)
    for d in range(B.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
    got = ctx.bands_read()
    ctx.close()
    assert_same_result(got, want, (n, n_items, n_probs, weighted))
    assert list(got[3]) == [1, 1, 1, 0] and got[1][:3, :, 0].any()
    return got


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_probs", [1, 8])
@pytest.mark.parametrize("n_items", [1, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_pure(n, n_items, n_probs, weighted):
    """1. No day kernel: uploaded arrays, bands_record over 7 days; the windows [0, 0], [1, 2], a gap day, [4, 5] and one that closes on a
    day never reached.  Wavefront and tile boundaries, the shared pass-0 histogram against one per probability, one and many items per
    workgroup, with and without a weight plane (and a mask); the observations' kernels with both."""
    run_pure(n, n_items, n_probs, weighted, observed=True)


def test_pure_beyond_one_tile_per_workgroup():
    """2. n = 256 * 256 + 1: the smallest size at which a workgroup of the capped grid walks more than one tile and the last tile is
    partial; 8 items, 8 probabilities, weights and observations."""
    rows, hdr, pairs, _, _ = run_pure(256 * 256 + 1, 8, 8, True, True)
    assert (hdr[:3, :, 2] != hdr[:3, :, 0]).any() and (pairs[:3, :, 0] >= 0).any() and (pairs[:3] == -1).any()


def band_windows(N):
    return windows_for(N)


def restated_by_steps(g, st, inputs, items, probs, win, N, obs):
    """Context B: no bands, step(d) and downloads per day, restated by the reference.  (the reference, B)"""
    ctx = loaded(st, inputs, N)
    want = B.HostSasBands(items, probs, win, g.n, None, None, obs)
    for d in range(N):
        ctx.step(d)
        want.add({v: ctx.download(v) for v in {it[0] for it in items}}, {"q_ss": inputs["q_ss"][d]})
    return want, ctx


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """3. A: bands on, run_days(0, N) in one call; A2: bands on, step(d) day by day.  B: none, step(d) and downloads per day, restated.
    A's rows, headers and pairs are B's bits and A ends in B's state."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items, probs, win = step_items(st), (0.05, 0.5, 0.95), band_windows(N)
    obs = -9.0 + 3.0 * np.random.default_rng(5).random((len(items), len(win[0])))
    obs[1, 0] = np.nan
    want, ctxB = restated_by_steps(g, st, inputs, items, probs, win, N, obs)
    assert want.closed[0] == 1 and want.hdr[:, 0, 0].any() and want.hdr[:, 1, 0].any() and want.hdr[:, 2, 0].any()   # the bulk item holds a number: not vacuous
    for by_step in (False, True):
        A = loaded(st, inputs, N)
        A.bands_configure(named(items), probs, win, obs=obs)
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
    """4. Bands together with points, totals, zonal totals and scores, configured in two different orders: each recorder's output is what
    it records alone."""
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
    probs, bobs = (0.0, 0.5, 1.0), sobs[:, 0, :]
    zone = (np.arange(g.n) % 2).astype(np.int32)
    wts = (np.arange(g.n) % 3 + 1).astype(np.uint16)
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    alone_b, alone_r, C, D = (loaded(st, inputs, N) for _ in range(4))
    recorders = {"bands": lambda c: c.bands_configure(named(items), probs, win, None, wts, bobs),
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
    assert rb[1][:, :, 0].any() and (rb[1][:, :, 2] != rb[1][:, :, 0]).any()
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
    """5. A second configure starts the count at 0 with an empty result; no items release everything, and reading or recording is then
    RH_ERR_STATE, as before the first configure; the argument errors name the offender and leave the configuration that was running."""
    from roger_amd._native import NativeError, SasContext

    n, items = 65, B.ITEMS8[:3]
    values, weights, obs = B.make_pure(n, items)
    ctx = SasContext(n, 30, forcing_days=3)
    for call in (ctx.bands_read, ctx.bands_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_bands_configure has not been called"):
            call()
    for wn, a in weights.items():
        ctx.upload(wn, a)
    good = dict(items=named(items), probs=(0.05, 0.5, 0.95), windows=B.PURE_WINDOWS, obs=obs)
    want = B.HostSasBands(items, good["probs"], B.PURE_WINDOWS, n, None, None, obs)
    ctx.bands_configure(**good)
    for d in range(3):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
        want.add(values[d], {wn: a[d % 3] for wn, a in weights.items()})
    bad = ((dict(items=[("tt50_q_ss", None, "mean")], obs=None), -3, "array tt50_q_ss is not held by this context"),
           (dict(items=[("maskCatch", None, "mean")], obs=None), -1, "array maskCatch is int32"),
           (dict(items=[("q_ss", None, "mean")], obs=None), -1, "array q_ss is a daily input"),
           (dict(items=[("sas_params_q_ss", None, "mean")], obs=None), -1, "array sas_params_q_ss is a parameter block"),
           (dict(items=[("sa_rz", None, "mean")], obs=None), -1, "array sa_rz is age-resolved"),
           (dict(items=[("C_rz", "C_in", "bulk")], obs=None), -1, "weight C_in is not a daily flux input"),
           (dict(items=[("C_rz", None, "bulk")], obs=None), -1, "array C_rz is BULK and has no weight"),
           (dict(items=[("C_rz", "q_ss", "last")], obs=None), -1, "array C_rz is LAST and has the weight q_ss"),
           (dict(items=[("C_rz", None, 3)], obs=None), -1, "kind 3 of array C_rz"),
           (dict(items=[("C_rz", None, "last"), ("C_rz", None, "last")], obs=None), -1, "array C_rz is given twice with the same weight and kind"),
           (dict(items=[(nm, None, "mean") for nm in ctx.names if nm.startswith("C_") and nm != "C_in"][:9], obs=None), -1, "n_items = 9 (0 ... 8)"),
           (dict(probs=tuple(np.linspace(0, 1, 9))), -1, "n_probs = 9 (1 ... 8)"),
           (dict(probs=()), -1, "n_probs = 0 (1 ... 8)"),
           (dict(probs=(0.5, 1.5)), -1, "probability 1 is 1.5"),
           (dict(probs=(np.nan,)), -1, "probability 0 is nan"),
           (dict(mask=np.zeros(n, dtype=np.uint8)), -1, "no cell takes part (0 of 65 cells"),
           (dict(weights=np.zeros(n, dtype=np.uint16)), -1, "no cell takes part"),
           (dict(mask=np.arange(n) % 2, weights=(np.arange(n) % 2 == 0).astype(np.uint16)), -1, "no cell takes part"),
           (dict(windows=(np.array([0, 2, 4, 6]), np.array([2, 3, 5, 9]))), -1, "window 1 starts on day 2, window 0 ends on day 2"),
           (dict(windows=(np.array([0, 3, 4, 6]), np.array([0, 2, 5, 9]))), -1, "window 1 is [3, 2]: its last day lies before its first"))
    for kw, code, text in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_bands_configure failed \(%d\)" % code) as e:
            ctx.bands_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    import ctypes as ct

    item = np.array([[ctx.index("C_rz"), -1, 2]], dtype=np.int32)
    pr, days = np.array([0.5]), np.array([0, 2], dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ct.c_void_p)   # noqa: E731
    for args in ((None, 1, p(pr), 1, None, None, None, p(days), p(days), 2), (p(item), 1, None, 1, None, None, None, p(days), p(days), 2),
                 (p(item), 1, p(pr), 1, None, None, None, None, p(days), 2), (p(item), 1, p(pr), 1, None, None, None, p(days), None, 2)):
        assert ctx._lib.rh_sas_bands_configure(ctx._h, *args) == -1 and b"null pointer" in ctx._lib.rh_sas_last_error(ctx._h)
    assert ctx._lib.rh_sas_bands_configure(ctx._h, p(item), 1, p(pr), 1, None, None, None, p(days), p(days), 0) == -1
    assert b"n_samples = 0" in ctx._lib.rh_sas_last_error(ctx._h)
    with pytest.raises(NativeError, match=r"rh_sas_bands_record failed \(-1\).*day = -1"):
        ctx.bands_record(-1)
    # the configuration that was running goes on
    for d in range(3, B.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.bands_record(d)
        want.add(values[d], {wn: a[d % 3] for wn, a in weights.items()})
    assert_same_result(ctx.bands_read(), want, "after the refusals")
    # a second configure: the count is 0 and nothing is recorded
    ctx.bands_configure(**good)
    rows, hdr, pairs, closed, days = ctx.bands_read()
    assert np.isnan(rows).all() and not hdr.any() and (pairs == -1).all() and not closed.any() and days == 0
    ctx.bands_configure([])
    for call in (ctx.bands_read, ctx.bands_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_bands_configure has not been called"):
            call()
    ctx.close()
