"""GPU: scores of the SAS context against observed samples (rh_sas_scores_*, k_sas_scores in roger_amd/csrc/rh_sas_scores.h), tolerance
zero.

The truth is tests/sas_scores_reference.py -- the host's window clock and the kernel's day in numpy -- applied to what was uploaded
where no day kernel runs, and to the downloads of a second context WITHOUT scores that steps day by day where one does.  The pure
inputs are the ones tests/test_sas_scores_reference.py shows to have teeth."""
import numpy as np
import pytest

import sas_binding as sb
import sas_scores_reference as S
from test_hip_sas import make_ctx
from test_hip_sas_points import daily_inputs, held_names, same_bits

pytestmark = pytest.mark.gpu


def named(items):
    """The items of the reference, (value, weight, kind int), as the binding takes them."""
    return [(v, w, int(k)) for v, w, k in items]


@pytest.mark.parametrize("n_series", [1, 3])
@pytest.mark.parametrize("n_items", [1, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_pure(n, n_items, n_series):
    """1. No day kernel: uploaded arrays, scores_record over 7 days; the windows [0, 0], [1, 2], a gap day, [4, 5] and one that closes
    on a day never reached."""
    from roger_amd._native import SasContext

    items = S.ITEMS16[:n_items]
    values, weights, obs = S.make_pure(n, items, n_series)
    series = S.pure_series(n) if n_series > 1 else None
    want = S.restate_pure(n, items, n_series)
    counted = want.moments[:, 2, :]
    scored = np.ones(n, dtype=bool) if series is None else series >= 0
    assert (counted.max(axis=1) >= 1).all() and (n == 1 or len(np.unique(counted[0][scored])) > 1)
    ctx = SasContext(n, 30, forcing_days=3)
    for w, a in weights.items():
        ctx.upload(w, a)
    ctx.scores_configure(named(items), obs, S.PURE_WINDOWS, series)
    for d in range(S.PURE_DAYS):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.scores_record(d)
    moments, closed, days = ctx.scores_read()
    ctx.close()
    assert days == S.PURE_DAYS and list(closed) == list(want.closed) == [1, 1, 1, 0]
    for j, it in enumerate(items):
        for m in range(S.NMOM):
            assert same_bits(moments[j, m], want.moments[j, m]), (n, it, m, moments[j, m][:4], want.moments[j, m][:4])
    if series is not None:
        assert not moments[:, :, series < 0].any()
    assert moments[:, 3].min() < 0                       # (delta values: negative sums)


def windows_for(N):
    first, last = np.array([0, 1, 3]), np.array([0, 2, 3])
    keep = first < N
    return first[keep], np.minimum(last[keep], N - 1)


def step_items(st):
    return [("C_q_ss" if st.anion else "C_iso_q_ss", "q_ss", S.BULK), ("C_rz", None, S.MEAN), ("C_rz", None, S.LAST)]


def loaded(st, inputs, N):
    ctx = make_ctx(st, forcing_days=N)
    for k, a in st.state.items():
        ctx.upload(k, a)
    for k, a in inputs.items():
        ctx.upload(k, a)
    return ctx


def observations(n_items, K, seed):
    rng = np.random.default_rng(seed)
    return -9.0 + 3.0 * rng.random((n_items, 1, K))


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """2. A: scores on, run_days(0, N) in one call.  B: none, step(d) and downloads per day, restated.  A's moments are B's bits and A
    ends in B's state."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items = step_items(st)
    win = windows_for(N)
    obs = observations(len(items), len(win[0]), 5)
    A, B = loaded(st, inputs, N), loaded(st, inputs, N)
    A.scores_configure(named(items), obs, win)
    A.run_days(0, N)
    moments, closed, days = A.scores_read()
    want = S.HostSasScores(items, obs, win, g.n)
    for d in range(N):
        B.step(d)
        want.add({v: B.download(v) for v in {it[0] for it in items}}, {"q_ss": inputs["q_ss"][d]})
    assert days == N and list(closed) == list(want.closed) and closed[0] == 1
    assert same_bits(moments, want.moments), (case, moments[:, :, 0], want.moments[:, :, 0])
    assert moments[0, 2].any() and moments[1, 2].any() and moments[2, 2].any()      # the bulk item counts a cell: it is not vacuous
    for name in held_names(A):
        a, b = A.download(name), B.download(name)
        assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
    A.close()
    B.close()


def test_beside_points_totals_and_zonal_totals():
    """3. Scores together with points, totals and zonal totals, configured in two different orders: each recorder's output is what it
    records alone."""
    from test_hip_sas_totals import step_items as totals_items

    g = sb.SasGolden("sas_stats_a30")
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items, titems = step_items(st), totals_items(st, g.stats)
    win = windows_for(N)
    obs = observations(len(items), len(win[0]), 6)
    zone = (np.arange(g.n) % 2).astype(np.int32)
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    alone_s, alone_r, C, D = (loaded(st, inputs, N) for _ in range(4))
    recorders = {"scores": lambda c: c.scores_configure(named(items), obs, win), "points": lambda c: c.points_configure(cells, pnames, capacity=N),
                 "totals": lambda c: c.totals_configure(titems, None, capacity=N), "zonal": lambda c: c.zonal_configure(titems, zone, 2, capacity=N)}
    recorders["scores"](alone_s)
    for key in ("points", "totals", "zonal"):
        recorders[key](alone_r)
    for ctx, order in ((C, ("scores", "points", "totals", "zonal")), (D, ("zonal", "totals", "points", "scores"))):
        for key in order:
            recorders[key](ctx)
    for ctx in (alone_s, alone_r, C, D):
        ctx.run_days(0, N)
    ms, cs, _ = alone_s.scores_read()
    assert ms[:, 2].any()
    want = [alone_r.points_read(0, N), alone_r.totals_read(0, N), alone_r.zonal_read(0, N)]
    for ctx in (C, D):
        m, c, days = ctx.scores_read()
        assert same_bits(m, ms) and list(c) == list(cs) and days == N
        for (tags, rows), (wtags, wrows) in zip((ctx.points_read(0, N), ctx.totals_read(0, N), ctx.zonal_read(0, N)), want):
            assert list(tags) == list(wtags)
            for key, a in rows.items():
                for b, wb in zip(*((x.values() if isinstance(x, dict) else [x]) for x in (a, wrows[key]))):
                    assert same_bits(b, wb), key
    # switched off, the others go on
    C.scores_configure([])
    C.step(N - 1)
    assert C.totals_count()[0] == N + 1
    for ctx in (alone_s, alone_r, C, D):
        ctx.close()


def test_configured_mid_window_reconfigured_and_switched_off():
    """4. A window that began before the count did (first_day < 0) is never compared and its `closed` stays 0; reconfiguring clears the
    moments and restarts the count; no items stop the launches, and reading is RH_ERR_STATE."""
    from roger_amd._native import NativeError, SasContext

    n, items = 65, S.ITEMS16[:3]
    values, weights, obs = S.make_pure(n, items, 1)
    obs = np.nan_to_num(obs[:, :, :2], nan=-8.0)
    win = (np.array([-1, 2]), np.array([1, 3]))
    ctx = SasContext(n, 30, forcing_days=3)
    for w, a in weights.items():
        ctx.upload(w, a)
    ctx.scores_configure(named(items), obs, win)
    want = S.HostSasScores(items, obs, win, n)
    for d in range(4):
        for v, a in values[d].items():
            ctx.upload(v, a)
        ctx.scores_record(d)
        want.add(values[d], {w: a[d % 3] for w, a in weights.items()})
        if d == 1:   # window 0 has just passed: nothing was compared, no accumulator was touched
            m, c, _ = ctx.scores_read()
            assert not m.any() and list(c) == [0, 0]
    moments, closed, days = ctx.scores_read()
    assert list(closed) == [0, 1] == list(want.closed) and days == 4
    assert same_bits(moments, want.moments) and moments[:, 2].max() == 1.0
    ctx.scores_configure(named(items), obs, win)
    moments, closed, days = ctx.scores_read()
    assert not moments.any() and not np.signbit(moments).any() and list(closed) == [0, 0] and days == 0
    ctx.scores_configure([])
    for call in (ctx.scores_read, ctx.scores_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_scores_configure has not been called"):
            call()
    ctx.close()


def test_refusals_name_the_offender_and_leave_the_series_running():
    """5. The argument errors of rh_sas_scores_configure; the entry points before it was called."""
    from roger_amd._native import NativeError, SasContext

    n = 5
    ctx = SasContext(n, 30, forcing_days=2)
    for call in (ctx.scores_read, ctx.scores_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_scores_configure has not been called"):
            call()
    C = np.arange(n, dtype=np.float64) - 7.5
    ctx.upload("C_rz", C)
    good = dict(items=[("C_rz", None, "last")], obs=np.full((1, 2, 2), -6.0), windows=(np.array([0, 2]), np.array([0, 3])),
                series=np.array([0, 1, -1, 1, 0], dtype=np.int32))
    ctx.scores_configure(**good)
    ctx.scores_record(0)
    one = np.full((1, 2, 2), -6.0)
    bad = ((dict(items=[("tt50_q_ss", None, "mean")]), -3, "array tt50_q_ss is not held by this context"),
           (dict(items=[("maskCatch", None, "mean")]), -1, "array maskCatch is int32"),
           (dict(items=[("q_ss", None, "mean")]), -1, "array q_ss is a daily input"),
           (dict(items=[("C_in", None, "mean")]), -1, "array C_in is a daily input"),
           (dict(items=[("sas_params_q_ss", None, "mean")]), -1, "array sas_params_q_ss is a parameter block"),
           (dict(items=[("sa_rz", None, "mean")]), -1, "array sa_rz is age-resolved"),
           (dict(items=[("C_rz", "C_in", "bulk")]), -1, "weight C_in is not a daily flux input"),
           (dict(items=[("C_rz", "C_ss", "bulk")]), -1, "weight C_ss is not a daily flux input"),
           (dict(items=[("C_rz", None, "bulk")]), -1, "array C_rz is BULK and has no weight"),
           (dict(items=[("C_rz", "q_ss", "mean")]), -1, "array C_rz is MEAN and has the weight q_ss"),
           (dict(items=[("C_rz", "q_ss", "last")]), -1, "array C_rz is LAST and has the weight q_ss"),
           (dict(items=[("C_rz", None, 3)]), -1, "kind 3 of array C_rz"),
           (dict(items=[("C_rz", None, "last"), ("C_rz", None, "mean"), ("C_rz", None, "last")], obs=np.zeros((3, 2, 2))), -1,
            "array C_rz is given twice with the same weight and kind"),
           (dict(items=[(nm, None, "mean") for nm in ctx.names if nm.startswith("C_") and nm != "C_in"][:17], obs=np.zeros((17, 2, 2))), -1,
            "n_items = 17 (0 ... 16)"),
           (dict(obs=np.zeros((1, 1025, 2)), series=None), -1, "n_series = 1025 (1 ... 1024)"),
           (dict(obs=one[:, :1]), -1, "series 1 of cell 1 (< 0: not scored, else 0 ... 0)"),
           (dict(series=np.full(n, -1, dtype=np.int32)), -1, "the series map scores no cell (0 of 5 cells)"),
           (dict(windows=(np.array([0, 2]), np.array([2, 3]))), -1, "window 1 starts on day 2, window 0 ends on day 2"),
           (dict(windows=(np.array([2, 0]), np.array([3, 1]))), -1, "window 1 starts on day 0, window 0 ends on day 3"),
           (dict(windows=(np.array([0, 3]), np.array([0, 2]))), -1, "window 1 is [3, 2]: its last day lies before its first"))
    for kw, code, text in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_scores_configure failed \(%d\)" % code) as e:
            ctx.scores_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    import ctypes as ct

    item = np.array([[ctx.index("C_rz"), -1, 2]], dtype=np.int32)
    days = np.array([0, 2], dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ct.c_void_p)   # noqa: E731
    for args in ((None, 1, None, 2, p(one), p(days), p(days), 2), (p(item), 1, None, 2, None, p(days), p(days), 2),
                 (p(item), 1, None, 2, p(one), None, p(days), 2), (p(item), 1, None, 2, p(one), p(days), None, 2)):
        assert ctx._lib.rh_sas_scores_configure(ctx._h, *args) == -1 and b"null pointer" in ctx._lib.rh_sas_last_error(ctx._h)
    assert ctx._lib.rh_sas_scores_configure(ctx._h, p(item), 1, None, 1, p(one), p(days), p(days), 0) == -1
    assert b"n_samples = 0" in ctx._lib.rh_sas_last_error(ctx._h)
    with pytest.raises(NativeError, match=r"rh_sas_scores_record failed \(-1\).*day = -1"):
        ctx.scores_record(-1)
    # the series that was running goes on: day 0 was scored before the refusals, the days 1 ... 3 after them
    for d in (1, 2, 3):
        ctx.scores_record(d)
    moments, closed, days_scored = ctx.scores_read()
    want = S.HostSasScores([("C_rz", None, S.LAST)], good["obs"], good["windows"], n, good["series"])
    for d in range(4):
        want.add({"C_rz": C})
    assert days_scored == 4 and list(closed) == [1, 1] and same_bits(moments, want.moments) and list(moments[0, 2]) == [2, 2, 0, 2, 2]
    ctx.close()


import test_host_package_sas_scores as HS  # noqa: E402

on_disk = HS.on_disk


def test_script_on_the_device_writes_the_file_the_double_is_restated_to(on_disk, tmp_path):
    """6. A setup script with `state.transport_scores` AND `state.diagnostics` on the real SasContext: the moments of
    `.transport_scores.nc` are the restatement applied to the fields `.collect.nc` holds for every day."""
    g, model = HS.scores_model("sas_stats_a30", tmp_path, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    model.state.sas_context.close()
    data = HS.assert_scores_restate_the_diagnostics(tmp_path, g)
    assert data["C_iso_q_ss_by_q_ss_n"].any()
