"""GPU: catchment totals of the SAS context (rh_sas_totals_*, kernels in roger_amd/csrc/rh_sas_totals.h), tolerance zero.

The truth is tests/sas_totals_reference.py -- the counting rules and both orders of summation in numpy -- applied to what was uploaded
where no day kernel runs, and to the downloads of a second context WITHOUT totals that steps day by day where one does.  The inputs are
the ones tests/test_sas_totals_reference.py shows to have teeth."""
import numpy as np
import pytest

import sas_binding as sb
import sas_totals_reference as R
from test_hip_sas import make_ctx
from test_hip_sas_points import daily_inputs, held_names, same_bits

pytestmark = pytest.mark.gpu


def key_of(item):
    return item if isinstance(item, str) else f"{item[0]}_by_{item[1]}"


def assert_row(rows, k, want, what):
    for key, block in want.items():
        got = R.as_block({s: a[k] for s, a in rows[key].items()})
        assert same_bits(got, block), (what, key, got[:6], block[:6])


def pure_context(n, ages):
    from roger_amd._native import SasContext

    ctx = SasContext(n, ages, forcing_days=3, keep_distributions=True)
    d = R.make_inputs(n, ages)
    for name, a in d.items():
        ctx.upload(name, a)
    return ctx, d


def check_masks_and_days(ctx, d, n):
    for mname, mask in R.masks(n).items():
        ctx.totals_configure(R.ITEMS, mask, capacity=8)
        assert ctx.totals_count() == (0, n if mask is None else int(np.count_nonzero(mask)))
        days = (0, 1, 2, 4, -1)            # day 4: row 1 of the 3-row daily inputs; -1: no daily row
        for i, day in enumerate(days):
            ctx.totals_record(tag=50 + i, day=day)
        tags, rows = ctx.totals_read(0, len(days))
        assert list(tags) == [50 + i for i in range(len(days))]
        for i, day in enumerate(days):
            assert_row(rows, i, R.want_row(d, R.ITEMS, mask, day), (n, mname, day))
        # nothing counted: the identity block; day < 0: weighted and DAILY items have no eligible cell, the others do
        assert list(R.as_block({s: a[0] for s, a in rows["C_q_ss_by_cpr_rz"].items()})) == [0.0, 0.0, 0.0, np.inf, -np.inf]
        assert rows["C_in"]["count"][4] == 0 and rows["tt_q_ss_by_q_ss"]["count"][4] == 0 and not rows["tt_q_ss_by_q_ss"]["sum"][4].any()
        assert rows["C_rz"]["count"][4] == rows["sa_s"]["count"][4] == ctx.totals_count()[1]
        assert same_bits(rows["C_in"]["sum"][1], rows["C_in"]["sum"][3]) and (n < 5 or not same_bits(rows["C_in"]["sum"][0], rows["C_in"]["sum"][1]))


@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 300])
@pytest.mark.parametrize("ages", [30, 63, 64, 255, 256, 1000])
def test_pure_reduction(ages, n):
    """1. No day kernel.  ages + 1 crosses 64, 256 and 1001 (one to four chunks of lanes); n below, on and above one run / one tile."""
    ctx, d = pure_context(n, ages)
    check_masks_and_days(ctx, d, n)
    ctx.close()


def test_pure_reduction_three_levels_and_the_ring():
    """1. n = 65 537: three levels of the age rule, a ragged last tile and a second round of accumulators in the width-1 rule; 8 records
    into a ring of 3, one array changed between records."""
    from roger_amd._native import NativeError

    n, ages = 65537, 30
    ctx, d = pure_context(n, ages)
    mask = R.masks(n)["runs"]
    items = ("C_rz", ("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s", ("TT_q_ss", "transp"))
    for m in (None, mask):
        ctx.totals_configure(items, m, capacity=3)
        ctx.totals_record(tag=0, day=2)
        assert_row(ctx.totals_read(0, 1)[1], 0, R.want_row(d, items, m, 2), "65537")
    ctx.totals_configure(items, mask, capacity=3)
    want = []
    for i in range(8):
        name = ("C_rz", "sa_s")[i % 2]
        d[name] = d[name] * 1.25 + 0.5
        ctx.upload(name, d[name])
        ctx.totals_record(tag=100 + i, day=i)
        want.append(R.want_row(d, items, mask, i))
    assert ctx.totals_count()[0] == 8
    for first, cnt in ((5, 3), (6, 2), (7, 1), (5, 1), (8, 0)):        # (5, 3): slots 2, 0, 1 -- across the wrap
        tags, rows = ctx.totals_read(first, cnt)
        assert list(tags) == [100 + k for k in range(first, first + cnt)]
        assert rows["sa_s"]["sum"].shape == (cnt, ages) and rows["C_rz"]["sum"].shape == (cnt,)
        for k in range(cnt):
            assert_row(rows, k, want[first + k], (first, cnt, k))
    for first in range(5):
        with pytest.raises(NativeError, match=r"rh_sas_totals_read failed \(-1\).*rows %d \.\.\. 4 have been overwritten" % first):
            ctx.totals_read(first, 1)
    with pytest.raises(NativeError, match=r"rh_sas_totals_read failed \(-1\).*overwritten"):
        ctx.totals_read(4, 4)
    with pytest.raises(NativeError, match=r"rh_sas_totals_read failed \(-1\).*not been recorded"):
        ctx.totals_read(7, 2)
    ctx.close()


def step_items(st, stats):
    if st.anion:
        return [("C_q_ss", "q_ss"), "M_rz", ("tt_q_ss", "q_ss"), ("mtt_q_ss", "q_ss"), ("TT_transp", "transp"), "sa_s", "q_ss"]
    return [("C_iso_q_ss", "q_ss"), "C_rz", ("tt_q_ss", "q_ss"), ("mtt_transp", "transp"), ("TT_transp", "transp"), "sa_s", "q_ss",
            ("C_iso_q_ss", "transp")] + (["tt50_q_ss"] if stats else [])


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_benchmark_a1000", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """2. A: totals on, run_days(0, N) in one call.  B: none, step(d) and downloads per day, restated.  Every recorded value is B's bits;
    A ends in B's state and outputs.  C, D: points and totals together, configured in either order, record the rows of each alone."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items = step_items(st, g.stats)
    mask = np.arange(g.n) % 4 != 1 if g.n > 2 else None
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    ctxs = []
    for _ in "ABCD":
        ctx = make_ctx(st, forcing_days=N)
        for k, a in st.state.items():
            ctx.upload(k, a)
        for k, a in inputs.items():
            ctx.upload(k, a)
        ctxs.append(ctx)
    A, B, C, D = ctxs
    A.totals_configure(items, mask, capacity=N)
    C.points_configure(cells, pnames, capacity=N)
    C.totals_configure(items, mask, capacity=N)
    D.totals_configure(items, mask, capacity=N)
    D.points_configure(cells, pnames, capacity=N)
    for ctx in (A, C, D):
        ctx.run_days(0, N)
    assert A.totals_count()[0] == N
    tags, rows = A.totals_read(0, N)
    assert list(tags) == list(range(N))
    for d in range(N):
        B.step(d)
        want = {}
        for it in items:
            v, w = (it, None) if isinstance(it, str) else it
            val = inputs[v][d] if v in inputs else B.download(v)
            want[key_of(it)] = R.item_block(val, None if w is None else inputs[w][d], mask)
        assert_row(rows, d, want, (case, "day", d))
    assert rows[key_of(items[2])]["sum"].any() and rows["sa_s"]["sum"].any() and rows[key_of(items[0])]["count"].any()
    for name in held_names(A):
        a, b = A.download(name), B.download(name)
        assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
    # points and totals together, in either order
    for ctx in (C, D):
        _, r2 = ctx.totals_read(0, N)
        for key in rows:
            for s in rows[key]:
                assert same_bits(r2[key][s], rows[key][s]), (case, key, s)
    _, pc = C.points_read(0, N)
    _, pd = D.points_read(0, N)
    for v in pnames:
        assert same_bits(pc[v], pd[v]), v
    A.points_configure(cells, pnames, capacity=1)
    A.totals_configure([])
    A.points_record()
    for v in pnames:
        assert same_bits(A.points_read(0, 1)[1][v][0], pc[v][N - 1]), v
    for ctx in ctxs:
        ctx.close()


def test_physical_closure():
    """3. A backward travel time distribution sums to 1 over the ages, so sum_T of the q_ss-weighted tt_q_ss sums, recorded over the
    cells whose tt_q_ss sums to 1 (the mask), equals the `wsum` of those cells within ages * n * 2^-52 * wsum (ages * n additions of
    non-negative terms)."""
    import math

    g = sb.SasGolden("sas_mixed_a70")
    st = g.new_state()
    g.load_state(st, 1)          # (the golden day 1 has no percolation: day 2 from the state after day 1)
    g.load_inputs(st, 2)
    ctx = make_ctx(st)
    for k, a in st.state.items():
        ctx.upload(k, a)
    for k, a in st.inp.items():
        ctx.upload(k, a[None, :])
    ctx.step(0)
    tt, q = ctx.download("tt_q_ss"), st.inp["q_ss"]
    ages = tt.shape[1]
    closed = np.abs(np.array([math.fsum(r) for r in np.nan_to_num(tt)]) - 1.0) <= ages * 2.0 ** -52
    assert (closed & (q > 0)).any()
    ctx.totals_configure([("tt_q_ss", "q_ss")], closed, capacity=1)
    ctx.totals_record(tag=0, day=0)              # (behind the completed day: the arrays the day's own row would read)
    blk = ctx.totals_read(0, 1)[1]["tt_q_ss_by_q_ss"]
    wsum = blk["wsum"][0]
    assert blk["count"][0] == np.count_nonzero(closed & (q > 0)) and abs(wsum - math.fsum(q[closed & (q > 0)])) <= g.n * 2.0 ** -52 * wsum
    bound = ages * g.n * 2.0 ** -52 * wsum
    print("closure: sum_T", math.fsum(blk["sum"][0]), "wsum", wsum, "bound", bound)
    assert wsum > 0 and abs(math.fsum(blk["sum"][0]) - wsum) <= bound
    ctx.close()


def test_refusals_name_the_offender_and_leave_the_series_running():
    """The argument errors of rh_sas_totals_configure; the four entry points before it was called."""
    from roger_amd._native import NativeError, SasContext

    n, ages = 5, 30
    ctx = SasContext(n, ages, keep_distributions=False)
    for call in (ctx.totals_count, lambda: ctx.totals_read(0, 0), ctx.totals_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_totals_configure has not been called"):
            call()
    C = np.arange(n, dtype=np.float64) - 7.0
    ctx.upload("C_rz", C)
    ctx.totals_configure(["C_rz", "sa_rz"], capacity=4)
    ctx.totals_record(tag=-3)
    bad = ((dict(items=["C_rz", "tt_q_ss"]), -3, "array tt_q_ss is not held by this context (age_statistics / keep_distributions"),
           (dict(items=["maskCatch"]), -1, "array maskCatch is int32"),
           (dict(items=["sas_params_q_ss"]), -1, "array sas_params_q_ss is a parameter block"),
           (dict(items=["C_rz", ("C_rz", "q_ss"), "C_rz"]), -1, "array C_rz is given twice with the same weight"),
           (dict(items=[("C_rz", "q_ss"), ("C_rz", "q_ss")]), -1, "array C_rz is given twice with the same weight"),
           (dict(items=[("C_rz", "C_in")]), -1, "weight C_in is not a daily flux input"),
           (dict(items=[("C_rz", "C_ss")]), -1, "weight C_ss is not a daily flux input"),
           (dict(mask=np.zeros(n, dtype=bool)), -1, "the mask holds no cell"),
           (dict(capacity=0), -1, "capacity = 0"),
           (dict(items=["sa_rz"], capacity=1 << 40), -1, "a ring above 2 GiB"),
           (dict(items=[nm for nm in ctx.names if nm.startswith("C_")] + ["S_rz_init", "S_ss_init", "inf_mat_rz", "inf_pf_rz", "inf_pf_ss", "evap_soil", "transp", "q_rz", "q_ss", "cpr_rz"]), -1, "n_items = 33 (0 ... 32)"))
    for kw, code, text in bad:
        args = dict(items=["C_rz"], mask=None, capacity=2)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_totals_configure failed \(%d\)" % code) as e:
            ctx.totals_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    ctx.totals_record(tag=9)
    assert ctx.totals_count() == (2, n)
    tags, rows = ctx.totals_read(0, 2)
    assert list(tags) == [-3, 9] and rows["sa_rz"]["sum"].shape == (2, ages)
    assert same_bits(R.as_block({s: a[1] for s, a in rows["C_rz"].items()}), R.item_block(C))
    ctx.totals_configure([])
    with pytest.raises(NativeError, match=r"failed \(-3\)"):
        ctx.totals_count()
    ctx.close()


import test_host_package_sas_totals as HP  # noqa: E402

on_disk = HP.on_disk


def test_script_on_the_device_restates_the_diagnostics_of_the_same_run(on_disk, tmp_path):
    """4. A setup script with `state.transport_totals` AND `state.diagnostics` on the real SasContext, the ring shorter than the run:
    every row of `.transport_totals.nc` is the restatement applied to the fields `.collect.nc` holds for that record."""
    g, _ = HP.totals_model("sas_stats_a30", tmp_path)
    mask = np.ones((g.nx, g.ny), dtype=bool)
    mask[0, 0] = False
    g, model = HP.totals_model("sas_stats_a30", tmp_path, mask=mask, capacity=2, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    assert model.state.sas_context.totals_count() == (g.ndays + 1, g.n - 1)
    model.state.sas_context.close()
    tot, _ = HP.assert_totals_restate_the_diagnostics(tmp_path, HP.ITEMS, mask, g.ndays)
    assert tot["tt_q_ss_by_q_ss_sum"][1:].any() and tot["C_iso_q_ss_by_q_ss_count"][1:].any()


@pytest.mark.parametrize("num_proc", [(2, 1)])
def test_two_ranks_combined_are_the_single_domain_within_the_orders_bound(on_disk, tmp_path, num_proc):
    """4. Two ranks (child processes, each with its block of the grid on the device) write `.0000.nc` and `.0001.nc`;
    `sas_totals.combine` of them against the single domain: every sum within n * 2^-52 * sum|t|, counts, minima and maxima equal."""
    HP.two_ranks_against_the_single_domain(tmp_path, num_proc, False, 97)
