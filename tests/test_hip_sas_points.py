"""GPU: time series at observation columns of the SAS context (rh_sas_points_*, k_sas_points in roger_amd/csrc/rh_sas_points.h),
tolerance zero.

k_sas_points is a pure gather: behind a completed day one launch copies, for every configured array and cell, `width` doubles (1, ages
or ages + 1) into the next row of a ring on the device.  The truth is what rh_sas_download returns: position-coded arrays where no day
kernel runs, a second context WITHOUT points that steps day by day and downloads after every day where one does."""
import numpy as np
import pytest

import sas_binding as sb
from test_hip_sas import make_ctx

pytestmark = pytest.mark.gpu

GATHERED = ("C_rz", "C_iso_q_ss", "tt_q_ss", "mtt_transp", "TT_q_ss", "sa_s")     # two scalars, ages, ages, ages + 1, ages


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def coded(ctx, j, name, bump=0.0):
    """array j, cell c, age a -> j * 1e9 + c * 1e4 + a (+ bump): every term is recoverable from the value, all exact in float64."""
    shape = ctx.shape(name)
    c = np.arange(shape[0], dtype=np.float64)
    v = j * 1e9 + c * 1e4 + bump
    return v if len(shape) == 1 else v[:, None] + np.arange(shape[1], dtype=np.float64)[None, :]


@pytest.mark.parametrize("n", [5, 300])
@pytest.mark.parametrize("ages", [30, 63, 64, 255, 256, 1000])
def test_pure_gather(ages, n):
    """1. No day kernel: a vector shorter than a wavefront, ages + 1 on 64 and on 256 / 257, a ragged multi-block tail; 8 records into a
    ring of 3, one array changed between records."""
    from roger_amd._native import NativeError, SasContext

    cells = [0, 1, n - 1] + ([63, 64, 255, 256] if n == 300 else [])
    ctx = SasContext(n, ages, keep_distributions=True)
    cur = {}
    for j, name in enumerate(GATHERED):
        cur[name] = coded(ctx, j, name)
        ctx.upload(name, cur[name])
        assert same_bits(ctx.download(name), cur[name])
    assert cur["TT_q_ss"].shape == (n, ages + 1) and cur["tt_q_ss"].shape == (n, ages)
    ctx.points_configure(cells, GATHERED, capacity=3)
    assert ctx.points_count() == 0
    want = []
    for i in range(8):
        j = i % len(GATHERED)
        cur[GATHERED[j]] = coded(ctx, j, GATHERED[j], bump=0.25 * (i + 1))
        ctx.upload(GATHERED[j], cur[GATHERED[j]])
        ctx.points_record(tag=100 + i)
        want.append({v: cur[v][cells].copy() for v in GATHERED})
    assert ctx.points_count() == 8
    for first, cnt in ((5, 3), (6, 2), (7, 1), (5, 1), (8, 0)):        # (5, 3): slots 2, 0, 1 -- across the wrap
        tags, rows = ctx.points_read(first, cnt)
        assert list(tags) == [100 + k for k in range(first, first + cnt)]
        for v in GATHERED:
            assert rows[v].shape == (cnt, len(cells)) + cur[v].shape[1:], (v, rows[v].shape)
            if cnt:
                assert same_bits(rows[v], np.stack([want[k][v] for k in range(first, first + cnt)])), (v, first, cnt)
    for first in range(5):
        with pytest.raises(NativeError, match=r"rh_sas_points_read failed \(-1\).*rows %d \.\.\. 4 have been overwritten" % first):
            ctx.points_read(first, 1)
    with pytest.raises(NativeError, match=r"rh_sas_points_read failed \(-1\).*overwritten"):
        ctx.points_read(4, 4)
    with pytest.raises(NativeError, match=r"rh_sas_points_read failed \(-1\).*not been recorded"):
        ctx.points_read(7, 2)
    ctx.close()


def daily_inputs(g, st, ndays):
    """{name: (ndays, n)}: the inputs of the golden days 1 ... ndays as rows of the daily arrays."""
    rows = {k: [] for k in st.inp}
    for d in range(1, ndays + 1):
        g.load_inputs(st, d)
        for k, a in st.inp.items():
            rows[k].append(a.copy())
    return {k: np.stack(v) for k, v in rows.items()}


def held_names(ctx):
    from roger_amd._native import NativeError

    out = []
    for name in ctx.names:
        try:
            ctx.shape(name)
        except NativeError:
            continue
        out.append(name)
    return out


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_benchmark_a1000", "sas_bromide_rk4_a30"])
def test_through_the_step(case):
    """2. A: forcing_days = N, points on, run_days(0, N) in one call.  B: no points, step(d) and downloads per day.  Every recorded value
    is B's bits; A ends in B's state and outputs."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    if st.anion:
        names = ["C_q_ss", "M_rz", "tt_q_ss", "mtt_q_ss", "TT_transp", "sa_s", "msa_rz"]
    else:
        names = ["C_iso_q_ss", "C_rz", "tt_q_ss", "mtt_transp", "TT_transp", "sa_s", "sa_rz"] + (["tt50_q_ss"] if g.stats else [])
    cells = sorted({0, g.n // 2, g.n - 1})
    ctxs = []
    for _ in "AB":
        ctx = make_ctx(st, forcing_days=N)
        for k, a in st.state.items():
            ctx.upload(k, a)
        for k, a in inputs.items():
            ctx.upload(k, a)
        ctxs.append(ctx)
    A, B = ctxs
    A.points_configure(cells, names, capacity=N)
    A.run_days(0, N)
    assert A.points_count() == N
    tags, rows = A.points_read(0, N)
    assert list(tags) == list(range(N))
    for d in range(N):
        B.step(d)
        for v in names:
            truth = B.download(v)[cells]
            assert same_bits(rows[v][d], truth), (case, v, "day", d)
    for v in ("tt_q_ss", "TT_transp", "sa_s"):
        assert np.any(np.nan_to_num(rows[v]) != 0), f"{v} never held a value"
    for name in held_names(A):
        a, b = A.download(name), B.download(name)
        assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
    for ctx in ctxs:
        ctx.close()


def test_what_a_context_does_not_hold_is_refused_by_name():
    """3. keep_distributions off: scalars and the state record, tt_q_ss is refused naming keep_distributions; the int array, a daily
    input and sas_params_* are refused; so is every malformed request, and a refused call leaves the series running."""
    from roger_amd._native import NativeError, SasContext

    n, ages = 5, 30
    ctx = SasContext(n, ages, keep_distributions=False)
    for call in (ctx.points_count, lambda: ctx.points_read(0, 0), ctx.points_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_points_configure has not been called"):
            call()
    sa = np.arange(n * ages, dtype=np.float64).reshape(n, ages) + 0.5
    C = np.arange(n, dtype=np.float64) - 7.0
    ctx.upload("sa_rz", sa)
    ctx.upload("C_rz", C)
    ctx.points_configure([4, 0], ["C_rz", "sa_rz"], capacity=4)
    ctx.points_record(tag=-3)
    bad = ((dict(names=["C_rz", "tt_q_ss"]), -3, "array tt_q_ss is not held by this context (age_statistics / keep_distributions"),
           (dict(names=["tt50_q_ss"]), -3, "array tt50_q_ss is not held"),
           (dict(names=["maskCatch"]), -1, "array maskCatch is int32"),
           (dict(names=["C_rz", "transp"]), -1, "array transp is an input of the step, not a per-cell result"),
           (dict(names=["sas_params_q_ss"]), -1, "array sas_params_q_ss is an input of the step, not a per-cell result"),
           (dict(names=["C_rz", "C_ss", "C_rz"]), -1, "array C_rz is given twice"),
           (dict(cells=[0, 5]), -1, "cell 5 is outside [0, 5)"), (dict(cells=[-1]), -1, "cell -1 is outside"),
           (dict(cells=[2, 4, 2]), -1, "cell 2 is given twice"),
           (dict(capacity=0), -1, "capacity = 0"), (dict(capacity=-2), -1, "capacity = -2"),
           (dict(names=["sa_rz"], capacity=1 << 40), -1, "a ring above 2 GiB"),
           (dict(names=["sa_rz"], capacity=(1 << 31) // (ages * 8) + 1), -1, "a ring above 2 GiB"))
    for kw, code, text in bad:
        args = dict(cells=[0], names=["C_rz"], capacity=2)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_points_configure failed \(%d\)" % code) as e:
            ctx.points_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    ids = (__import__("ctypes").c_int * 1)(len(ctx.names))
    cell = np.zeros(1, dtype=np.int64)
    assert ctx._lib.rh_sas_points_configure(ctx._h, cell.ctypes.data, 1, ids, 1, 2) == -1
    assert "unknown array id %d" % len(ctx.names) in ctx._lib.rh_sas_last_error(ctx._h).decode()
    for kw, text in ((dict(cells=list(range(5)) * 52), "n_cells = 260"), (dict(names=[nm for nm in ctx.names[:40]]), "n_arrays = 40")):
        args = dict(cells=[0], names=["C_rz"], capacity=2)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_points_configure failed \(-1\)") as e:
            ctx.points_configure(**args)
        assert text in str(e.value)
    # every refusal left the series running
    ctx.points_record(tag=9)
    assert ctx.points_count() == 2
    tags, rows = ctx.points_read(0, 2)
    assert list(tags) == [-3, 9] and rows["C_rz"].shape == (2, 2) and rows["sa_rz"].shape == (2, 2, ages)
    assert same_bits(rows["C_rz"][1], C[[4, 0]]) and same_bits(rows["sa_rz"][0], sa[[4, 0]])
    ctx.close()


def small_problem():
    g = sb.SasGolden("sas_stats_a30")
    st = g.new_state()
    g.load_state(st, 0)
    g.load_inputs(st, 1)
    ctx = make_ctx(st)
    for k, a in st.state.items():
        ctx.upload(k, a)
    for k, a in st.inp.items():
        ctx.upload(k, a[None, :])
    return g, ctx


def test_switching_off_and_on_starts_at_row_0():
    """4."""
    from roger_amd._native import NativeError

    g, ctx = small_problem()
    ctx.points_configure([0, g.n - 1], ["C_rz", "tt_q_ss"], capacity=2)
    ctx.step(0)
    ctx.step(0)
    ctx.step(0)
    assert ctx.points_count() == 3
    ctx.points_configure([], [])
    ctx.step(0)                                  # (nothing to record into)
    for call in (ctx.points_count, lambda: ctx.points_read(0, 1), ctx.points_record):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.points_configure([g.n - 1], ["sa_s"], capacity=2)
    assert ctx.points_count() == 0
    ctx.step(0)
    tags, rows = ctx.points_read(0, 1)
    assert list(tags) == [0] and same_bits(rows["sa_s"][0], ctx.download("sa_s")[[g.n - 1]])
    ctx.close()


def test_stages_record_nothing():
    """5. rh_sas_stages records no row, whatever the mask; rh_sas_step does; a driver that steps by stage calls points_record."""
    from roger_amd._native import SAS_STAGES

    g, ctx = small_problem()
    ctx.points_configure([0, 1], ["C_rz", "sa_rz"], capacity=8)
    ctx.stages(0, SAS_STAGES["ALL"])
    ctx.stages(0, SAS_STAGES["INF_RZ"] | SAS_STAGES["EVAP"])
    ctx.sync()
    assert ctx.points_count() == 0
    ctx.step(0)
    assert ctx.points_count() == 1
    ctx.stages(0, SAS_STAGES["ALL"])
    ctx.points_record(tag=77)
    assert ctx.points_count() == 2
    tags, rows = ctx.points_read(0, 2)
    assert list(tags) == [0, 77]
    for v in ("C_rz", "sa_rz"):
        assert same_bits(rows[v][1], ctx.download(v)[[0, 1]]), v
    assert not same_bits(rows["sa_rz"][0], rows["sa_rz"][1])     # (two days apart: the state has aged)
    ctx.stages(0, SAS_STAGES["RESCALE"])
    ctx.sync()
    assert ctx.points_count() == 2
    ctx.close()


def test_script_on_the_device_writes_what_the_variables_held(tmp_path):
    """6. The script of tests/test_sas_points_reference.py's first test with the real SasContext."""
    import test_sas_points_reference as T
    from roger_amd import runtime_settings as rs

    prev = rs.diskless_mode
    object.__setattr__(rs, "diskless_mode", False)
    try:
        g, _ = T.points_model("sas_stats_a30", tmp_path, None)
        cells = T.corners(g)
        g, model = T.points_model("sas_stats_a30", tmp_path, cells, capacity=4)
        model.setup()
        model.warmup(repeat=0)
        first = (0, 0, {v: T.held(model.state, v, cells) for v in T.VARS})
        notes = T.run_and_note(model, cells, T.VARS)
        assert len(notes) == g.ndays and model.state.sas_context.points_count() == g.ndays + 1
        data, dims = T.assert_file_holds(tmp_path, first, notes, T.VARS)
        assert dims["TT_transp"] == ("Time", "point", "nages") and dims["C_rz"] == ("Time", "point")
        for v in T.VARS:
            assert np.any(np.nan_to_num(data[v][1:]) != 0), v
        model.state.sas_context.close()
    finally:
        object.__setattr__(rs, "diskless_mode", prev)
