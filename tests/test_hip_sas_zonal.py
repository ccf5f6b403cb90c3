"""GPU: zonal totals of the SAS context (rh_sas_zonal_*, kernels in roger_amd/csrc/rh_sas_zonal.h), tolerance zero.

The truth is the SHIPPED rule of the catchment totals, tests/sas_totals_reference.py: the block of zone z must be
item_block(values, weight, zone == z) -- applied to what was uploaded where no day kernel runs, and to the downloads of a second context
WITHOUT recorders that steps day by day where one does.  tests/test_sas_zonal_reference.py shows that these inputs and zone maps can
tell a wrong order of summation from the right one."""
import numpy as np
import pytest

import sas_binding as sb
import sas_totals_reference as R
import sas_zonal_reference as Z
from test_hip_sas import make_ctx
from test_hip_sas_points import daily_inputs, held_names, same_bits
from test_hip_sas_totals import key_of, pure_context, step_items

pytestmark = pytest.mark.gpu

IDENTITY = [0.0, 0.0, 0.0, np.inf, -np.inf]
DAYS = (0, 1, 2, 4, -1)            # day 4: row 1 of the 3-row daily inputs; -1: no daily row


def want_blocks(d, items, zone, nz, day, cache=None, version=None):
    """{item: [block of zone z for z in 0 ... nz - 1]} by the totals' rule with mask = (zone == z)."""
    out = {}
    r = day % 3 if day >= 0 else None
    for it in items:
        v, w = (it, None) if isinstance(it, str) else it
        live = day >= 0 or (w is None and v not in R.DAILY)
        daily = v in R.DAILY or w is not None
        key = (key_of(it), r if (daily and live) else None, live, None if version is None else version.get(v, 0))
        if cache is None or key not in cache:
            val = d[v][r if r is not None else 0] if v in R.DAILY else d[v]
            wt = None if w is None else d[w][r if r is not None else 0]
            blocks = [R.item_block(val, wt, zone == z, live) for z in range(nz)]
            if cache is None:
                out[key_of(it)] = blocks
                continue
            cache[key] = blocks
        out[key_of(it)] = cache[key]
    return out


def assert_rows(rows, k, want, what):
    for key, blocks in want.items():
        got = Z.as_blocks(rows[key], k)
        for z, block in enumerate(blocks):
            assert same_bits(got[z], block), (what, key, z, got[z][:6], block[:6])


@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 300])
@pytest.mark.parametrize("ages", [30, 64, 256, 1000])
def test_pure_reduction(ages, n):
    """1. No day kernel.  ages + 1 crosses one to four chunks of lanes; n below, on and above one tile; every map; a zone without a cell
    records the identity block."""
    ctx, d = pure_context(n, ages)
    for mname, (zone, nz) in Z.zone_maps(n).items():
        ctx.zonal_configure(R.ITEMS, zone, nz, capacity=8)
        rows_total, ncells = ctx.zonal_count()
        assert rows_total == 0 and list(ncells) == list(np.bincount(zone[zone >= 0], minlength=nz))
        for i, day in enumerate(DAYS):
            ctx.zonal_record(tag=50 + i, day=day)
        tags, rows = ctx.zonal_read(0, len(DAYS))
        assert list(tags) == [50 + i for i in range(len(DAYS))]
        cache = {}
        for i, day in enumerate(DAYS):
            assert_rows(rows, i, want_blocks(d, R.ITEMS, zone, nz, day, cache), (n, ages, mname, day))
        empty = int(np.flatnonzero(ncells == 0)[0])
        for i in range(len(DAYS)):
            assert list(Z.as_blocks(rows["C_rz"], i)[empty]) == IDENTITY
            blk = Z.as_blocks(rows["tt_q_ss_by_q_ss"], i)[empty]
            assert same_bits(blk, np.zeros(2 + ages)), (mname, i)
        assert not rows["C_in"]["count"][4].any() and not rows["tt_q_ss_by_q_ss"]["sum"][4].any()
        assert list(rows["C_rz"]["count"][4]) == list(ncells) == list(rows["sa_s"]["count"][4])
    ctx.close()


def test_the_many_zones_map():
    """1. 300 zones over 1000 cells: about a cell per slot, more slots than cells in a tile's wavefront."""
    n, ages = 1000, 30
    ctx, d = pure_context(n, ages)
    zone, nz = Z.zone_maps(n)["many"]
    items = ("C_rz", ("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s")
    ctx.zonal_configure(items, zone, nz, capacity=2)
    ctx.zonal_record(tag=1, day=1)
    ctx.zonal_record(tag=2, day=-1)
    _, rows = ctx.zonal_read(0, 2)
    assert_rows(rows, 0, want_blocks(d, items, zone, nz, 1), "many")
    assert_rows(rows, 1, want_blocks(d, items, zone, nz, -1), "many, no daily row")
    ctx.close()


def test_three_levels_and_the_ring():
    """2. n = 65 837: three levels of the age rule, a ragged last tile, a second round of accumulators; the `sparse` map has a zone that
    lives beyond cell 65 536 only.  8 records into a ring of 3, one array changed between records."""
    from roger_amd._native import NativeError

    n, ages = 65837, 30
    ctx, d = pure_context(n, ages)
    items = ("C_rz", ("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), "sa_s", ("TT_q_ss", "transp"))
    maps = Z.zone_maps(n)
    for mname in ("mix", "blocks"):
        zone, nz = maps[mname]
        ctx.zonal_configure(items, zone, nz, capacity=3)
        ctx.zonal_record(tag=0, day=2)
        assert_rows(ctx.zonal_read(0, 1)[1], 0, want_blocks(d, items, zone, nz, 2), mname)
    zone, nz = maps["sparse"]
    ctx.zonal_configure(items, zone, nz, capacity=3)
    want, cache, version = [], {}, {}
    for i in range(8):
        name = ("C_rz", "sa_s")[i % 2]
        d[name] = d[name] * 1.25 + 0.5
        version[name] = i
        ctx.upload(name, d[name])
        ctx.zonal_record(tag=100 + i, day=i)
        want.append(want_blocks(d, items, zone, nz, i, cache, version))
    assert ctx.zonal_count()[0] == 8
    for first, cnt in ((5, 3), (6, 2), (7, 1), (5, 1), (8, 0)):        # (5, 3): slots 2, 0, 1 -- across the wrap
        tags, rows = ctx.zonal_read(first, cnt)
        assert list(tags) == [100 + k for k in range(first, first + cnt)]
        assert rows["sa_s"]["sum"].shape == (cnt, nz, ages) and rows["C_rz"]["sum"].shape == (cnt, nz)
        for k in range(cnt):
            assert_rows(rows, k, want[first + k], (first, cnt, k))
    for first in range(5):
        with pytest.raises(NativeError, match=r"rh_sas_zonal_read failed \(-1\).*rows %d \.\.\. 4 have been overwritten" % first):
            ctx.zonal_read(first, 1)
    with pytest.raises(NativeError, match=r"rh_sas_zonal_read failed \(-1\).*overwritten"):
        ctx.zonal_read(4, 4)
    with pytest.raises(NativeError, match=r"rh_sas_zonal_read failed \(-1\).*not been recorded"):
        ctx.zonal_read(7, 2)
    ctx.close()


def test_a_zone_is_the_shipped_recorder_with_that_mask():
    """3. One context, both recorders: for three zones of the `mix` map totals_configure(items, zone == z) + totals_record give the bits
    of zone z's block."""
    n, ages = 65837, 30
    ctx, _ = pure_context(n, ages)
    zone, nz = Z.zone_maps(n)["mix"]
    ctx.zonal_configure(R.ITEMS, zone, nz, capacity=1)
    ctx.zonal_record(tag=0, day=1)
    _, rows = ctx.zonal_read(0, 1)
    for z in (0, 2, nz - 1):
        ctx.totals_configure(R.ITEMS, zone == z, capacity=1)
        ctx.totals_record(tag=0, day=1)
        _, tot = ctx.totals_read(0, 1)
        for key, stats in tot.items():
            assert same_bits(Z.as_blocks(rows[key], 0)[z], R.as_block({s: a[0] for s, a in stats.items()})), (z, key)
    ctx.close()


@pytest.mark.parametrize("case", ["sas_stats_a30", "sas_mixed_a70", "sas_bromide_rk4_a30", "sas_benchmark_a1000"])
def test_through_the_step(case):
    """4. A: the recorder on, run_days(0, N) in one call.  B: no recorder, step(d) and downloads per day, restated.  Every recorded value
    is B's bits and A ends in B's state.  C, D, E: points, totals and zonal totals together, configured in three orders, record the rows
    of each alone -- the points' and the totals' restated from B as well."""
    g = sb.SasGolden(case)
    N = min(g.ndays, 4)
    st = g.new_state()
    g.load_state(st, 0)
    inputs = daily_inputs(g, st, N)
    items = step_items(st, g.stats)
    zone = (np.arange(g.n) % 3).astype(np.int32)
    zone[zone == 1] = 2 if g.n > 2 else 1                       # (n_zones = 4: ids 1 and 3 without a cell where n > 2)
    if g.n > 4:
        zone[3] = -1
    nz = 4
    mask = np.arange(g.n) % 4 != 1 if g.n > 2 else None
    pnames, cells = ["C_rz", "tt_q_ss", "sa_s"], sorted({0, g.n - 1})
    ctxs = []
    for _ in "ABCDE":
        ctx = make_ctx(st, forcing_days=N)
        for k, a in st.state.items():
            ctx.upload(k, a)
        for k, a in inputs.items():
            ctx.upload(k, a)
        ctxs.append(ctx)
    A, B, C, D, E = ctxs
    A.zonal_configure(items, zone, nz, capacity=N)
    C.points_configure(cells, pnames, capacity=N)
    C.totals_configure(items, mask, capacity=N)
    C.zonal_configure(items, zone, nz, capacity=N)
    D.zonal_configure(items, zone, nz, capacity=N)
    D.totals_configure(items, mask, capacity=N)
    D.points_configure(cells, pnames, capacity=N)
    E.totals_configure(items, mask, capacity=N)
    E.zonal_configure(items, zone, nz, capacity=N)
    E.points_configure(cells, pnames, capacity=N)
    for ctx in (A, C, D, E):
        ctx.run_days(0, N)
    assert A.zonal_count()[0] == N
    tags, rows = A.zonal_read(0, N)
    assert list(tags) == list(range(N))
    together = [(ctx.zonal_read(0, N)[1], ctx.totals_read(0, N)[1], ctx.points_read(0, N)[1]) for ctx in (C, D, E)]
    for d in range(N):
        B.step(d)
        held = {v: (inputs[v][d] if v in inputs else B.download(v)) for v in {x for it in items for x in ((it,) if isinstance(it, str) else it)}}
        want = {key_of(it): [R.item_block(held[it if isinstance(it, str) else it[0]], None if isinstance(it, str) else inputs[it[1]][d], zone == z)
                             for z in range(nz)] for it in items}
        assert_rows(rows, d, want, (case, "day", d))
        alone = {key_of(it): R.item_block(held[it if isinstance(it, str) else it[0]], None if isinstance(it, str) else inputs[it[1]][d], mask)
                 for it in items}
        for zr, tr, pr in together:
            assert_rows(zr, d, want, (case, "together", d))
            for key, block in alone.items():
                assert same_bits(R.as_block({s: a[d] for s, a in tr[key].items()}), block), (case, "totals beside", key, d)
            for v in pnames:
                assert same_bits(pr[v][d], B.download(v)[cells]), (case, "points beside", v, d)
    assert rows[key_of(items[2])]["sum"].any() and rows["sa_s"]["sum"].any() and rows[key_of(items[0])]["count"].any()
    for name in held_names(A):
        a, b = A.download(name), B.download(name)
        assert a.dtype == b.dtype and (same_bits(a, b) if a.dtype.kind == "f" else (a == b).all()), (case, name)
    # switched off, the others go on
    C.zonal_configure([])
    C.totals_record(tag=7, day=N - 1)
    assert C.totals_count()[0] == N + 1
    for ctx in ctxs:
        ctx.close()


def test_refusals_name_the_offender_and_leave_the_series_running():
    """5. The argument errors of rh_sas_zonal_configure; the four entry points before it was called."""
    from roger_amd._native import NativeError, SasContext

    n, ages = 5, 30
    ctx = SasContext(n, ages, keep_distributions=False)
    for call in (ctx.zonal_count, lambda: ctx.zonal_read(0, 0), ctx.zonal_record):
        with pytest.raises(NativeError, match=r"failed \(-3\).*rh_sas_zonal_configure has not been called"):
            call()
    C = np.arange(n, dtype=np.float64) - 7.0
    ctx.upload("C_rz", C)
    zone = np.array([0, 1, -1, 1, 0], dtype=np.int32)
    ctx.zonal_configure(["C_rz", "sa_rz"], zone, 3, capacity=4)
    ctx.zonal_record(tag=-3)
    bad = ((dict(items=["C_rz", "tt_q_ss"]), -3, "array tt_q_ss is not held by this context (age_statistics / keep_distributions"),
           (dict(items=["maskCatch"]), -1, "array maskCatch is int32"),
           (dict(items=["sas_params_q_ss"]), -1, "array sas_params_q_ss is a parameter block"),
           (dict(items=["C_rz", ("C_rz", "q_ss"), "C_rz"]), -1, "array C_rz is given twice with the same weight"),
           (dict(items=[("C_rz", "C_in")]), -1, "weight C_in is not a daily flux input"),
           (dict(n_zones=0), -1, "n_zones = 0 (1 ... 1024)"),
           (dict(n_zones=1025), -1, "n_zones = 1025 (1 ... 1024)"),
           (dict(n_zones=1), -1, "zone id 1 of cell 1 (-1: outside, else 0 ... 0)"),
           (dict(zones=np.array([0, 1, -2, 1, 0], dtype=np.int32)), -1, "zone id -2 of cell 2"),
           (dict(zones=np.full(n, -1, dtype=np.int32)), -1, "the map holds no cell in any zone (0 of 5 cells)"),
           (dict(capacity=0), -1, "capacity = 0"),
           (dict(items=["sa_rz"], capacity=1 << 40), -1, "a ring above 2 GiB"),
           (dict(items=[nm for nm in ctx.names if nm.startswith("C_")] + ["S_rz_init", "S_ss_init", "inf_mat_rz", "inf_pf_rz", "inf_pf_ss", "evap_soil", "transp", "q_rz", "q_ss", "cpr_rz"]), -1, "n_items = 33 (0 ... 32)"))
    for kw, code, text in bad:
        args = dict(items=["C_rz"], zones=zone, n_zones=3, capacity=2)
        args.update(kw)
        with pytest.raises(NativeError, match=r"rh_sas_zonal_configure failed \(%d\)" % code) as e:
            ctx.zonal_configure(**args)
        assert text in str(e.value), (text, str(e.value))
    ctx.zonal_record(tag=9)
    rows_total, ncells = ctx.zonal_count()
    assert rows_total == 2 and list(ncells) == [2, 2, 0]
    tags, rows = ctx.zonal_read(0, 2)
    assert list(tags) == [-3, 9] and rows["sa_rz"]["sum"].shape == (2, 3, ages)
    for z in range(3):
        assert same_bits(Z.as_blocks(rows["C_rz"], 1)[z], R.item_block(C, None, zone == z))
    ctx.zonal_configure([])
    with pytest.raises(NativeError, match=r"failed \(-3\)"):
        ctx.zonal_count()
    ctx.close()


import test_host_package_sas_zonal as HZ  # noqa: E402

on_disk = HZ.on_disk


def test_script_on_the_device_restates_the_diagnostics_of_the_same_run(on_disk, tmp_path):
    """6. A setup script with `state.transport_zonal_totals` AND `state.diagnostics` on the real SasContext, the ring shorter than the
    run: every block of `.transport_zonal_totals.nc` is the totals' rule applied to the fields `.collect.nc` holds for that record."""
    g, _ = HZ.zonal_model("sas_stats_a30", tmp_path)
    zones = HZ.zone_map(g)
    g, model = HZ.zonal_model("sas_stats_a30", tmp_path, zones=zones, capacity=2, diagnose=True)
    model.setup()
    model.warmup(repeat=0)
    model.run()
    rows_total, ncells = model.state.sas_context.zonal_count()
    assert rows_total == g.ndays + 1 and list(ncells) == [int((zones == i).sum()) for i in (3, 7, 12)]
    model.state.sas_context.close()
    zon, _ = HZ.assert_zonal_restate_the_diagnostics(tmp_path, HZ.ITEMS, zones, g.ndays)
    assert zon["tt_q_ss_by_q_ss_sum"][1:].any() and zon["C_iso_q_ss_by_q_ss_count"][1:].any()


@pytest.mark.parametrize("num_proc", [(2, 1)])
def test_two_ranks_combined_are_the_single_domain_within_the_orders_bound(on_disk, tmp_path, num_proc):
    """7. Two ranks (child processes, each with its block of the grid on the device) write `.0000.nc` and `.0001.nc`;
    `sas_zonal_totals.combine` of them against the single domain: every sum within n * 2^-52 * sum|t|, counts, minima and maxima equal."""
    HZ.two_ranks_against_the_single_domain(tmp_path, num_proc, False, 43)
