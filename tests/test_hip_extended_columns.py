"""The columns of tests/extended_columns.py through the kernels: water land uses (lu_id 14 / 20 / 999: columns the setup kernels take out
of the catchment), every land use of the tables, groundwater within reach of the soil ("mixed"), water in the depressions.  Needs a
real MI355X: `pytest -m gpu`.  tests/test_physics_host_vs_oracle.py compares the same column code with the oracle routine by routine on
the CPU; here the real kernels run it, over 1 000 columns = 15 full wavefronts and one of 40 lanes, in two layouts:

  interleaved   the land uses cycle over the columns: every wavefront is mixed
  blocks        wavefronts 0-4 are whole: all lakes, all rivers, all outside the catchment, all sealed (lu_id 0), all identical columns
                of lu_id 8 with the groundwater at 3 m -- the wave votes (RH_WAVE_ALL, the dry paths) and the per-wave parameter words
                are then taken over lanes that are all masked / all alike; the rest is interleaved

The run: 12 days of the combo forcing (all step classes) starting on 29 April, so the third day changes the month."""
import functools

import numpy as np
import pytest

import extended_columns as E
from golden_util import ATOL, RTOL, compare, compare_bulk, load_case

pytestmark = pytest.mark.gpu

NX, NY = 40, 25
N = NX * NY
SEED = E.RUN_SEED
NDAYS = 12
LAYOUTS = ("interleaved", "blocks")


@pytest.fixture(scope="module")
def native():
    from roger_amd import _native as N_

    N_.load()
    return N_


def _luts(lateral):
    g, _, _ = load_case("svat_hetero_combo")
    luts = (g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    if lateral:
        luts += (load_case("oned_hetero_combo")[0]["lut_mlms"],)
    return luts


def _context(native, lateral, snapshot, names, scal_row):
    import hip_util as H

    luts = _luts(lateral)
    ctx = native.Context(NX, NY, enable_lateral_flow=int(lateral))
    H.upload_snapshot(ctx, snapshot, names)
    ctx.set_scalars(H.scalars_from_row(scal_row))
    ctx.set_luts(*luts[:4])
    if lateral:
        ctx.set_lut_mlms(luts[4])
    return ctx


@functools.lru_cache(maxsize=None)
def oracle_run(layout, lateral):
    """The oracle's free run, computed once and left unchanged: the start, the state before and after about 20 steps spread over the
    run with every step class among them (the first step of a rain event, a daily step, the month change), and the end."""
    import oracle_binding as ob

    ob.build()
    st = E.run_start(ob, NX, NY, SEED, "mixed", layout, _luts(lateral), lateral)
    names = list(st.names)
    F = E.run_forcing(NDAYS)
    drv = ob.ForcingDriver(F)
    run = dict(names=names, F=F, start=(st.snapshot(), st.scalars_row()), pairs=[], kinds=set(), lu=st.planes["lu_id"].copy(),
               mask=st.planes["maskCatch"].copy())
    seen = {}
    step = 0
    while st.scal.time < NDAYS * 86400:
        step += 1
        before = (st.snapshot(), st.scalars_row())
        event_before = int(st.scal.event_id[1])
        pd, td, ed, monthly = drv.before_step(st)
        ok = st.step(pd, td, ed, monthly)
        kind = (int(st.scal.dt_secs), event_before == 0 and int(st.scal.event_id[0]) >= 1, bool(monthly))
        seen[kind] = seen.get(kind, 0) + 1
        if seen[kind] <= 2 or step % 12 == 0:
            run["pairs"].append((step, before, (st.snapshot(), st.scalars_row(), int(ok))))
            run["kinds"].add(kind)
    run["end"] = (st.snapshot(), st.scalars_row())
    run["nsteps"] = step
    for a in [run["start"][0], run["end"][0], run["lu"], run["mask"]] + [x for _, b, c in run["pairs"] for x in (b[0], b[1], c[0], c[1])]:
        a.setflags(write=False)
    return run


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
def test_setup_kernels_take_the_water_columns_out_of_the_catchment(native, oracle, lateral):
    """rh_topo ... rh_initial_conditions on the device from the primaries: the masks exactly, every plane as the oracle's kernels leave it."""
    import hip_util as H

    p = E.extended_params(NX, NY, SEED, "mixed", "blocks")
    luts = _luts(lateral)
    st = oracle.OracleState(N)
    E.load_primaries(st, p, luts, lateral)
    names = list(st.names)
    ctx = _context(native, lateral, st.snapshot(), names, st.scalars_row())
    st.topo()
    st.params_surface()
    st.params_soil()
    for entry in ("rh_topo", "rh_params_surface", "rh_params_soil"):
        ctx.call(entry)
    if lateral:
        st.params_lateral(luts[4])
        ctx.call("rh_params_lateral")
    E.load_initial_state(st, p)
    for nm in ("theta_rz", "theta_rz_m1", "theta_ss", "theta_ss_m1", "S_dep", "S_dep_m1"):
        ctx.upload(nm, st.planes[nm])
    st.initial_conditions()
    ctx.call("rh_initial_conditions")
    for mask in ("maskCatch", "maskRiver", "maskLake"):
        np.testing.assert_array_equal(ctx.download(mask), st.planes[mask], err_msg=mask)
    water = np.isin(st.planes["lu_id"], E.LU_WATER)
    assert water.sum() >= 3 * E.BLOCK + 60 and (st.planes["maskCatch"][water] == 0).all() and (st.planes["maskCatch"][~water] == 1).all()
    compare(H.download_snapshot(ctx, names), st.snapshot(), names, what="setup kernels")
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_steps_from_the_oracles_states(native, oracle, layout, lateral):
    """One fused step from the oracle's state k-1 gives the oracle's state k: every plane at RTOL / ATOL, the scalar row and sanity_ok
    exactly."""
    import hip_util as H

    run = oracle_run(layout, lateral)
    names, F = run["names"], run["F"]
    assert 16 <= len(run["pairs"]) <= 30, len(run["pairs"])
    assert {k[0] for k in run["kinds"]} == {600, 3600, 86400}                 # every step class,
    assert any(k[1] for k in run["kinds"]) and any(k[2] for k in run["kinds"])   # the first step of a rain event, the month change
    ctx = _context(native, lateral, run["start"][0], names, run["start"][1])
    for step, (snap0, row0), (snap1, row1, ok) in run["pairs"]:
        H.upload_snapshot(ctx, snap0, names)
        ctx.set_scalars(H.scalars_from_row(row0))
        s = ctx.get_scalars()
        if s.time % 86400:   # mid-day: hand over the forcing the oracle took at midnight
            i0 = s.itt_forc - 144
            ctx.set_forcing_day(*[F[v][i0:i0 + 144] for v in ("PREC", "TA", "PET")])
        monthly = H.HipForcingDriver(ctx, F).before_step()
        ctx.step(monthly)
        s = ctx.get_scalars()
        np.testing.assert_array_equal(H.scalars_to_row(s), row1, err_msg=f"{layout} step {step}")
        assert int(s.sanity_ok) == ok, f"{layout} step {step}: sanity_ok {s.sanity_ok}, the oracle's {ok}"
        compare(H.download_snapshot(ctx, names), snap1, names, rtol=RTOL, atol=ATOL, what=f"{layout} single step {step}")
    ctx.close()


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return a == b


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
def test_run_steps_over_whole_wavefronts_of_one_kind_equals_the_routine_path(native, oracle, lateral):
    """Layout "blocks": ONE rh_run_steps call over the whole run (an eager first step, then the lazy pipelines with the per-wave
    parameter words and the dry-path votes) leaves every plane, bit for bit and NaN for NaN, and the scalars as the same steps driven
    routine by routine (rh_adaptive_dt + rh_params_surface at the month change + rh_step_core + rh_after_timestep)."""
    import hip_util as H

    run = oracle_run("blocks", lateral)
    names, F = run["names"], run["F"]
    assert (run["mask"][:3 * E.BLOCK] == 0).all() and (run["lu"][3 * E.BLOCK:4 * E.BLOCK] == 0).all()    # the layout is what the docstring says
    ref = _context(native, lateral, run["start"][0], names, run["start"][1])
    held = [nm for nm, _ in ref.planes[: ref.planes_held]]
    nsteps, months = 0, 0
    while True:
        s = ref.get_scalars()
        if s.time >= NDAYS * 86400:
            break
        if s.time % 86400 == 0:
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(F["YEAR"][i]), int(F["MONTH"][i]), int(F["DOY"][i])
            s.itt_forc = i + 144
            ref.set_scalars(s)
            ref.set_forcing_day(*[F[v][i:i + 144] for v in ("PREC", "TA", "PET")])
        ref.call("rh_adaptive_dt")
        if (s.month[1] != s.month[0]) and (s.itt > 1):
            ref.call("rh_params_surface")
            months += 1
        ref.call("rh_step_core")
        ref.call("rh_after_timestep")
        nsteps += 1
        assert nsteps <= 400
    assert nsteps == run["nsteps"] and months == 1, (nsteps, run["nsteps"], months)
    want_scal = H.scalars_to_row(ref.get_scalars())
    want = {nm: ref.download(nm) for nm in held}
    ref.close()

    ctx = _context(native, lateral, run["start"][0], names, run["start"][1])
    ctx.set_forcing_series(F)
    ctx.run_steps(nsteps)
    s = ctx.get_scalars()
    assert ctx.sparse_steps() > nsteps // 2, ctx.sparse_steps()   # (the lazy sparse kernel ran)
    np.testing.assert_array_equal(H.scalars_to_row(s), want_scal)
    np.testing.assert_array_equal(want_scal, run["end"][1])
    for nm in held:
        got = ctx.download(nm)
        ok = same_bits(got, want[nm])
        assert ok.all(), (nm, np.flatnonzero(~ok)[:10], got[~ok][:5], want[nm][~ok][:5])
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_svat_free_run_against_the_oracle(native, oracle, layout):
    """As test_hip_parity.py::test_vs_oracle_hetero_4096, on these columns: the HIP path tracks the oracle over the 12 days
    (tests/test_physics_host_vs_oracle.py runs the same comparison with the host-compiled core and stays inside the same bounds)."""
    import hip_util as H

    run = oracle_run(layout, False)
    names, F = run["names"], run["F"]
    checks = {step: after for step, _, after in run["pairs"]}
    ctx = _context(native, False, run["start"][0], names, run["start"][1])
    hdrv = H.HipForcingDriver(ctx, F)
    for step in range(1, run["nsteps"] + 1):
        ctx.step(hdrv.before_step())
        if step in checks:
            snap, row, ok = checks[step]
            s = ctx.get_scalars()
            np.testing.assert_array_equal(H.scalars_to_row(s), row, err_msg=f"step {step}")
            assert int(s.sanity_ok) == ok
            compare_bulk(H.download_snapshot(ctx, names), snap, names, what=f"{layout} step {step}")
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), run["end"][1])
    compare_bulk(H.download_snapshot(ctx, names), run["end"][0], names, what=f"{layout} final")
    assert run["nsteps"] > 100
    ctx.close()
