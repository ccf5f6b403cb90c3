"""The crop columns of tests/crop_columns.py (lu_id 500-599) through the kernels.  Needs a real MI355X: `pytest -m gpu`.
tests/test_physics_host_vs_oracle_crops.py compares the same column code with the oracle routine by routine on the CPU and holds the
census of the branches; here the real kernels run it, over 1 000 columns = 15 full wavefronts and one of 40 lanes, in two layouts:

  interleaved   two columns of three are crops (500, 501, 510, 550, 597, 598, 599 in turn), the third an ordinary or a water land use
  blocks        wavefronts 0-4 are whole: all 550 and saturated (every lane takes the anoxia branch, transp_coeff 0), all 599, all 500,
                all 550 with identical primaries (the per-wave parameter words over crop lanes), and one of 32 lanes of 550 followed by
                32 of lu_id 8 (the anoxia `if` diverges inside the wave); the rest is interleaved

and from two start states: "as_set_up" (the setup kernels' planes: anoxia is the only way a crop transpires) and "grown" (ground cover,
basal coefficients, ground storage, ground throughfall and a carried k_stress_transp overwritten on the crop columns, the same values
in the oracle's state and uploaded to the context).

The run: 12 days of the combo forcing starting on 29 April.  The first two steps are daily steps with snowfall; the third changes the
month, and rt_params_surface puts the crops' planes back to the set-up values on both sides -- k_stress_transp excepted, which no setup
kernel writes: a crop column holds min(uploaded value, 1) to the end of the run, and that is asserted from the inputs."""
import functools

import numpy as np
import pytest

import crop_columns as CC
import extended_columns as E
from golden_util import ATOL, RTOL, compare, compare_bulk, load_case

pytestmark = pytest.mark.gpu

NX, NY = 40, 25
N = NX * NY
SEED = CC.RUN_SEED
NDAYS = 12
LAYOUTS = ("interleaved", "blocks")
TA_FM = 0.0


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


def pair_census(names, before, after, monthly):
    """The crop branches one step of the oracle took, from its states before and after the step (interception and evapotranspiration
    read theta_rz, the ground storage and the snow cover as the step found them; prec and ta are the step's own)."""
    b = {k: before[names.index(k)] for k in ("lu_id", "theta_rz", "theta_sat", "S_int_ground", "S_int_ground_tot", "S_snow")}
    a = {k: after[names.index(k)] for k in ("transp", "prec", "ta", "int_rain_ground", "int_rain_top", "int_snow_ground", "int_snow_top")}
    lu = b["lu_id"]
    anoxic = (lu > 500) & (lu < 599) & (b["theta_rz"] >= 0.8 * b["theta_sat"])
    out = dict(anoxic_transp=int((anoxic & (a["transp"] > 0)).sum()), ground_599_blocked=0, partial_throughfall=0)
    if not monthly:     # (a monthly step recomputes the ground storage's capacity before it intercepts)
        wet, liquid = a["prec"] > 0, a["ta"] > TA_FM
        room = b["S_int_ground"] < b["S_int_ground_tot"]
        out["ground_599_blocked"] = int(((lu == 599) & wet & room & (~liquid | (b["S_snow"] <= 0))).sum())
        got = np.where(liquid, a["int_rain_ground"], a["int_snow_ground"])
        fell = a["prec"] - np.where(liquid, a["int_rain_top"], a["int_snow_top"])
        out["partial_throughfall"] = int((CC.is_crop(lu) & (lu < 598) & wet & (got > 0) & (got < fell)).sum())
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(layout, lateral, start):
    """The oracle's free run, computed once and left unchanged: the start, the state before and after about 20 steps spread over the
    run with every step class among them (the first step of a rain event, a daily step, the month change), and the end."""
    import oracle_binding as ob

    ob.build()
    st = CC.crop_start(ob, NX, NY, SEED, layout, _luts(lateral), lateral, start, month=E.START_MONTH)
    names = list(st.names)
    F = E.run_forcing(NDAYS)
    drv = ob.ForcingDriver(F)
    run = dict(names=names, F=F, start=(st.snapshot(), st.scalars_row()), pairs=[], kinds=set(), lu=st.planes["lu_id"].copy(),
               mask=st.planes["maskCatch"].copy(), k_stress0=st.planes["k_stress_transp"].copy(),
               census=dict(anoxic_transp=0, ground_599_blocked=0, partial_throughfall=0), month_step=None)
    seen = {}
    step = 0
    while st.scal.time < NDAYS * 86400:
        step += 1
        before = (st.snapshot(), st.scalars_row())
        event_before = int(st.scal.event_id[1])
        pd, td, ed, monthly = drv.before_step(st)
        ok = st.step(pd, td, ed, monthly)
        if monthly and run["month_step"] is None:
            run["month_step"] = step
        kind = (int(st.scal.dt_secs), event_before == 0 and int(st.scal.event_id[0]) >= 1, bool(monthly))
        seen[kind] = seen.get(kind, 0) + 1
        if seen[kind] <= 2 or step % 12 == 0:
            after = st.snapshot()
            run["pairs"].append((step, before, (after, st.scalars_row(), int(ok))))
            run["kinds"].add(kind)
            for k, v in pair_census(names, before[0], after, monthly).items():
                run["census"][k] += int(v > 0)
    run["end"] = (st.snapshot(), st.scalars_row())
    run["nsteps"] = step
    for a in [run["start"][0], run["end"][0], run["lu"], run["mask"], run["k_stress0"]] + [x for _, b, c in run["pairs"] for x in (b[0], b[1], c[0], c[1])]:
        a.setflags(write=False)
    return run


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def carried(k0):
    """What a crop column's k_stress_transp holds after any number of steps: min(value at the start, 1)."""
    return np.where(k0 > 1, 1.0, k0)


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
def test_setup_kernels_on_crop_columns(native, oracle, lateral):
    """rh_topo ... rh_initial_conditions on the device from the primaries, layout "blocks": the masks exactly, every plane as the
    oracle's kernels leave it; the crops' root depth and ground throughfall from the primaries alone."""
    import hip_util as H

    p = CC.crop_params(NX, NY, SEED, "blocks")
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
    lu = p["lu_id"].ravel()
    crop = CC.is_crop(lu)
    assert crop.sum() >= 0.6 * N and (st.planes["maskCatch"][crop] == 1).all()
    np.testing.assert_array_equal(ctx.download("z_root")[crop], np.minimum(200.0, 0.9 * p["z_soil"].ravel())[crop])
    np.testing.assert_array_equal(ctx.download("throughfall_coeff_ground"), np.where((lu >= 500) & (lu <= 597), 1.0, 0.0))
    compare(H.download_snapshot(ctx, names), st.snapshot(), names, what="setup kernels")
    ctx.close()


@pytest.mark.parametrize("start", CC.STARTS)
@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_steps_from_the_oracles_states(native, oracle, layout, lateral, start):
    """One fused step from the oracle's state k-1 gives the oracle's state k: every plane at RTOL / ATOL, the scalar row and sanity_ok
    exactly.  Among the pairs, counted from the oracle's states: a step in which an anoxic crop transpires and, from "grown", one in
    which lu_id 599 keeps its ground storage shut and one with a partial ground throughfall."""
    import hip_util as H

    run = oracle_run(layout, lateral, start)
    names, F = run["names"], run["F"]
    assert 16 <= len(run["pairs"]) <= 30, len(run["pairs"])
    assert {k[0] for k in run["kinds"]} == {600, 3600, 86400}                 # every step class,
    assert any(k[1] for k in run["kinds"]) and any(k[2] for k in run["kinds"])   # the first step of a rain event, the month change
    print("PAIRS", layout, lateral, start, len(run["pairs"]), run["census"])
    assert run["census"]["anoxic_transp"] > 0, run["census"]
    if start == "grown":
        assert run["census"]["ground_599_blocked"] > 0 and run["census"]["partial_throughfall"] > 0, run["census"]
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
        compare(H.download_snapshot(ctx, names), snap1, names, rtol=RTOL, atol=ATOL, what=f"{layout} {start} single step {step}")
    ctx.close()


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
def test_run_steps_carries_k_stress_transp_and_equals_the_routine_path(native, oracle, lateral):
    """Layout "blocks", "grown": ONE rh_run_steps call over the whole run (an eager first step, then the lazy pipelines, most of them
    sparse: the only ones with a store set of their own) leaves every plane, bit for bit and NaN for NaN, and the scalars as the same
    steps driven routine by routine (rh_adaptive_dt + rh_params_surface at the month change + rh_step_core + rh_after_timestep).
    The same run split before the month change and at its end: a crop column's k_stress_transp is min(uploaded value, 1), bit for
    bit -- from the inputs, so a pipeline that stopped loading the plane fails here even where both device paths agree."""
    import hip_util as H

    run = oracle_run("blocks", lateral, "grown")
    names, F = run["names"], run["F"]
    lu, k0 = run["lu"], run["k_stress0"]
    crop = CC.is_crop(lu)
    assert (lu[:CC.BLOCK] == 550).all() and (lu[CC.BLOCK:2 * CC.BLOCK] == 599).all() and (lu[CC.UNIFORM] == 550).all()    # the layout is what the docstring says
    assert set(np.unique(k0[crop]).tolist()) == set(CC.K_STRESS) and (run["mask"][crop] == 1).all()
    want_k = carried(k0)
    assert same_bits(run["end"][0][names.index("k_stress_transp")][crop], want_k[crop]).all()      # (the oracle carries it too)
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

    split = run["month_step"] - 1
    assert split >= 1
    ctx = _context(native, lateral, run["start"][0], names, run["start"][1])
    ctx.set_forcing_series(F)
    ctx.run_steps(split)
    got = ctx.download("k_stress_transp")
    ok = same_bits(got, want_k) | ~crop
    assert ok.all(), ("before the month change", np.flatnonzero(~ok)[:10], got[~ok][:5], want_k[~ok][:5])
    ctx.run_steps(nsteps - split)
    got = ctx.download("k_stress_transp")
    ok = same_bits(got, want_k) | ~crop
    assert ok.all(), ("at the end", np.flatnonzero(~ok)[:10], got[~ok][:5], want_k[~ok][:5])
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), want_scal)
    for nm in held:
        assert same_bits(ctx.download(nm), want[nm]).all(), ("split run", nm)
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_svat_free_run_against_the_oracle(native, oracle, layout):
    """The HIP path tracks the oracle over the 12 days from "grown" (tests/test_physics_host_vs_oracle_crops.py runs the same
    comparison with the host-compiled core and stays inside the same bounds)."""
    import hip_util as H

    run = oracle_run(layout, False, "grown")
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


def test_routed_steps_with_crops(native, oracle):
    """enable_routing_1D: 20 x 16 cells of the routed hillslope (test_hip_routing._tiled_case), a third of them turned into crops with
    the "grown" planes on both sides; 30 single routed steps, each from the oracle's state -- the routed pipelines of
    rt_evapotranspiration have load and store sets of their own."""
    import hip_util as H
    from golden_util import ROUTING_CASES
    from test_hip_routing import _tiled_case

    g, names, forcing = load_case(ROUTING_CASES[0])
    nx, ny = 20, 16
    st, ctx = _tiled_case(native, oracle, g, names, nx, ny, np.random.default_rng(21))
    n = nx * ny
    lu = st.planes["lu_id"].copy()
    third = np.arange(n) % 3 == 0
    lu[third] = np.array(CC.CROP_LU)[np.arange(int(third.sum())) % len(CC.CROP_LU)]
    st.planes["lu_id"][:] = lu
    grown = CC.apply_grown(st.planes, lu, SEED)
    ctx.upload("lu_id", lu)
    for k in grown:
        ctx.upload(k, st.planes[k])
    crop = CC.is_crop(lu)
    k0 = st.planes["k_stress_transp"].copy()
    assert crop.sum() == int(third.sum()) >= n // 3 and (st.planes["maskCatch"][crop] == 1).all()
    odrv, hdrv = oracle.ForcingDriver(forcing), H.HipForcingDriver(ctx, forcing)
    moved, transpired = 0.0, 0
    for step in range(1, 31):
        H.upload_snapshot(ctx, st.snapshot(names), names)
        pd, td, ed, monthly = odrv.before_step(st)
        st.step(pd, td, ed, monthly)
        assert hdrv.before_step() == monthly
        ctx.step_routed(monthly)
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), st.scalars_row(), err_msg=f"step {step}")
        compare_bulk(H.download_snapshot(ctx, names), st.snapshot(names), names, what=f"routed step {step}")
        moved += float(ctx.download("q_sur_in").sum() + ctx.download("q_sub_in").sum())
        transpired += int((st.planes["transp"][crop] > 0).sum())
    got = ctx.download("k_stress_transp")
    assert same_bits(got, carried(k0))[crop].all()
    assert moved > 1.0, "no water was routed: the test would not see the gather"
    assert transpired >= 30, transpired      # (from the oracle's states: crops did transpire on the way)
    ctx.close()
