"""The edge columns of tests/edge_columns.py through the kernels.  Needs a real MI355X: `pytest -m gpu`.
tests/test_physics_host_vs_oracle_edges.py compares the same column code with the oracle routine by routine on the CPU and holds the
census of the arms; here the real kernels run it, over 1 000 columns = 15 full wavefronts and one of 40 lanes, in two layouts:

  interleaved   cold forests, snow packs, soils that fill and setup edges in turn
  blocks        every wavefront holds one kind (wave w: kind w % 4); under the per-cell forcing waves 0-3 and 12-15 take the series as
                it is, 4-7 the one whose precipitation comes three slots later and 8-11 a precipitation weight of zero: an all-snow,
                an all-saturated and an all-dry wave next to waves in an event -- where the per-wavefront shortcuts of rh_step.h
                decide for 64 columns at once

The run: the 8 days of edge_columns.edge_forcing (frost in all three classes of the conifers' snow capacity, a mild thaw, heavy rain
with a pause, moderate rain with two pauses, a dry day), shared by all columns or per cell."""
import functools

import numpy as np
import pytest

import edge_columns as EC
import extended_columns as E
from golden_util import ATOL, RTOL, compare, compare_bulk, load_case

pytestmark = pytest.mark.gpu

NX, NY = 40, 25
N = NX * NY
LAYOUTS = ("interleaved", "blocks")
FLAGS = ("cold_forest_snowfall", "canopy_room_below_snowfall", "canopy_room_takes_snowfall", "canopy_drips", "one_pack_melts_out_another_not",
         "root_zone_overfills_above_a_full_subsoil")
PER_CELL_FLAGS = ("pause_starts_for_some", "pause_ends_for_some")


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


def step_flags(names, before, after, event_before):
    """The arms one step of the oracle took, from its states before and after the step."""
    a = {k: after[names.index(k)] for k in ("lu_id", "ta", "prec", "int_snow_top", "throughfall_coeff_top", "snow_melt", "swe",
                                            "snow_melt_drip", "q_hof", "S_lp_rz", "S_ac_rz", "S_fp_rz", "S_ufc_rz", "S_lp_ss", "S_fp_ss", "S_ac_ss",
                                            "S_ufc_ss", "maskCatch")}
    catch, conifer = a["maskCatch"] == 1, (a["lu_id"] >= 10) & (a["lu_id"] <= 12)
    want = a["prec"] * (1. - a["throughfall_coeff_top"])
    took = catch & conifer & (a["int_snow_top"] > 0)
    melts = catch & (a["snow_melt"] > 0)
    prec_m1 = before[names.index("prec")]          # (the step's own prec_m1: after_timestep has moved the time levels on in `after`)
    start = (a["prec"] == 0) & (prec_m1 != 0)
    end = (a["prec"] != 0) & (prec_m1 == 0)
    return dict(
        cold_forest_snowfall=bool((catch & conifer & (a["ta"] < -3) & (a["prec"] > 0)).any()),
        canopy_room_below_snowfall=bool((took & (a["int_snow_top"] < want)).any()),
        canopy_room_takes_snowfall=bool((took & (a["int_snow_top"] == want)).any()),
        canopy_drips=bool((catch & (a["snow_melt_drip"] > 0)).any()),
        one_pack_melts_out_another_not=bool((melts & (a["swe"] == 0)).any() and (melts & (a["swe"] > 0)).any()),
        root_zone_overfills_above_a_full_subsoil=bool((catch & (a["q_hof"] > 0) & (a["S_lp_rz"] == a["S_ac_rz"]) & (a["S_fp_rz"] == a["S_ufc_rz"])
                                                      & (a["S_lp_ss"] + a["S_fp_ss"] >= a["S_ac_ss"] + a["S_ufc_ss"])).any()),
        pause_starts_for_some=bool(event_before >= 1 and (catch & start).any() and (catch & ~start & (a["prec"] != 0)).any()
                                   and (catch & ~start & (a["prec"] == 0)).any()),
        pause_ends_for_some=bool(event_before >= 1 and (catch & end).any() and (catch & ~end & (a["prec"] == 0)).any()),
    )


@functools.lru_cache(maxsize=None)
def oracle_run(layout, lateral, per_cell):
    """The oracle's free run, computed once and left unchanged: the start, the state before and after the first two steps of every
    step class, the first two steps in which each arm of step_flags is taken and every twelfth step, and the end."""
    import oracle_binding as ob

    ob.build()
    st = EC.edge_start(ob, NX, NY, layout, _luts(lateral), lateral)
    names = list(st.names)
    F = EC.edge_forcing()
    cells = EC.cell_forcing(F, N, layout) if per_cell else None
    drv = ob.ForcingDriver(F, weights=cells[1], stations=cells[0]) if per_cell else ob.ForcingDriver(F)
    run = dict(names=names, F=F, cells=cells, start=(st.snapshot(), st.scalars_row()), pairs=[], kinds=set(), seen=dict.fromkeys(FLAGS + PER_CELL_FLAGS, 0),
               lu=st.planes["lu_id"].copy(), swe0=st.planes["swe"].copy())
    seen_kind = {}
    step = 0
    while st.scal.time < EC.NDAYS * 86400:
        step += 1
        before = (st.snapshot(), st.scalars_row())
        event_before = int(st.scal.event_id[1])
        pd, td, ed, monthly = drv.before_step(st)
        assert not monthly
        ok = st.step(pd, td, ed, monthly)
        after = st.snapshot()
        kind = (int(st.scal.dt_secs), event_before == 0 and int(st.scal.event_id[0]) >= 1)
        seen_kind[kind] = seen_kind.get(kind, 0) + 1
        flags = [k for k, v in step_flags(names, before[0], after, event_before).items() if v and run["seen"][k] < 2]
        if seen_kind[kind] <= 2 or step % 12 == 0 or flags:
            run["pairs"].append((step, before, (after, st.scalars_row(), int(ok))))
            run["kinds"].add(kind)
            for k in flags:
                run["seen"][k] += 1
    run["end"] = (st.snapshot(), st.scalars_row())
    run["nsteps"] = step
    for a in [run["start"][0], run["end"][0], run["lu"], run["swe0"]] + [x for _, b, c in run["pairs"] for x in (b[0], b[1], c[0], c[1])]:
        a.setflags(write=False)
    return run


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def hand_over_day(ctx, F, cells, midnight_only=False):
    """The set_forcing hook: at midnight the calendar and the day (per cell where `cells` is given); mid-day, unless midnight_only,
    the day the oracle took at midnight.  Returns the month-change flag."""
    s = ctx.get_scalars()
    i = None
    if s.time % 86400 == 0:
        i = s.itt_forc
        s.itt_day = 0
        s.year[1], s.month[1], s.doy[1] = int(F["YEAR"][i]), int(F["MONTH"][i]), int(F["DOY"][i])
        s.itt_forc = i + 144
        ctx.set_scalars(s)
    elif not midnight_only:
        i = s.itt_forc - 144
    if i is not None:
        ctx.set_forcing_day(*(EC.cell_day(F, *cells, i) if cells else [F[v][i:i + 144] for v in ("PREC", "TA", "PET")]))
    return (s.month[1] != s.month[0]) and (s.itt > 1)


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_setup_kernels_on_edge_columns(native, oracle, layout, lateral):
    """rh_topo ... rh_initial_conditions on the device from the primaries: the masks exactly, every plane as the oracle's kernels leave
    it; rew, sand and the root depth at the edges from the primaries alone."""
    import hip_util as H

    p = EC.edge_params(NX, NY, EC.SEED, layout)
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
    EC.load_pack(st, p)
    for nm in ("theta_rz", "theta_rz_m1", "theta_ss", "theta_ss_m1", "S_dep", "S_dep_m1", "swe", "swe_m1", "S_snow", "S_snow_m1"):
        ctx.upload(nm, st.planes[nm])
    st.initial_conditions()
    ctx.call("rh_initial_conditions")
    for mask in ("maskCatch", "maskRiver", "maskLake"):
        np.testing.assert_array_equal(ctx.download(mask), st.planes[mask], err_msg=mask)
    pwp, ac, z_soil, lu = (p[k].ravel() for k in ("theta_pwp", "theta_ac", "z_soil", "lu_id"))
    crop = (lu >= 500) & (lu < 600)
    s = st.settings
    rew, sand, z_root, clay = (ctx.download(k) for k in ("rew", "sand", "z_root", "clay"))
    assert (pwp < s.theta_rew_min).sum() >= 30 and (pwp > s.theta_rew_max).sum() >= 30 and (ac > 0.24).sum() >= 30
    np.testing.assert_array_equal(rew[pwp < s.theta_rew_min], s.rew_min)
    np.testing.assert_array_equal(rew[pwp > s.theta_rew_max], s.rew_max)
    np.testing.assert_array_equal(sand[ac > 0.24], 1.0)
    np.testing.assert_array_equal(z_root[crop], np.where(z_soil <= 200.0, z_soil * 0.9, 200.0)[crop])
    assert (crop & (z_soil <= 200.0)).sum() >= 10 and (clay == s.clay_min).sum() >= 30
    assert ((z_root == s.zroot_to_zsoil_max * z_soil) & ~crop).sum() >= 30
    assert (p["theta_rz0"].ravel() <= pwp).sum() >= 30
    compare(H.download_snapshot(ctx, names), st.snapshot(), names, what="setup kernels")
    ctx.close()


@pytest.mark.parametrize("per_cell", [False, True], ids=["shared", "per_cell"])
@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_steps_from_the_oracles_states(native, oracle, layout, lateral, per_cell):
    """One fused step from the oracle's state k-1 gives the oracle's state k: every plane at RTOL / ATOL, the scalar row and sanity_ok
    exactly.  Among the pairs, counted from the oracle's states: steps that take each arm of step_flags."""
    import hip_util as H

    run = oracle_run(layout, lateral, per_cell)
    names, F, cells = run["names"], run["F"], run["cells"]
    print("PAIRS", layout, lateral, per_cell, len(run["pairs"]), run["nsteps"], run["seen"])
    assert 16 <= len(run["pairs"]) <= 60, len(run["pairs"])
    assert {k[0] for k in run["kinds"]} == {600, 3600, 86400} and any(k[1] for k in run["kinds"])
    # (the lateral drainage of the oneD model has emptied the large pores again by the end of the step: the over-filled root zone shows
    # in the states between the routines only, where tests/test_physics_host_vs_oracle_edges.py counts it)
    for k in FLAGS[:-1 if lateral else None] + (PER_CELL_FLAGS if per_cell else ()):
        assert run["seen"][k] > 0, f"{k}: no step of the oracle's run takes it"
    ctx = _context(native, lateral, run["start"][0], names, run["start"][1])
    for step, (snap0, row0), (snap1, row1, ok) in run["pairs"]:
        H.upload_snapshot(ctx, snap0, names)
        ctx.set_scalars(H.scalars_from_row(row0))
        monthly = hand_over_day(ctx, F, cells)
        ctx.step(monthly)
        s = ctx.get_scalars()
        np.testing.assert_array_equal(H.scalars_to_row(s), row1, err_msg=f"{layout} step {step}")
        assert int(s.sanity_ok) == ok, f"{layout} step {step}: sanity_ok {s.sanity_ok}, the oracle's {ok}"
        compare(H.download_snapshot(ctx, names), snap1, names, rtol=RTOL, atol=ATOL, what=f"{layout} single step {step}")
    ctx.close()


@pytest.mark.parametrize("per_cell", [False, True], ids=["shared", "per_cell"])
@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
def test_run_steps_over_whole_wavefronts_of_one_kind_equals_the_routine_path(native, oracle, lateral, per_cell):
    """Layout "blocks": ONE rh_run_steps call over the whole run (an eager first step, then the lazy pipelines with the per-wave
    parameter words and the dry-path votes) leaves every plane, bit for bit and NaN for NaN, and the scalars as the same steps driven
    routine by routine (rh_adaptive_dt + rh_step_core + rh_after_timestep).  per_cell: the device forms every column's day from two
    stations' series and the weights, the routine path gets the per-cell days from the host; waves 8-11 stay dry through the rain
    days while their neighbours are in an event."""
    import hip_util as H

    run = oracle_run("blocks", lateral, per_cell)
    names, F, cells = run["names"], run["F"], run["cells"]
    if per_cell:
        assert (cells[1]["prec_weight"][8 * EC.BLOCK:12 * EC.BLOCK] == 0).all() and (cells[1]["prec_weight"][:8 * EC.BLOCK] == 1).all()
        assert (cells[0]["station_index"][4 * EC.BLOCK:8 * EC.BLOCK] == 1).all()
    kind = EC.kind_of(N, "blocks")
    assert all(np.unique(kind[w * EC.BLOCK:(w + 1) * EC.BLOCK]).size == 1 for w in range(N // EC.BLOCK))     # the layout is what the docstring says
    assert np.isin(run["lu"][:EC.BLOCK], EC.FOREST_LU).all() and (run["swe0"][EC.BLOCK:2 * EC.BLOCK] > 0).all()
    ref = _context(native, lateral, run["start"][0], names, run["start"][1])
    held = [nm for nm, _ in ref.planes[: ref.planes_held]]
    nsteps = 0
    while ref.get_scalars().time < EC.NDAYS * 86400:
        monthly = hand_over_day(ref, F, cells, midnight_only=True)
        assert not monthly
        ref.call("rh_adaptive_dt")
        ref.call("rh_step_core")
        ref.call("rh_after_timestep")
        nsteps += 1
        assert nsteps <= 600
    assert nsteps == run["nsteps"], (nsteps, run["nsteps"])
    want_scal = H.scalars_to_row(ref.get_scalars())
    want = {nm: ref.download(nm) for nm in held}
    ref.close()

    ctx = _context(native, lateral, run["start"][0], names, run["start"][1])
    if per_cell:
        stations, weights = cells
        ctx.set_forcing_stations(dict(F, PREC=stations["PREC"], TA=stations["TA"], PET=stations["PET"]), stations["station_index"])
        ctx.set_forcing_weights(weights["prec_weight"], weights["ta_offset"], weights["pet_weight"])
    else:
        ctx.set_forcing_series(F)
    ctx.run_steps(nsteps)
    s = ctx.get_scalars()
    np.testing.assert_array_equal(H.scalars_to_row(s), want_scal)
    np.testing.assert_array_equal(want_scal, run["end"][1])
    for nm in held:
        got = ctx.download(nm)
        ok = same_bits(got, want[nm])
        assert ok.all(), (nm, np.flatnonzero(~ok)[:10], got[~ok][:5], want[nm][~ok][:5])
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_svat_free_run_against_the_oracle(native, oracle, layout):
    """The HIP path tracks the oracle over the 8 days (tests/test_physics_host_vs_oracle_edges.py runs the same comparison with the
    host-compiled core and stays inside the same bounds)."""
    import hip_util as H

    run = oracle_run(layout, False, False)
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
    assert run["nsteps"] > 40
    ctx.close()


def test_svat_free_run_with_per_cell_forcing_against_the_oracle(native, oracle):
    """Layout "blocks", the forcing per cell and formed on the device (two stations and a precipitation weight of zero): one rh_run_steps
    call over the 8 days against the oracle, which gets the same per-cell days from the host."""
    import hip_util as H

    run = oracle_run("blocks", False, True)
    names, F, (stations, weights) = run["names"], run["F"], run["cells"]
    ctx = _context(native, False, run["start"][0], names, run["start"][1])
    ctx.set_forcing_stations(dict(F, PREC=stations["PREC"], TA=stations["TA"], PET=stations["PET"]), stations["station_index"])
    ctx.set_forcing_weights(weights["prec_weight"], weights["ta_offset"], weights["pet_weight"])
    ctx.run_steps(run["nsteps"])
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), run["end"][1])
    compare_bulk(H.download_snapshot(ctx, names), run["end"][0], names, what="per-cell free run")
    ctx.close()
