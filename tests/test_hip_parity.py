"""HIP path (through the C ABI) against the golden vectors of the reference NumPy backend and
against the oracle.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

from golden_util import (ATOL, CASES, ONED_CASES, ONED_TIE_COLUMNS, RTOL, TieTracker, STATION_CASES, WEIGHTED_CASES, compare, compare_bulk,
                         deviating_columns, is_lateral, load_case, load_stations, load_weights)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from roger_amd import _native as N

    N.load()
    return N


def _ctx(native, g, names, key="state0", scal_key="scal0"):
    import hip_util as H

    nx, ny = (int(v) for v in g["nx_ny"])
    ctx = native.Context(nx, ny, enable_lateral_flow=int(is_lateral(g)))
    H.upload_snapshot(ctx, g[key], names)
    ctx.set_scalars(H.scalars_from_row(g[scal_key] if isinstance(scal_key, str) else scal_key))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    if is_lateral(g):
        ctx.set_lut_mlms(g["lut_mlms"])
    return ctx


@pytest.mark.parametrize("case", CASES)
def test_trajectory_golden(native, case):
    """Fused rh_svat_step reproduces the reference trajectory (all planes at the stored steps, the integer scalars exactly at
    every step).  oneD combo case: every column but the few that part from the reference at a residue tie
    over the WHOLE trajectory; which columns those are is decided by the data (golden_util.TieTracker: a rounding residue in a water
    store of the reference's state or the device's)."""
    import hip_util as H

    g, names, forcing = load_case(case)
    ctx = _ctx(native, g, names)
    drv = H.HipForcingDriver(ctx, forcing)
    nsteps = int(g["nsteps"])
    checked = 0
    ties = TieTracker.for_case(case, names, ctx.n)
    for step in range(1, nsteps + 1):
        monthly = drv.before_step()
        ctx.step(monthly)
        s = ctx.get_scalars()
        np.testing.assert_array_equal(H.scalars_to_row(s), g["scal"][step - 1], err_msg=f"{case} scalars step {step}")
        assert s.sanity_ok == 1
        key = f"s{step:05d}"
        if key in g.files:
            if ties:   # every column without a rounding residue in a water store (its own state or the reference's): 1e-10 throughout
                ties.check(H.download_snapshot(ctx, names), g[key], step, what=case)
            else:
                compare(H.download_snapshot(ctx, names), g[key], names, what=f"{case} step {step}")
            checked += 1
    if ties:
        print(f"TIES {case}: tie-exposed columns (first stored step with a residue) {ties.exposed}")
        assert len(ties.exposed) <= ONED_TIE_COLUMNS[case] + 1
    assert checked >= 3
    ctx.close()


@pytest.mark.parametrize("case", ONED_CASES)
def test_single_steps_from_reference_states(native, case):
    """oneD model: one fused step from the reference's state k-1 gives the reference's state k."""
    import hip_util as H

    g, names, forcing = load_case(case)
    have = sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit())
    pairs = [k for k in have if k - 1 in have and k >= 2]
    assert len(pairs) >= 20
    for k in pairs:
        ctx = _ctx(native, g, names, key=f"s{k - 1:05d}", scal_key=g["scal"][k - 2])
        s = ctx.get_scalars()
        if s.time % 86400:   # mid-day: hand over the forcing the reference took at midnight
            i0 = s.itt_forc - 144
            ctx.set_forcing_day(*[forcing[v][i0:i0 + 144] for v in ("PREC", "TA", "PET")])
        monthly = H.HipForcingDriver(ctx, forcing).before_step()
        ctx.step(monthly)
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][k - 1], err_msg=f"step {k}")
        compare(H.download_snapshot(ctx, names), g[f"s{k:05d}"], names, what=f"{case} single step {k}")
        ctx.close()


ROUTINE_ENTRY = {
    "calculate_interception": ("rh_interception",),
    "calculate_evapotranspiration": ("rh_evapotranspiration",),
    "calculate_snow": ("rh_snow",),
    "calculate_infiltration": ("rh_infiltration",),
    "calculate_subsurface_runoff": ("rh_subsurface_runoff",),
    "calculate_capillary_rise": ("rh_capillary_rise",),
    "calculate_soil": ("rh_storage",),
}


@pytest.mark.parametrize("case", CASES)
def test_per_routine_golden(native, case):
    """One entry point per reference routine: state before the routine in, state after it out."""
    import hip_util as H

    g, names, _ = load_case(case)
    order = ["adaptive_time_stepping", "calculate_interception", "calculate_evapotranspiration", "calculate_snow",
             "calculate_infiltration", "calculate_subsurface_runoff", "calculate_capillary_rise", "calculate_soil"]
    steps = sorted({int(k[1:6]) for k in g.files if k.startswith("r") and k.endswith("_calc_storage")})
    n = 0
    for step in steps:
        for prev, cur in zip(order[:-1], order[1:]):
            kp = f"r{step:05d}_{prev}"
            ctx = _ctx(native, g, names, key=kp, scal_key=kp + "_scal")
            for entry in ROUTINE_ENTRY[cur]:
                ctx.call(entry)
            ref = g[f"r{step:05d}_calc_storage"] if cur == "calculate_soil" else g[f"r{step:05d}_{cur}"]
            compare(H.download_snapshot(ctx, names), ref, names, what=f"{case} step {step} {cur}")
            ctx.close()
            n += 1
    assert n >= 7


@pytest.mark.parametrize("case", CASES)
def test_setup_kernels_golden(native, case):
    import hip_util as H

    g, names, _ = load_case(case)
    ctx = _ctx(native, g, names, key="pre_surface")
    ctx.call("rh_topo")
    ctx.call("rh_params_surface")
    compare(H.download_snapshot(ctx, names), g["pre_params"], names, what=f"{case} surface params")
    ctx.close()
    ctx = _ctx(native, g, names, key="pre_params")
    ctx.call("rh_params_soil")
    if is_lateral(g):
        ctx.call("rh_params_lateral")
    got, ref = H.download_snapshot(ctx, names), g["pre_ic"]
    for nm in ("theta_rz", "theta_rz_m1", "theta_ss", "theta_ss_m1", "S_sur", "S_sur_m1"):
        got[names.index(nm)] = ref[names.index(nm)]
    compare(got, ref, names, what=f"{case} soil params")
    ctx.close()
    ctx = _ctx(native, g, names, key="pre_ic")
    ctx.call("rh_initial_conditions")
    compare(H.download_snapshot(ctx, names), g["state0"], names, what=f"{case} initial conditions")
    ctx.close()


def _oracle_setup(ob, nx, ny, seed, luts):
    """Heterogeneous start state built with the oracle's setup kernels (same recipe as the
    golden generator's hetero_params)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from extended_columns import oracle_state
    from make_golden import hetero_params

    return oracle_state(ob, hetero_params(nx, ny, seed=seed), luts, lateral=False)   # (no z_gw among the primaries: 1000 m)


@pytest.mark.parametrize("per_cell", [False, True])
def test_vs_oracle_hetero_4096(native, oracle, per_cell):
    """64x64 heterogeneous columns, 12 days of the combo forcing (all step classes): the HIP path
    tracks the oracle on every plane; also with the forcing handed over per cell."""
    import hip_util as H
    from roger_amd.forcing import combo_forcing

    g, names, _ = load_case("svat_hetero_combo")
    luts = (g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    nx = ny = 64
    st = _oracle_setup(oracle, nx, ny, 123, luts)
    onames = st.names
    ctx = native.Context(nx, ny)
    H.upload_snapshot(ctx, st.snapshot(), onames)
    ctx.set_scalars(H.scalars_from_row(st.scalars_row()))
    ctx.set_luts(*luts)
    F = combo_forcing(ndays=12)
    odrv = oracle.ForcingDriver(F)
    hdrv = H.HipForcingDriver(ctx, F, per_cell=per_cell)
    step = 0
    while st.scal.time < 12 * 86400:
        step += 1
        pd, td, ed, monthly = odrv.before_step(st)
        st.step(pd, td, ed, monthly)
        m2 = hdrv.before_step()
        assert m2 == monthly
        ctx.step(m2)
        if step % 25 == 0 or step < 3:
            np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), st.scalars_row())
            compare_bulk(H.download_snapshot(ctx, onames), st.snapshot(), onames, what=f"step {step}")
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), st.scalars_row())
    compare_bulk(H.download_snapshot(ctx, onames), st.snapshot(), onames, what="final")
    assert step > 100
    ctx.close()


@pytest.mark.parametrize("nx,ny,lateral", [(1000, 1000, False), (3200, 3125, False), (3200, 3125, True)])
def test_full_size_properties(native, oracle, nx, ny, lateral):
    """BASELINE configs[1] size (nx*ny = 10^6), the north-star size (10^7), and BASELINE configs[3] -- the oneD model with lateral
    subsurface flow at 3200 x 3125 columns, its own uniform parameters (the reference's start state of oned_uniform_benchmark) and
    heavy rain so that a perched water table forms and the lateral branches run: size-independent properties -- every column equals
    the single-column oracle run bit-for-tolerance, the mass balance closes, the sanity flag holds."""
    import hip_util as H
    from roger_amd.forcing import toy_forcing

    g, names, _ = load_case("oned_uniform_benchmark" if lateral else "svat_uniform_rain")
    luts = (g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    # oracle: the 6-cell uniform golden start state, one column is enough
    st = oracle.OracleState(6)
    st.load_snapshot(g["state0"], names)
    st.load_scalars(g["scal0"])
    st.set_luts(*luts)
    st.settings.enable_lateral_flow = int(lateral)
    ctx = native.Context(nx, ny, enable_lateral_flow=int(lateral))
    for row, nm in zip(g["state0"], names):
        if nm in ctx.index:
            ctx.upload(nm, np.full(nx * ny, row[0]))
    ctx.set_scalars(H.scalars_from_row(g["scal0"]))
    ctx.set_luts(*luts)
    if lateral:
        ctx.set_lut_mlms(g["lut_mlms"])
    F = toy_forcing("heavyrain" if lateral else "rain", ndays=4 if lateral else 3)
    odrv = oracle.ForcingDriver(F)
    hdrv = H.HipForcingDriver(ctx, F)
    for step in range(90 if lateral else 30):
        pd, td, ed, monthly = odrv.before_step(st)
        st.step(pd, td, ed, monthly)
        ctx.step(hdrv.before_step())
    s = ctx.get_scalars()
    assert s.sanity_ok == 1
    np.testing.assert_array_equal(H.scalars_to_row(s), st.scalars_row())
    ref = st.snapshot()
    check = ("S", "S_rz", "S_ss", "theta_rz", "theta_ss", "z0", "q_ss", "aet", "inf_mat_rz", "z_wf", "dS_num_error")
    if lateral:
        check += ("q_sub", "q_sub_rz", "q_sub_ss", "q_sub_mp_ss", "z_sat", "z_sat_layer_3", "S_zsat")
        assert ref[names.index("q_sub")][0] > 0.05 and ref[names.index("z_sat")][0] > 100   # the lateral branches did run
    for nm in check:
        col = ctx.download(nm)
        assert col.min() == col.max(), nm  # identical inputs -> identical columns
        r = ref[names.index(nm)][0]
        assert abs(col[0] - r) <= ATOL + RTOL * abs(r), (nm, col[0], r)
    assert ctx.download("dS_num_error").max() < 1e-9
    ctx.close()


@pytest.mark.parametrize("case", ["svat_hetero_combo", "svat_hetero_heavyrain", "oned_hetero_heavyrain"])
def test_device_hooks_golden(native, case):
    """rh_run_steps: forcing series resident on the device, `set_forcing`/`set_parameters` hooks
    and the month-change decision taken on the device, no host round trip per step."""
    import hip_util as H

    g, names, forcing = load_case(case)
    ctx = _ctx(native, g, names)
    ctx.set_forcing_series(forcing)
    nsteps = int(g["nsteps"])
    done = 0
    for step in sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit()):
        ctx.run_steps(step - done)
        done = step
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][step - 1])
        compare(H.download_snapshot(ctx, names), g[f"s{step:05d}"], names, what=f"{case} step {step}")
    assert done == nsteps
    ctx.close()


def test_phased_stepper_single_rank(native):
    """The multi-GPU orchestration (expand -> all-reduce -> compress between the phases) with one
    rank equals rh_run_steps."""
    import torch

    import hip_util as H
    from roger_amd.distributed import HipPhases, PhasedStepper

    g, names, forcing = load_case("svat_hetero_combo")
    a, b, c, d = (_ctx(native, g, names) for _ in range(4))
    for ctx in (a, b, c, d):
        ctx.set_forcing_series(forcing)
    dev = torch.device("cuda", 0)
    a.run_steps(120)
    # always_exchange: spread / fold the predicate words through the exchange buffers although there is no peer
    PhasedStepper(HipPhases(b, dev), always_exchange=True).run(120)                       # one exchange per step, format folded into the kernels
    PhasedStepper(HipPhases(c, dev, one_exchange=False), always_exchange=True).run(120)   # three-phase protocol
    PhasedStepper(HipPhases(d, dev, fused_exchange=False), always_exchange=True).run(120)  # one exchange, separate expand / compress
    torch.cuda.synchronize()
    for other in (b, c, d):
        np.testing.assert_array_equal(H.scalars_to_row(a.get_scalars()), H.scalars_to_row(other.get_scalars()))
        np.testing.assert_array_equal(H.download_snapshot(a, names), H.download_snapshot(other, names))
    for ctx in (a, b, c, d):
        ctx.close()


def test_weighted_station_forcing_on_device(native, oracle):
    """BASELINE configs[4] shape (Eberbaechle: 80 x 53 columns of 25 m^2, station forcing with per-cell prec_weight,
    ta_offset, pet_weight, examples/catchment_scale/eberbaechle/svat_distributed/svat.py:169-186, 276-296): the device
    forms the per-cell day from the resident series and the weights and steps without the host; the oracle gets the
    same per-cell arrays from the host.  Heterogeneous synthetic parameter maps (seed 7), 6 days, all step classes."""
    import hip_util as H
    from roger_amd.forcing import combo_forcing

    g, names, _ = load_case("svat_hetero_combo")
    luts = (g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    nx, ny = 80, 53
    n = nx * ny
    st = _oracle_setup(oracle, nx, ny, 7, luts)
    onames = st.names
    ctx = native.Context(nx, ny)
    H.upload_snapshot(ctx, st.snapshot(), onames)
    ctx.set_scalars(H.scalars_from_row(st.scalars_row()))
    ctx.set_luts(*luts)
    rng = np.random.default_rng(7)
    pw, toff, ew = rng.uniform(0.8, 1.3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.85, 1.15, n)
    F = combo_forcing(ndays=6)
    ctx.set_forcing_series(F)
    ctx.set_forcing_weights(pw, toff, ew)
    s = st.scal
    steps = 0
    while s.time < 6 * 86400:
        if s.time % 86400 == 0:      # the setup's set_forcing hook, host side for the oracle
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(F["YEAR"][i]), int(F["MONTH"][i]), int(F["DOY"][i])
            day = (F["PREC"][i:i + 144][None, :] * pw[:, None], F["TA"][i:i + 144][None, :] + toff[:, None],
                   F["PET"][i:i + 144][None, :] * ew[:, None])
            s.itt_forc = i + 144
        monthly = (s.month[1] != s.month[0]) and (s.itt > 1)
        st.step(*day, monthly)
        steps += 1
    ctx.run_steps(steps)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), st.scalars_row())
    compare_bulk(H.download_snapshot(ctx, onames), st.snapshot(), onames, what=f"weighted forcing, {steps} steps")
    assert len({600, 3600, 86400} & {int(st.scal.dt_secs)}) == 1 and steps > 40
    ctx.close()


@pytest.fixture(params=["one kernel", "split"])
def cell_agg_split(request, monkeypatch):
    """The per-cell aggregates in one kernel (grids below 65 536 columns) or as the hourly + the daily kernel (above; forced here)."""
    if request.param == "split":
        monkeypatch.setenv("RH_CELL_AGG_SPLIT_MIN", "1")
    else:
        monkeypatch.delenv("RH_CELL_AGG_SPLIT_MIN", raising=False)
    return request.param


@pytest.mark.parametrize("case", WEIGHTED_CASES)
def test_weighted_station_forcing_golden(native, case, cell_agg_split):
    """BASELINE configs[4] pinned by the reference itself: the golden run's set_forcing multiplies / offsets the station's measured
    series (first 40 days of the shipped Eberbaechle PREC/TA/PET.txt) by per-cell prec_weight / ta_offset / pet_weight
    (examples/catchment_scale/eberbaechle/svat_distributed/svat.py:169-186, 276-296).  The device forms every column's day from
    the resident series and the three weight planes (rh_set_forcing_weights) and steps without the host: integer scalars exact,
    all planes at the stored steps; snow falls on part of the grid only, so the per-cell predicates decide the step length."""
    import hip_util as H

    g, names, forcing = load_case(case)
    w = load_weights(g)
    ctx = _ctx(native, g, names)
    ctx.set_forcing_series(forcing)
    ctx.set_forcing_weights(w["prec_weight"], w["ta_offset"], w["pet_weight"])
    done = 0
    for step in sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit()):
        ctx.run_steps(step - done)
        done = step
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][step - 1], err_msg=f"step {step}")
        compare(H.download_snapshot(ctx, names), g[f"s{step:05d}"], names, what=f"{case} step {step}")
    assert done == int(g["nsteps"]) and ctx.get_scalars().sanity_ok == 1
    # ... and with the per-cell day handed over by the host hook each midnight (rh_set_forcing_day(per_cell=1)), step by step
    ctx2 = _ctx(native, g, names)
    for step in range(1, 120):
        s = ctx2.get_scalars()
        if s.time % 86400 == 0:
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(forcing["YEAR"][i]), int(forcing["MONTH"][i]), int(forcing["DOY"][i])
            s.itt_forc = i + 144
            ctx2.set_scalars(s)
            ctx2.set_forcing_day(forcing["PREC"][i:i + 144][None, :] * w["prec_weight"][:, None],
                                 forcing["TA"][i:i + 144][None, :] + w["ta_offset"][:, None],
                                 forcing["PET"][i:i + 144][None, :] * w["pet_weight"][:, None])
        ctx2.step((s.month[1] != s.month[0]) and (s.itt > 1))
        np.testing.assert_array_equal(H.scalars_to_row(ctx2.get_scalars()), g["scal"][step - 1], err_msg=f"host hook, step {step}")
        if f"s{step:05d}" in g.files:
            compare(H.download_snapshot(ctx2, names), g[f"s{step:05d}"], names, what=f"{case} host hook, step {step}")
    ctx.close()
    ctx2.close()


@pytest.mark.parametrize("case", STATION_CASES)
def test_station_mapped_forcing_golden(native, case, cell_agg_split):
    """settings.enable_distributed_input: three stations' series resident on the device, every column mapped
    to one of them (one column to none: zeros), per-cell weights on top -- the reference's own run of such a setup
    (roger/bmimodels/svat_dist/svat_dist.py:274-322) reproduced by rh_set_forcing_stations + rh_set_forcing_weights + rh_run_steps, no
    host in the loop; and with the per-cell day handed over by the host every midnight (the transposed (144, n) layout)."""
    import hip_util as H
    import oracle_binding as ob

    g, names, forcing = load_case(case)
    st, w = load_stations(g), load_weights(g)
    ctx = _ctx(native, g, names)
    ctx.set_forcing_stations(dict(PREC=st["PREC"], TA=st["TA"], PET=st["PET"], YEAR=forcing["YEAR"], MONTH=forcing["MONTH"], DOY=forcing["DOY"]),
                             st["station_index"])
    ctx.set_forcing_weights(w["prec_weight"], w["ta_offset"], w["pet_weight"])
    done = 0
    for step in sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit()):
        ctx.run_steps(step - done)
        done = step
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][step - 1], err_msg=f"step {step}")
        compare(H.download_snapshot(ctx, names), g[f"s{step:05d}"], names, what=f"{case} step {step}")
    assert done == int(g["nsteps"])
    ctx.close()
    ctx2 = _ctx(native, g, names)
    drv = ob.ForcingDriver(forcing, weights=w, stations=st)
    for step in range(1, int(g["nsteps"]) + 1):
        s = ctx2.get_scalars()
        if s.time % 86400 == 0:
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(forcing["YEAR"][i]), int(forcing["MONTH"][i]), int(forcing["DOY"][i])
            s.itt_forc = i + 144
            ctx2.set_scalars(s)
            ctx2.set_forcing_day(*drv.day_slice(i))
        ctx2.step((s.month[1] != s.month[0]) and (s.itt > 1))
        np.testing.assert_array_equal(H.scalars_to_row(ctx2.get_scalars()), g["scal"][step - 1], err_msg=f"host hook, step {step}")
        if f"s{step:05d}" in g.files:
            compare(H.download_snapshot(ctx2, names), g[f"s{step:05d}"], names, what=f"{case} host hook, step {step}")
    ctx2.close()


def test_timing_detail_reports_time_step_classes():
    """rh_timing_detail: dt_secs of every timed step from the device-side log, one kernel duration each; the classes
    add up to the simulated time."""
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    ctx = create_svat(64, 32, device=0)
    ctx.set_forcing_series(combo_forcing(ndays=30))
    ctx.run_steps(3)
    s0 = ctx.get_scalars()
    ctx.enable_timing(True)
    ctx.run_steps(150)
    ms, dts = ctx.timing_detail()
    ctx.enable_timing(False)
    s1 = ctx.get_scalars()
    assert len(ms) == len(dts) == 150 and (ms > 0).all()
    assert set(np.unique(dts)) <= {600, 3600, 86400} and len(np.unique(dts)) >= 2
    assert int(dts.sum()) == s1.time - s0.time
    ctx.close()


def test_placement_probing_keeps_the_fastest_candidate():
    """rh_create with rh_config.placement_probes > 1: the chosen arena is the candidate on which the streaming kernel was
    fastest (eight candidates by default); small grids and RH_PLACEMENT_PROBES=1 do not probe; results do not depend on where the arena lands."""
    import os

    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat

    forcing = combo_forcing(ndays=30)
    default = create_svat(512, 512, device=0)          # up to eight candidates by default
    assert 2 <= len(default.placement_report()) <= 8
    default.close()
    ctx = create_svat(512, 512, device=0, placement_probes=8)
    rep = ctx.placement_report()
    assert 2 <= len(rep) <= 8 and rep[0] == min(rep) and min(rep) > 0
    ctx.set_forcing_series(forcing)
    ctx.run_steps(40)
    a = {k: ctx.download(k) for k in ("S_rz", "S_ss", "swe", "q_ss", "aet")}
    ctx.close()
    small = create_svat(64, 64, device=0)
    assert small.placement_report() == []
    small.close()
    os.environ["RH_PLACEMENT_PROBES"] = "1"
    try:
        ctx = create_svat(512, 512, device=0, placement_probes=8)   # the environment overrides the configuration
        assert ctx.placement_report() == []
        ctx.set_forcing_series(forcing)
        ctx.run_steps(40)
        for k, v in a.items():
            np.testing.assert_array_equal(ctx.download(k), v, err_msg=k)
        ctx.close()
    finally:
        del os.environ["RH_PLACEMENT_PROBES"]


def test_tail_control_equals_control_kernel(native):
    """The control part of a step (hooks, predicates, forcing aggregates, dt and event bookkeeping) formed by the tail of the
    previous fused kernel (last wavefront done; S_next / X_next) against the control kernel in front of every step
    (RH_NO_TAIL_CTRL): the same scalars after every call and the same planes, with scalar reads, uploads, host-side scalar changes,
    timing switches and host-driven steps in between."""
    import os

    import hip_util as H

    g, names, forcing = load_case("svat_hetero_combo")

    def run(tail):
        if tail:
            os.environ.pop("RH_NO_TAIL_CTRL", None)
        else:
            os.environ["RH_NO_TAIL_CTRL"] = "1"
        try:
            ctx = _ctx(native, g, names)
        finally:
            os.environ.pop("RH_NO_TAIL_CTRL", None)
        ctx.set_forcing_series(forcing)
        out = []
        for n in (1, 1, 2, 35, 1, 60):
            ctx.run_steps(n)
            out.append(H.scalars_to_row(ctx.get_scalars()))
        out.append(H.download_snapshot(ctx, names))
        ctx.upload("S_dep", ctx.download("S_dep") * 0.5)           # planes touched: the pending control part is dropped
        ctx.run_steps(20)
        s = ctx.get_scalars()
        ctx.set_scalars(s)                                         # scalars touched
        ctx.run_steps(20)
        ctx.enable_timing(True)
        ctx.run_steps(7)
        ms, dts = ctx.timing_detail()
        ctx.enable_timing(False)
        out.append(np.asarray(dts, dtype=np.float64))
        drv = H.HipForcingDriver(ctx, forcing)                     # host-driven hooks after device-driven ones
        for _ in range(30):
            ctx.step(drv.before_step())
        ctx.run_steps(25)
        out.append(H.scalars_to_row(ctx.get_scalars()))
        out.append(H.download_snapshot(ctx, names))
        ctx.close()
        return out

    a, b = run(True), run(False)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"item {k}")


def test_exhausted_forcing_series_is_reported(native):
    """A step that begins a day beyond the end of the resident series would run on the previous day's forcing: reported as
    RH_ERR_STATE by rh_get_scalars / rh_sync (the reference fails on the short slice); running exactly to the end is fine."""
    import hip_util as H

    g, names, forcing = load_case("svat_uniform_rain")
    ctx = _ctx(native, g, names)
    ctx.set_forcing_series(forcing)
    ctx.run_steps(int(g["nsteps"]))
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][-1])   # no error: nothing ran beyond the series
    ctx.sync()
    ctx.run_steps(1)
    with pytest.raises(native.NativeError, match="forcing series"):
        ctx.get_scalars()
    with pytest.raises(native.NativeError, match="forcing series"):
        ctx.sync()
    ctx.set_forcing_series(forcing)    # a new series clears the condition
    ctx.sync()
    ctx.close()


def test_lazy_rotation_equals_eager(native):
    """Device-driven steps skip the tau -> taum1 stores (and the X_m1 loads) while nothing but the fused kernel touches the
    planes, and materialise the X_m1 planes on demand: every plane, X_m1 included, equals the eager run's
    (RH_NO_LAZY_ROTATION) at any point -- also with uploads, per-routine calls and downloads in between."""
    import os

    import hip_util as H

    g, names, forcing = load_case("svat_hetero_combo")

    def run(lazy):
        if lazy:
            os.environ.pop("RH_NO_LAZY_ROTATION", None)
        else:
            os.environ["RH_NO_LAZY_ROTATION"] = "1"
        try:
            ctx = _ctx(native, g, names)
        finally:
            os.environ.pop("RH_NO_LAZY_ROTATION", None)
        ctx.set_forcing_series(forcing)
        snaps = []
        ctx.run_steps(37)
        snaps.append(H.download_snapshot(ctx, names))            # materialises
        ctx.run_steps(5)
        ctx.upload("S_dep", ctx.download("S_dep") * 0.5)           # the host changes a plane: the next step is eager again
        ctx.run_steps(40)
        snaps.append(H.download_snapshot(ctx, names))
        ctx.call("rh_interception")                               # a per-routine entry point in between
        ctx.run_steps(30)
        snaps.append(H.download_snapshot(ctx, names))
        snaps.append(H.scalars_to_row(ctx.get_scalars()))
        ctx.close()
        return snaps

    a, b = run(True), run(False)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"snapshot {k}")
    for xm1 in ("S_rz_m1", "swe_m1", "theta_m1"):     # after a complete step the rotation holds in what the host sees
        np.testing.assert_array_equal(a[2][names.index(xm1)], a[2][names.index(xm1[:-3])], err_msg=xm1)


@pytest.mark.parametrize("case", ["oned_hetero_combo", "svat_hetero_heavyrain"])
def test_month_change_inside_device_driven_steps(native, oracle, case):
    """The month changes on the third day: the fused kernel takes its pipeline with the monthly surface parameters in front (decided on
    the device, `k_step<2, LATERAL, .>`), also for the oneD model, whose goldens never cross a month.  Against the oracle, whose driver
    decides on the host: step by step from the oracle's state (residue ties of the oneD columns)."""
    import hip_util as H
    from golden_util import configure_settings
    from roger_amd.forcing import combo_forcing

    g, names, _ = load_case(case)
    F = {k: np.array(v) for k, v in combo_forcing(ndays=8).items()}
    F["MONTH"] = np.where(np.arange(F["MONTH"].size) < 2 * 144, 4, 5).astype(F["MONTH"].dtype)   # April -> May: the vegetation tables differ
    F["DOY"] = (119 + np.arange(F["DOY"].size) // 144).astype(F["DOY"].dtype)
    rng = np.random.default_rng(4)
    src = np.asarray(g["state0"])
    nx, ny = 24, 20
    snap = src[:, rng.integers(0, src.shape[1], nx * ny)].copy()
    st = oracle.OracleState(nx * ny)
    st.load_snapshot(snap, names)
    st.load_scalars(g["scal0"])
    st.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    configure_settings(st.settings, g)
    st.settings.nx, st.settings.ny = nx, ny
    st.scal.month[0] = st.scal.month[1] = 4
    st.scal.doy[0] = st.scal.doy[1] = 119
    ctx = native.Context(nx, ny, enable_lateral_flow=int(is_lateral(g)))
    H.upload_snapshot(ctx, snap, names)
    ctx.set_scalars(H.scalars_from_row(st.scalars_row()))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    if is_lateral(g):
        ctx.set_lut_mlms(g["lut_mlms"])
    ctx.set_forcing_series(F)
    odrv = oracle.ForcingDriver(F)
    gc0 = st.planes["ground_cover"].copy()
    changed = 0
    for step in range(1, 81):
        if step > 2:   # (the second dry day leaves a residue of -4e-16 mm in a subsoil's large pores whose sign decides the percolation)
            H.upload_snapshot(ctx, st.snapshot(names), names)
        pd, td, ed, monthly = odrv.before_step(st)
        changed += int(monthly)
        st.step(pd, td, ed, monthly)
        ctx.run_steps(1)
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), st.scalars_row(), err_msg=f"step {step}")
        compare_bulk(H.download_snapshot(ctx, names), st.snapshot(names), names, what=f"{case} step {step}")
    assert changed == 1 and not np.array_equal(gc0, st.planes["ground_cover"])
    ctx.close()


def test_per_cell_forcing_keeps_the_rotation_pending(native, monkeypatch):
    """With per-cell forcing the selected prec / ta are applied inside the fused kernel (from the per-cell aggregates) and the predicate
    kernels read tau planes only, so nothing writes a plane between two fused steps and the tau -> taum1 copies stay pending as with
    shared forcing.  RH_NO_DEFERRED_SELECT=1: the selection kernel stores prec / ta itself (eager fused kernel) -- the same bits."""
    import hip_util as H

    g, names, forcing = load_case(WEIGHTED_CASES[0])
    w = load_weights(g)
    out = {}
    for mode in ("deferred", "stored"):
        if mode == "stored":
            monkeypatch.setenv("RH_NO_DEFERRED_SELECT", "1")
        else:
            monkeypatch.delenv("RH_NO_DEFERRED_SELECT", raising=False)
        ctx = _ctx(native, g, names)
        ctx.set_forcing_series(forcing)
        ctx.set_forcing_weights(w["prec_weight"], w["ta_offset"], w["pet_weight"])
        ctx.run_steps(int(g["nsteps"]))
        lazy, _ = ctx.step_mode()
        assert lazy == (mode == "deferred"), mode
        out[mode] = (H.scalars_to_row(ctx.get_scalars()), H.download_snapshot(ctx, names))
        ctx.close()
    np.testing.assert_array_equal(out["deferred"][0], out["stored"][0])
    assert np.array_equal(out["deferred"][1], out["stored"][1], equal_nan=True)


@pytest.mark.parametrize("case", [WEIGHTED_CASES[0], STATION_CASES[0]])
def test_one_launch_front_equals_the_predicate_kernels(native, monkeypatch, case, cell_agg_split):
    """Per-cell forcing, round 4: ONE per-column launch in front of the fused kernel (k_cell_front: the columns' aggregates, word 1's
    terms for every candidate selection, the bookkeeping by its last wavefront) against the five launches of the predicate-kernel
    generation (RH_PER_CELL_OLD_FRONT=1): the same scalars after every call and the same planes, bit for bit -- device-side hooks, in
    pieces that end inside days."""
    import hip_util as H

    g, names, forcing = load_case(case)
    w = load_weights(g)
    nsteps = int(g["nsteps"])
    out = {}
    for mode in ("front", "old"):
        if mode == "old":
            monkeypatch.setenv("RH_PER_CELL_OLD_FRONT", "1")
        else:
            monkeypatch.delenv("RH_PER_CELL_OLD_FRONT", raising=False)
        ctx = _ctx(native, g, names)
        st = load_stations(g)
        if st is not None:
            ctx.set_forcing_stations(dict(PREC=st["PREC"], TA=st["TA"], PET=st["PET"], YEAR=forcing["YEAR"], MONTH=forcing["MONTH"],
                                          DOY=forcing["DOY"]), st["station_index"])
        else:
            ctx.set_forcing_series(forcing)
        ctx.set_forcing_weights(w["prec_weight"], w["ta_offset"], w["pet_weight"])
        rows, done = [], 0
        for stop in sorted({7, 50, 51, nsteps // 2, nsteps}):
            ctx.run_steps(stop - done)
            done = stop
            rows.append((H.scalars_to_row(ctx.get_scalars()), H.download_snapshot(ctx, names)))
        out[mode] = rows
        ctx.close()
    for (sa, pa), (sb, pb) in zip(out["front"], out["old"]):
        np.testing.assert_array_equal(sa, sb)
        assert np.array_equal(pa, pb, equal_nan=True)
    np.testing.assert_array_equal(out["front"][-1][0], g["scal"][nsteps - 1])


def test_hooks_phase_between_fused_steps(native):
    """rh_hooks_phase rewrites the control scalars (itt_forc, itt_day, the calendar) and the day's forcing: a control part that the
    previous fused kernel's tail formed for the next step is stale after it.  [rh_hooks_phase; rh_svat_step] per step
    equals rh_run_steps over several midnights and a month change."""
    import hip_util as H

    g, names, forcing = load_case("svat_hetero_combo")
    nsteps = int(g["nsteps"])
    a = _ctx(native, g, names)
    a.set_forcing_series(forcing)
    a.run_steps(nsteps)
    b = _ctx(native, g, names)
    b.set_forcing_series(forcing)
    days = set()
    for _ in range(nsteps):
        b.call("rh_hooks_phase")
        b.step(-1)
        days.add(b.get_scalars().time // 86400)
    assert len(days) >= 10
    np.testing.assert_array_equal(H.scalars_to_row(a.get_scalars()), H.scalars_to_row(b.get_scalars()))
    np.testing.assert_array_equal(H.scalars_to_row(b.get_scalars()), g["scal"][nsteps - 1])
    np.testing.assert_array_equal(H.download_snapshot(a, names), H.download_snapshot(b, names))
    a.close()
    b.close()


@pytest.mark.parametrize("case", ["svat_hetero_combo", "oned_hetero_heavyrain"])
def test_time_limit_stops_the_run_on_the_device(native, case):
    """rh_set_time_limit: `while vs.time - start_time < runlen: step()` (roger/roger.py:548-556) decided by the control part on the
    device.  More steps are enqueued than the run has left; exactly the reference's steps run, the step that reaches the limit
    stores every plane (the others of the call ran with sparse stores), the launches behind it change nothing -- accumulators
    included --, and a later limit continues the run."""
    import hip_util as H

    g, names, forcing = load_case(case)
    stops = sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit())
    stop = next(s for s in stops if s >= 40)     # a stored step: its end time is the limit
    t_stop = int(g["scal"][stop - 1][1])
    ctx = _ctx(native, g, names)
    ctx.set_forcing_series(forcing)
    ctx.diag_configure(rate=["S_fp_rz"], collect=["S_lp_rz"], n_slots=64)   # (state planes: sparse stores stay on)
    ctx.set_time_limit(t_stop)
    ctx.enable_timing(True)
    ctx.run_steps(stop + 37)
    ms, dts = ctx.timing_detail()
    ctx.enable_timing(False)
    assert len(ms) == stop + 37 and (dts[:stop] > 0).all() and (dts[stop:] == 0).all()   # the launches behind the limit did nothing
    assert ctx.sparse_steps() >= stop - 2
    s = ctx.get_scalars()
    np.testing.assert_array_equal(H.scalars_to_row(s), g["scal"][stop - 1])
    snap = H.download_snapshot(ctx, names)
    compare(snap, g[f"s{stop:05d}"], names, what=f"{case}: stopped by the time limit at step {stop}")
    day = (t_stop - 1) // 86400     # the output interval the last step belongs to
    acc = ctx.diag_download("S_fp_rz", day % 64), ctx.diag_steps(day % 64)
    ctx.run_steps(5)                                                   # over: nothing is even enqueued
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][stop - 1])
    np.testing.assert_array_equal(H.download_snapshot(ctx, names), snap)
    np.testing.assert_array_equal(ctx.diag_download("S_fp_rz", day % 64), acc[0])
    assert ctx.diag_steps(day % 64) == acc[1]
    nxt = next(s for s in stops if s > stop)
    ctx.set_time_limit(int(g["scal"][nxt - 1][1]))                     # the run goes on to the next stored step
    ctx.run_steps(10 * (nxt - stop) + 100)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][nxt - 1])
    compare(H.download_snapshot(ctx, names), g[f"s{nxt:05d}"], names, what=f"{case}: second limit, step {nxt}")
    ctx.set_time_limit(None)
    ctx.run_steps(3)
    np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][nxt + 2])
    ctx.close()


def test_eberbaechle_full_series_80x53(native):
    """BASELINE configs[4] as written (VERDICT r2 missing #4): catchment_scale Eberbaechle, 80 x 53 = 4 240 columns of 25 m, per-cell
    prec_weight / ta_offset / pet_weight on the station's FULL 2019-2022 series (157 824 ten-minute records, read from the shipped
    text files), stepped on the device without the host in the loop (rh_set_forcing_series + rh_set_forcing_weights + rh_run_steps).
    The grid repeats the twelve parameter sets and weights of the reference's golden run (`parameters.nc` is not shipped), so the
    global predicates -- and with them every step length -- are the golden run's: the step length of EVERY one of the 14 622 steps
    (the device's own log), the integer scalars and every plane of every column at the stored steps are the reference's."""
    import os

    import hip_util as H
    from golden_util import GOLDEN_DIR
    from roger_amd.forcing import forcing_from_txt

    g, names, _ = load_case("svat_eberbaechle_full")
    forcing = forcing_from_txt(os.path.join(GOLDEN_DIR, "eberbaechle_full_input"))
    w = load_weights(g)
    nx, ny, n12 = 80, 53, 12
    rep = np.arange(nx * ny) % n12
    ctx = native.Context(nx, ny)
    for row, nm in zip(g["state0"], names):
        if nm in ctx.index and ctx.index[nm] < ctx.planes_held:
            ctx.upload(nm, row[rep])
    ctx.set_scalars(H.scalars_from_row(g["scal0"]))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    ctx.set_forcing_series(forcing)
    ctx.set_forcing_weights(w["prec_weight"][rep], w["ta_offset"][rep], w["pet_weight"][rep])
    nsteps = int(g["nsteps"])
    ctx.enable_timing(True)
    done = 0
    import time

    t0 = time.perf_counter()
    for step in sorted(int(k[1:]) for k in g.files if k.startswith("s") and k[1:].isdigit()):
        ctx.run_steps(step - done)
        done = step
        np.testing.assert_array_equal(H.scalars_to_row(ctx.get_scalars()), g["scal"][step - 1], err_msg=f"step {step}")
        got = H.download_snapshot(ctx, names)
        compare(got, g[f"s{step:05d}"][:, rep], names, what=f"Eberbaechle 80 x 53, step {step}")
    wall = time.perf_counter() - t0
    assert done == nsteps and ctx.get_scalars().sanity_ok == 1 and ctx.get_scalars().time == 1096 * 86400
    ms, dts = ctx.timing_detail()
    np.testing.assert_array_equal(dts, g["scal"][:, 2].astype(np.int32))     # the step length of every step
    print(f"EBERBAECHLE 80x53 full series: {nsteps} steps in {wall:.2f} s incl. 18 state downloads ({nsteps / wall:.0f} steps/s, "
          f"{nsteps * nx * ny / wall:.3e} cell-timesteps/s); fused kernel {ms.mean() * 1e3:.1f} us per step")
    ctx.close()


def test_window_sums_are_numpys(native):
    """The hourly window sums (np.sum over a 144-slot series masked to [itd, itd + 6), adaptive_time_stepping.py:400-420) as the kernels
    form them -- one of eight rotations of numpy's pairwise tree where the window lies inside one 72-block, the general path otherwise --
    against numpy's own sum over the masked vector, for EVERY window start incl. the ones that leave the day or straddle slot 72, on
    values whose sums depend on the order of the additions."""
    from roger_amd import _native as N

    rng = np.random.default_rng(11)
    for trial in range(6):
        v = rng.uniform(-1.0, 1.0, 144) * 10.0 ** rng.integers(-12, 6, 144)
        if trial == 1:
            v[rng.integers(0, 144, 40)] = 0.0
            v[rng.integers(0, 144, 10)] = -0.0
        itd = np.arange(-7, 146, dtype=np.int64)
        fast, general = N.selftest_window_sum(v, itd)
        want = np.empty(itd.size)
        k = np.arange(144)
        for j, t in enumerate(itd):
            want[j] = np.sum(np.where((k >= t) & (k < t + 6), v, 0.0))
        assert np.array_equal(general.view(np.int64), want.view(np.int64))
        assert np.array_equal(fast.view(np.int64), want.view(np.int64))
