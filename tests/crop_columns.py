"""Columns with crops (lu_id 500-599), for the tests that pin the crop branches of rh_physics.h to the oracle: the carried and clamped
k_stress_transp and the anoxia override of rt_evapotranspiration, the ground storage lu_id 599 never fills and the partial ground
throughfall of rt_interception, throughfall_coeff_ground of rt_params_surface and the 200 mm roots of rt_params_soil.  None of them
needs a row of the look-up tables.  Crop phenology itself (enable_crop_phenology, core/crop.py) is not part of this project: the planes
that module owns are set by hand here (start state "grown").

Built on extended_columns (its primaries, its oracle_state, its forcing) with a generator of its own; extended_columns.LU_POOL and
what depends on its sequence stay as they are.

Land uses      two columns of three are crops, cycling through CROP_LU: every bound of the four predicates from both sides (500 and 599
               are crops without anoxia, 597 / 598 straddle the throughfall bound); the third cycles through OTHER_LU (ordinary and
               water land uses), so that wavefronts are mixed
Soils          theta_ac, theta_ufc and theta_pwp are rounded to multiples of 2**-10: their sums, and the products with z_root = 200 mm,
               are then exact, so a root zone filled to theta_sat has S_lp_rz / S_ac_rz == 1 exactly and one at field capacity == 0
Water content  theta_rz0 = theta_pwp + theta_ufc + f * theta_ac with f cycling through F_POOL per column (period 4 against the land
               uses' 7: every pair occurs).  Every second crop column with f == 0 gets theta_ac <= 0.2 * theta_fc, so that field
               capacity lies above the anoxia threshold 0.8 * theta_sat: ratio 0, transp_coeff 1
Layouts        "interleaved"; "blocks" puts five whole wavefronts in front (BLOCK_KINDS), the rest interleaved
Start states   "as_set_up": what the setup kernels leave -- for crops ground_cover = basal_transp_coeff = S_int_ground_tot = 0,
               throughfall_coeff_ground = 1 for 500..597, z_root = 200: anoxia is the only way a crop transpires;
               "grown": the planes of grown_planes() overwritten on the crop columns.  k_stress_transp has a single time level.
               The month change of run_forcing runs rt_params_surface, which puts the crops' planes back to the set-up values (not
               k_stress_transp: no setup kernel writes it)."""
import numpy as np

import extended_columns as E

CROP_LU = (500, 501, 510, 550, 597, 598, 599)
OTHER_LU = (8, 10, 0, 13, 14, 20)
F_POOL = (0.0, 0.3, 0.7, 1.0)
K_STRESS = (0.0, 0.3, 0.7, 1.0, 1.4)        # 1.4: the clamp
S_INT_GROUND_TOT = (0.0, 0.4, 1.0, 2.5)
BLOCK = E.BLOCK
# layout "blocks": (lu_id, f or None for the cycle) of the whole wavefronts in front; the fifth is half 550, half lu_id 8
BLOCK_KINDS = ((550, 1.0), (599, None), (500, None), (550, 0.3), ((550, 8), None))
UNIFORM = slice(3 * BLOCK, 4 * BLOCK)       # identical primaries: the per-wave parameter words over crop lanes
DIVERGENT = slice(4 * BLOCK, 5 * BLOCK)
STARTS = ("as_set_up", "grown")
GRID = 1.0 / 1024
# The seed of the 1000-column runs, chosen as extended_columns.RUN_SEED was: the first whose columns stay inside golden_util.compare_bulk
# over the 12-day free run in both layouts, measured with the host-compiled column code against the oracle
# (tests/test_physics_host_vs_oracle_crops.py: the free-run test), not with the device.  32 was the first tried and met no residue tie.
RUN_SEED = 32


def is_crop(lu):
    lu = np.asarray(lu)
    return (lu >= 500) & (lu < 600)


def _cycle(n):
    """lu_id and f of n interleaved columns."""
    i = np.arange(n)
    crop = i % 3 != 2
    j = np.cumsum(crop) - 1             # the how-manieth crop
    k = np.cumsum(~crop) - 1
    lu = np.where(crop, np.array(CROP_LU)[j % len(CROP_LU)], np.array(OTHER_LU)[k % len(OTHER_LU)])
    f = np.where(crop, np.array(F_POOL)[j % len(F_POOL)], np.array(F_POOL)[k % len(F_POOL)])
    low_ac = crop & (f == 0.0) & ((j // (len(CROP_LU) * len(F_POOL))) % 2 == 0)
    return lu, f, low_ac


def crop_params(nx, ny, seed, layout="interleaved", groundwater="mixed"):
    """extended_params(nx, ny, seed, groundwater) with lu_id, sealing, the three porosities (rounded) and theta_rz0 overridden."""
    if layout not in ("interleaved", "blocks"):
        raise ValueError(f"layout {layout!r}: 'interleaved' or 'blocks'")
    n = nx * ny
    p = {k: np.array(v).reshape(n) for k, v in E.extended_params(nx, ny, seed, groundwater, "interleaved").items()}
    rng = np.random.default_rng([int(seed), 500])
    for k in ("theta_ac", "theta_ufc", "theta_pwp"):
        p[k] = np.round(p[k] / GRID) * GRID
    if layout == "blocks":
        head = BLOCK * len(BLOCK_KINDS)
        if n < head:
            raise ValueError(f"layout 'blocks' needs at least {head} columns")
        lu, f, low_ac = _cycle(n - head)
        cyc = np.array(F_POOL)[np.arange(BLOCK) % len(F_POOL)]
        hl, hf = [], []
        for kind, fk in BLOCK_KINDS:
            hl.append(np.repeat(kind, BLOCK // 2) if isinstance(kind, tuple) else np.full(BLOCK, kind))
            hf.append(cyc if fk is None else np.full(BLOCK, fk))
        lu, f, low_ac = np.concatenate(hl + [lu]), np.concatenate(hf + [f]), np.concatenate([np.zeros(head, dtype=bool), low_ac])
        for k in p:
            p[k][UNIFORM] = p[k][UNIFORM.start]
        p["z_gw"][UNIFORM] = E.UNIFORM_Z_GW
        low_ac[UNIFORM] = True        # (f = 0.3: anoxic with theta_ac <= 0.4 * theta_fc)
    else:
        lu, f, low_ac = _cycle(n)
    fc = p["theta_ufc"] + p["theta_pwp"]
    p["theta_ac"] = np.where(low_ac, np.minimum(p["theta_ac"], np.maximum(np.floor(0.2 * fc / GRID), 1.0) * GRID), p["theta_ac"])
    p["lu_id"] = lu
    p["sealing"] = np.where(lu == 0, rng.uniform(0.2, 0.8, n), 0.0)
    if layout == "blocks":
        p["sealing"][UNIFORM] = 0.0
    p["f_rz0"] = f
    p["theta_rz0"] = p["theta_pwp"] + p["theta_ufc"] + f * p["theta_ac"]
    return {k: v.reshape(nx, ny) for k, v in p.items()}


def grown_planes(lu, seed):
    """The planes the reference's crop module owns, for every column (only the crop columns' values are used)."""
    lu = np.asarray(lu).ravel()
    n = lu.size
    rng = np.random.default_rng([int(seed), 599])
    gc = rng.uniform(0.1, 0.9, n)
    lai = np.log(1 / (1 - gc)) / np.log(1 / 0.7)
    return dict(ground_cover=gc, lai=lai, basal_transp_coeff=rng.uniform(0.2, 1.1, n), basal_evap_coeff=1 - gc,
                S_int_ground_tot=rng.choice(S_INT_GROUND_TOT, n),
                throughfall_coeff_ground=np.where(lu < 598, np.where(lai > 1, 0.1, 1 - lai), 0.0),
                k_stress_transp=rng.choice(K_STRESS, n))


def apply_grown(planes, lu, seed):
    """Overwrites grown_planes on the crop columns of `planes` (a dict of arrays, in place); returns what was written."""
    g = grown_planes(lu, seed)
    crop = is_crop(np.asarray(lu).ravel())
    for k, v in g.items():
        planes[k][crop] = v[crop]
    return g


def crop_start(ob, nx, ny, seed, layout, luts, lateral=False, start="as_set_up", month=None, groundwater="mixed"):
    """The oracle's start state of crop_params; month: the calendar of run_forcing (extended_columns.START_MONTH), as run_start."""
    if start not in STARTS:
        raise ValueError(f"start {start!r}: one of {STARTS}")
    p = crop_params(nx, ny, seed, layout, groundwater)
    st = E.oracle_state(ob, p, luts, lateral)
    if month is not None:
        st.scal.month[0] = st.scal.month[1] = month
        st.scal.doy[0] = st.scal.doy[1] = E.START_DOY
        st.params_surface()
    if start == "grown":
        apply_grown(st.planes, st.planes["lu_id"], seed)
    return st
