"""Columns and a forcing for the branch directions of rh_physics.h that no other column set takes (tools/physics_branches.py measures
them; profiles/physics_branches.txt holds the lists): the tests that pin those arms to the oracle are
tests/test_physics_host_vs_oracle_edges.py (host) and tests/test_hip_edge_columns.py (device).

Built on extended_columns (its primaries, its load_primaries) with a generator of its own.  Four kinds of column:

forest    lu_id 10 / 11 / 12 and 5 as a control, in turn.  The forcing's frost days pass through the three temperature classes of
          h_swe_top_tot (below -3, -3 .. -1, above -1) with a snowfall that fits the canopy's room (0.3 mm) and ones that exceed it
          (12, 25 and 60 mm in a daily step against 9 .. 50 mm of room): `room >= want` and `room < want` for the canopy, and under
          it a ground storage that takes all that falls through (0.03 mm) or fills up
pack      a snow pack at the start, 0.5 / 8 / 60 / 300 mm in turn: on the first thaw (0.5 degrees, 36 mm of potential melt in a daily
          step) the thin packs melt out (`pot > swe`) and the thick ones do not, in the same step
filling   120 .. 200 mm of soil, ks 0.05 .. 0.3 mm/h, an air capacity of 2 %, root zone and subsoil filled to the brim at the start, under
          the heavy rain of day 5: the large pores of the root zone over-fill above a full subsoil
setup     primaries at the edges of the setup kernels: theta_pwp below theta_rew_min, inside the range and above theta_rew_max;
          theta_ac above 0.24 (the sand clamp); a theta_pwp so low that the clay content falls to clay_min; 120 .. 200 mm of soil under
          a land use whose tabulated root depth is deeper (zroot_to_zsoil_max * z_soil) and under a crop (0.9 * z_soil); a start water
          content at and below theta_pwp

Layouts   "interleaved": the kinds in turn; "blocks": whole wavefronts of 64 columns hold one kind (wave w holds kind w % 4)
Forcing   edge_forcing(): 8 days.  Shared by all columns, or per cell (cell_forcing): three groups -- the series itself, the series
          with its precipitation 3 slots later (in some 10-minute slot an event or a pause starts for one group and not yet for the
          other) and a precipitation weight of zero (nothing ever starts).  In "blocks" waves 0-3 and 12-15 are of the first group,
          4-7 of the second and 8-11 of the third: an all-dry wave of every kind next to waves in an event.

What the reference cannot represent, and is therefore not drawn: z_soil == 0.  calc_parameters_root_zone gives z_root = 0 there, and
the initial conditions divide by it (soil.py: theta_rz = (S_fp_rz + S_lp_rz) / z_root + theta_pwp = 0 / 0): the column is NaN from the
start.  Nor a negative theta_ac (the lower sand clamp)."""
import numpy as np

import extended_columns as E

KINDS = ("forest", "pack", "filling", "setup")
BLOCK = E.BLOCK
FOREST_LU = (10, 11, 12, 5)
PACK_SWE = (0.5, 8.0, 60.0, 300.0)
PACK_LU = (8, 5, 13, 10, 6)
SHALLOW = (120.0, 150.0, 200.0)
SETUP_LU = (8, 550, 0, 5, 10, 599)
THETA_PWP = (0.01, 0.1, 0.3)           # below theta_rew_min = 0.02, inside, above theta_rew_max = 0.24
THETA_AC = (0.3, 0.1)                  # 0.3 / 0.24 > 1: the sand clamp
F_RZ0 = (-0.5, 0.0, 0.6)               # theta_rz0 = theta_pwp + f * theta_ufc (f < 0: below the wilting point)
NDAYS = 8
SHIFT = 3
SEED = 32
GROUPS = ("as_is", "later", "never")


def kind_of(n, layout):
    """The kind (index into KINDS) of each of n columns."""
    if layout not in ("interleaved", "blocks"):
        raise ValueError(f"layout {layout!r}: 'interleaved' or 'blocks'")
    i = np.arange(n)
    return (i // BLOCK) % len(KINDS) if layout == "blocks" else i % len(KINDS)


def group_of(n, layout):
    """The forcing group (index into GROUPS) of each of n columns under the per-cell forcing."""
    i = np.arange(n)
    return (i // (BLOCK * len(KINDS))) % len(GROUPS) if layout == "blocks" else (i // len(KINDS)) % len(GROUPS)


def edge_params(nx, ny, seed=SEED, layout="interleaved"):
    """extended_params(nx, ny, seed, "deep") with the kinds' primaries overridden, and swe0 (the snow pack at the start) added."""
    n = nx * ny
    p = {k: np.array(v).reshape(n) for k, v in E.extended_params(nx, ny, seed, "deep", "interleaved").items()}
    rng = np.random.default_rng([int(seed), 1122])
    kind = kind_of(n, layout)
    j = np.arange(n) // len(KINDS) if layout == "interleaved" else np.arange(n) % BLOCK     # the how-manieth of its kind (of its wave)
    lu = np.full(n, 8)
    swe0 = np.zeros(n)
    forest, pack, filling, setup = (kind == k for k in range(len(KINDS)))
    lu[forest] = np.array(FOREST_LU)[j[forest] % len(FOREST_LU)]
    lu[pack] = np.array(PACK_LU)[j[pack] % len(PACK_LU)]
    swe0[pack] = np.array(PACK_SWE)[j[pack] % len(PACK_SWE)]
    # a soil that fills
    p["z_soil"][filling] = np.array(SHALLOW)[j[filling] % len(SHALLOW)]
    p["ks"][filling] = rng.uniform(0.05, 0.3, n)[filling]
    p["theta_ac"][filling] = 0.02
    # setup edges
    lu[setup] = np.array(SETUP_LU)[j[setup] % len(SETUP_LU)]
    p["theta_pwp"][setup] = rng.choice(THETA_PWP, n)[setup]
    p["theta_ac"][setup] = rng.choice(THETA_AC, n)[setup]
    p["z_soil"][setup] = np.where(rng.random(n) < 0.5, rng.choice(SHALLOW, n), p["z_soil"])[setup]
    p["lmpv"] = np.minimum(p["lmpv"], np.round(p["z_soil"] * 0.95))
    p["lu_id"] = lu
    p["sealing"] = np.where(lu == 0, rng.uniform(0.2, 0.8, n), 0.0)
    sat = p["theta_ac"] + p["theta_ufc"] + p["theta_pwp"]
    f = rng.choice(F_RZ0, n)
    p["theta_rz0"] = np.where(setup, p["theta_pwp"] + f * np.where(f < 0, p["theta_pwp"], p["theta_ufc"]), p["theta_rz0"])
    p["theta_ss0"] = np.where(setup, p["theta_pwp"] + rng.choice(F_RZ0, n).clip(0) * p["theta_ufc"], p["theta_ss0"])
    p["theta_rz0"] = np.where(filling, sat, p["theta_rz0"])
    p["theta_ss0"] = np.where(filling, sat, p["theta_ss0"])
    p["swe0"] = swe0
    return {k: v.reshape(nx, ny) for k, v in p.items()}


def edge_forcing():
    """Eight days: frost with a snowfall below the canopy's room, cold frost with one above it, the middle class, frost above -1 degree,
    a mild thaw, heavy rain with a pause, moderate rain with two pauses, a dry day."""
    from roger_amd.forcing import _pack

    rng = np.random.default_rng([SEED, 8])
    prec = np.zeros(NDAYS * 144)
    ta = np.array([-5.0, -5.0, -2.0, -0.5, 0.5, 9.0, 11.0, 16.0])
    pet = np.array([0.4, 0.5, 0.6, 0.8, 1.0, 2.5, 2.0, 3.5])
    prec[20:30] = 0.03                                  # day 0: 0.3 mm
    prec[144 + 10:144 + 130] = 0.5                      # day 1: 60 mm
    prec[2 * 144 + 30:2 * 144 + 80] = 0.5               # day 2: 25 mm
    prec[3 * 144 + 40:3 * 144 + 70] = 0.4               # day 3: 12 mm
    k = 5 * 144 + 30                                    # day 5: heavy rain (10-minute steps), a pause, more of it
    prec[k:k + 18] = rng.uniform(0.5, 9, 18)
    prec[k + 30:k + 48] = rng.uniform(0.5, 9, 18)
    k = 6 * 144 + 12                                    # day 6: moderate rain with two pauses
    prec[k:k + 12] = rng.uniform(0.1, 1.2, 12)
    prec[k + 24:k + 40] = rng.uniform(0.1, 0.9, 16)
    prec[k + 60:k + 66] = rng.uniform(0.1, 0.9, 6)
    return _pack(prec, ta, pet, NDAYS, start="2018-01-20")


def cell_forcing(F, n, layout):
    """(stations, weights) of the per-cell forcing for oracle_binding.ForcingDriver(F, weights, stations) and for
    Context.set_forcing_stations / set_forcing_weights: two series (F's, and F's with the precipitation SHIFT slots later) and a
    precipitation weight of zero for the third group."""
    g = group_of(n, layout)
    later = np.roll(F["PREC"], SHIFT)
    later[:SHIFT] = 0.0
    stations = dict(PREC=np.stack([F["PREC"], later]), TA=np.stack([F["TA"], F["TA"]]), PET=np.stack([F["PET"], F["PET"]]),
                    station_index=np.where(g == 1, 1, 0).astype(np.int32))
    weights = dict(prec_weight=np.where(g == 2, 0.0, 1.0), ta_offset=np.zeros(n), pet_weight=np.ones(n))
    return stations, weights


def cell_day(F, stations, weights, i):
    """The (n, 144) arrays of the day that starts at slot i, as ForcingDriver.day_slice forms them."""
    idx = stations["station_index"]
    return (stations["PREC"][idx, i:i + 144] * weights["prec_weight"][:, None], stations["TA"][idx, i:i + 144] + weights["ta_offset"][:, None],
            stations["PET"][idx, i:i + 144] * weights["pet_weight"][:, None])


def load_pack(st, p):
    """The snow pack at the start, ahead of rt_initial_conditions (which sums S_sur)."""
    for nm in ("swe", "swe_m1", "S_snow", "S_snow_m1"):
        st.planes[nm][:] = p["swe0"].ravel()


def edge_start(ob, nx, ny, layout, luts, lateral=False, seed=SEED):
    """The oracle's start state of edge_params: extended_columns.oracle_state with the snow pack loaded ahead of the initial conditions."""
    p = edge_params(nx, ny, seed, layout)
    st = ob.OracleState(nx * ny)
    E.load_primaries(st, p, luts, lateral)
    st.topo()
    st.params_surface()
    st.params_soil()
    if lateral and len(luts) > 4:
        st.params_lateral(luts[4])
    E.load_initial_state(st, p)
    load_pack(st, p)
    st.initial_conditions()
    return st
