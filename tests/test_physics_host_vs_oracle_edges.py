"""The branch directions of the device's column code (roger_amd/csrc/rh_physics.h, compiled for the host) that no other column set
takes, against the oracle, on the columns and the forcing of tests/edge_columns.py and with the walk of
tests/test_physics_host_vs_oracle.py: every routine at every step from the ORACLE's state, the whole core in one call, for SVAT and
oneD, in both layouts, with the forcing shared by all columns and handed over per cell.  tools/physics_branches.py measures which
directions the walks take (profiles/physics_branches.txt).

A census over the oracle's states alone keeps the tests from passing by not arriving: for every arm it counts the (column, step)
pairs that take it and those that do not, and both must be positive.  Three arms one would look for among these columns cannot be taken by
any finite state, in the oracle as little as in rh_physics.h; the census holds what stands next to them, and the walk asserts that
they stay untaken:

  h_melt's `full` (melt > swe)            melt is `pot` where pot <= swe and `swe` where pot > swe: never above swe.  What a thin pack
                                          takes is the second select (`pot > swe`: melt_out), which is counted
  the drip's `wtmx <= 0 && over`          h_melt leaves swe_top at exactly 0 (swe += -swe), so wtmx = 0 and q_ret = S_int_top; with
                                          `over`, S_int_top > S_int_top_tot >= 0 = wtmx: the first select (`q_ret > wtmx`) has it
  q_sof > 0                               the two clamps ahead of it leave S_fp_rz <= S_ufc_rz and S_lp_rz <= S_ac_rz, and rounding is
                                          monotonic: the sum cannot exceed S_ac_rz + S_ufc_rz.  Counted instead: a root zone whose
                                          large pores over-fill (the excess goes back to the surface) above a full subsoil

CENSUS, measured (column, step) pairs "taken / not taken" per walk: printed by test_census_every_arm_both_ways."""
import functools

import numpy as np
import pytest

import edge_columns as EC
import extended_columns as E
import host_physics as HP
from test_physics_host_vs_oracle import NX, NY, N, Blocks, _luts, _twin, walk_from

LAYOUTS = ("interleaved", "blocks")


class EdgeCensus:
    """Observer of walk_from: per arm [taken, not taken], from the oracle's planes alone."""

    def __init__(self, st):
        self.st, self.s = st, st.settings
        self.c = {}
        self.keep = {}
        self.bad = []
        self.both_melts_in_one_step = 0

    def count(self, arm, taken, among):
        c = self.c.setdefault(arm, [0, 0])
        c[0] += int((taken & among).sum())
        c[1] += int((~taken & among).sum())

    def before(self, name, P):
        if name == "rt_interception":
            self.keep = {k: P[k].copy() for k in ("S_int_ground", "S_int_ground_tot", "throughfall_coeff_top", "throughfall_coeff_ground")}
        elif name == "rt_snow":
            self.keep = {k: P[k].copy() for k in ("swe", "swe_top", "S_int_top", "S_int_top_tot", "snow_ground")}
        elif name == "rt_infiltration":
            self.keep = {k: P[k].copy() for k in ("prec", "prec_m1")}
            self.keep["conds"] = HP.infiltration_conds(self.st)

    def after(self, name, P, H, step):
        K, catch = self.keep, P["maskCatch"] == 1
        lu, ta = P["lu_id"], P["ta"]
        if name == "rt_interception":
            frozen, wet = ta <= self.s.ta_fm, P["prec"] > 0
            for x in (10, 11, 12):
                self.count(f"cold_forest_{x}", ta < -3, catch & (lu == x))
                self.count(f"mid_forest_{x}", (ta >= -3) & (ta <= -1), catch & (lu == x))
                self.count(f"warm_forest_{x}", ta > -1, catch & (lu == x))
            want = P["prec"] * (1. - K["throughfall_coeff_top"])
            self.count("int_snow_top_positive", P["int_snow_top"] > 0, catch & frozen & wet)
            self.count("canopy_room_below_snowfall", P["int_snow_top"] < want, catch & frozen & wet & (P["int_snow_top"] > 0))
            snow = P["prec"] - P["int_snow_top"]
            want = snow * (1. - K["throughfall_coeff_ground"])
            room = K["S_int_ground_tot"] - K["S_int_ground"]
            self.count("ground_room_takes_all_snow", room >= want, catch & frozen & wet & (room > 0) & (lu != 599))
        elif name == "rt_snow":
            pot = self.s.sf * (ta - self.s.ta_fm) * float(self.st.scal.dt)
            swe = K["swe"] + np.where(ta <= self.s.ta_fm, K["snow_ground"], 0.0)
            melting = catch & (pot > 0) & (swe > 0)
            self.count("pack_melts_out", pot > swe, melting)
            self.both_melts_in_one_step += int((melting & (pot > swe)).any() and (melting & (pot <= swe)).any())
            self.count("canopy_drips", P["snow_melt_drip"] > 0, catch & (lu >= 10) & (lu <= 12))
            self.count("canopy_over_its_liquid_capacity", K["S_int_top"] > K["S_int_top_tot"], catch & (K["S_int_top"] > 0))
            for who, planes in (("oracle", P), ("host routine", H)):
                if (planes["swe_top"][catch] != 0).any() and len(self.bad) < 6:
                    self.bad.append(f"step {step}: {who}: swe_top is not zero behind rt_snow")
        elif name == "rt_infiltration":
            c1, c2, c3, c4, c5 = K["conds"]
            p0, pm = K["prec"], K["prec_m1"]
            if c2:
                self.count("pause_starts_here", (p0 == 0) & (pm != 0), catch)
                self.count("pause_start_elsewhere_rain_goes_on", p0 != 0, catch & ~((p0 == 0) & (pm != 0)))
            if c3:
                self.count("pause_ends_here", (p0 != 0) & (pm == 0), catch)
                self.count("pause_end_elsewhere_still_dry", p0 == 0, catch & ~((p0 != 0) & (pm == 0)))
            full_ss = (P["S_lp_ss"] + P["S_fp_ss"]) >= (P["S_ac_ss"] + P["S_ufc_ss"])
            self.count("root_zone_overfills_above_a_full_subsoil", (P["S_lp_rz"] == P["S_ac_rz"]) & (P["S_fp_rz"] == P["S_ufc_rz"]) & (P["q_hof"] > 0),
                       catch & full_ss)
            for who, planes in (("oracle", P), ("host routine", H)):
                if (planes["q_sof"] != 0).any() and len(self.bad) < 6:
                    self.bad.append(f"step {step}: {who}: q_sof is not zero")


def _driver(ob, F, per_cell, layout):
    if not per_cell:
        return None
    stations, weights = EC.cell_forcing(F, N, layout)
    return ob.ForcingDriver(F, weights=weights, stations=stations)


@functools.lru_cache(maxsize=None)
def edge_walk(lateral, layout, per_cell):
    """(mismatches per routine, the walk's own census, the arms' census, violations, steps with both kinds of melt)"""
    import oracle_binding as ob

    ob.build()
    st = EC.edge_start(ob, NX, NY, layout, _luts(lateral), lateral)
    obs = EdgeCensus(st)
    F = EC.edge_forcing()
    bad, census = walk_from(ob, st, F, lateral, obs, driver=_driver(ob, F, per_cell, layout))
    return bad, census, obs.c, obs.bad, obs.both_melts_in_one_step


WALKS = [(False, "interleaved", False), (True, "interleaved", True), (False, "blocks", True), (True, "blocks", False)]


def _id(w):
    return f"{'oneD' if w[0] else 'svat'}-{w[1]}-{'per_cell' if w[2] else 'shared'}"


def setup_census(p, planes, settings):
    """Per setup edge [taken, not taken], from the primaries and the oracle's planes."""
    pwp, ac, z_soil, lu = (p[k].ravel() for k in ("theta_pwp", "theta_ac", "z_soil", "lu_id"))
    crop = (lu >= 500) & (lu < 600)
    c = {}

    def count(arm, taken, among=np.ones(pwp.size, dtype=bool)):
        c[arm] = [int((taken & among).sum()), int((~taken & among).sum())]

    count("theta_pwp_below_rew_min", pwp < settings.theta_rew_min)
    count("theta_pwp_in_rew_range", (pwp >= settings.theta_rew_min) & (pwp <= settings.theta_rew_max))
    count("theta_pwp_above_rew_max", pwp > settings.theta_rew_max)
    count("sand_clamped_at_1", ac / 0.24 > 1)
    count("clay_clamped_at_clay_min", planes["clay"] == settings.clay_min)
    count("tabulated_roots_reach_the_soil_depth", planes["z_root"] == settings.zroot_to_zsoil_max * z_soil, ~crop)
    count("crop_roots_reach_the_soil_depth", z_soil <= 200.0, crop)
    count("theta_rz_at_or_below_theta_pwp", p["theta_rz0"].ravel() <= pwp)
    count("theta_ss_at_or_below_theta_pwp", p["theta_ss0"].ravel() <= pwp)
    return c


@pytest.mark.parametrize("lateral", [False, True], ids=["svat", "oneD"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_setup_kernels_on_edge_columns(oracle, lateral, layout):
    """rt_topo, rt_params_surface, rt_params_soil and rt_initial_conditions from the primaries: every plane; every setup edge is
    among the columns, from both sides; and, from the primaries alone, rew, sand and the root depth at the edges."""
    p = EC.edge_params(NX, NY, EC.SEED, layout)
    luts = _luts(lateral)
    a = oracle.OracleState(N)
    E.load_primaries(a, p, luts, lateral)
    A = Blocks(a)
    B, host = _twin(oracle, a)
    B.take(A)
    X = HP.StepCtx(month_tau=int(a.scal.month[1]), sel_p=-1, sel_w=-1)
    for name, oracle_routine in (("rt_topo", a.topo), ("rt_params_surface", a.params_surface), ("rt_params_soil", a.params_soil),
                                 ("rt_initial_conditions", a.initial_conditions)):
        if name == "rt_initial_conditions":
            if lateral:
                a.params_lateral(luts[4])
            E.load_initial_state(a, p)
            EC.load_pack(a, p)
            B.take(A)
        oracle_routine()
        host.call(name, X)
        msg = B.equals(A, name)
        assert msg is None, msg
        B.take(A)
    s = a.settings
    c = setup_census(p, a.planes, s)
    print("SETUP CENSUS", layout, c)
    for arm, (taken, kept) in c.items():
        assert taken > 0 and kept > 0, f"{arm}: {taken} columns take it, {kept} do not"
    pwp, ac, z_soil, lu = (p[k].ravel() for k in ("theta_pwp", "theta_ac", "z_soil", "lu_id"))
    crop = (lu >= 500) & (lu < 600)
    for who, planes in (("oracle", a.planes), ("host", B.st.planes)):      # from the primaries alone
        np.testing.assert_array_equal(planes["rew"][pwp < s.theta_rew_min], s.rew_min, err_msg=who)
        np.testing.assert_array_equal(planes["rew"][pwp > s.theta_rew_max], s.rew_max, err_msg=who)
        np.testing.assert_array_equal(planes["sand"][ac > 0.24], 1.0, err_msg=who)
        np.testing.assert_array_equal(planes["z_root"][crop], np.where(z_soil <= 200.0, z_soil * 0.9, 200.0)[crop], err_msg=who)
        assert (planes["clay"] >= s.clay_min).all() and (planes["z_root"] < z_soil).all(), who
        np.testing.assert_array_equal(planes["theta_fp_rz"][p["theta_rz0"].ravel() <= pwp], 0.0, err_msg=who)
    for k in ("theta_rz", "theta_ss", "z_root", "S_rz", "S_ss", "k_rz", "h_rz", "clay", "rew", "tew"):      # no edge column starts as NaN
        assert np.isfinite(a.planes[k]).all(), k
    kind = EC.kind_of(N, layout)
    if layout == "blocks":
        assert all(np.unique(kind[w * EC.BLOCK:(w + 1) * EC.BLOCK]).size == 1 for w in range(N // EC.BLOCK))
    assert set(kind.tolist()) == set(range(len(EC.KINDS)))


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_each_routine_from_the_oracles_state(w):
    """The oracle's state before a routine through the device's routine equals the oracle's state after its own, at every step, on
    every plane at golden_util.RTOL / ATOL (integer planes exactly)."""
    bad, census, _, _, _ = edge_walk(*w)
    bad = {k: v for k, v in bad.items() if k != census["core"]}
    assert not bad, "\n".join(m for v in bad.values() for m in v)
    assert census["dt"] == {600, 3600, 86400} and census["steps"] > 40


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_whole_core_from_the_oracles_state(w):
    """rt_step_core[_lateral] in one call from the oracle's state after adaptive_dt, and the sanity bit it returns."""
    bad, census, _, _, _ = edge_walk(*w)
    assert census["core"] not in bad, "\n".join(bad[census["core"]])


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_the_arms_no_finite_state_takes_stay_untaken(w):
    """swe_top is exactly zero behind every rt_snow and q_sof is zero behind every rt_infiltration, in the oracle's state and in the
    host-compiled routine's: what the module's docstring derives."""
    _, _, _, violations, _ = edge_walk(*w)
    assert not violations, "\n".join(violations)


PER_CELL_ARMS = ("pause_start_elsewhere_rain_goes_on", "pause_end_elsewhere_still_dry")


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_census_every_arm_both_ways(w):
    """From the oracle's states, never from the code under test: every arm is taken by some (column, step) pairs and not taken by
    others.  With one forcing shared by all columns a pause starts and ends everywhere at once: there the arm that keeps the event's
    planes is not taken, which is what the per-cell walks are for."""
    _, census, c, _, both = edge_walk(*w)
    print("EDGE CENSUS", _id(w), c, "steps with a pack melting out and another not:", both)
    assert {10, 11, 12, 5, 550, 599, 0} <= census["lu"]
    for arm in ("pause_starts_here", "pause_ends_here", "root_zone_overfills_above_a_full_subsoil", "pack_melts_out", "cold_forest_11"):
        assert arm in c, f"{arm}: never evaluated"
    for arm, (taken, kept) in c.items():
        if not w[2] and arm in PER_CELL_ARMS:
            continue
        assert taken > 0, f"{arm}: no (column, step) pair takes it ({kept} do not)"
        if w[2] or arm not in ("pause_starts_here", "pause_ends_here"):
            assert kept > 0, f"{arm}: every (column, step) pair takes it ({taken})"
    if w[2]:
        for arm in PER_CELL_ARMS:
            assert arm in c, f"{arm}: never evaluated"
    assert both > 0, "pack_melts_out: no step in which one pack melts out and another does not"


@pytest.mark.parametrize("per_cell", [False, True], ids=["shared", "per_cell"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_free_run_of_the_host_core_stays_with_the_oracle(oracle, layout, per_cell):
    """The SVAT free run of test_hip_edge_columns.py with the host-compiled rt_step_core in place of the device: over the 8 days the
    two trajectories stay inside compare_bulk's present bounds on these columns, so the GPU test may rely on them."""
    from golden_util import compare_bulk

    st = EC.edge_start(oracle, NX, NY, layout, _luts(False), False)
    hs = oracle.OracleState(N)
    hs.luts, hs.settings = st.luts, st.settings
    hs.load_snapshot(st.snapshot(), st.names)
    hs.load_scalars(st.scalars_row())
    host = HP.HostColumns(hs)
    F = EC.edge_forcing()
    odrv, hdrv = (_driver(oracle, F, per_cell, layout) or oracle.ForcingDriver(F) for _ in range(2))
    step = 0
    while st.scal.time < EC.NDAYS * 86400:
        step += 1
        pd, td, ed, monthly = odrv.before_step(st)
        ok = st.step(pd, td, ed, monthly)
        pd, td, ed, monthly_h = hdrv.before_step(hs)
        assert not monthly and not monthly_h
        s = hs.scal
        hs.adaptive_dt(pd, td, ed)       # (the control part is not under test here: the oracle's, on the host run's own state)
        X = HP.step_ctx_from(hs)
        s.itt += 1
        s.time += s.dt_secs
        ok_h = host.call("rt_step_core", X)
        host.call("rt_after_timestep", X)
        for k in ("event_id", "year", "month", "doy"):
            getattr(s, k)[0] = getattr(s, k)[1]
        np.testing.assert_array_equal(hs.scalars_row(), st.scalars_row(), err_msg=f"step {step}")
        assert bool(ok_h) == bool(ok), f"step {step}: sanity bit {ok_h}, the oracle's {int(ok)}"
        if step % 25 == 0 or step < 3:
            compare_bulk(hs.snapshot(), st.snapshot(), st.names, what=f"{layout} step {step}")
    compare_bulk(hs.snapshot(), st.snapshot(), st.names, what=f"{layout} final")
    assert step > 40
