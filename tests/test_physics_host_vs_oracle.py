"""The device's column code (roger_amd/csrc/rh_physics.h, compiled for the host: tests/host_physics.cpp) against the oracle, routine
by routine, on columns the golden recipe never draws (tests/extended_columns.py): the water land uses 14 / 20 / 999 and with them columns
outside the catchment, every land use of the look-up tables and of the root-depth code, groundwater within reach of the soil, a
depression storage.  Crops (lu_id 500-599) go the same walk in tests/test_physics_host_vs_oracle_crops.py, on the columns of
tests/crop_columns.py; crop phenology itself (enable_crop_phenology) is out of scope.

Every comparison starts from the ORACLE's state: a copy of it before a routine goes through the host-compiled device routine and must
equal the oracle's state after its own routine on every plane, at the tolerance the project states for "HIP path against the oracle"
(golden_util.RTOL / ATOL) -- one routine from a common state has no drift, so there is no bulk allowance.  A disagreement names the
routine, the step and the plane.  A census over the oracle's states keeps the tests from passing by not reaching the branches.

What these tests cannot see: the cut `zgw - z_soil > 10000 ? 0 : cpr` in h_sub_pot_percolation_ss (and in the oracle).  cpr only decides
whether q_pot_ss is zeroed, it is already zero where the subsoil drains, and where it does not drain q_pot_ss is zero before the cut:
with or without that line every plane is the same, in both files."""
import functools

import numpy as np
import pytest

import extended_columns as E
import host_physics as HP
from golden_util import ATOL, RTOL, compare, compare_bulk, load_case

NX, NY = 40, 25
N = NX * NY
SEED = E.RUN_SEED
NDAYS = 12


def _luts(lateral):
    g, _, _ = load_case("svat_hetero_combo")
    luts = (g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    if lateral:
        luts += (load_case("oned_hetero_combo")[0]["lut_mlms"],)
    return luts


def _forcing(kind):
    from roger_amd.forcing import combo_forcing

    if kind == "combo":
        return combo_forcing(ndays=NDAYS)
    return E.run_forcing(ndays=8)   # the forcing of test_hip_parity.py::test_month_change_inside_device_driven_steps: April -> May on the third day


class Blocks:
    """An OracleState whose float64 and int32 planes are rows of two contiguous blocks: a snapshot is two copies, a comparison one call."""

    def __init__(self, st):
        self.st = st
        self.fnames = [nm for nm, ii in zip(st.names, st.is_int) if not ii]
        self.inames = [nm for nm, ii in zip(st.names, st.is_int) if ii]
        self.F = np.zeros((len(self.fnames), st.n))
        self.I = np.zeros((len(self.inames), st.n), dtype=np.int32)
        for block, names in ((self.F, self.fnames), (self.I, self.inames)):
            for k, nm in enumerate(names):
                block[k] = st.planes[nm]
                st.planes[nm] = block[k]
        st._refresh_ptrs()

    def take(self, other):
        self.F[:] = other.F
        self.I[:] = other.I

    def _surely_equal(self, ref):
        """golden_util.compare's own criterion (the same bits, or close) on the planes that differ at all; a False is for compare to judge."""
        if not hasattr(self, "_same"):
            self._same = np.empty(self.F.shape, dtype=bool)
        np.equal(self.F.view(np.uint64), ref.F.view(np.uint64), out=self._same)
        rows = np.flatnonzero(~self._same.all(axis=1))
        if rows.size:
            got, want = self.F[rows], ref.F[rows]
            with np.errstate(all="ignore"):
                if not (self._same[rows] | (np.abs(got - want) <= ATOL + RTOL * np.abs(want))).all():
                    return False
        return np.array_equal(self.I, ref.I)

    def equals(self, ref, what):
        """This state against `ref` on every plane (integer planes exactly); the message of a mismatch, or None."""
        if self._surely_equal(ref):
            return None
        try:
            compare(self.F, ref.F, self.fnames, rtol=RTOL, atol=ATOL, what=what)
            compare(self.I, ref.I, self.inames, rtol=0.0, atol=0.0, what=what)
        except AssertionError as e:
            return str(e)
        return None


def _twin(ob, st):
    tw = ob.OracleState(st.n)
    tw.luts, tw.settings = st.luts, st.settings
    b = Blocks(tw)
    return b, HP.HostColumns(tw)


def _start(ob, lateral, groundwater, layout="interleaved", month=None):
    if month is not None:
        return E.run_start(ob, NX, NY, SEED, groundwater, layout, _luts(lateral), lateral)
    return E.oracle_state(ob, E.extended_params(NX, NY, SEED, groundwater, layout), _luts(lateral), lateral)


@functools.lru_cache(maxsize=None)
def walk(lateral, groundwater, forcing_kind):
    """The oracle, routine by routine, through the forcing; the host-compiled device routines on copies of its states.
    Returns (mismatches per routine: first messages, census from the oracle's states)."""
    import oracle_binding as ob

    ob.build()
    st = _start(ob, lateral, groundwater, month=4 if forcing_kind == "month_change" else None)
    return walk_from(ob, st, _forcing(forcing_kind), lateral)


def walk_from(ob, st, F, lateral, observer=None, driver=None):
    """walk() from the start state `st` through the forcing `F`.  observer: before(name, P) sees the oracle's planes P ahead of every
    routine of the step, after(name, P, H, step) the oracle's planes behind it and those the host-compiled routine left (H).
    driver: an oracle_binding.ForcingDriver over F in place of the plain one (per-cell weights, stations)."""
    O = Blocks(st)
    T, host = _twin(ob, st)      # one routine at a time
    W, whole = _twin(ob, st)     # the whole core in one call
    drv = driver if driver is not None else ob.ForcingDriver(F)
    sub, err, core = (("rt_subsurface_runoff_lateral", "rt_num_error_lateral", "rt_step_core_lateral") if lateral
                      else ("rt_subsurface_runoff", "rt_num_error", "rt_step_core"))
    routines = (("rt_interception", st.interception), ("rt_evapotranspiration", st.evapotranspiration), ("rt_snow", st.snow),
                ("rt_infiltration", st.infiltration), (sub, st.subsurface_runoff), ("rt_capillary_rise", st.capillary_rise),
                ("rt_storage", st.storage), (err, st.num_error))
    bad = {}
    P = st.planes
    catch = None
    zgw = P["z_gw"] * 1000
    census = dict(steps=0, monthly=0, catch_steps=0, shallow=0, near_no_percolation=0, dep=0, dt=set())
    ndays = int(F["PREC"].size // 144)
    while st.scal.time < ndays * 86400:
        pd, td, ed, monthly = drv.before_step(st)
        cond_time = int(st.scal.time % 86400 == 0)
        st.adaptive_dt(pd, td, ed)
        st.scal.itt += 1
        st.scal.time += st.scal.dt_secs
        step = int(st.scal.itt)
        X = HP.step_ctx_from(st, cond_time)
        if monthly:
            T.take(O)
            st.params_surface()
            host.call("rt_params_surface", X)
            msg = T.equals(O, f"rt_params_surface, step {step}")
            if msg:
                bad.setdefault("rt_params_surface", []).append(msg)
        W.take(O)
        ok_whole = whole.call(core, X)
        for name, oracle_routine in routines:
            T.take(O)
            if observer is not None:
                observer.before(name, P)
            ok_o = oracle_routine()
            ok_h = host.call(name, X)
            if observer is not None:
                observer.after(name, P, T.st.planes, step)
            msg = T.equals(O, f"{name}, step {step} (dt {st.scal.dt_secs} s)")
            if msg is None and name == err and bool(ok_h) != bool(ok_o):
                msg = f"{name}, step {step}: sanity bit {ok_h}, the oracle's {int(ok_o)}"
            if msg:
                bad.setdefault(name, []).append(msg)
            if name == sub:     # census: the oracle's state behind the percolation
                catch = P["maskCatch"] == 1
                census["catch_steps"] += int(catch.sum())
                census["shallow"] += int((catch & (P["z_gw"] <= 10) & (zgw > P["z_soil"]) & (P["z_sat"] > 0)).sum())
                gap = zgw - P["z_soil"]
                census["near_no_percolation"] += int((catch & (gap > 0) & (gap <= 10000) & (P["q_pot_ss"] == 0)).sum())
        msg = W.equals(O, f"{core}, step {step} (dt {st.scal.dt_secs} s)")
        if msg is None and bool(ok_whole) != bool(st.scal.sanity_ok):
            msg = f"{core}, step {step}: sanity bit {ok_whole}, the oracle's {int(st.scal.sanity_ok)}"
        if msg:
            bad.setdefault(core, []).append(msg)
        census["dep"] += int((catch & (P["S_dep"] > 0)).sum())
        census["steps"] += 1
        census["monthly"] += int(monthly)
        census["dt"].add(int(st.scal.dt_secs))
        st.after_timestep()
    census.update(lu=set(np.unique(P["lu_id"]).tolist()), river=int(((P["lu_id"] == 20) & (P["maskRiver"] == 1) & (P["maskCatch"] == 0)).sum()),
                  lake=int(((P["lu_id"] == 14) & (P["maskLake"] == 1) & (P["maskCatch"] == 0)).sum()),
                  outside=int(((P["lu_id"] == 999) & (P["maskCatch"] == 0)).sum()),
                  below_gw=int((catch & (P["z_soil"] >= zgw)).sum()), core=core)
    return {k: v[:3] + ([f"... {len(v)} steps in all"] if len(v) > 3 else []) for k, v in bad.items()}, census


WALKS = [(lateral, gw, "combo") for lateral in (False, True) for gw in ("mixed", "above_soil_base")] + [(False, "mixed", "month_change"),
                                                                                                     (True, "mixed", "month_change")]


def _id(w):
    return f"{'oneD' if w[0] else 'svat'}-{w[1]}-{w[2]}"


@pytest.mark.parametrize("lateral", [False, True])
@pytest.mark.parametrize("groundwater", ["mixed", "above_soil_base"])
def test_setup_kernels(oracle, lateral, groundwater):
    """rh_topo, rh_params_surface, rh_params_soil and rh_initial_conditions from the same primaries: every plane, the masks exactly."""
    p = E.extended_params(NX, NY, SEED, groundwater, "interleaved")
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
            B.take(A)       # (one routine at a time from the oracle's state, as everywhere here)
        oracle_routine()
        host.call(name, X)
        for mask in ("maskCatch", "maskRiver", "maskLake"):
            np.testing.assert_array_equal(B.st.planes[mask], a.planes[mask], err_msg=f"{name}: {mask}")
        msg = B.equals(A, name)
        assert msg is None, msg
        B.take(A)
    lu = a.planes["lu_id"]
    assert (a.planes["maskCatch"][np.isin(lu, E.LU_WATER)] == 0).all() and (a.planes["maskCatch"][~np.isin(lu, E.LU_WATER)] == 1).all()
    assert (a.planes["maskRiver"] == (lu == 20)).all() and (a.planes["maskLake"] == (lu == 14)).all()


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_each_routine_from_the_oracles_state(w):
    """Every routine of the step at every step of 12 days of the combo forcing (and over a change of month, which runs the monthly
    surface parameters): the oracle's state before the routine through the device's routine equals the oracle's state after its own."""
    bad, census = walk(*w)
    bad = {k: v for k, v in bad.items() if k != census["core"]}
    assert not bad, "\n".join(m for v in bad.values() for m in v)
    assert census["dt"] == {600, 3600, 86400} and census["steps"] > 60
    assert census["monthly"] == (1 if w[2] == "month_change" else 0)


@pytest.mark.parametrize("w", WALKS, ids=_id)
def test_whole_core_from_the_oracles_state(w):
    """rt_step_core[_lateral] in one call from the oracle's state after adaptive_dt, and the sanity bit it returns."""
    bad, census = walk(*w)
    assert census["core"] not in bad, "\n".join(bad[census["core"]])


@pytest.mark.parametrize("w", WALKS[:4], ids=_id)
def test_census_the_branches_were_reached(w):
    """From the oracle's states, never from the code under test."""
    _, c = walk(*w)
    print("CENSUS", _id(w), {k: v for k, v in c.items() if k != "lu"})
    if w[1] == "mixed":
        assert c["shallow"] >= 0.10 * c["catch_steps"], (c["shallow"], c["catch_steps"])      # groundwater within 10 m below a water table
    else:
        assert c["below_gw"] >= 100, c["below_gw"]                                            # the soil's base stands in the groundwater
    assert c["near_no_percolation"] >= 1     # groundwater at most 10 m below the soil's base and nothing percolates
    assert c["river"] >= 30 and c["lake"] >= 30 and c["outside"] >= 30, (c["river"], c["lake"], c["outside"])
    assert c["lu"] == set(E.LU_POOL.tolist())
    assert c["dep"] >= 1


@pytest.mark.parametrize("layout", ["interleaved", "blocks"])
def test_free_run_of_the_host_core_stays_with_the_oracle(oracle, layout):
    """The SVAT free run of test_hip_extended_columns.py (the same columns, the same forcing with its change of month) with the
    host-compiled rt_step_core in place of the device: over 12 days the two trajectories stay inside compare_bulk's present bounds on
    these columns, so the GPU test may rely on them."""
    st = _start(oracle, False, "mixed", layout, month=E.START_MONTH)
    hs = oracle.OracleState(N)
    hs.luts, hs.settings = st.luts, st.settings
    hs.load_snapshot(st.snapshot(), st.names)
    hs.load_scalars(st.scalars_row())
    host = HP.HostColumns(hs)
    F = E.run_forcing(ndays=NDAYS)
    odrv, hdrv = oracle.ForcingDriver(F), oracle.ForcingDriver(F)
    step = 0
    while st.scal.time < NDAYS * 86400:
        step += 1
        pd, td, ed, monthly = odrv.before_step(st)
        ok = st.step(pd, td, ed, monthly)
        pd, td, ed, monthly_h = hdrv.before_step(hs)
        assert monthly_h == monthly
        s = hs.scal
        hs.adaptive_dt(pd, td, ed)       # (the control part is not under test here: the oracle's, on the host run's own state)
        X = HP.step_ctx_from(hs)
        s.itt += 1
        s.time += s.dt_secs
        if monthly_h:
            host.call("rt_params_surface", X)
        ok_h = host.call("rt_step_core", X)
        host.call("rt_after_timestep", X)
        for k in ("event_id", "year", "month", "doy"):
            getattr(s, k)[0] = getattr(s, k)[1]
        np.testing.assert_array_equal(hs.scalars_row(), st.scalars_row(), err_msg=f"step {step}")
        assert bool(ok_h) == bool(ok), f"step {step}: sanity bit {ok_h}, the oracle's {int(ok)}"
        if step % 25 == 0 or step < 3:
            compare_bulk(hs.snapshot(), st.snapshot(), st.names, what=f"{layout} step {step}")
    compare_bulk(hs.snapshot(), st.snapshot(), st.names, what=f"{layout} final")
    assert step > 100
