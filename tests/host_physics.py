"""ctypes binding of tests/host_physics.cpp: the device's column code (roger_amd/csrc/rh_physics.h) compiled for the host, one entry
point per routine of the fused step, over structure-of-arrays snapshots laid out like the oracle's -- test infrastructure only.

The library is built once per session into a temporary directory (the flags of tests/test_substep_dry_paths.py, without a sanitizer:
it is loaded into Python).  Planes are mapped BY NAME onto oracle_binding.plane_names(); a name one side lacks is an error."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "host_physics.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
INCLUDES = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "roger_amd", "csrc")]

ROUTINES = ("rt_interception", "rt_evapotranspiration", "rt_snow", "rt_infiltration", "rt_subsurface_runoff",
            "rt_subsurface_runoff_lateral", "rt_capillary_rise", "rt_storage", "rt_num_error", "rt_num_error_lateral", "rt_step_core",
            "rt_step_core_lateral", "rt_after_timestep", "rt_after_timestep_oned", "rt_topo", "rt_params_surface", "rt_params_soil",
            "rt_initial_conditions")


class Consts(C.Structure):   # rh_col.h
    _fields_ = [(k, C.c_double) for k in (
        "pi", "r_mp", "l_sc", "sf", "ta_fm", "rmax", "transp_water_stress", "atol", "rtol", "clay_min", "clay_max", "theta_rew_min",
        "theta_rew_max", "rew_min", "rew_max", "z_evap_max", "zroot_to_zsoil_max", "a_bc", "b_bc")] + [
        ("end_event", C.c_int64), ("hpi", C.c_int64), ("dx", C.c_double), ("lateral", C.c_int), ("dy", C.c_double), ("routing", C.c_int)]


class StepCtx(C.Structure):   # rh_col.h
    _fields_ = [("dt", C.c_double), ("agg", C.c_double * 9), ("month_tau", C.c_int64), ("sel_daily", C.c_int), ("sel_hourly", C.c_int),
                ("sel_10min", C.c_int), ("sel_p", C.c_int), ("prec_sel", C.c_double), ("ta_sel", C.c_double), ("sel_w", C.c_int),
                ("pet_sel_w", C.c_double), ("ta_sel_w", C.c_double), ("cond1", C.c_int), ("cond2", C.c_int), ("cond3", C.c_int),
                ("cond4", C.c_int), ("cond5", C.c_int), ("cond_time", C.c_int), ("dt_secs_prelim", C.c_int64), ("itt_day", C.c_int64),
                ("apply_sel", C.c_int), ("forc_exhausted", C.c_int), ("halt", C.c_int), ("last", C.c_int)]


class Luts(C.Structure):   # rh_col.h
    _fields_ = [("ilu", C.c_double * (25 * 13)), ("gc", C.c_double * (25 * 13)), ("gcm", C.c_double * (25 * 2)), ("rdlu", C.c_double * (25 * 7))]


def compile_command(out, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler")
    return [cxx, *FLAGS, *extra, *INCLUDES, SOURCE, "-o", str(out), "-lm"]


_lib = None
_tmp = None


def lib(prebuilt=None):
    """Builds (once per session) and loads the library.  prebuilt, or the environment variable HOST_PHYSICS_SO: the path of a library
    built elsewhere with compile_command, loaded as it is (tools/physics_branches.py: a coverage build)."""
    global _lib, _tmp
    if _lib is None:
        prebuilt = prebuilt or os.environ.get("HOST_PHYSICS_SO")
        if prebuilt:
            so = os.path.abspath(prebuilt)
        else:
            _tmp = tempfile.TemporaryDirectory(prefix="host_physics_")
            so = os.path.join(_tmp.name, "libhost_physics.so")
            subprocess.run(compile_command(so, ("-shared", "-fPIC")), check=True)
        L = C.CDLL(so)
        L.host_plane_name.restype = C.c_char_p
        L.host_plane_name.argtypes = [C.c_int]
        L.host_sizeof.restype = C.c_int64
        for k, t in enumerate((Consts, StepCtx, Luts)):
            if L.host_sizeof(k) != C.sizeof(t):
                raise RuntimeError(f"{t.__name__}: {C.sizeof(t)} bytes here, {L.host_sizeof(k)} in rh_col.h")
        for r in ROUTINES:
            f = getattr(L, "host_" + r)
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Consts), C.POINTER(StepCtx), C.POINTER(Luts)]
        _lib = L
    return _lib


def plane_table():
    L = lib()
    return [(L.host_plane_name(p).decode(), bool(L.host_plane_is_int(p))) for p in range(L.host_num_planes())]


def consts_from(settings):
    """rh_col.h's Consts from the oracle's settings (oracle_binding.OcSettings)."""
    K = Consts()
    for k, _ in Consts._fields_:
        if k == "lateral":
            K.lateral = int(settings.enable_lateral_flow)
        elif k == "routing":
            K.routing = int(settings.enable_routing_1D)
        else:
            setattr(K, k, getattr(settings, k))
    return K


def luts_from(luts):
    """luts: dict(ilu, gc, gcm, rdlu) as OracleState.luts holds them."""
    out = Luts()
    for k in ("ilu", "gc", "gcm", "rdlu"):
        a = np.ascontiguousarray(luts[k], dtype=np.float64).ravel()
        dst = getattr(out, k)
        if a.size != len(dst):
            raise ValueError(f"look-up table {k}: {a.size} values, rh_col.h holds {len(dst)}")
        dst[:] = a.tolist()
    return out


def infiltration_conds(st):
    """cond1..5 of calculate_infiltration (infiltration.py:2155-2167) from the oracle's scalars and prec planes after adaptive_dt."""
    s, P = st.scal, st.planes
    p0, pm1_n0 = bool((P["prec"] == 0).any()), bool((P["prec_m1"] != 0).any())
    pn0, pm1_0 = bool((P["prec"] != 0).any()), bool((P["prec_m1"] == 0).any())
    e0, e1 = int(s.event_id[0]), int(s.event_id[1])
    return (int(e0 == 0 and e1 >= 1), int(p0 and pm1_n0 and e0 >= 1), int(pn0 and pm1_0 and e0 == e1), int(e0 >= 1 and e1 == 0), int(e1 >= 1))


def step_ctx_from(st, cond_time=0):
    """StepCtx from the oracle's scalars after adaptive_dt.  The oracle has applied the prec / ta / pet selection to the planes already:
    no selection is left to the routine (sel_p = sel_w = -1, apply_sel = 0)."""
    X = StepCtx()
    X.dt = float(st.scal.dt)
    X.month_tau = int(st.scal.month[1])
    X.cond1, X.cond2, X.cond3, X.cond4, X.cond5 = infiltration_conds(st)
    X.cond_time = int(cond_time)
    X.itt_day = int(st.scal.itt_day)
    X.dt_secs_prelim = int(st.scal.dt_secs)
    X.sel_p = X.sel_w = -1
    X.apply_sel = 0
    return X


class HostColumns:
    """The routines over the planes of an oracle_binding.OracleState (the arrays are used in place)."""

    def __init__(self, st):
        self.st = st
        table = plane_table()
        here, there = [nm for nm, _ in table], list(st.names)
        missing = [nm for nm in here if nm not in st.planes] + [nm for nm in there if nm not in here]
        if missing:
            raise KeyError(f"planes only one of rh_fields.def / the oracle has: {missing}")
        for nm, is_int in table:
            want = np.int32 if is_int else np.float64
            if st.planes[nm].dtype != want:
                raise TypeError(f"plane {nm}: {st.planes[nm].dtype} in the oracle, {np.dtype(want)} in rh_fields.def")
        self.order = here
        self.K = consts_from(st.settings)
        self.L = luts_from(st.luts) if st.luts else Luts()
        self.rebind()

    def rebind(self):
        """(after the state's arrays were replaced)"""
        arr = (C.c_void_p * len(self.order))()
        for p, nm in enumerate(self.order):
            a = self.st.planes[nm]
            assert a.flags.c_contiguous and a.size == self.st.n
            arr[p] = a.ctypes.data
        self._ptrs = arr

    def call(self, routine, X=None):
        """Runs host_<routine> over all columns; returns its sanity bit."""
        X = X if X is not None else StepCtx(month_tau=int(self.st.scal.month[1]), sel_p=-1, sel_w=-1)
        return int(getattr(lib(), "host_" + routine)(self._ptrs, C.c_int64(self.st.n), C.byref(self.K), C.byref(X), C.byref(self.L)))
