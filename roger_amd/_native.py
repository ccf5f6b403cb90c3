"""ctypes binding of libroger_hip.so (the C ABI declared in include/roger_hip.h and include/roger_hip_sas.h).

This module is the only place the host package touches the native library.  There is no CPU
fallback: if the library or a GPU is missing, creating a context raises.

In reading order: the library and its declarations (read from the two headers), the constants, the helpers that prepare
arguments, the module's functions, Context (SVAT / oneD), SasContext (offline transport).
"""
import ctypes as C
import os
import re

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROGER_HIP_LIB", os.path.join(PKG, "libroger_hip.so"))  # override: kernel experiments
INCLUDE = os.path.join(os.path.dirname(PKG), "include")   # where roger_amd/build.py compiles from


# -- what this binding was written for: the version and the structures are stated by hand, everything else is read from the headers --
ABI_VERSION = 25  # include/roger_hip.h: RH_ABI_VERSION


class RhConfig(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("device", C.c_int32), ("enable_lateral_flow", C.c_int32)] + [
        (k, C.c_double) for k in (
            "pi", "r_mp", "l_sc", "sf", "ta_fm", "rmax", "transp_water_stress", "atol", "rtol", "clay_min",
            "clay_max", "theta_rew_min", "theta_rew_max", "rew_min", "rew_max", "z_evap_max", "zroot_to_zsoil_max",
            "a_bc", "b_bc")
    ] + [("end_event", C.c_int64), ("hpi", C.c_int64), ("dx", C.c_double), ("placement_probes", C.c_int32), ("enable_routing_1D", C.c_int32),
         ("dy", C.c_double)]


class RhScalars(C.Structure):
    _fields_ = [
        ("itt", C.c_int64), ("time", C.c_int64), ("dt_secs", C.c_int64), ("itt_day", C.c_int64),
        ("itt_forc", C.c_int64), ("time_event0", C.c_int64), ("event_id_counter", C.c_int64),
        ("event_id", C.c_int64 * 2), ("year", C.c_int64 * 2), ("month", C.c_int64 * 2), ("doy", C.c_int64 * 2),
        ("dt", C.c_double), ("sanity_ok", C.c_int64),
    ]


class RhSasConfig(C.Structure):
    _fields_ = [("n_cells", C.c_int64), ("ages", C.c_int32), ("substeps", C.c_int32), ("device", C.c_int32),
                ("forcing_days", C.c_int32), ("age_statistics", C.c_int32), ("keep_distributions", C.c_int32),
                ("vsmow", C.c_double), ("d18O_min", C.c_double), ("d18O_max", C.c_double),
                ("tracer", C.c_int32), ("solver", C.c_int32)]


class NativeError(RuntimeError):
    pass


# -- the declarations: the two headers are the one statement of the C ABI -------------------------------------------
_C_TYPES = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}


def _c_type(function, decl, named):
    """The ctypes type of one parameter (`named`: its name may follow the type) or of the return type of `function`: `char *` is
    c_char_p, any other pointer c_void_p, a scalar what _C_TYPES says, and anything else is refused -- nothing falls back to int."""
    tokens = [t for t in re.findall(r"\w+|\S", decl) if t != "const"]
    if "*" in tokens:
        return C.c_char_p if tokens[:2] == ["char", "*"] and tokens.count("*") == 1 else C.c_void_p
    ctype = " ".join(tokens[:-1] if named and len(tokens) > 1 else tokens)
    if ctype == "void" and not named:
        return None
    if ctype not in _C_TYPES:
        raise NativeError(f"{function}: no ctypes type is declared for the C type '{ctype}' (roger_amd/_native.py: _C_TYPES)")
    return _C_TYPES[ctype]


def _prototypes(header_text):
    """{name: (restype, argtypes)} of every `ret rh_xxx(params);` of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)
    out = {}
    for statement in re.split(r"[;{}]", text):
        if not re.search(r"\brh_\w+\s*\(", statement):
            continue
        m = re.fullmatch(r"\s*(.*?)\b(rh_\w+)\s*\(([^()]*)\)\s*", statement, flags=re.S)
        if not m:
            raise NativeError(f"{' '.join(statement.split())!r} is not a prototype `ret rh_xxx(params);`")
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        out[name] = (_c_type(name, ret, False), [_c_type(name, p, True) for p in params])
    return out


def _header_prototypes(header):
    path = os.path.join(INCLUDE, header)
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: the binding reads the C ABI from the headers the library is compiled from")
    with open(path) as f:
        return _prototypes(f.read())


_PROTOTYPES = _header_prototypes("roger_hip.h")
_SAS_PROTOTYPES = _header_prototypes("roger_hip_sas.h")
DECLARED_SYMBOLS = tuple(_PROTOTYPES)
SAS_DECLARED_SYMBOLS = tuple(_SAS_PROTOTYPES)

_lib = None


class _Missing:
    def __init__(self, name):
        self.name = name

    def __call__(self, *a, **k):
        raise NativeError(f"{self.name} is not exported by {LIB_PATH}")


class _Tolerant:
    def __init__(self, lib):
        self.__dict__["_lib"] = lib
        self.__dict__["_missing"] = {}

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            return self._missing.setdefault(name, _Missing(name))


def load():
    """Load the shared library and declare every function of roger_hip.h and roger_hip_sas.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} not found: build it with `python -m roger_amd.build` (there is no CPU fallback)")
    # PyTorch-ROCm bundles its own HIP runtime (libamdhip64).  Two HIP runtimes in one process do
    # not work ("No HIP GPUs are available" from whichever initialises second), so when torch is
    # installed let it load its copy first; libroger_hip.so then binds to the same one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    if os.environ.get("RH_OLD_VARIANT"):   # A/B against a library built from an older commit (tools/ab_variants.sh): entry points
        lib = _Tolerant(lib)               # it lacks are declared on a stand-in that raises when called
    # the structures above are laid out for ONE version of include/roger_hip.h: a library built from another one would read past
    # (or short of) the caller's rh_config / rh_sas_config.  RH_OLD_VARIANT=1 (A/B against a library of an older commit) accepts
    # an older library, whose structures are prefixes of today's.  (Asked first, so that a library of another version is refused for
    # its version and not for a function it lacks: `int rh_abi_version(void)` is callable as ctypes finds it.)
    got = int(lib.rh_abi_version())
    if got != ABI_VERSION and not (os.environ.get("RH_OLD_VARIANT") and got < ABI_VERSION):
        raise NativeError(f"{LIB_PATH} implements ABI version {got}, this binding is written for version {ABI_VERSION} "
                          "(include/roger_hip.h: RH_ABI_VERSION): rebuild with `python -m roger_amd.build --force`")
    for name, (restype, argtypes) in {**_PROTOTYPES, **_SAS_PROTOTYPES}.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


# -- constants ----------------------------------------------------------------------------------------------------------
# the planes of the routing (settings.enable_routing_1D): the last ones of include/rh_fields.def, held by routing contexts only
ROUTING_PLANES = ("flow_dir_topo", "outer_boundary", "k_st", "q_sur_out", "q_sur_in", "q_sub_out", "q_sub_in", "q_sub_in_rz", "q_sub_in_ss")

# RH_SAS_TRACER_*.  Deuterium runs the isotope kernels of oxygen-18 with its own constants in the vsmow / d18O_min /
# d18O_max fields of rh_sas_config (roger/core/transport.py:315-340, roger/settings.py:79-81)
SAS_TRACERS = {"oxygen18": 0, "deuterium": 0, "bromide": 1, "chloride": 2, "virtualtracer": 3}
# RH_SAS_SOLVER_*: settings.sas_solver
SAS_SOLVERS = {"deterministic": 0, "Euler": 1, "RK4": 2}
DEUTERIUM_DEFAULTS = {"vsmow": 155.76e-6, "d18O_min": -160.0, "d18O_max": 0.0}

# RH_SAS_SCORES_*: how a sample's window is aggregated (include/roger_hip_sas.h)
SAS_SCORES_KINDS = {"bulk": 0, "mean": 1, "last": 2}

# stage bits of rh_sas_stages (include/roger_hip_sas.h)
SAS_STAGES = dict(INF_RZ=1, EVAP=2, TRANSP=4, Q_RZ=8, INF_SS=16, Q_SS=32, CPR=64, STORAGE=128, AGEING=256, ALL=511,
                  RESCALE=512)

# the DAILY arrays of include/rh_sas_arrays.def
DAILY_INPUTS = ("inf_mat_rz", "inf_pf_rz", "inf_pf_ss", "evap_soil", "transp", "q_rz", "q_ss", "cpr_rz", "C_in")


# -- arguments: each conversion once; a method gives its name and the nouns of its message ----------------------------------
_COLUMNS = ("has", "values", " columns")   # the SVAT side: "the mask has 5 values, the context 6 columns"
_CELLS = ("has", "cells", "")              # the transport side: "the mask has 5 cells, the context 6"


def _ptr(a):
    """The address of a numpy array's data for a pointer parameter; None stays None (NULL)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ints(values, n=None):
    """A C int array of the values (n: of so many), never of length 0."""
    return (C.c_int * max(1, len(values) if n is None else n))(*values)


def _sized(method, what, a, n, nouns):
    """`a`, which holds one element for each of the context's n cells."""
    if a.size != n:
        raise ValueError(f"{method}: the {what} {nouns[0]} {a.size} {nouns[1]}, the context {n}{nouns[2]}")
    return a


def _byte_mask(method, mask, n, nouns):
    """The per-cell mask as bytes 0 / 1."""
    return _sized(method, "mask", np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8), n, nouns)


def _cell_map(method, what, values, n, nouns, lowest=None):
    """The per-cell map (`what`: "zone map", "series map") as int32.  lowest: an index below it or beyond int32 is clipped to the ends
    instead of wrapping into the range (out of range stays out of range: the library refuses it)."""
    a = np.asarray(values).reshape(-1)
    if lowest is not None:
        a = np.clip(_sized(method, what, a, n, nouns), lowest, 2 ** 31 - 1)
    return _sized(method, what, np.ascontiguousarray(a, dtype=np.int32), n, nouns)


def _weights(method, weights, n, nouns, refusal):
    """The per-cell likelihood weights as uint16; `refusal(wt)`: the method's words for weights that are not integers within 0 ... 65535."""
    wt = _sized(method, "weights", np.asarray(weights).reshape(-1), n, nouns)
    if wt.dtype.kind not in "iu" or (wt.size and (int(wt.min()) < 0 or int(wt.max()) > 65535)):
        raise ValueError(f"{method}: {refusal(wt)}")
    return np.ascontiguousarray(wt, dtype=np.uint16)


def _window_pair(windows):
    """(first_day, last_day) of the sample windows, int64 (K,) each."""
    first, last = (np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in windows)
    return first, last


# -- module functions -----------------------------------------------------------------------------------------------------
def totals_item_name(value, weight=None):
    """The name of a totals item in rows and files: `<value>` or `<value>_by_<weight>`."""
    return value if weight is None else f"{value}_by_{weight}"


def sas_selftest_div(a, d):
    """a / d by the SAS kernel's hoisted-reciprocal division (rh_sas_selftest_div)."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    d = np.ascontiguousarray(np.broadcast_to(d, a.shape), dtype=np.float64)
    out = np.empty_like(a)
    rc = lib.rh_sas_selftest_div(_ptr(a), _ptr(d), _ptr(out), a.size)
    if rc != 0:
        raise NativeError(f"rh_sas_selftest_div failed ({rc})")
    return out


def sas_selftest_pow(x, k):
    """x ** k by the SAS kernel's own routine (rh_sas_selftest_pow)."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    k = np.ascontiguousarray(np.broadcast_to(k, x.shape), dtype=np.float64)
    out = np.empty_like(x)
    rc = lib.rh_sas_selftest_pow(_ptr(x), _ptr(k), _ptr(out), x.size)
    if rc != 0:
        raise NativeError(f"rh_sas_selftest_pow failed ({rc})")
    return out


def selftest_window_sum(v144, itd):
    """np.sum over the series masked to [itd, itd + 6) as the kernels form it: (by their function, by its general path) per window start."""
    lib = load()
    v = np.ascontiguousarray(v144, dtype=np.float64)
    t = np.ascontiguousarray(itd, dtype=np.int64)
    if v.size != 144:
        raise ValueError("selftest_window_sum: a series of 144 slots")
    out = np.empty(2 * t.size, dtype=np.float64)
    rc = lib.rh_selftest_window_sum(_ptr(v), _ptr(t), t.size, _ptr(out))
    if rc != 0:
        raise NativeError(f"rh_selftest_window_sum failed ({rc})")
    return out[0::2], out[1::2]


def selftest_pow(x, y):
    """x ** y by the kernels' own power function (rh_pow.h) on the device."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty_like(x)
    rc = lib.rh_selftest_pow(_ptr(x), _ptr(y), _ptr(out), x.size)
    if rc != 0:
        raise NativeError(f"rh_selftest_pow failed ({rc})")
    return out


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (ncclGetUniqueId): created on rank 0, handed to every rank's `comm_init`."""
    lib = load()
    buf = C.create_string_buffer(128)
    if lib.rh_comm_unique_id(buf) != 0:
        raise NativeError(f"rh_comm_unique_id failed: {lib.rh_last_error(None).decode()}")
    return buf.raw


def plane_table():
    lib = load()
    n = lib.rh_num_planes()
    return [(lib.rh_plane_name(i).decode(), bool(lib.rh_plane_is_int(i))) for i in range(n)]


class Context:
    """One device arena + stream (rh_ctx).  Thin, 1:1 with the C ABI."""

    def __init__(self, nx, ny, device=0, **settings):
        self._h = None
        lib = load()
        cfg = RhConfig()
        lib.rh_default_config(C.byref(cfg))
        cfg.nx, cfg.ny, cfg.device = int(nx), int(ny), int(device)
        for k, v in settings.items():
            if not hasattr(cfg, k):
                raise AttributeError(f"unknown setting {k}")
            setattr(cfg, k, v)
        h = C.c_void_p()
        rc = lib.rh_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise NativeError(f"rh_create failed ({rc}): {lib.rh_last_error(None).decode()}")
        self._h = h
        self._lib = lib
        self.nx, self.ny, self.n = int(nx), int(ny), int(nx) * int(ny)
        self.planes = plane_table()
        self.index = {nm: i for i, (nm, _) in enumerate(self.planes)}
        self.planes_held = int(lib.rh_planes_held(h))   # (the routing's planes exist in routing contexts only)
        self.lateral = bool(cfg.enable_lateral_flow)
        self.routing = bool(cfg.enable_routing_1D)
        # what a configure call leaves for its read, as long as nothing is configured
        self._diag_names = []
        self._points_shape = (0, 0)          # (names, cells)
        self._totals_nv = 0
        self._zonal_shape = (0, 0)           # (zones, names)
        self._scores_shape = (0, 0)          # (items, intervals)
        self._events_shape = (0, 0)          # (items, slots)
        self._durations_shape = (0, [])      # (items, [edges of every item])
        self._bands_shape = (0, 0)           # (items, probs); with zones (items, zones, probs)

    def close(self):
        if self._h:
            self._lib.rh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise NativeError(f"{what} failed ({rc}): {self._lib.rh_last_error(self._h).decode()}")

    def _ids(self, names):
        """The planes' indices as a C int array."""
        return _ints([self.index[n] for n in names])

    # -- planes -----------------------------------------------------------------------------
    def dtype_of(self, name):
        return np.int32 if self.planes[self.index[name]][1] else np.float64

    def upload(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=self.dtype_of(name)).reshape(-1)
        if a.size != self.n:
            raise ValueError(f"{name}: expected {self.n} values, got {a.size}")
        self._check(self._lib.rh_upload(self._h, self.index[name], _ptr(a), a.nbytes), f"rh_upload({name})")

    def download(self, name):
        out = np.empty(self.n, dtype=self.dtype_of(name))
        self._check(self._lib.rh_download(self._h, self.index[name], _ptr(out), out.nbytes), f"rh_download({name})")
        return out

    def device_ptr(self, name):
        return self._lib.rh_plane_device_ptr(self._h, self.index[name])

    # -- scalars / tables / forcing -----------------------------------------------------------
    def set_scalars(self, s):
        self._check(self._lib.rh_set_scalars(self._h, C.byref(s)), "rh_set_scalars")

    def get_scalars(self):
        s = RhScalars()
        self._check(self._lib.rh_get_scalars(self._h, C.byref(s)), "rh_get_scalars")
        return s

    def set_luts(self, ilu, gc, gcm, rdlu):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (ilu, gc, gcm, rdlu)]
        for a, shape in zip(arrs, ((25, 13), (25, 13), (25, 2), (25, 7))):
            if a.shape != shape:
                raise ValueError(f"look-up table has shape {a.shape}, expected {shape}")
        self._check(self._lib.rh_set_luts(self._h, *[_ptr(a) for a in arrs]), "rh_set_luts")

    def set_lut_mlms(self, mlms):
        a = np.ascontiguousarray(mlms, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 9:
            raise ValueError(f"lut_mlms has shape {a.shape}, expected (n_slope, 9)")
        self._check(self._lib.rh_set_lut_mlms(self._h, _ptr(a), a.shape[0]), "rh_set_lut_mlms")

    def set_forcing_day(self, prec_day, ta_day, pet_day):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (prec_day, ta_day, pet_day)]
        per_cell = arrs[0].ndim > 1
        want = (self.n, 144) if per_cell else (144,)
        for a in arrs:
            if a.reshape(want).shape != want:
                raise ValueError("forcing must be (144,) or (n_cells, 144)")
        self._check(self._lib.rh_set_forcing_day(self._h, *[_ptr(a) for a in arrs], int(per_cell)), "rh_set_forcing_day")

    def set_forcing_series(self, F):
        """F: dict with PREC, TA, PET (float64) and YEAR, MONTH, DOY (int64) 10-minute vectors."""
        f = [np.ascontiguousarray(F[k], dtype=np.float64) for k in ("PREC", "TA", "PET")]
        c = [np.ascontiguousarray(F[k], dtype=np.int64) for k in ("YEAR", "MONTH", "DOY")]
        n = f[0].size
        if any(a.size != n for a in f + c):
            raise ValueError("forcing vectors differ in length")
        self._check(self._lib.rh_set_forcing_series(self._h, *[_ptr(a) for a in f + c], n), "rh_set_forcing_series")

    def set_forcing_stations(self, F, station_index):
        """F: PREC, TA, PET as (n_stations, nitt_forc) float64 and YEAR, MONTH, DOY (nitt_forc,) int64; station_index: per cell the row
        of its station (< 0: none).  settings.enable_distributed_input (roger/bmimodels/svat_dist/svat_dist.py:274-310)."""
        f = [np.ascontiguousarray(F[k], dtype=np.float64) for k in ("PREC", "TA", "PET")]
        c = [np.ascontiguousarray(F[k], dtype=np.int64) for k in ("YEAR", "MONTH", "DOY")]
        ns, nitt = f[0].shape
        if any(a.shape != (ns, nitt) for a in f) or any(a.shape != (nitt,) for a in c):
            raise ValueError("station forcing: PREC / TA / PET must be (n_stations, nitt_forc), the calendar (nitt_forc,)")
        idx = np.ascontiguousarray(station_index, dtype=np.int32).reshape(-1)
        if idx.size != self.n or idx.max() >= ns:
            raise ValueError("station_index: one row index per cell, below the number of stations")
        self._check(self._lib.rh_set_forcing_stations(self._h, *[_ptr(a) for a in f + c], nitt, ns, _ptr(idx)), "rh_set_forcing_stations")

    def run_steps(self, nsteps):
        self._check(self._lib.rh_run_steps(self._h, int(nsteps)), "rh_run_steps")

    # -- routing (settings.enable_routing_1D) -----------------------------------------------------
    def step_routed(self, monthly=False):
        self._check(self._lib.rh_step_routed(self._h, -1 if monthly is None else int(bool(monthly))), "rh_step_routed")

    def route_out(self, which):
        self._check(self._lib.rh_route_out(self._h, int(which)), "rh_route_out")

    def route_in(self, which):
        self._check(self._lib.rh_route_in(self._h, int(which)), "rh_route_in")

    def route_edges(self, which):
        """(lo, hi): q_out of the rank's edge columns x = 0 and x = nx - 1 (the west / east parts of what the neighbours' halos take)."""
        lo, hi = np.empty(self.ny), np.empty(self.ny)
        self._check(self._lib.rh_route_get_edges(self._h, int(which), _ptr(lo), _ptr(hi)), "rh_route_get_edges")
        return lo, hi

    def route_static_edges(self):
        """(flow_dir_lo, flow_dir_hi, mask_lo, mask_hi) of the rank's edge columns."""
        a = [np.empty(self.ny, dtype=np.int32) for _ in range(4)]
        self._check(self._lib.rh_route_get_static_edges(self._h, *[_ptr(x) for x in a]), "rh_route_get_static_edges")
        return tuple(a)

    def route_set_halo(self, side, q=None, flow_dir=None, mask=None):
        keep = [None if x is None else np.ascontiguousarray(x, dtype=dt) for x, dt in ((q, np.float64), (flow_dir, np.int32), (mask, np.int32))]
        for x in keep:
            if x is not None and x.size != self.ny:
                raise ValueError(f"a halo column has ny = {self.ny} values, got {x.size}")
        self._check(self._lib.rh_route_set_halo(self._h, int(side), *[_ptr(x) for x in keep]), "rh_route_set_halo")

    # -- routines -----------------------------------------------------------------------------
    def call(self, entry):
        self._check(getattr(self._lib, entry)(self._h), entry)

    def step(self, monthly=False):
        self._check(self._lib.rh_svat_step(self._h, int(bool(monthly))), "rh_svat_step")

    def step_scalars(self, monthly=False):
        """rh_svat_step + the read-back of the scalars in ONE native call (a driver that keeps its hooks on the host needs vs.time
        before the next step); returns the RhScalars after the step."""
        s = RhScalars()
        rc = self._lib.rh_svat_step_scalars(self._h, 1 if monthly else 0, C.byref(s))
        if rc != 0:
            self._check(rc, "rh_svat_step_scalars")
        return s

    def step_phase3(self, monthly=False):
        # monthly: False/True, or -1 to use the month-change flag computed on the device
        self._check(self._lib.rh_step_phase3(self._h, int(monthly)), "rh_step_phase3")

    def set_forcing_weights(self, prec_weight=None, ta_offset=None, pet_weight=None):
        """Per-cell weights on the resident series (prec * w, ta + offset, pet * w); None x 3 clears them."""
        if prec_weight is None and ta_offset is None and pet_weight is None:
            self._check(self._lib.rh_set_forcing_weights(self._h, None, None, None), "rh_set_forcing_weights")
            return
        arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (prec_weight, ta_offset, pet_weight)]
        if any(a.size != self.n for a in arrs):
            raise ValueError("weights must have one value per cell")
        self._check(self._lib.rh_set_forcing_weights(self._h, *[_ptr(a) for a in arrs]), "rh_set_forcing_weights")

    def diag_configure(self, rate=(), collect=(), n_slots=1):
        """Device-side daily accumulators: `rate` variables are summed per day, `collect` variables keep their
        end-of-day value (time level tau); n_slots days stay resident."""
        r, c = self._ids(list(rate)), self._ids(list(collect))
        self._check(self._lib.rh_diag_configure(self._h, r, len(rate), c, len(collect), int(n_slots)), "rh_diag_configure")
        self._diag_names = list(rate) + list(collect)   # (a refused configuration leaves the previous one, names included)

    def diag_download(self, name, slot):
        a = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.rh_diag_download(self._h, self._diag_names.index(name), int(slot), _ptr(a), a.nbytes), "rh_diag_download")
        return a

    def diag_steps(self, slot):
        """Steps accumulated in a day slot (divide a rate variable by it for the "average" diagnostic)."""
        n = C.c_int64()
        self._check(self._lib.rh_diag_steps(self._h, int(slot), C.byref(n)), "rh_diag_steps")
        return n.value

    def diag_set_interval(self, seconds):
        self._check(self._lib.rh_diag_set_interval(self._h, C.c_int64(int(seconds))), "rh_diag_set_interval")

    def diag_slot_times(self, slot):
        """(start time of the interval's first step or -1, end time of its last step) of a slot."""
        t0, t1 = C.c_int64(), C.c_int64()
        self._check(self._lib.rh_diag_slot_times(self._h, int(slot), C.byref(t0), C.byref(t1)), "rh_diag_slot_times")
        return t0.value, t1.value

    def diag_upload(self, name, slot, values):
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        self._check(self._lib.rh_diag_upload(self._h, self._diag_names.index(name), int(slot), _ptr(a), a.nbytes), "rh_diag_upload")

    def diag_set_slot_state(self, slot, steps, t_start, t_end):
        self._check(self._lib.rh_diag_set_slot_state(self._h, int(slot), int(steps), int(t_start), int(t_end)), "rh_diag_set_slot_state")

    def diag_device_ptr(self, name, slot):
        return self._lib.rh_diag_device_ptr(self._h, self._diag_names.index(name), int(slot))

    def _ring_read(self, fn, first, n, hdr_width, shape):
        """Rows [first, first + n) of an observer's ring through its read entry point `fn`: (hdr int64 (n, hdr_width), values float64
        (n,) + shape)."""
        n = int(n)
        hdr = np.empty((n, hdr_width), dtype=np.int64)
        values = np.empty((n,) + tuple(shape), dtype=np.float64)
        self._check(getattr(self._lib, fn)(self._h, int(first), n, _ptr(hdr), _ptr(values), values.nbytes), fn)
        return hdr, values

    # -- time series at observation columns (rh_points_*) ---------------------------------------
    def points_configure(self, cells, names, capacity=4096):
        """Record `names` (float64 planes) at `cells` (interior indices of this context's block, C order) after every step, in a ring of
        `capacity` rows on the device.  No cells or no names: release the buffers and stop recording."""
        c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1)
        names = list(names)
        self._check(self._lib.rh_points_configure(self._h, _ptr(c), c.size, self._ids(names), len(names), int(capacity)), "rh_points_configure")
        self._points_shape = (len(names), c.size)   # (a refused configuration leaves the previous one)

    def points_count(self):
        """Rows recorded since points_configure."""
        n = C.c_int64()
        self._check(self._lib.rh_points_count(self._h, C.byref(n)), "rh_points_count")
        return n.value

    def points_read(self, first, n):
        """Rows [first, first + n) of the ring: (hdr int64 (n, 3): itt, time at the end of the step, dt_secs; values float64 (n, V, K))."""
        return self._ring_read("rh_points_read", first, n, 3, self._points_shape)

    # -- catchment totals (rh_totals_*) ----------------------------------------------------------
    def totals_configure(self, names, mask=None, capacity=4096):
        """Record the sum, minimum and maximum of `names` (float64 planes) over the columns of `mask` (a flag per interior column of
        this context's block, C order; None: every column) after every step, in a ring of `capacity` rows on the device.  No names:
        release the buffers and stop recording."""
        names = list(names)
        ids = self._ids(names)
        m = None if mask is None else _byte_mask("totals_configure", mask, self.n, _COLUMNS)
        self._check(self._lib.rh_totals_configure(self._h, _ptr(m), ids, len(names), int(capacity)), "rh_totals_configure")
        self._totals_nv = len(names)   # (a refused configuration leaves the previous one)

    def totals_count(self):
        """(rows recorded since totals_configure, columns inside the mask)."""
        n, cells = C.c_int64(), C.c_int64()
        self._check(self._lib.rh_totals_count(self._h, C.byref(n), C.byref(cells)), "rh_totals_count")
        return n.value, cells.value

    def totals_read(self, first, n):
        """Rows [first, first + n) of the ring: (hdr int64 (n, 3): itt, time at the end of the step, dt_secs; values float64 (n, V, 3):
        sum, min, max)."""
        return self._ring_read("rh_totals_read", first, n, 3, (self._totals_nv, 3))

    # -- zonal totals (rh_zonal_*) ---------------------------------------------------------------
    def zonal_configure(self, names, zones=None, n_zones=0, capacity=4096):
        """Record the sum, minimum and maximum of `names` (float64 planes) for every zone of `zones` (an int per interior column of this
        context's block, C order: -1 outside, else 0 ... n_zones - 1) after every step, in a ring of `capacity` rows on the device.  No
        names: release the buffers and stop recording."""
        names = list(names)
        ids = self._ids(names)
        z = _cell_map("zonal_configure", "zone map", zones, self.n, _COLUMNS) if names else None
        self._check(self._lib.rh_zonal_configure(self._h, _ptr(z), int(n_zones), ids, len(names), int(capacity)), "rh_zonal_configure")
        self._zonal_shape = (int(n_zones) if names else 0, len(names))   # (a refused configuration leaves the previous one)

    def zonal_count(self):
        """(rows recorded since zonal_configure, columns of every zone: int64 (n_zones,))."""
        n = C.c_int64()
        nz = self._zonal_shape[0]
        cells = np.zeros(max(1, nz), dtype=np.int64)
        self._check(self._lib.rh_zonal_count(self._h, C.byref(n), _ptr(cells)), "rh_zonal_count")
        return n.value, cells[:nz]

    def zonal_read(self, first, n):
        """Rows [first, first + n) of the ring: (hdr int64 (n, 3): itt, time at the end of the step, dt_secs; values float64
        (n, Z, V, 3): sum, min, max)."""
        return self._ring_read("rh_zonal_read", first, n, 3, self._zonal_shape + (3,))

    # -- scores against observed series (rh_scores_*) ------------------------------------------------
    def scores_configure(self, names, kinds=(), obs=None, series=None, interval=86400, t_first=0):
        """After every step aggregate `names` (float64 planes; kinds: 0 sum over the interval, 1 value at its end) to the observation
        interval and, at every interval's end, add the comparison with `obs` (n_items, n_series, n_intervals; NaN: missing) into four
        moments per column that stay on the device.  `series`: the series of every interior column of this context's block (C order,
        < 0: not scored), None: every column series 0.  Interval k is (t_first + k interval, t_first + (k + 1) interval].  No names:
        release the buffers and stop."""
        names = list(names)
        ids = self._ids(names)
        kd = _ints([int(k) for k in kinds], len(names))
        o, sr, shape = None, None, (0, 0, 0)
        if names:
            o = np.ascontiguousarray(obs, dtype=np.float64)
            if o.ndim != 3 or o.shape[0] != len(names) or len(kinds) != len(names):
                raise ValueError(f"scores_configure: observations of shape {o.shape} and {len(kinds)} kinds for {len(names)} items "
                                 "((n_items, n_series, n_intervals))")
            shape = o.shape
            if series is not None:
                sr = _cell_map("scores_configure", "series map", series, self.n, _COLUMNS)
        self._check(self._lib.rh_scores_configure(self._h, ids, kd, len(names), _ptr(o), int(shape[1]), int(shape[2]), _ptr(sr),
                                                  int(interval), int(t_first)), "rh_scores_configure")
        self._scores_shape = (len(names), int(shape[2]) if names else 0)   # (a refused configuration leaves the previous one)

    def scores_read(self):
        """(moments float64 (n_items, 5, n): acc, m1 = sum sim, m2 = sum sim^2, m3 = sum sim obs, m4 = sum (sim - obs)^2;
        closed uint8 (n_intervals,)).  Synchronises."""
        ni, nk = self._scores_shape
        moments = np.empty((ni, 5, self.n), dtype=np.float64)
        closed = np.empty(nk, dtype=np.uint8)
        self._check(self._lib.rh_scores_read(self._h, _ptr(moments), moments.nbytes, _ptr(closed), closed.nbytes), "rh_scores_read")
        return moments, closed

    def scores_restore(self, moments, closed, t_first):
        """Replace the moments and the closed flags (as scores_read gave them) and the start of interval 0 by those of an interrupted
        run: after scores_configure, before the next step."""
        m = np.ascontiguousarray(moments, dtype=np.float64)
        c = np.ascontiguousarray(closed, dtype=np.uint8)
        self._check(self._lib.rh_scores_restore(self._h, _ptr(m), m.nbytes, _ptr(c), c.nbytes, int(t_first)), "rh_scores_restore")

    # -- event outputs (rh_events_*) -----------------------------------------------------------------
    def events_configure(self, names, kinds=(), n_slots=1):
        """After every step of a rainfall event accumulate `names` (float64 planes; kinds: 0 sum, 1 peak of value / dt, 2 first, 3 last)
        into the event's slot (event id mod n_slots) on the device.  No names: release the buffers and stop."""
        names = list(names)
        if len(kinds) != len(names):
            raise ValueError(f"events_configure: {len(kinds)} kinds for {len(names)} items")
        ids = self._ids(names)
        kd = _ints([int(k) for k in kinds])
        self._check(self._lib.rh_events_configure(self._h, ids, kd, len(names), int(n_slots) if names else 0), "rh_events_configure")
        self._events_shape = (len(names), int(n_slots) if names else 0)   # (a refused configuration leaves the previous one)

    def events_read(self, slots=None):
        """(headers int64 (n_slots, 6): event id, steps, t0 of the first step, t1 of the last, steps of 600 s, steps of 3600 s -- -1 each
        while untouched; values {slot: float64 (n_items, n)} of the `slots` asked for (None: every touched one); lost: a step found
        its slot unread).  Synchronises."""
        ni, ns = self._events_shape
        hdr = np.empty((ns, 6), dtype=np.int64)
        self._check(self._lib.rh_events_headers(self._h, _ptr(hdr), hdr.nbytes), "rh_events_headers")
        if slots is None:
            slots = [s for s in range(ns) if hdr[s, 0] >= 0]
        values = {}
        for s in slots:
            a = np.empty((ni, self.n), dtype=np.float64)
            for j in range(ni):
                self._check(self._lib.rh_events_download(self._h, j, int(s), _ptr(a[j]), a[j].nbytes), "rh_events_download")
            values[int(s)] = a
        lost = C.c_int()
        self._check(self._lib.rh_events_lost(self._h, C.byref(lost)), "rh_events_lost")
        return hdr, values, bool(lost.value)

    def events_set_drained(self, event_id):
        """Publish the highest event id that has been read out: the slots of the events up to it may be taken again."""
        self._check(self._lib.rh_events_set_drained(self._h, int(event_id)), "rh_events_set_drained")

    def events_state(self):
        """(ids int64 (n_slots,): the event id every slot holds for the kernel, -1: none; running; drained).  Synchronises."""
        ids = np.empty(self._events_shape[1], dtype=np.int64)
        running, drained = C.c_int64(), C.c_int64()
        self._check(self._lib.rh_events_state(self._h, _ptr(ids), ids.nbytes, C.byref(running), C.byref(drained)), "rh_events_state")
        return ids, running.value, drained.value

    def events_restore(self, hdr, ids, running, drained, lost=False, values=None):
        """Replace the headers, the slots' ids, `running`, `drained`, `lost` and the maps {slot: (n_items, n)} of the events that were not
        read out by those of an interrupted run: after events_configure, before the next step."""
        h = np.ascontiguousarray(hdr, dtype=np.int64)
        i = np.ascontiguousarray(ids, dtype=np.int64)
        values = dict(values or {})
        slots = np.ascontiguousarray(sorted(values), dtype=np.int32)
        maps = np.ascontiguousarray(np.stack([np.asarray(values[s], dtype=np.float64) for s in sorted(values)])) if values else np.zeros((0,))
        self._check(self._lib.rh_events_restore(self._h, _ptr(h), h.nbytes, _ptr(i), i.nbytes, int(running), int(drained), int(bool(lost)),
                                                _ptr(slots) if values else None, len(values), _ptr(maps) if values else None, maps.nbytes),
                    "rh_events_restore")

    # -- duration curves (rh_durations_*) ------------------------------------------------------------
    def durations_configure(self, names, kinds=(), edges=(), spells=(), mask=None, interval=86400, t_first=0):
        """After every step aggregate `names` (float64 planes; kinds: 0 sum over the interval, 1 value at its end) to the interval and, at
        every counted interval's end, count the value into the column's histogram over `edges[j]` (ascending, finite, at most 63; shared by
        all columns), keep its extremes and, with spells[j] = (side, threshold) (side 0: below, 1: at or above; None: no spell), the run
        lengths.  `mask`: a byte per interior column of this context's block (C order, 0: not counted), None: every column.  The first
        counted interval starts at t_first.  No names: release the buffers and stop."""
        names = list(names)
        ni = len(names)
        edges = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
        spells = list(spells) if len(spells) else [None] * ni
        if len(kinds) != ni or len(edges) != ni or len(spells) != ni:
            raise ValueError(f"durations_configure: {len(kinds)} kinds, {len(edges)} edge lists and {len(spells)} spells for {ni} items")
        ids = self._ids(names)
        kd = _ints([int(k) for k in kinds])
        ne = _ints([int(e.size) for e in edges])
        sd = _ints([0 if s is None else int(s[0]) for s in spells])
        thr = np.array([np.nan if s is None else float(s[1]) for s in spells] or [np.nan], dtype=np.float64)
        flat = np.ascontiguousarray(np.concatenate(edges + [np.zeros(1)]), dtype=np.float64)
        mk = _byte_mask("durations_configure", mask, self.n, _COLUMNS) if names and mask is not None else None
        self._check(self._lib.rh_durations_configure(self._h, ids, kd, ne, ni, _ptr(flat), _ptr(thr), sd, _ptr(mk), int(interval), int(t_first)),
                    "rh_durations_configure")
        self._durations_shape = (ni, [int(e.size) for e in edges])   # (a refused configuration leaves the previous one)

    def durations_read(self):
        """(counts: one uint32 (m_j + 2, n) per item, the NaN bin last; values float64 (n_items, 3, n): acc, min, max; spells uint32
        (n_items, 3, n): run, longest, n_spells).  Synchronises."""
        ni, ms = self._durations_shape
        counts = np.empty((sum(m + 2 for m in ms), self.n), dtype=np.uint32)
        values = np.empty((ni, 3, self.n), dtype=np.float64)
        spells = np.empty((ni, 3, self.n), dtype=np.uint32)
        self._check(self._lib.rh_durations_read(self._h, _ptr(counts), counts.nbytes, _ptr(values), values.nbytes, _ptr(spells), spells.nbytes),
                    "rh_durations_read")
        offs = np.concatenate([[0], np.cumsum([m + 2 for m in ms])]).astype(int)
        return [counts[offs[j]:offs[j + 1]] for j in range(ni)], values, spells

    def durations_restore(self, counts, values, spells):
        """Replace the counters, the float planes and the spell planes (as durations_read gave them) by those of an interrupted run:
        after durations_configure, before the next step."""
        c = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.uint32) for a in counts]), dtype=np.uint32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        sp = np.ascontiguousarray(spells, dtype=np.uint32)
        self._check(self._lib.rh_durations_restore(self._h, _ptr(c), c.nbytes, _ptr(v), v.nbytes, _ptr(sp), sp.nbytes), "rh_durations_restore")

    # -- ensemble bands (rh_bands_*) -------------------------------------------------------------------
    def bands_configure(self, names, kinds=(), probs=(0.05, 0.5, 0.95), interval=86400, t_first=0, mask=None, capacity=4096, zones=None, n_zones=None, weights=None):
        """After every step aggregate `names` (at most 8 float64 planes; kinds: 0 sum over the interval, 1 value at its end) to the
        interval and, at every counted interval's end, record the exact quantiles ACROSS the columns of `mask` (a byte per interior column
        of this context's block, C order; None: every column) at `probs` (at most 8, within [0, 1]) as one row of a ring of `capacity`
        rows on the device.  The first counted interval starts at t_first.  No names: release the buffers and stop.
        `zones`: an index 0 ... n_zones - 1 per interior column (negative: the column takes no part; a `mask` is folded into it), and the
        row holds the bands of every zone -- block z bit for bit what mask = (zones == z) gives (rh_bands_configure_zonal; read with
        bands_zonal_read).  n_zones (default: the largest index + 1) may name zones that no column of this block has.
        `weights`: a uint16 per interior column of this block, and the row holds the likelihood-weighted quantiles -- column i counts as
        weights[i] identical members, 0: the column takes no part (a `mask` is folded into it) -- with the rows' weight sums beside them
        (rh_bands_configure_weighted; bands_read, bands_weight_sums).  Not together with `zones`."""
        names = list(names)
        ni = len(names)
        if len(kinds) != ni:
            raise ValueError(f"bands_configure: {len(kinds)} kinds for {ni} items")
        pr = np.ascontiguousarray(np.asarray(list(probs) or [0.0], dtype=np.float64).reshape(-1))
        npr = len(list(probs))
        ids = self._ids(names)
        kd = _ints([int(k) for k in kinds])
        mk = _byte_mask("bands_configure", mask, self.n, _COLUMNS) if names and mask is not None else None
        if names and weights is not None:
            if zones is not None:
                raise ValueError("bands_configure: weights with zones is not built")
            wt = _weights("bands_configure", weights, self.n, ("have",) + _COLUMNS[1:],
                          lambda wt: f"the weights are integers 0 ... 65535 (got dtype {wt.dtype}, {wt.min()} ... {wt.max()})")
            if mk is not None:
                wt = np.where(mk != 0, wt, np.uint16(0))
            self._check(self._lib.rh_bands_configure_weighted(self._h, ids, kd, ni, _ptr(pr), npr, int(interval), int(t_first), _ptr(wt), int(capacity)),
                        "rh_bands_configure_weighted")
            self._bands_shape = (ni, npr)   # (a refused configuration leaves the previous one)
            return
        if names and zones is not None:
            zn = _cell_map("bands_configure", "zone map", zones, self.n, _COLUMNS, lowest=-1)
            if mk is not None:
                zn = np.where(mk != 0, zn, np.int32(-1))
            nz = int(zn.max()) + 1 if n_zones is None else int(n_zones)
            self._check(self._lib.rh_bands_configure_zonal(self._h, ids, kd, ni, _ptr(pr), npr, int(interval), int(t_first), _ptr(zn), nz, int(capacity)),
                        "rh_bands_configure_zonal")
            self._bands_shape = (ni, nz, npr)   # (a refused configuration leaves the previous one)
            return
        self._check(self._lib.rh_bands_configure(self._h, ids, kd, ni, _ptr(pr), npr, int(interval), int(t_first), _ptr(mk), int(capacity)),
                    "rh_bands_configure")
        self._bands_shape = (ni, npr if ni else 0)   # (a refused configuration leaves the previous one)

    def _bands_items_zones_probs(self):
        """(items, zones or None, probs) of the configuration."""
        shape = self._bands_shape
        return shape if len(shape) == 3 else (shape[0], None, shape[1])

    def bands_count(self):
        """Rows recorded since bands_configure (with or without zones)."""
        n = C.c_int64()
        self._check(self._lib.rh_bands_count(self._h, C.byref(n)), "rh_bands_count")
        return n.value

    def bands_state(self):
        """The SUM accumulators of the interval under way, float64 (n_items, n) (with or without zones).  Synchronises."""
        acc = np.empty((self._bands_shape[0], self.n), dtype=np.float64)
        self._check(self._lib.rh_bands_state(self._h, _ptr(acc), acc.nbytes), "rh_bands_state")
        return acc

    def bands_restore(self, acc, rows):
        """Replace the accumulators (as bands_state gave them) and the count of rows by those of an interrupted run: after
        bands_configure, before the next step.  The rows before `rows` are not on the device: read from `rows` on."""
        a = np.ascontiguousarray(acc, dtype=np.float64)
        self._check(self._lib.rh_bands_restore(self._h, _ptr(a), a.nbytes, int(rows)), "rh_bands_restore")

    def bands_read(self, first, n):
        """Rows [first, first + n) of the ring: (hdr int64 (n, 2 + 2 * items): k, t1, then per item m and n_nan; values float64
        (n, items, probs))."""
        ni, _, npr = self._bands_items_zones_probs()   # (configured per zone: the call refuses)
        return self._ring_read("rh_bands_read", first, n, 2 + 2 * ni, (ni, npr))

    def bands_weight_sums(self, first, n):
        """The weight sums W of the rows [first, first + n) of a configuration with weights: int64 (n, items)."""
        n = int(n)
        wsum = np.empty((n, self._bands_shape[0]), dtype=np.int64)
        self._check(self._lib.rh_bands_weight_sums(self._h, int(first), n, _ptr(wsum), wsum.nbytes), "rh_bands_weight_sums")
        return wsum

    def bands_observations(self, obs, first_index=0):
        """Observations behind bands_configure: float64 (items, intervals) -- with zones (items, zones, intervals) -- NaN: missing, an
        all-NaN series: an item without observations.  Row interval k reads element k + first_index; beyond the series: missing.  From
        then on every counted interval records per item (and zone) the int64 pair (below, equal): the members, or with weights their
        weights, below and equal to the observation, -1 where it is missing (rh_bands_observations; bands_obs_read).  None, or no
        intervals: release them.  Every bands_configure drops them."""
        ni, nz, _ = self._bands_items_zones_probs()
        if obs is None or np.asarray(obs).size == 0:
            self._check(self._lib.rh_bands_observations(self._h, None, 1 if nz is None else nz, 0, 0), "rh_bands_observations")
            return
        o = np.ascontiguousarray(obs, dtype=np.float64)
        if o.ndim == 2:
            o = o[:, None, :]
        if o.ndim != 3 or (ni and o.shape[0] != ni):   # (nothing configured: the call refuses)
            raise ValueError(f"bands_observations: the observations have shape {np.shape(obs)}, the bands {ni} items ((items, intervals) or (items, series, intervals))")
        self._check(self._lib.rh_bands_observations(self._h, _ptr(o), int(o.shape[1]), int(o.shape[2]), int(first_index)), "rh_bands_observations")

    def bands_obs_read(self, first, n):
        """The pairs of the rows [first, first + n): int64 (n, items, 2) {below, equal} -- with zones (n, items, zones, 2) -- -1 where the
        observation is missing."""
        n = int(n)
        ni, nz, _ = self._bands_items_zones_probs()
        pairs = np.empty((n, ni) + (() if nz is None else (nz,)) + (2,), dtype=np.int64)
        self._check(self._lib.rh_bands_obs_read(self._h, int(first), n, _ptr(pairs), pairs.nbytes), "rh_bands_obs_read")
        return pairs

    def bands_zonal_read(self, first, n):
        """Rows [first, first + n) of the ring of a configuration with zones: (hdr int64 (n, 2): k, t1; counts int64 (n, items, zones, 2):
        m, n_nan; values float64 (n, items, zones, probs))."""
        n = int(n)
        ni, nz, npr = self._bands_items_zones_probs()
        nz = nz or 0   # (configured without zones: the call refuses)
        hdr = np.empty((n, 2), dtype=np.int64)
        counts = np.empty((n, ni, nz, 2), dtype=np.int64)
        values = np.empty((n, ni, nz, npr), dtype=np.float64)
        self._check(self._lib.rh_bands_zonal_read(self._h, int(first), n, _ptr(hdr), _ptr(counts), counts.nbytes, _ptr(values), values.nbytes),
                    "rh_bands_zonal_read")
        return hdr, counts, values

    def pure_output_planes(self):
        """Names of the planes the fused step of this context's model only produces (not stored by the steps of an rh_run_steps call
        that another step follows)."""
        model = 2 if self.routing else int(self.lateral)
        return [nm for nm, p in self.index.items() if self._lib.rh_plane_is_pure_output(model, p) == 1]

    def set_time_limit(self, t_end):
        """No step begins at or beyond model time t_end (None / negative: no limit): rh_run_steps(n) then runs at most n steps."""
        self._check(self._lib.rh_set_time_limit(self._h, -1 if t_end is None else int(t_end)), "rh_set_time_limit")

    def param_stats(self):
        """(fraction of the wavefronts whose derived parameters are not loaded, bytes per column of parameter loads that are one element
        per wave) -- how the lazy variants of the fused kernel will read the parameter planes as they are now."""
        d, u = C.c_double(), C.c_double()
        self._check(self._lib.rh_param_stats(self._h, C.byref(d), C.byref(u)), "rh_param_stats")
        return d.value, u.value

    def sparse_steps(self):
        return int(self._lib.rh_sparse_steps(self._h))

    def step_mode(self):
        """(lazy, tail) of the last fused step: it deferred the tau -> taum1 copies / its last wavefront formed the next step's control part."""
        m = self._lib.rh_step_mode(self._h)
        return bool(m & 1), bool(m & 2)

    # -- multi-GPU stepping without the host in the loop (RCCL from C) -------------------------------------------------
    def comm_init(self, unique_id, nranks, rank):
        """Every rank, collectively: an RCCL communicator on this context's device from rank 0's `comm_unique_id()` bytes."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.rh_comm_init(self._h, buf, int(nranks), int(rank)), "rh_comm_init")

    def comm_init_torch(self, group=None):
        """The same through an initialised torch.distributed process group: rank 0 creates the id, broadcast to the others."""
        import torch.distributed as dist

        rank, world = (dist.get_rank(group), dist.get_world_size(group)) if dist.is_initialized() else (0, 1)
        box = [comm_unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        self.comm_init(box[0], world, rank)

    def comm_info(self):
        """(ranks, this rank) of the communicator the context holds, as RCCL reports them (ncclCommCount, ncclCommUserRank)."""
        n, r = C.c_int(), C.c_int()
        self._check(self._lib.rh_comm_info(self._h, C.byref(n), C.byref(r)), "rh_comm_info")
        return n.value, r.value

    def comm_set_grid(self, px, py):
        """The process grid (px, py) of the communicator, ranks x-fastest (distributed.proc_rank_to_index); (nranks, 1) until called.
        The routing exchanges its halo with the neighbours in x and y (and the corners) of this grid."""
        self._check(self._lib.rh_comm_set_grid(self._h, int(px), int(py)), "rh_comm_set_grid")

    def run_steps_dist(self, nsteps):
        self._check(self._lib.rh_run_steps_dist(self._h, int(nsteps)), "rh_run_steps_dist")

    def placement_report(self):
        """Streaming-kernel time (ms) on every candidate arena rh_create probed, the chosen one first ([]: probing off)."""
        buf = (C.c_double * 32)()
        n = self._lib.rh_placement_report(self._h, buf, 32)
        return [float(buf[k]) for k in range(min(n, 32))]

    def step_finish(self, monthly=-1):
        self._check(self._lib.rh_step_finish(self._h, int(monthly)), "rh_step_finish")

    def step_summary_expand(self, dev_dst64):
        """rh_step_summary with the summary word also written as 64 int32 (0 / 1) to the device pointer."""
        self._check(self._lib.rh_step_summary_expand(self._h, C.c_void_p(dev_dst64)), "rh_step_summary_expand")

    def step_finish_compress(self, dev_src64, monthly=-1):
        """rh_step_finish from the all-reduced 64 int32 at the device pointer."""
        self._check(self._lib.rh_step_finish_compress(self._h, int(monthly), C.c_void_p(dev_src64)), "rh_step_finish_compress")

    def sync(self):
        self.call("rh_sync")

    def set_stream(self, stream_handle):
        self._check(self._lib.rh_set_stream(self._h, C.c_void_p(stream_handle)), "rh_set_stream")

    def predicates_expand(self, word, dev_ptr):
        self._check(self._lib.rh_predicates_expand(self._h, int(word), C.c_void_p(dev_ptr)), "rh_predicates_expand")

    def predicates_compress(self, word, dev_ptr):
        self._check(self._lib.rh_predicates_compress(self._h, int(word), C.c_void_p(dev_ptr)),
                    "rh_predicates_compress")

    def calibrate_copy(self, src_plane0, dst_plane0, nplanes):
        self._check(self._lib.rh_calibrate_copy(self._h, src_plane0, dst_plane0, nplanes), "rh_calibrate_copy")

    def predicate_words_ptr(self):
        return self._lib.rh_predicate_words(self._h)

    def enable_timing(self, on=True):
        self._check(self._lib.rh_enable_timing(self._h, int(on)), "rh_enable_timing")

    def timing_summary(self):
        """(total kernel ms, launches) of the fused kernel since enable_timing(True)."""
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._lib.rh_timing_summary(self._h, C.byref(ms), C.byref(cnt)), "rh_timing_summary")
        return float(ms.value), int(cnt.value)

    def timing_detail(self, cap=65536):
        """(kernel ms, dt_secs) per timed launch since enable_timing(True): the time-step class of every step."""
        ms = np.zeros(cap, dtype=np.float64)
        dts = np.zeros(cap, dtype=np.int32)
        cnt = C.c_int64()
        self._check(self._lib.rh_timing_detail(self._h, _ptr(ms), _ptr(dts), cap, C.byref(cnt)), "rh_timing_detail")
        k = min(int(cnt.value), cap)
        return ms[:k], dts[:k]


class SasContext:
    """One SAS / oxygen-18 transport problem on the device (rh_sas_ctx).  Thin, 1:1 with the C ABI."""

    def __init__(self, n_cells, ages, substeps=1, device=0, forcing_days=1, age_statistics=False,
                 keep_distributions=False, tracer="oxygen18", solver="deterministic", **settings):
        self._h = None
        lib = load()
        cfg = RhSasConfig()
        lib.rh_sas_default_config(C.byref(cfg))
        if tracer not in SAS_TRACERS:
            raise ValueError(f"tracer {tracer!r}: the hip backend transports {sorted(SAS_TRACERS)}")
        cfg.tracer = SAS_TRACERS[tracer]
        self.tracer = tracer
        if solver not in SAS_SOLVERS:
            raise ValueError(f"solver {solver!r}: the hip backend implements {sorted(SAS_SOLVERS)}")
        cfg.solver = SAS_SOLVERS[solver]
        self.solver = solver
        if tracer == "deuterium":
            settings = {**DEUTERIUM_DEFAULTS, **settings}
        cfg.n_cells, cfg.ages, cfg.substeps, cfg.device = int(n_cells), int(ages), int(substeps), int(device)
        cfg.forcing_days = int(forcing_days)
        cfg.age_statistics, cfg.keep_distributions = int(bool(age_statistics)), int(bool(keep_distributions))
        for k, v in settings.items():
            if k not in ("vsmow", "d18O_min", "d18O_max"):
                raise AttributeError(f"unknown setting {k}")
            setattr(cfg, k, v)
        h = C.c_void_p()
        rc = lib.rh_sas_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise NativeError(f"rh_sas_create failed ({rc}): {lib.rh_sas_last_error(None).decode()}")
        self._h, self._lib, self.cfg = h, lib, cfg
        self.n, self.ages, self.substeps, self.forcing_days = cfg.n_cells, cfg.ages, cfg.substeps, cfg.forcing_days
        self.names = [lib.rh_sas_array_name(i).decode() for i in range(lib.rh_sas_num_arrays())]
        self._index = {nm: i for i, nm in enumerate(self.names)}
        # what a configure call leaves for its read, as long as nothing is configured
        self._points_names, self._points_widths, self._points_ncells = [], [], 0
        self._totals_items = []              # [(key, width)]
        self._zonal_items, self._zonal_nzones = [], 0
        self._scores_shape = (0, 0)          # (items, samples)
        self._bands_shape = (0, 0, 0)        # (windows, items, probs); with zones (windows, items, zones, probs)
        self._age_bands_items, self._age_bands_shape = [], (0, 0)   # [(name, width)], (windows, probs)
        self._age_bands_zones = 0                                   # 0: the plain configuration
        self._age_window_items, self._age_window_shape, self._age_window_zones = [], (0, 0), 0   # the same of age_window_bands_configure

    def _check(self, rc, what):
        if rc != 0:
            raise NativeError(f"{what} failed ({rc}): {self._lib.rh_sas_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            self._lib.rh_sas_destroy(self._h)
            self._h = None

    __del__ = close

    def index(self, name):
        try:
            return self._index[name]
        except KeyError:
            raise KeyError(f"unknown SAS array {name!r}") from None

    def _ids(self, names):
        """The arrays' indices as a C int array."""
        return _ints([self.index(v) for v in names])

    def shape(self, name):
        """Logical shape of an array held by this context."""
        i = self.index(name)
        elems = self._lib.rh_sas_array_elems(self._h, i)
        if elems == 0:
            raise NativeError(f"array {name} is not held by this context (age_statistics / keep_distributions / tracer)")
        if name in DAILY_INPUTS:
            return (self.forcing_days, self.n)
        if elems == self.n:
            return (self.n,)
        return (self.n, elems // self.n)

    def dtype(self, name):
        return np.int32 if self._lib.rh_sas_array_is_int(self.index(name)) else np.float64

    def upload(self, name, host):
        a = np.ascontiguousarray(host, dtype=self.dtype(name))
        if a.shape != self.shape(name):
            raise ValueError(f"{name}: shape {a.shape}, expected {self.shape(name)}")
        self._check(self._lib.rh_sas_upload(self._h, self.index(name), _ptr(a), a.nbytes), f"rh_sas_upload({name})")

    def download(self, name):
        a = np.empty(self.shape(name), dtype=self.dtype(name))
        self._check(self._lib.rh_sas_download(self._h, self.index(name), _ptr(a), a.nbytes), f"rh_sas_download({name})")
        return a

    def upload_cells(self, name, first_cell, host):
        """Rows [first_cell, first_cell + len(host)) of a per-cell array."""
        a = np.ascontiguousarray(host, dtype=self.dtype(name))
        if a.shape[1:] != self.shape(name)[1:]:
            raise ValueError(f"{name}: row shape {a.shape[1:]}, expected {self.shape(name)[1:]}")
        self._check(self._lib.rh_sas_upload_cells(self._h, self.index(name), int(first_cell), a.shape[0], _ptr(a), a.nbytes),
                    f"rh_sas_upload_cells({name})")

    def download_cells(self, name, first_cell, n_cells):
        a = np.empty((int(n_cells),) + self.shape(name)[1:], dtype=self.dtype(name))
        self._check(self._lib.rh_sas_download_cells(self._h, self.index(name), int(first_cell), a.shape[0], _ptr(a), a.nbytes),
                    f"rh_sas_download_cells({name})")
        return a

    def set_daily_from_device(self, name, day_row, dev_ptr):
        """Row `day_row` of a daily input from n float64 on the device (e.g. Context.diag_device_ptr)."""
        self._check(self._lib.rh_sas_set_daily_from_device(self._h, self.index(name), int(day_row), C.c_void_p(dev_ptr)),
                    f"rh_sas_set_daily_from_device({name})")

    def device_ptr(self, name):
        return self._lib.rh_sas_array_device_ptr(self._h, self.index(name))

    def stages(self, day, mask):
        self._check(self._lib.rh_sas_stages(self._h, int(day), int(mask)), "rh_sas_stages")

    def step(self, day):
        self._check(self._lib.rh_sas_step(self._h, int(day)), "rh_sas_step")

    def run_days(self, day0, ndays):
        self._check(self._lib.rh_sas_run_days(self._h, int(day0), int(ndays)), "rh_sas_run_days")

    def sync(self):
        self._check(self._lib.rh_sas_sync(self._h), "rh_sas_sync")

    def set_stream(self, stream):
        self._check(self._lib.rh_sas_set_stream(self._h, C.c_void_p(stream)), "rh_sas_set_stream")

    def enable_timing(self, on=True):
        self._check(self._lib.rh_sas_enable_timing(self._h, int(on)), "rh_sas_enable_timing")

    def timing_summary(self):
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._lib.rh_sas_timing_summary(self._h, C.byref(ms), C.byref(cnt)), "rh_sas_timing_summary")
        return ms.value, cnt.value

    def _ring_read(self, what, first, n):
        """(n, tags (n,) int64, values float64 (n, row elements)) of the rows [first, first + n) of the ring rh_sas_<what>_*."""
        n = int(n)
        elems = C.c_int64()
        self._check(getattr(self._lib, f"rh_sas_{what}_row_elems")(self._h, C.byref(elems)), f"rh_sas_{what}_row_elems")
        tags, values = np.empty(n, dtype=np.int64), np.empty((n, elems.value), dtype=np.float64)
        self._check(getattr(self._lib, f"rh_sas_{what}_read")(self._h, int(first), n, _ptr(tags), _ptr(values), values.nbytes), f"rh_sas_{what}_read")
        return n, tags, values

    def _weighted_items(self, items):
        """(the items as (value, weight or None), their ids int32 (n_items, 2): -1 for no weight) of what the totals take: an array's
        name or (array, weight)."""
        items = [(it, None) if isinstance(it, str) else (it[0], it[1]) for it in items]
        return items, np.array([[self.index(v), -1 if w is None else self.index(w)] for v, w in items], dtype=np.int32).reshape(-1, 2)

    def _window_items(self, items):
        """(the items as (value, weight or None, kind int), their ids int32 (n_items, 3)) of what the scores and the bands take: the kind
        by its name or its number."""
        items = [(v, w, SAS_SCORES_KINDS[k] if isinstance(k, str) else int(k)) for v, w, k in items]
        return items, np.array([[self.index(v), -1 if w is None else self.index(w), k] for v, w, k in items], dtype=np.int32).reshape(-1, 3)

    def _totals_layout(self, items):
        """[(an item's key in rows and files, its width)] of the (value, weight) items of an accepted totals configuration."""
        return [(totals_item_name(v, w), 1 if v in DAILY_INPUTS else int(np.prod(self.shape(v)[1:], dtype=np.int64))) for v, w in items]

    @staticmethod
    def _totals_rows(values, layout, one_zone=False):
        """{item: {"wsum", "count", "sum"[, "min", "max"]}} of rows (n, Z, elements of a zone's part), every statistic a copy (n, Z) and
        "sum" of an age item (n, Z, width); one_zone: Z is 1 and the axis is dropped."""
        cut = (lambda a: a[:, 0].copy()) if one_zone else (lambda a: a.copy())
        out, off = {}, 0
        for key, w in layout:
            d = {"wsum": cut(values[:, :, off]), "count": cut(values[:, :, off + 1])}
            if w == 1:
                d.update(sum=cut(values[:, :, off + 2]), min=cut(values[:, :, off + 3]), max=cut(values[:, :, off + 4]))
                off += 5
            else:
                d["sum"] = cut(values[:, :, off + 2:off + 2 + w])
                off += 2 + w
            out[key] = d
        return out

    # -- time series at observation columns (rh_sas_points_*) -----------------------------------
    def points_configure(self, cells, names, capacity=4096):
        """Record `names` (arrays of the registry) at the local cells `cells` after every day into a ring of `capacity` rows; empty
        cells or names switch the recorder off."""
        names = list(names)
        c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1)
        self._check(self._lib.rh_sas_points_configure(self._h, _ptr(c), c.size, self._ids(names), len(names), int(capacity)),
                    "rh_sas_points_configure")
        # (a refused configuration leaves the previous one)
        on = bool(c.size and names)
        self._points_names = names if on else []
        self._points_widths = [int(np.prod(self.shape(v)[1:], dtype=np.int64)) for v in self._points_names]
        self._points_ncells = int(c.size) if on else 0

    def points_record(self, tag=0):
        """One row now (the initial values; a driver that steps by stage)."""
        self._check(self._lib.rh_sas_points_record(self._h, int(tag)), "rh_sas_points_record")

    def points_count(self):
        """Rows recorded since points_configure."""
        n = C.c_int64()
        self._check(self._lib.rh_sas_points_count(self._h, C.byref(n)), "rh_sas_points_count")
        return n.value

    def points_read(self, first, n):
        """(tags (n,) int64, {name: (n, K) or (n, K, width) float64}) of the rows [first, first + n) that are still resident."""
        n, tags, values = self._ring_read("points", first, n)
        out, off, K = {}, 0, self._points_ncells
        for v, w in zip(self._points_names, self._points_widths):
            block = values[:, off:off + K * w]
            out[v] = block.copy() if w == 1 else block.reshape(n, K, w).copy()
            off += K * w
        return tags, out

    # -- catchment totals (rh_sas_totals_*) -------------------------------------------------------
    def totals_configure(self, items, mask=None, capacity=4096):
        """Reduce `items` over the cells where `mask` is set (None: all) after every day into a ring of `capacity` rows.  An item is
        an array's name or (array, weight) with a daily flux input as weight; no items switch the recorder off."""
        items, flat = self._weighted_items(items)
        m = None if mask is None else _byte_mask("totals_configure", mask, self.n, _CELLS)
        self._check(self._lib.rh_sas_totals_configure(self._h, _ptr(m), _ptr(flat), len(items), int(capacity)), "rh_sas_totals_configure")
        # (a refused configuration leaves the previous one)
        self._totals_items = self._totals_layout(items)

    def totals_record(self, tag=0, day=-1):
        """One row now (the initial values; a driver that steps by stage).  day < 0: no daily row, so an item with a weight or a daily
        value has no eligible cell."""
        self._check(self._lib.rh_sas_totals_record(self._h, int(tag), int(day)), "rh_sas_totals_record")

    def totals_count(self):
        """(rows recorded since totals_configure, cells inside the mask)."""
        rows, ncells = C.c_int64(), C.c_int64()
        self._check(self._lib.rh_sas_totals_count(self._h, C.byref(rows), C.byref(ncells)), "rh_sas_totals_count")
        return rows.value, ncells.value

    def totals_read(self, first, n):
        """(tags (n,) int64, {item: {"wsum", "count", "sum"[, "min", "max"]}}) of the rows [first, first + n) that are still resident;
        an item's key is `<array>` or `<array>_by_<weight>`, its statistics are (n,) float64, "sum" of an age item (n, width)."""
        n, tags, values = self._ring_read("totals", first, n)
        return tags, self._totals_rows(values[:, None, :], self._totals_items, one_zone=True)

    # -- zonal totals (rh_sas_zonal_*) ------------------------------------------------------------
    def zonal_configure(self, items, zones=None, n_zones=0, capacity=4096):
        """Reduce `items` (as totals_configure) over the cells of every zone of `zones` -- an index per cell, -1: outside, else
        0 ... n_zones - 1 -- after every day into a ring of `capacity` rows; no items switch the recorder off."""
        items, flat = self._weighted_items(items)
        z = None if zones is None else _cell_map("zonal_configure", "zone map", zones, self.n, _CELLS)
        self._check(self._lib.rh_sas_zonal_configure(self._h, _ptr(z), int(n_zones), _ptr(flat), len(items), int(capacity)), "rh_sas_zonal_configure")
        # (a refused configuration leaves the previous one)
        self._zonal_items = self._totals_layout(items)
        self._zonal_nzones = int(n_zones) if items else 0

    def zonal_record(self, tag=0, day=-1):
        """One row now; day < 0: no daily row (as totals_record)."""
        self._check(self._lib.rh_sas_zonal_record(self._h, int(tag), int(day)), "rh_sas_zonal_record")

    def zonal_count(self):
        """(rows recorded since zonal_configure, cells of every zone: int64 (n_zones,))."""
        rows = C.c_int64()
        nz = self._zonal_nzones
        cells = np.zeros(max(1, nz), dtype=np.int64)
        self._check(self._lib.rh_sas_zonal_count(self._h, C.byref(rows), _ptr(cells)), "rh_sas_zonal_count")
        return rows.value, cells[:nz]

    def zonal_read(self, first, n):
        """(tags (n,) int64, {item: {"wsum", "count", "sum"[, "min", "max"]}}) of the rows [first, first + n) that are still resident;
        the statistics are (n, Z) float64, "sum" of an age item (n, Z, width)."""
        n, tags, values = self._ring_read("zonal", first, n)
        return tags, self._totals_rows(values.reshape(n, self._zonal_nzones, values.shape[1] // self._zonal_nzones), self._zonal_items)

    # -- scores against observed samples (rh_sas_scores_*) ----------------------------------------
    def scores_configure(self, items, obs=None, windows=None, series=None):
        """Score `items` against `obs` (n_items, n_series, n_samples; NaN: missing) over the windows (first_day, last_day), int (K,)
        each, inclusive, in the context's count of scored days, which restarts at 0 here.  An item is (value, weight or None, kind)
        with kind "bulk" (flux-weighted mean over the window, needs a weight), "mean" or "last".  `series`: the series of every cell
        (< 0: not scored), None: every cell series 0.  No items: release everything and stop."""
        items, flat = self._window_items(items)
        o = first = last = sr = None
        shape = (0, 0, 0)
        if items:
            o = np.ascontiguousarray(obs, dtype=np.float64)
            first, last = _window_pair(windows)
            if o.ndim != 3 or o.shape[0] != len(items) or o.shape[2] != first.size or last.size != first.size:
                raise ValueError(f"scores_configure: observations of shape {o.shape} and windows of {first.size} and {last.size} days "
                                 f"for {len(items)} items ((n_items, n_series, n_samples))")
            shape = o.shape
            if series is not None:
                sr = _cell_map("scores_configure", "series map", series, self.n, _CELLS)
        self._check(self._lib.rh_sas_scores_configure(self._h, _ptr(flat), len(items), _ptr(sr), int(shape[1]), _ptr(o), _ptr(first), _ptr(last),
                                                      int(shape[2])), "rh_sas_scores_configure")
        self._scores_shape = (len(items), int(shape[2]))   # (a refused configuration leaves the previous one)

    def scores_record(self, day=0):
        """Score now as the next day of the count, `day` the row of the daily inputs (a driver that steps by stage)."""
        self._check(self._lib.rh_sas_scores_record(self._h, int(day)), "rh_sas_scores_record")

    def scores_read(self):
        """(moments float64 (n_items, 9, n): num, den, n, m1 = sum sim, m2 = sum sim^2, m3 = sum sim obs, m4 = sum (sim - obs)^2,
        so = sum obs, soo = sum obs^2; closed uint8 (n_samples,); days scored since scores_configure).  Synchronises."""
        ni, nk = self._scores_shape
        moments = np.empty((ni, 9, self.n), dtype=np.float64)
        closed = np.empty(nk, dtype=np.uint8)
        days = C.c_int64()
        self._check(self._lib.rh_sas_scores_read(self._h, _ptr(moments), moments.nbytes, _ptr(closed), closed.nbytes, C.byref(days)),
                    "rh_sas_scores_read")
        return moments, closed, days.value

    # -- transport bands: quantiles across the cells per sample window (rh_sas_bands_*) --------------
    def _bands_arguments(self, method, probs, windows, mask, weights, zones=None):
        """(probs float64 (P,), first_day and last_day int64 (K,), mask uint8 (n,) or None, weights uint16 (n,) or None) of what
        bands_configure and age_bands_configure take alike; `zones` are only measured here, with the mask and the weights."""
        if windows is None or len(windows) != 2:
            raise ValueError(f"{method}: windows = (first_day, last_day), two integer arrays (K,)")
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        first, last = _window_pair(windows)
        if first.size != last.size:
            raise ValueError(f"{method}: windows of {first.size} and {last.size} days")
        have = ("have",) + _CELLS[1:]   # ("the mask have 5 cells, the context 6": one sentence for the three)
        for name, a in (("mask", mask), ("weights", weights), ("zones", zones)):
            if a is not None:
                _sized(method, name, np.asarray(a), self.n, have)
        mk = None if mask is None else _byte_mask(method, mask, self.n, have)
        wt = None if weights is None else _weights(method, weights, self.n, have,
                                                   lambda wt: f"weights of dtype {wt.dtype} (integers within 0 ... 65535)")
        return pr, first, last, mk, wt

    def bands_configure(self, items, probs=(), windows=None, mask=None, weights=None, obs=None, zones=None, n_zones=None):
        """The exact quantiles `probs` (each within [0, 1]) ACROSS the cells of the window values of `items` -- (value, weight or None,
        kind) as scores_configure takes them -- over the windows (first_day, last_day), int (K,) each, inclusive, in the context's count
        of recorded days, which restarts at 0 here.  `mask`: (n,), 0: the cell takes no part; `weights`: (n,) integers 0 ... 65535, the
        likelihood weight of every cell, 0: no part; `obs`: (n_items, K) float64, NaN: missing -- where the observation falls is counted
        too.  No items: release everything and stop.
        `zones`: (n,) integers, -1: outside every zone, else 0 ... n_zones - 1 (default: the largest index + 1) -- the bands of every zone in
        one run, block z bit for bit what mask = (zones == z) & mask gives; `obs` is then (n_items, n_zones, K), and bands_read returns
        the zone axis behind the items' (rh_sas_bands_configure_zonal).  With weights a zone holds at most 65536 participating cells."""
        items, flat = self._window_items(items)
        pr = first = last = mk = wt = o = zn = None
        nz = 0
        if items:
            pr, first, last, mk, wt = self._bands_arguments("bands_configure", probs, windows, mask, weights, zones)
            if zones is not None:
                zn = np.asarray(zones).reshape(-1)
                if zn.dtype.kind not in "iu":
                    raise ValueError(f"bands_configure: zones of dtype {zn.dtype} (integers: -1 or 0 ... n_zones - 1)")
                nz = int(n_zones) if n_zones is not None else int(zn.max()) + 1 if zn.size else 0
                zn = _cell_map("bands_configure", "zones", zn, self.n, _CELLS, lowest=-2)
            if obs is not None:
                o = np.ascontiguousarray(obs, dtype=np.float64)
                want = (len(items), first.size) if zn is None else (len(items), nz, first.size)
                if o.shape != want:
                    raise ValueError(f"bands_configure: observations of shape {o.shape} for {len(items)} items{'' if zn is None else f', {nz} zones'} and "
                                     f"{first.size} windows")
        nk, npr = 0 if first is None else first.size, 0 if pr is None else pr.size
        if zn is not None:
            self._check(self._lib.rh_sas_bands_configure_zonal(self._h, _ptr(flat), len(items), _ptr(pr), npr, _ptr(zn), nz, _ptr(mk), _ptr(wt), _ptr(o),
                                                               _ptr(first), _ptr(last), nk), "rh_sas_bands_configure_zonal")
            self._bands_shape = (nk, len(items), nz, npr)   # (a refused configuration leaves the previous one)
            return
        self._check(self._lib.rh_sas_bands_configure(self._h, _ptr(flat), len(items), _ptr(pr), npr, _ptr(mk), _ptr(wt), _ptr(o),
                                                     _ptr(first), _ptr(last), nk), "rh_sas_bands_configure")
        self._bands_shape = (nk, len(items), npr)   # (a refused configuration leaves the previous one)

    def bands_record(self, day=0):
        """Record now as the next day of the count, `day` the row of the daily inputs (a driver that steps by stage)."""
        self._check(self._lib.rh_sas_bands_record(self._h, int(day)), "rh_sas_bands_record")

    def bands_read(self):
        """(rows float64 (K, n_items, n_probs), NaN until the window closed; hdr int64 (K, n_items, 3): m, n_nan, W; pairs int64
        (K, n_items, 2): below, equal, -1 without an observation; closed uint8 (K,); days recorded since bands_configure).  Configured with
        zones: rows (K, n_items, n_zones, n_probs), hdr (K, n_items, n_zones, 3), pairs (K, n_items, n_zones, 2).  Synchronises."""
        *lead, npr = self._bands_shape
        nk, zonal = lead[0], len(lead) == 3
        rows = np.empty((*lead, npr), dtype=np.float64)
        hdr = np.empty((*lead, 3), dtype=np.int64)
        pairs = np.empty((*lead, 2), dtype=np.int64)
        closed = np.empty(nk, dtype=np.uint8)
        days = C.c_int64()
        name = "rh_sas_bands_zonal_read" if zonal else "rh_sas_bands_read"
        self._check(getattr(self._lib, name)(self._h, _ptr(rows), rows.nbytes, _ptr(hdr), hdr.nbytes, _ptr(pairs), pairs.nbytes, _ptr(closed),
                                             closed.nbytes, C.byref(days)), name)
        return rows, hdr, pairs, closed, days.value

    # -- transport bands by age: the bands of every age class of an age-resolved array (rh_sas_age_bands_*) --------------
    def age_bands_configure(self, items, probs=(), windows=None, mask=None, weights=None, zones=None, n_zones=None):
        """The exact quantiles `probs` ACROSS the cells for EVERY age class of the age-resolved arrays `items` -- an array's name, or
        (value, None, "last") as bands_configure takes an item; window means are not built -- on the closing day of each of the windows
        (first_day, last_day), int (K,) each, inclusive, in this recorder's own count of recorded days, which restarts at 0 here.  `mask`
        and `weights` as bands_configure takes them; with weights at most 65536 cells take part.  Block (item, age class a) is bit for
        bit what bands_configure records for the width-1 values A[:, a] with kind "last".  No items: release everything and stop.
        `zones`: (n,) integers, -1: outside every zone, else 0 ... n_zones - 1 (default: the largest index + 1) -- the bands by age of every
        zone in one run, block (zone z, age class a) bit for bit what mask = (zones == z) & mask gives; age_bands_read then returns the
        zone axis in front of the age axis (rh_sas_age_bands_configure_zonal).  With weights the bound of 65536 participating cells
        holds per zone, not in total."""
        items, flat = self._window_items([(it, None, "last") if isinstance(it, str) else it for it in items])
        pr, first, last, mk, wt, zn, nz = self._age_arguments("age_bands_configure", items, probs, windows, mask, weights, zones, n_zones)
        nk, npr = 0 if first is None else first.size, 0 if pr is None else pr.size
        if zn is not None:
            self._check(self._lib.rh_sas_age_bands_configure_zonal(self._h, _ptr(flat), len(items), _ptr(pr), npr, _ptr(zn), nz, _ptr(mk), _ptr(wt),
                                                                   _ptr(first), _ptr(last), nk), "rh_sas_age_bands_configure_zonal")
        else:
            self._check(self._lib.rh_sas_age_bands_configure(self._h, _ptr(flat), len(items), _ptr(pr), npr, _ptr(mk), _ptr(wt), _ptr(first),
                                                             _ptr(last), nk), "rh_sas_age_bands_configure")
        # (a refused configuration leaves the previous one)
        self._age_bands_items = [(v, int(np.prod(self.shape(v)[1:], dtype=np.int64))) for v, _, _ in items]
        self._age_bands_shape = (nk, npr)
        self._age_bands_zones = 0 if zn is None else nz

    def _age_arguments(self, method, items, probs, windows, mask, weights, zones, n_zones):
        """_bands_arguments and (the zone map int32 (n,) or None, n_zones) of what both observers by age take; without items all None and 0."""
        if not items:
            return None, None, None, None, None, None, 0
        pr, first, last, mk, wt = self._bands_arguments(method, probs, windows, mask, weights, zones)
        zn, nz = None, 0
        if zones is not None:
            zn = np.asarray(zones).reshape(-1)
            if zn.dtype.kind not in "iu":
                raise ValueError(f"{method}: zones of dtype {zn.dtype} (integers: -1 or 0 ... n_zones - 1)")
            nz = int(n_zones) if n_zones is not None else int(zn.max()) + 1 if zn.size else 0
            zn = _cell_map(method, "zones", zn, self.n, _CELLS, lowest=-2)
        return pr, first, last, mk, wt, zn, nz

    def _age_read(self, prefix, name, layout, shape, nz):
        """What age_bands_read and age_window_bands_read return: the row count by `prefix`_row_elems, the read by the function `name`."""
        total = C.c_int64()
        self._check(getattr(self._lib, prefix + "_row_elems")(self._h, C.byref(total)), prefix + "_row_elems")
        nk, npr = shape
        rows = np.empty((nk, total.value * max(nz, 1), npr), dtype=np.float64)
        hdr = np.empty((nk, total.value * max(nz, 1), 3), dtype=np.int64)
        closed = np.empty(nk, dtype=np.uint8)
        days = C.c_int64()
        self._check(getattr(self._lib, name)(self._h, _ptr(rows), rows.nbytes, _ptr(hdr), hdr.nbytes, _ptr(closed), closed.nbytes, C.byref(days)), name)
        out_rows, out_hdr, off = {}, {}, 0
        for v, w in layout:
            wz = w * max(nz, 1)
            lead = (nk, nz, w) if nz else (nk, w)
            out_rows[v], out_hdr[v] = rows[:, off:off + wz].reshape(*lead, npr).copy(), hdr[:, off:off + wz].reshape(*lead, 3).copy()
            off += wz
        return out_rows, out_hdr, closed, days.value

    def age_bands_record(self, day=0):
        """Record now as the next day of the count (a driver that steps by stage).  `day` (>= 0) is the row of the daily inputs, as for
        bands_record; it is checked and otherwise ignored today, because every item is "last" and reads no daily input."""
        self._check(self._lib.rh_sas_age_bands_record(self._h, int(day)), "rh_sas_age_bands_record")

    def age_bands_read(self):
        """(rows {name: float64 (K, W, n_probs)}, NaN until the window closed; hdr {name: int64 (K, W, 3)}: m, n_nan, W per age class;
        closed uint8 (K,); days recorded since age_bands_configure), W the item's width (ages or ages + 1).  Configured with zones: rows
        {name: (K, n_zones, W, n_probs)}, hdr {name: (K, n_zones, W, 3)}.  Synchronises."""
        nz = self._age_bands_zones
        return self._age_read("rh_sas_age_bands", "rh_sas_age_bands_zonal_read" if nz else "rh_sas_age_bands_read", self._age_bands_items,
                              self._age_bands_shape, nz)

    # -- window means of the bands by age: the band of a bulk sample's age-resolved value (rh_sas_age_window_bands_*) --------------
    def age_window_bands_configure(self, items, probs=(), windows=None, mask=None, weights=None, zones=None, n_zones=None):
        """The exact quantiles `probs` ACROSS the cells for every age class of the WINDOW MEANS of the age-resolved arrays `items`:
        ("tt_q_ss", "q_ss", "bulk") -- the mean over the window's days weighted by the daily flux, a bottle's travel time distribution --
        or ("sa_s", None, "mean").  Everything else as age_bands_configure takes it, `zones` included; "last" belongs there.  Block (item,
        [zone z,] age class a) is bit for bit what bands_configure records for the width-1 values A[:, a] with the same weight and kind.
        An observer of its own beside age_bands_*: 16 bytes per participating cell and age class stay on the device, and every day of
        an open window launches.  No items: release everything and stop."""
        items, flat = self._window_items(items)
        pr, first, last, mk, wt, zn, nz = self._age_arguments("age_window_bands_configure", items, probs, windows, mask, weights, zones, n_zones)
        nk, npr = 0 if first is None else first.size, 0 if pr is None else pr.size
        self._check(self._lib.rh_sas_age_window_bands_configure(self._h, _ptr(flat), len(items), _ptr(pr), npr, _ptr(zn), nz, _ptr(mk), _ptr(wt),
                                                                _ptr(first), _ptr(last), nk), "rh_sas_age_window_bands_configure")
        # (a refused configuration leaves the previous one)
        self._age_window_items = [(v, int(np.prod(self.shape(v)[1:], dtype=np.int64))) for v, _, _ in items]
        self._age_window_shape = (nk, npr)
        self._age_window_zones = 0 if zn is None else nz

    def age_window_bands_record(self, day=0):
        """Record now as the next day of the count, `day` the row of the daily weights (a driver that steps by stage)."""
        self._check(self._lib.rh_sas_age_window_bands_record(self._h, int(day)), "rh_sas_age_window_bands_record")

    def age_window_bands_read(self):
        """(rows {name: float64 (K, [n_zones,] W, n_probs)}, hdr {name: int64 (K, [n_zones,] W, 3)}, closed uint8 (K,), days recorded since
        age_window_bands_configure), as age_bands_read returns them.  Synchronises."""
        return self._age_read("rh_sas_age_window_bands", "rh_sas_age_window_bands_read", self._age_window_items, self._age_window_shape,
                              self._age_window_zones)
