"""The C-ABI library loads and exports every entry point include/roger_hip.h declares; the binding declares each with the
types of its prototype, read from the headers, and refuses a type it does not know; the
generated load/store sets are up to date.  No compute calls (CPU-only suite)."""
import ctypes
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions(header="roger_hip.h"):
    txt = open(os.path.join(REPO, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rh_\w+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from roger_amd import _native
    from roger_amd.build import build_native

    build_native()
    lib = ctypes.CDLL(_native.LIB_PATH)
    declared = _declared_functions()
    assert len(declared) >= 40
    missing = [f for f in declared if not hasattr(lib, f)]
    assert not missing, missing
    # the binding declares the same set
    assert sorted(_native.DECLARED_SYMBOLS) == declared
    # include/roger_hip_sas.h
    declared_sas = _declared_functions("roger_hip_sas.h")
    assert len(declared_sas) >= 19
    missing = [f for f in declared_sas if not hasattr(lib, f)]
    assert not missing, missing
    assert sorted(_native.SAS_DECLARED_SYMBOLS) == declared_sas


def _declared_parameter_counts(header):
    """{name: number of parameters} of a header by this test's own reading: the top-level commas of the parameter list + 1, 0 for (void)."""
    txt = open(os.path.join(REPO, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: 0 if params.strip() == "void" else params.count(",") + 1 for name, params in re.findall(r"\b(rh_\w+)\s*\(([^()]*)\)", txt)}


vp, cp, i32, i64, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
# written by hand from include/roger_hip.h and include/roger_hip_sas.h: every row of the mapping the headers use -- `char *` as a parameter
# and as a return, other pointers (to a context, a structure, a context pointer, void, double, int32_t, int64_t, unsigned char, uint16_t), int,
# int64_t, size_t, (void), a void return, a pointer return
PINNED = {
    "rh_create": (i32, [vp, vp]),
    "rh_destroy": (None, [vp]),
    "rh_last_error": (cp, [vp]),
    "rh_abi_version": (i32, []),
    "rh_plane_index": (i32, [cp]),
    "rh_num_cells": (i64, [vp]),
    "rh_plane_device_ptr": (vp, [vp, i32]),
    "rh_upload": (i32, [vp, i32, vp, sz]),
    "rh_diag_set_slot_state": (i32, [vp, i32, i64, i64, i64]),
    "rh_set_forcing_stations": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i32, vp]),
    "rh_timing_detail": (i32, [vp, vp, vp, i64, vp]),
    "rh_scores_configure": (i32, [vp, vp, vp, i32, vp, i32, i64, vp, i64, i64]),
    "rh_svat_step_scalars": (i32, [vp, i32, vp]),
    "rh_sas_bands_configure_zonal": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, i64]),
    "rh_sas_bands_read": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp]),
    "rh_sas_array_elems": (i64, [vp, i32]),
    "rh_sas_array_name": (cp, [i32]),
}


def test_declared_types_of_pinned_functions():
    """What load() set on the library object, against signatures written by hand; the two rows of the mapping no header function uses
    today (a double and an int32_t passed by value) through the parser alone."""
    from roger_amd import _native

    lib = _native.load()
    for name, (restype, argtypes) in PINNED.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    got = _native._prototypes("double rh_a(const rh_ctx *ctx, double x, int32_t k, const int32_t *v, size_t bytes);\n"
                              "const char *rh_b(void);\nvoid *rh_c(const char *name, char **out);")
    assert got == {"rh_a": (ctypes.c_double, [vp, ctypes.c_double, i32, vp, sz]), "rh_b": (cp, []), "rh_c": (vp, [cp, vp])}


def test_every_declared_function_has_its_parameter_count():
    from roger_amd import _native

    lib = _native.load()
    allowed = {vp, cp, i32, i64, sz, ctypes.c_double}
    seen = 0
    for header in ("roger_hip.h", "roger_hip_sas.h"):
        counts = _declared_parameter_counts(header)
        assert sorted(counts) == _declared_functions(header)
        for name, n in counts.items():
            fn = getattr(lib, name)
            assert len(fn.argtypes) == n, (name, fn.argtypes, n)
            assert set(fn.argtypes) <= allowed, (name, fn.argtypes)
            assert fn.restype is None or fn.restype in allowed, (name, fn.restype)
            seen += 1
    assert seen == len(_native.DECLARED_SYMBOLS) + len(_native.SAS_DECLARED_SYMBOLS) >= 40 + 19


def test_parser_refuses_what_it_does_not_know():
    import pytest

    from roger_amd import _native

    with pytest.raises(_native.NativeError, match=r"rh_x.*'float'"):
        _native._prototypes("typedef struct rh_ctx rh_ctx;\nint rh_x(rh_ctx *ctx, float v);\n")
    with pytest.raises(_native.NativeError, match=r"rh_x.*'float'"):
        _native._prototypes("float rh_x(rh_ctx *ctx);\n")
    with pytest.raises(_native.NativeError, match=r"rh_x.*'unsigned int'"):
        _native._prototypes("int rh_x(unsigned int n);\n")
    with pytest.raises(_native.NativeError, match="rh_x.*is not a prototype"):
        _native._prototypes("int rh_x(int (*callback)(int));\n")
    got = _native._prototypes("#define RH_CALL(x) \\\n    rh_macro(x)\n/* int rh_gone(int a); */\n// int rh_gone_too(int a);\n"
                              "int rh_y(rh_ctx *ctx, /* a, b, */ int64_t n, // , int m,\n         const double *v);\n")
    assert got == {"rh_y": (i32, [vp, i64, vp])}


def test_old_variant_loads_a_library_that_lacks_symbols(monkeypatch):
    """RH_OLD_VARIANT=1: the declarations run over the stand-in, and a function the library lacks raises only when it is called --
    declared as load()'s loop declares one -- in a fresh process, because a process loads the library once."""
    from roger_amd.build import build_native

    build_native()
    monkeypatch.setenv("RH_OLD_VARIANT", "1")
    code = ("import ctypes\n"
            "from roger_amd import _native\n"
            "lib = _native.load()\n"
            "assert isinstance(lib, _native._Tolerant) and lib.rh_num_planes() > 0 and lib.rh_num_cells.restype is ctypes.c_int64\n"
            "absent = lib.rh_not_in_this_library\n"
            "absent.restype = ctypes.c_int\n"
            "absent.argtypes = [ctypes.c_void_p]\n"
            "try:\n"
            "    absent(None)\n"
            "except _native.NativeError as e:\n"
            "    assert 'rh_not_in_this_library is not exported by' in str(e)\n"
            "    print('refused when called')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "refused when called"


def test_sas_array_registry_matches_def():
    from roger_amd import _native

    txt = open(os.path.join(REPO, "include", "rh_sas_arrays.def")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    arrays = re.findall(r"RH_SAS_ARRAY\((\w+),\s*(\w+),\s*(\w+)\)", txt)
    lib = _native.load()
    assert lib.rh_sas_num_arrays() == len(arrays)
    for i, (name, kind, _when) in enumerate(arrays):
        assert lib.rh_sas_array_name(i).decode() == name
        assert lib.rh_sas_array_index(name.encode()) == i
        assert bool(lib.rh_sas_array_is_int(i)) == (kind == "MASK")
    assert lib.rh_sas_array_index(b"no_such_array") == -1
    assert set(_native.DAILY_INPUTS) == {n for n, k, _ in arrays if k == "DAILY"}


def test_plane_registry_matches_fields_def():
    from roger_amd import _native

    txt = open(os.path.join(REPO, "include", "rh_fields.def")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    fields = re.findall(r"RH_FIELD\((\w+),\s*(\w+),\s*(\d)\)", txt)
    expect = []
    for name, typ, lv in fields:
        expect.append((name, typ == "I32"))
        if lv == "2":
            expect.append((name + "_m1", typ == "I32"))
    assert _native.plane_table() == expect
    lib = _native.load()
    assert lib.rh_plane_index(b"theta_rz_m1") == [n for n, _ in expect].index("theta_rz_m1")
    assert lib.rh_plane_index(b"no_such_plane") == -1


def test_generated_sets_are_current():
    inc = os.path.join(REPO, "roger_amd", "csrc", "rh_sets.inc")
    before = open(inc).read()
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_sets.py")], check=True)
    assert open(inc).read() == before, "rh_sets.inc is stale: run tools/gen_sets.py"
    # the fused step stores what the reference writes per step: 153 planes = 1224 B, plus `prec`,
    # which the summary path selects inside the fused kernel instead of in a pass of its own
    m = re.search(r"// rt_step: loads (\d+) planes, stores (\d+) planes", before)
    assert m and int(m.group(2)) == 154
    # lazy rotation: over the stages of a sequence the lazy sets store the same planes but the 30 X_m1 of the rotation
    # pairs, load none of them, and fill exactly the X_m1 that the step reads from X's register
    rot = set(re.search(r"#define RH_ROTATION_FIELDS\(X\) (.*)", before).group(1).replace("X(", "").replace(")", "").split())
    assert len(rot) == 30
    for seq in ("step", "step_monthly", "step_lateral", "step_lateral_monthly"):
        def planes(kind):
            out = []
            for line in re.findall(rf"#define RH_SEQ_{seq}_{kind}_\w+\(\w\)(.*)", before):
                out += re.findall(r"\w\((\w+)(?:, \w+)?\)", line)
            return out
        eager = set(planes("STORE")) | {x + "_m1" for x in planes("ROT")}
        lazy = set(planes("LSTORE"))
        assert eager - lazy == {x + "_m1" for x in rot}, seq
        assert not {p for p in planes("LLOAD") if p in {x + "_m1" for x in rot}}, seq
        assert set(planes("LLOAD")) <= set(planes("LOAD")) and len(planes("LLOAD")) == len(set(planes("LLOAD"))), seq
        assert set(planes("ALIAS")) <= {x + "_m1" for x in rot} and len(planes("ALIAS")) == 11, seq


def test_no_gpu_means_loud_failure():
    import torch

    from roger_amd import _native

    if torch.cuda.is_available():
        import pytest

        pytest.skip("a GPU is present")
    import pytest

    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        _native.Context(2, 2)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        _native.SasContext(4, 40)


def test_integration_stub_names_every_config_field():
    """INTEGRATION.md shows the ctypes structs a maintainer would add on the reference's side: they must carry every field of rh_config /
    rh_sas_config in the header's order (a shorter struct would let rh_default_config write past it)."""
    import os
    import re

    from roger_amd import _native

    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    for cls, start in ((_native.RhConfig, "class RhConfig(C.Structure)"), (_native.RhSasConfig, "class RhSasConfig(C.Structure)")):
        block = doc[doc.index(start):]
        block = block[:block.index("\n\n")]
        names = re.findall(r'"(\w+)"', block)
        assert names == [n for n, _ in cls._fields_], (cls.__name__, names)
