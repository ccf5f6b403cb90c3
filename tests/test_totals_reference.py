"""CPU: the totals' reduction order (tests/totals_reference.py: tree_totals) against math.fsum and hand-worked values, the host
package's copy of it, `combine`, the validation, and the host package's AreaTotals on the oracle double: a RogerSetup script ends with
a `.totals.nc` whose rows are tree_totals of the double's own planes after every step."""
import math

import numpy as np
import pytest

from golden_util import load_case
from totals_reference import TotalsOracleContext, same_bits, tree_totals

B = 2.0 ** 60      # B + 1 == B and B + 2 == B in float64 (ulp(B) = 256): where a 1 meets B decides the result
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 256, 257, 1000, 4099, 65537, 70001])
def test_tree_against_fsum(n):
    rng = np.random.default_rng(n)
    v = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    for mask in (None, rng.random(n) < 0.5 if n > 1 else np.array([True])):
        sel = v if mask is None else v[mask]
        s, lo, hi = tree_totals(v, mask)
        bound = len(sel) * EPS * np.abs(sel).max()
        assert abs(s - math.fsum(sel)) <= bound, (n, s, math.fsum(sel), bound)
        assert lo == sel.min() and hi == sel.max()


def cols(n, **at):
    v = np.zeros(n)
    for k, x in at.items():
        v[int(k[1:])] = x
    return v


# (columns, values, the sum worked by hand, why)
HAND = [
    (3, cols(3, c0=B, c1=1.0, c2=-B), 1.0, "stride 2: B + -B = 0 and 1 + identity; stride 1: 0 + 1 (left to right: 0)"),
    (64, cols(64, c0=B, c1=-B, c32=1.0), 0.0, "stride 32: lane 0 = B + 1 = B, lane 1 = -B; stride 1: B + -B (left to right: 1)"),
    (65, cols(65, c0=B, c1=-B, c32=1.0, c64=1.0), 1.0, "wavefront 0 = 0 as above, wavefront 1 = 1 (left to right: 2)"),
    (256, cols(256, c0=B, c64=1.0, c128=-B, c192=1.0), 0.0, "(B + 1) + (-B + 1) = B + -B (left to right: 1)"),
    (257, cols(257, c0=B, c255=1.0, c256=-B), 0.0, "tile 0 = (B + 0) + (0 + 1) = B, tile 1 = -B; accumulators 0 and 1 meet at stride 1"),
    (65537, cols(65537, c0=B, c256=1.0, c65536=-B), 1.0,
     "257 tiles: accumulator 0 = (0 + B) + -B = 0 (tiles 0 and 256), accumulator 1 = 1 (in tile order: B + 1 + -B = 0; the first 256 "
     "tiles only: B)"),
]


@pytest.mark.parametrize("n,v,want,why", HAND, ids=[str(h[0]) for h in HAND])
def test_tree_against_hand_worked_values(n, v, want, why):
    from roger_amd import totals

    assert B + 1.0 == B and B + 2.0 == B
    for f in (tree_totals, totals.tree_totals):      # the restatement, and the host package's own (record 0 of the file)
        s, lo, hi = f(v)
        assert same_bits(s, want), (f.__module__, n, s, want, why)
        assert (lo, hi) == (-B, B)
    rng = np.random.default_rng(n)
    r = rng.normal(size=n)
    m = rng.random(n) < 0.5
    assert same_bits(tree_totals(r, m), totals.tree_totals(r, m)) and same_bits(tree_totals(r), totals.tree_totals(r))


def test_masked_columns_contribute_the_identity():
    v = np.array([B, 1.0, -B])
    assert tree_totals(v, [1, 0, 1]) == (0.0, -B, B)
    assert tree_totals(v, [0, 1, 0]) == (1.0, 1.0, 1.0)
    assert tree_totals(v, [0, 1, 1]) == (-B, -B, 1.0)
    assert tree_totals(-np.ones(300), np.arange(300) == 299) == (-1.0, -1.0, -1.0)
    s = tree_totals(np.array([-0.0, -0.0]))[0]
    assert s == 0 and not np.signbit(s), "the identity of the sum is +0.0: -0.0 + +0.0 = +0.0"


def test_combine_two_half_domain_files(tmp_path):
    from nc_util import netcdf_file

    from roger_amd import totals

    rng = np.random.default_rng(3)
    nrec, names = 7, ["prec", "S_rz"]
    hdr = np.stack([np.arange(nrec), np.arange(nrec) * 600, np.full(nrec, 600)], axis=1).astype(np.int64)
    hdr[0, 2] = 0
    planes = rng.normal(size=(nrec, len(names), 600))
    halves, paths = [slice(0, 300), slice(300, 600)], []
    masks = [rng.random(300) < 0.7, rng.random(300) < 0.4]
    per_rank = []
    for r, (h, m) in enumerate(zip(halves, masks)):
        values = np.array([[tree_totals(planes[k, j, h], m) for j in range(len(names))] for k in range(nrec)])
        per_rank.append(values)
        paths.append(str(tmp_path / f"run.totals.{r:04d}.nc"))
        totals._write_file(paths[-1], totals._file_variables(hdr, values, names, int(m.sum()), "2018-01-01 00:00:00"), "run")
    out = str(tmp_path / "run.totals.nc")
    totals.combine(paths, out)
    f = netcdf_file(out)
    ncells = int(masks[0].sum() + masks[1].sum())
    assert int(np.reshape(f.variables["ncells"][:], -1)[0]) == ncells
    np.testing.assert_array_equal(f.variables["itt"][:], hdr[:, 0])
    np.testing.assert_array_equal(f.variables["dt"][:], hdr[:, 2])
    np.testing.assert_array_equal(f.variables["Time"][:], hdr[:, 1] / 86400.0)
    for j, v in enumerate(names):
        a, b = per_rank[0][:, j], per_rank[1][:, j]
        assert same_bits(f.variables[f"{v}_sum"][:], a[:, 0] + b[:, 0])
        np.testing.assert_array_equal(f.variables[f"{v}_min"][:], np.minimum(a[:, 1], b[:, 1]))
        np.testing.assert_array_equal(f.variables[f"{v}_max"][:], np.maximum(a[:, 2], b[:, 2]))
        assert same_bits(f.variables[f"{v}_mean"][:], (a[:, 0] + b[:, 0]) / ncells)
        both = np.concatenate(masks)
        np.testing.assert_allclose(f.variables[f"{v}_sum"][:], [math.fsum(planes[k, j][both]) for k in range(nrec)], rtol=0, atol=600 * EPS * 5)
    # files of other steps are refused
    hdr2 = hdr.copy()
    hdr2[3, 0] += 1
    other = str(tmp_path / "other.totals.0001.nc")
    totals._write_file(other, totals._file_variables(hdr2, per_rank[1], names, 5, "2018-01-01 00:00:00"), "run")
    with pytest.raises(ValueError, match="itt of .*other.totals.0001.nc differs"):
        totals.combine([paths[0], other], str(tmp_path / "refused.nc"))
    hdr2 = hdr.copy()
    hdr2[3, 1] += 600
    totals._write_file(other, totals._file_variables(hdr2, per_rank[1], names, 5, "2018-01-01 00:00:00"), "run")
    with pytest.raises(ValueError, match="Time of .*other.totals.0001.nc differs"):
        totals.combine([paths[0], other], str(tmp_path / "refused.nc"))


def test_local_mask_is_the_ranks_block():
    from roger_amd.distributed import proc_rank_to_index
    from roger_amd.totals import local_mask

    field = np.arange(24).reshape(6, 4)
    for r in range(4):
        bx, by = proc_rank_to_index(r, (2, 2))
        np.testing.assert_array_equal(local_mask(field, 6, 4, (2, 2), r), field[bx * 3:(bx + 1) * 3, by * 2:(by + 1) * 2].reshape(-1))
    np.testing.assert_array_equal(local_mask(field, 6, 4, (1, 1), 0), field.reshape(-1))


@pytest.fixture
def totals_backend(monkeypatch, oracle):
    from roger_amd import _native

    made = []

    def make(*a, **k):
        made.append(TotalsOracleContext(*a, **k))
        return made[-1]

    monkeypatch.setattr(_native, "Context", make)
    monkeypatch.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
    return made


VARS = ["theta_rz", "q_ss", "swe", "S_rz", "prec"]
MASK = np.random.default_rng(11).random((4, 4)) < 0.6


def make_model(tmp_path, mask=MASK, variables=VARS, capacity=8, ndays=6, **kw):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays, **kw)

    def set_diagnostics(self, state):
        state.totals.mask = mask
        state.totals.output_variables = list(variables)
        state.totals.base_output_path = str(tmp_path)
        state.totals.capacity = capacity

    type(model).set_diagnostics = roger_routine(set_diagnostics)
    return model, g


@pytest.mark.parametrize("mask", [MASK, None], ids=["masked", "all"])
@pytest.mark.parametrize("script_hooks,by_routine", [(None, False), ("plain", False), ("plain", True)])
def test_script_writes_tree_totals_of_the_doubles_planes(totals_backend, tmp_path, monkeypatch, script_hooks, by_routine, mask):
    """svat_hetero_combo, capacity 8: the ring is drained many times (rounds of device steps; the host loop's step calls) and the
    file holds every step."""
    from nc_util import netcdf_file

    if by_routine:
        monkeypatch.setenv("RH_STEP_BY_ROUTINE", "1")
    assert 0 < MASK.sum() < MASK.size
    model, g = make_model(tmp_path, mask=mask, script_hooks=script_hooks)
    assert tuple(int(v) for v in g["nx_ny"]) == MASK.shape
    model.setup()
    ctx = totals_backend[-1]
    initial = np.array([tree_totals(ctx.download(v), mask) for v in VARS])
    reads = []
    read = ctx.totals_read
    ctx.totals_read = lambda first, n: (reads.append((first, n)), read(first, n))[1]
    model.run()
    trace = ctx.totals_trace
    ncells = MASK.size if mask is None else int(MASK.sum())
    assert len(trace) > 5 * 8 and ctx.totals_count() == (len(trace), ncells)
    assert len(reads) >= len(trace) // 8 and max(n for _, n in reads) <= 8, "the ring was not drained in pieces of at most its capacity"
    f = netcdf_file(str(tmp_path / "GoldenSVAT.totals.nc"))
    t = f.variables["Time"][:]
    assert len(t) == len(trace) + 1 and t[0] == 0 and np.all(np.diff(t) > 0) and t[-1] * 86400 == model.state.settings.runlen
    assert f.variables["Time"].time_origin == b"2018-01-01 00:00:00" and f.variables["dt"].units == b"s"
    np.testing.assert_array_equal(f.variables["dt"][:], [0] + [h[2] for h, _ in trace])
    np.testing.assert_array_equal(f.variables["itt"][:], [0] + [h[0] for h, _ in trace])
    np.testing.assert_array_equal(t[1:], np.array([h[1] for h, _ in trace]) / 86400.0)
    assert f.variables["ncells"].dimensions == () and int(np.reshape(f.variables["ncells"][:], -1)[0]) == ncells
    for j, v in enumerate(VARS):
        for k, stat in enumerate(("sum", "min", "max")):
            a = f.variables[f"{v}_{stat}"][:]
            assert f.variables[f"{v}_{stat}"].dimensions == ("Time",) and a.dtype == np.float64
            assert same_bits(a[0], initial[j, k]), f"{v}_{stat}: record 0 holds the initial values"
            assert same_bits(a[1:], np.array([vals[j, k] for _, vals in trace])), f"{v}_{stat}"
        assert same_bits(f.variables[f"{v}_mean"][:], f.variables[f"{v}_sum"][:] / ncells)
        assert np.any(f.variables[f"{v}_sum"][:] != 0), v
        assert np.all(f.variables[f"{v}_min"][:] <= f.variables[f"{v}_max"][:])
    assert f.variables["theta_rz_sum"].units == b"-" and f.variables["q_ss_max"].units == b"mm/dt"


def test_run_device_called_directly(totals_backend, tmp_path):
    """run_device(n) drains before and after; more steps than the ring holds are refused before anything is enqueued."""
    model, _ = make_model(tmp_path)
    model.setup()
    ctx = totals_backend[-1]
    model.run_device(8)
    model.run_device(5)
    assert ctx.totals_count()[0] == 13 and sum(len(h) for h in model.state.totals._hdr) == 14
    itt = int(model.state.variables.itt)
    with pytest.raises(RuntimeError, match="shorter pieces"):
        model.run_device(9)
    assert int(model.state.variables.itt) == itt == 13 and ctx.totals_count()[0] == 13


def test_validation(totals_backend, tmp_path):
    for kw, exc, text in ((dict(mask=np.ones((4, 5), dtype=bool)), ValueError, r"mask has shape \(4, 5\)"),
                          (dict(mask=np.ones(16, dtype=bool)), ValueError, r"mask has shape \(16,\)"),
                          (dict(mask=np.zeros((4, 4), dtype=bool)), ValueError, "mask holds no column"),
                          (dict(variables=["theta_rz", "lu_id"]), NotImplementedError, "'lu_id' is not a float64"),
                          (dict(variables=["no_such_variable"]), NotImplementedError, "no_such_variable"),
                          (dict(variables=["prec"] * 33), ValueError, "33 variables"),
                          (dict(capacity=0), ValueError, "capacity = 0")):
        model, g = make_model(tmp_path, **kw)
        with pytest.raises(exc, match=text):
            model.setup()
    # nothing asked for: nothing configured, no file
    model, _ = make_model(tmp_path, variables=[], ndays=1)
    model.setup()
    model.run()
    assert totals_backend[-1]._tring is None and not list(tmp_path.iterdir())


def test_offline_transport_is_refused(tmp_path):
    from roger_amd import totals
    from roger_amd.state import RogerState

    st = RogerState()
    with st.settings.unlock():
        st.settings.enable_offline_transport = True
    st.totals.output_variables = ["C_s"]
    with pytest.raises(NotImplementedError, match="offline transport"):
        totals.initialize(st)
