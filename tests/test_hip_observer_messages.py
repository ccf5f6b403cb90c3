"""GPU: the refusals that the observers' host code shares, text for text, and the ring's read across its wrap.

Six rings -- points, catchment totals and zonal totals of the step context (rh_*_read: rh_observers.h) and of the SAS context
(rh_sas_*_read: rh_sas.hip) -- refuse a range with the same two sentences and copy a resident range in at most two pieces; five configure
calls of the step context refuse a plane id with the same two sentences.  The texts below are written out as the C sources spelled them
when every function carried its own copy, so they hold whoever forms them now.

The smallest set-up that wraps: 257 columns (two tiles of 256), a capacity of 3 rows, five rows recorded: rows 2, 3, 4 are resident in
slots 2, 0, 1."""
import ctypes as C

import numpy as np
import pytest

from test_hip_points import make_ctx, same_bits

pytestmark = pytest.mark.gpu

N, CAP, ROWS = 257, 3, 5
PLANES = ("theta", "S_rz")
CELLS = (0, 255, 256)
ZONES = np.arange(N, dtype=np.int32) % 2
RH_ERR_ARG = -1

# what a row is made of, as the size check of every ring names it
LAYOUT = {
    "rh_points": "n_rows x n_planes x n_cells float64",
    "rh_totals": "n_rows x n_planes x 3 float64",
    "rh_zonal": "n_rows x n_zones x n_planes x 3 float64",
    "rh_sas_points": "n_rows x row_elems float64",
    "rh_sas_totals": "n_rows x row_elems float64",
    "rh_sas_zonal": "n_rows x row_elems float64",
}
RINGS = tuple(LAYOUT)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Ring:
    """One ring behind the C ABI: read(first, n, extra_bytes) -> (rc, the context's error text, headers or tags, values)."""

    def __init__(self, ctx, prefix, row_elems):
        self.ctx, self.prefix, self.row_elems = ctx, prefix, row_elems
        self.hdr_elems = 1 if prefix.startswith("rh_sas") else 3
        self.last_error = ctx._lib.rh_sas_last_error if prefix.startswith("rh_sas") else ctx._lib.rh_last_error

    def read(self, first, n, extra_bytes=0):
        hdr = np.full((max(n, 0), self.hdr_elems), -7, dtype=np.int64)
        values = np.full((max(n, 0), self.row_elems), np.nan)
        rc = getattr(self.ctx._lib, self.prefix + "_read")(self.ctx._h, first, n, vp(hdr), vp(values), values.nbytes + extra_bytes)
        return rc, self.last_error(self.ctx._h).decode(), hdr, values


@pytest.fixture(scope="module")
def step_ctx():
    """All six observers of the step context on 257 x 1 SVAT, the three rings with 3 rows, five steps recorded."""
    ctx, _ = make_ctx(N, 1, False)
    ctx.points_configure(CELLS, PLANES, capacity=CAP)
    ctx.totals_configure(PLANES, None, capacity=CAP)
    ctx.zonal_configure(PLANES, ZONES, 2, capacity=CAP)
    ctx.scores_configure(("theta",), kinds=(1,), obs=np.zeros((1, 1, 4)), interval=86400, t_first=0)
    ctx.events_configure(("theta",), kinds=(0,), n_slots=1)
    ctx.run_steps(ROWS)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def sas_ctx():
    """The three rings of a SAS context of 257 cells with 3 rows, five rows recorded, C_rz changed between them."""
    from roger_amd._native import SasContext

    ctx = SasContext(N, 30, forcing_days=1)
    ctx.points_configure(CELLS, ["C_rz"], capacity=CAP)
    ctx.totals_configure(["C_rz"], None, capacity=CAP)
    ctx.zonal_configure(["C_rz"], ZONES, 2, capacity=CAP)
    for k in range(ROWS):
        ctx.upload("C_rz", np.random.default_rng(k).random(N) + k)
        ctx.points_record(tag=100 + k)
        ctx.totals_record(tag=200 + k)
        ctx.zonal_record(tag=300 + k)
    yield ctx
    ctx.close()


@pytest.fixture
def ring(request, step_ctx, sas_ctx):
    prefix = request.param
    if prefix.startswith("rh_sas"):
        elems = C.c_int64()
        assert getattr(sas_ctx._lib, prefix + "_row_elems")(sas_ctx._h, C.byref(elems)) == 0
        return Ring(sas_ctx, prefix, elems.value)
    nv = len(PLANES)
    return Ring(step_ctx, prefix, {"rh_points": nv * len(CELLS), "rh_totals": nv * 3, "rh_zonal": 2 * nv * 3}[prefix])


ring_cases = pytest.mark.parametrize("ring", RINGS, indirect=True)


@ring_cases
def test_rows_that_have_not_been_recorded(ring):
    rc, err, _, _ = ring.read(ROWS, 1)
    assert (rc, err) == (RH_ERR_ARG, f"{ring.prefix}_read: rows 5 ... 5 have not been recorded (5 rows so far)")


@ring_cases
def test_rows_that_have_been_overwritten(ring):
    rc, err, _, _ = ring.read(0, 1)
    assert (rc, err) == (RH_ERR_ARG, f"{ring.prefix}_read: rows 0 ... 1 have been overwritten (the ring holds the last 3 of 5 rows)")


@ring_cases
def test_a_wrong_size_names_the_rows_layout(ring):
    rc, err, _, _ = ring.read(ROWS - CAP, CAP, extra_bytes=8)
    assert (rc, err) == (RH_ERR_ARG, f"{ring.prefix}_read: size mismatch ({LAYOUT[ring.prefix]})")


@ring_cases
def test_a_read_across_the_wrap_equals_its_rows_read_singly(ring):
    rc, err, hdr, values = ring.read(ROWS - CAP, CAP)
    assert rc == 0, err
    assert not np.isnan(values).any() and (hdr != -7).all()
    for k in range(CAP):
        rc, err, h1, v1 = ring.read(ROWS - CAP + k, 1)
        assert rc == 0, err
        assert (h1[0] == hdr[k]).all() and same_bits(v1[0], values[k]), (ring.prefix, k)
    if ring.hdr_elems == 1:
        assert not same_bits(values[0], values[1]) and not same_bits(values[1], values[2]), "the rows do not tell the slots apart"
        assert list(hdr[:, 0]) == [hdr[0, 0] + k for k in range(CAP)] and hdr[0, 0] % 100 == ROWS - CAP
    else:
        assert list(hdr[:, 0]) == [ROWS - CAP + 1 + k for k in range(CAP)]      # itt of the steps 3, 4, 5


@ring_cases
def test_no_rows_at_the_end_are_read(ring):
    rc, err, _, _ = ring.read(ROWS, 0)
    assert rc == 0, err


def configure_with_plane(ctx, who, plane):
    """The configure call `who` of the step context with ONE plane id and otherwise valid arguments -> (rc, error text)."""
    lib, h = ctx._lib, ctx._h
    ids, kinds = (C.c_int * 1)(plane), (C.c_int * 1)(0)
    cells, obs = np.array(CELLS, dtype=np.int64), np.zeros((1, 1, 4))
    rc = {
        "rh_points_configure": lambda: lib.rh_points_configure(h, vp(cells), cells.size, ids, 1, CAP),
        "rh_totals_configure": lambda: lib.rh_totals_configure(h, None, ids, 1, CAP),
        "rh_zonal_configure": lambda: lib.rh_zonal_configure(h, vp(ZONES), 2, ids, 1, CAP),
        "rh_scores_configure": lambda: lib.rh_scores_configure(h, ids, kinds, 1, vp(obs), 1, 4, None, 86400, 0),
        "rh_events_configure": lambda: lib.rh_events_configure(h, ids, kinds, 1, 1),
    }[who]()
    return rc, lib.rh_last_error(h).decode()


# the tail that the scores' and the event outputs' texts carry
TAIL = {"rh_points_configure": "", "rh_totals_configure": "", "rh_zonal_configure": "",
        "rh_scores_configure": " (plane ids must name float64 planes)", "rh_events_configure": " (plane ids must name float64 planes)"}


def assert_still_configured(ctx):
    assert ctx.points_count() == ROWS and ctx.totals_count() == (ROWS, N)
    rows, cells = ctx.zonal_count()
    assert rows == ROWS and list(cells) == [129, 128]
    moments, closed = ctx.scores_read()
    assert moments.shape == (1, 5, N) and closed.shape == (4,)
    assert ctx.events_read()[0].shape == (1, 6)


@pytest.mark.parametrize("bad", ["minus_one", "planes_held"])
@pytest.mark.parametrize("who", list(TAIL))
def test_a_plane_id_the_context_does_not_hold(step_ctx, who, bad):
    plane = -1 if bad == "minus_one" else step_ctx.planes_held
    rc, err = configure_with_plane(step_ctx, who, plane)
    assert (rc, err) == (RH_ERR_ARG, f"{who}: plane id {plane} is not held by this context{TAIL[who]}")
    assert_still_configured(step_ctx)


@pytest.mark.parametrize("who", list(TAIL))
def test_an_int32_plane(step_ctx, who):
    name = next(nm for nm, is_int in step_ctx.planes[: step_ctx.planes_held] if is_int)
    rc, err = configure_with_plane(step_ctx, who, step_ctx.index[name])
    tail = " (plane ids must name float64 planes)" if TAIL[who] else " (float64 planes only)"
    assert (rc, err) == (RH_ERR_ARG, f"{who}: plane {name} is int32{tail}")
    assert_still_configured(step_ctx)
