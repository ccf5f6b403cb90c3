"""GPU: the refusals that the observers' host code shares, text for text, and the ring's read across its wrap.

Six rings -- points, catchment totals and zonal totals of the step context (rh_*_read: rh_observers.h) and of the SAS context
(rh_sas_*_read: rh_sas_observers.h) -- refuse a range with the same two sentences and copy a resident range in at most two pieces; five
configure calls of the step context refuse a plane id with the same two sentences.  The texts below are written out as the C sources
spelled them when every function carried its own copy, so they hold whoever forms them now.

The transport context's part (at the end): the item and window rules that rh_sas_scores_configure, rh_sas_bands_configure and
rh_sas_bands_configure_zonal share, the "has not been called" answer of every call of the five transport observers, and the window clock
that the scores and the bands share, on a context of 5 cells that is never stepped.

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


# ---- the transport context: what rh_sas_scores_configure and the two bands calls share, text for text ----
SAS_N = 5
SAS_C = np.arange(SAS_N, dtype=np.float64) - 7.5
SAS_ZONES = np.array([0, 1, -1, 1, 0], dtype=np.int32)
SAS_WINDOW_CALLS = ("rh_sas_scores_configure", "rh_sas_bands_configure", "rh_sas_bands_configure_zonal")
BULK, MEAN, LAST = 0, 1, 2
RH_ERR_STATE = -3


def small_sas():
    from roger_amd._native import SasContext

    ctx = SasContext(SAS_N, 30, forcing_days=2)
    ctx.upload("C_rz", SAS_C)
    return ctx


def sas_error(ctx, rc):
    return rc, ctx._lib.rh_sas_last_error(ctx._h).decode()


def configure_windows_raw(ctx, who, items, first=(0, 2), last=(0, 3)):
    """The configure call `who` through the C ABI with an int32 item array (value, weight, kind) and otherwise valid arguments
    -> (rc, error text)."""
    lib, h = ctx._lib, ctx._h
    it = np.array(items, dtype=np.int32).reshape(-1, 3)
    first, last = np.array(first, dtype=np.int64), np.array(last, dtype=np.int64)
    probs = np.array([0.0, 0.5, 1.0])
    if who == "rh_sas_scores_configure":
        obs = np.full((len(it), 1, first.size), -6.0)
        return sas_error(ctx, lib.rh_sas_scores_configure(h, vp(it), len(it), None, 1, vp(obs), vp(first), vp(last), first.size))
    if who == "rh_sas_bands_configure":
        return sas_error(ctx, lib.rh_sas_bands_configure(h, vp(it), len(it), vp(probs), probs.size, None, None, None, vp(first), vp(last), first.size))
    return sas_error(ctx, lib.rh_sas_bands_configure_zonal(h, vp(it), len(it), vp(probs), probs.size, vp(SAS_ZONES), 2, None, None, None, vp(first),
                                                           vp(last), first.size))


def configure_windows_valid(ctx, who, items=(("C_rz", None, "last"),), windows=((0, 2), (0, 3))):
    """A valid configuration through the wrapper, and the function that reads it."""
    items, windows = list(items), tuple(np.array(w) for w in windows)
    if who == "rh_sas_scores_configure":
        ctx.scores_configure(items, obs=np.full((len(items), 1, windows[0].size), -6.0), windows=windows)
        return ctx.scores_read
    zonal = who == "rh_sas_bands_configure_zonal"
    ctx.bands_configure(items, probs=(0.0, 0.5, 1.0), windows=windows, zones=SAS_ZONES if zonal else None, n_zones=2 if zonal else None)
    return ctx.bands_read


def same_reading(a, b):
    return len(a) == len(b) and all(same_bits(x, y) if getattr(x, "dtype", None) == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("who", SAS_WINDOW_CALLS)
def test_the_item_and_window_rules_of_the_transport_windows(who):
    """Every shared refusal of the three calls with its whole text and code, the two phrases that differ per caller, which rule speaks
    first for an age-resolved BULK item without a weight; the configuration that was running reads afterwards what it read before."""
    ctx = small_sas()
    read = configure_windows_valid(ctx, who)
    record = ctx.scores_record if who == "rh_sas_scores_configure" else ctx.bands_record
    record(0)
    before = read()
    ix = ctx.index
    scored = who == "rh_sas_scores_configure"
    params_are = "are not scored" if scored else "have no band"
    one_value = "a sample is compared with one value per cell" if scored else "a band is over one value per cell"
    C_rz = ix("C_rz")
    cases = (
        ([(9999, -1, LAST)], {}, RH_ERR_ARG, "unknown array id 9999"),
        ([(C_rz, 9999, BULK)], {}, RH_ERR_ARG, "unknown weight id 9999"),
        ([(C_rz, -1, 3)], {}, RH_ERR_ARG, "kind 3 of array C_rz (0: BULK, 1: MEAN, 2: LAST)"),
        ([(C_rz, -1, LAST), (C_rz, -1, MEAN), (C_rz, -1, LAST)], {}, RH_ERR_ARG, "array C_rz is given twice with the same weight and kind"),
        ([(ix("maskCatch"), -1, MEAN)], {}, RH_ERR_ARG, "array maskCatch is int32 (float64 arrays only)"),
        ([(ix("sas_params_q_ss"), -1, MEAN)], {}, RH_ERR_ARG,
         f"array sas_params_q_ss is a parameter block of the step (sas_params_* {params_are})"),
        ([(ix("q_ss"), -1, MEAN)], {}, RH_ERR_ARG, "array q_ss is a daily input of the step, not a result (daily inputs are weights here)"),
        ([(ix("sa_rz"), -1, MEAN)], {}, RH_ERR_ARG, f"array sa_rz is age-resolved ({one_value})"),
        ([(C_rz, ix("C_in"), BULK)], {}, RH_ERR_ARG, "weight C_in is not a daily flux input (inf_mat_rz ... cpr_rz)"),
        ([(C_rz, -1, BULK)], {}, RH_ERR_ARG, "array C_rz is BULK and has no weight"),
        ([(C_rz, ix("q_ss"), MEAN)], {}, RH_ERR_ARG, "array C_rz is MEAN and has the weight q_ss (only BULK takes one)"),
        ([(ix("tt50_q_ss"), -1, MEAN)], {}, RH_ERR_STATE,
         "array tt50_q_ss is not held by this context (age_statistics / keep_distributions / tracer)"),
        ([(C_rz, -1, LAST)], dict(first=(0, 3), last=(0, 2)), RH_ERR_ARG, "window 1 is [3, 2]: its last day lies before its first"),
        ([(C_rz, -1, LAST)], dict(first=(0, 2), last=(2, 3)), RH_ERR_ARG,
         "window 1 starts on day 2, window 0 ends on day 2 (windows are in increasing order and do not overlap)"),
        # precedence: age-resolved is said before BULK without a weight
        ([(ix("sa_rz"), -1, BULK)], {}, RH_ERR_ARG, f"array sa_rz is age-resolved ({one_value})"),
    )
    for items, windows, code, text in cases:
        assert configure_windows_raw(ctx, who, items, **windows) == (code, f"{who}: {text}"), text
    assert same_reading(read(), before)
    ctx.close()




def sas_observer_calls(ctx):
    """Every _record, _count, _row_elems and _read of the five transport observers, with arguments that ask for no rows and give no bytes:
    [(function, its configure function, call -> rc)]."""
    lib, h = ctx._lib, ctx._h
    i64, buf, byte, cells = C.c_int64(), np.zeros(64), np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int64)
    n, p64 = C.byref(i64), C.cast(vp(cells), C.POINTER(C.c_int64))
    no_rows = (0, 0, vp(cells), vp(buf), 0)
    no_bands = (vp(buf), 0, vp(cells), 0, vp(cells), 0, vp(byte), 0, n)
    P, T, Z, S, B = (f"rh_sas_{o}_configure" for o in ("points", "totals", "zonal", "scores", "bands"))
    return [("rh_sas_points_record", P, lambda: lib.rh_sas_points_record(h, 0)),
            ("rh_sas_points_count", P, lambda: lib.rh_sas_points_count(h, n)),
            ("rh_sas_points_row_elems", P, lambda: lib.rh_sas_points_row_elems(h, n)),
            ("rh_sas_points_read", P, lambda: lib.rh_sas_points_read(h, *no_rows)),
            ("rh_sas_totals_record", T, lambda: lib.rh_sas_totals_record(h, 0, -1)),
            ("rh_sas_totals_count", T, lambda: lib.rh_sas_totals_count(h, n, p64)),
            ("rh_sas_totals_row_elems", T, lambda: lib.rh_sas_totals_row_elems(h, n)),
            ("rh_sas_totals_read", T, lambda: lib.rh_sas_totals_read(h, *no_rows)),
            ("rh_sas_zonal_record", Z, lambda: lib.rh_sas_zonal_record(h, 0, -1)),
            ("rh_sas_zonal_count", Z, lambda: lib.rh_sas_zonal_count(h, n, vp(cells))),
            ("rh_sas_zonal_row_elems", Z, lambda: lib.rh_sas_zonal_row_elems(h, n)),
            ("rh_sas_zonal_read", Z, lambda: lib.rh_sas_zonal_read(h, *no_rows)),
            ("rh_sas_scores_record", S, lambda: lib.rh_sas_scores_record(h, 0)),
            ("rh_sas_scores_read", S, lambda: lib.rh_sas_scores_read(h, vp(buf), 0, vp(byte), 0, n)),
            ("rh_sas_bands_record", B, lambda: lib.rh_sas_bands_record(h, 0)),
            ("rh_sas_bands_read", B, lambda: lib.rh_sas_bands_read(h, *no_bands)),
            ("rh_sas_bands_zonal_read", "rh_sas_bands_configure_zonal", lambda: lib.rh_sas_bands_zonal_read(h, *no_bands))]


def test_the_transport_observers_calls_before_configure_and_after_a_release():
    """`<function>: <configure function> has not been called`, RH_ERR_STATE, from every call of the five observers: on a new context and
    after each observer was configured and released; the zonal read on plain bands, and the plain read's own text on bands per zone."""
    ctx = small_sas()

    def assert_all_off():
        for name, conf, call in sas_observer_calls(ctx):
            assert sas_error(ctx, call()) == (RH_ERR_STATE, f"{name}: {conf} has not been called"), name

    assert_all_off()
    ctx.points_configure([0, 4], ["C_rz"], capacity=2)
    ctx.totals_configure(["C_rz"], None, capacity=2)
    ctx.zonal_configure(["C_rz"], SAS_ZONES, 2, capacity=2)
    configure_windows_valid(ctx, "rh_sas_scores_configure")
    configure_windows_valid(ctx, "rh_sas_bands_configure")
    for name, conf, call in sas_observer_calls(ctx):
        rc, text = sas_error(ctx, call())
        if name == "rh_sas_bands_zonal_read":
            assert (rc, text) == (RH_ERR_STATE, "rh_sas_bands_zonal_read: rh_sas_bands_configure_zonal has not been called")
        else:   # (every observer is on: the call succeeds, or a read says that it got no bytes for its windows)
            assert rc == 0 or (rc == RH_ERR_ARG and text.startswith(f"{name}: size mismatch")), (name, rc, text)
    configure_windows_valid(ctx, "rh_sas_bands_configure_zonal")
    plain_read = dict((name, call) for name, _, call in sas_observer_calls(ctx))["rh_sas_bands_read"]
    assert sas_error(ctx, plain_read()) == (RH_ERR_STATE,
                                            "rh_sas_bands_read: the bands are configured per zone (read them with rh_sas_bands_zonal_read)")
    ctx.points_configure([], [])
    ctx.totals_configure([])
    ctx.zonal_configure([])
    ctx.scores_configure([])
    ctx.bands_configure([])
    assert_all_off()
    ctx.close()


@pytest.mark.parametrize("kind", [LAST, MEAN], ids=["last", "mean"])
def test_the_clock_that_scores_and_bands_share(kind):
    """Nine days over the windows [-1, 1], [2, 2], [3, 4], [6, 7]: window 0 starts before the count and is never open, window 1 is a single
    day, days 5 and 8 lie outside every window.  A LAST item launches on closing days only, a MEAN item on every day of an open window;
    both observers close the windows 1 ... 3, count 9 days and hold what their host restatements hold, bit for bit."""
    import sas_bands_reference as B
    import sas_scores_reference as S

    ctx = small_sas()
    windows = (np.array([-1, 2, 3, 6]), np.array([1, 2, 4, 7]))
    items, probs = [("C_rz", None, kind)], (0.0, 0.5, 1.0)
    obs = np.array([[[-6.0, -5.5, np.nan, -7.5]]])
    ctx.scores_configure(items, obs=obs, windows=windows)
    ctx.bands_configure(items, probs=probs, windows=windows, obs=obs[:, 0])
    want_s = S.HostSasScores(items, obs, windows, SAS_N)
    want_b = B.HostSasBands(items, probs, windows, SAS_N, obs=obs[:, 0])
    for _ in range(9):
        assert ctx._lib.rh_sas_scores_record(ctx._h, 0) == 0 and ctx._lib.rh_sas_bands_record(ctx._h, 0) == 0
        want_s.add({"C_rz": SAS_C})
        want_b.add({"C_rz": SAS_C})
    moments, closed_s, days_s = ctx.scores_read()
    rows, hdr, pairs, closed_b, days_b = ctx.bands_read()
    assert list(closed_s) == [0, 1, 1, 1] and list(closed_b) == [0, 1, 1, 1] and days_s == 9 and days_b == 9
    assert list(want_s.closed) == [0, 1, 1, 1] and list(want_b.closed) == [0, 1, 1, 1]
    assert np.isnan(rows[0]).all() and not hdr[0].any() and (pairs[0] == -1).all()
    assert not np.isnan(rows[1:]).any() and (hdr[1:, 0, 0] == SAS_N).all()
    assert same_bits(rows, want_b.rows) and np.array_equal(hdr, want_b.hdr) and np.array_equal(pairs, want_b.pairs)
    assert same_bits(moments, want_s.moments) and list(moments[0, 2]) == [2.0] * SAS_N   # (the windows 1 and 3 have an observation)
    ctx.close()
