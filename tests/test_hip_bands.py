"""GPU: ensemble bands (rh_bands_*, k_bands and k_bands_select in roger_amd/csrc/rh_bands.h) against the host restatement
(tests/bands_reference.py: np.sort and the rank formula): every value by bits, every integer exactly.

The reference is tests/test_hip_points.py's kind: a context WITHOUT observers that steps one step at a time and downloads the planes and
the clock after every step; the restatement forms the rows from them.  Grids: the seeded heterogeneous SVAT columns at 257 x 1 (one
column in the second tile) and 40 x 25 (several tiles, a ragged last one), over 8 days of the combo forcing: 150 steps of all three step
classes.  Items: q_ss summed (a pure output: the KEEP variant of the sparse kernel runs) and theta_rz at the interval's end.

The crafted-value tests put their values into theta_irr, a float64 PARAMETER plane: the step reads it for the irrigation demand only (a
pure output nothing else reads) and never writes it, so what was uploaded before a step is what the observer sees behind it.  They run
under a forcing without precipitation, where every step is a day and closes a daily interval."""
import functools

import numpy as np
import pytest

from bands_reference import LAST, SUM, HostBands, quantiles_of, rank_of
from test_hip_points import NDAYS, NSTEPS, Reference, make_ctx

pytestmark = pytest.mark.gpu

NAMES, KINDS = ("q_ss", "theta_rz"), (SUM, LAST)
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
DAY = 86400
GRIDS = [(257, 1), (40, 25)]
PLANE = "theta_irr"
SELECT_GRID = 256     # roger_amd/csrc/rh_select.h: RH_SELECT_MAX_GRID, the workgroups that stride over the tiles of 256 keys


def mask_of(n):
    """tests/test_hip_durations.py's mask: a single hole, a whole empty wavefront and, on 40 x 25, a whole empty tile."""
    from test_hip_scores import series_of

    return (series_of(n, "holes")[0] >= 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(nx, ny):
    ref = Reference(nx, ny, False, NAMES, until=NDAYS * DAY, final=True)
    assert len(ref.hdr) == NSTEPS and set(ref.hdr[:, 2]) == {600, 3600, DAY}
    assert np.any(ref.planes["q_ss"] != 0) and np.ptp(ref.planes["theta_rz"][-1]) > 0
    return ref


def expected(ref, iv, mask=None, t_first=0, first=0, nsteps=NSTEPS, probs=PROBS):
    h = HostBands(KINDS, probs, ref.planes[NAMES[0]].shape[1], mask, iv, t_first)
    for k in range(first, nsteps):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in NAMES])
    return h.rows()


def assert_rows(got, want, what):
    (hdr, values), (whdr, wvalues) = got, want
    np.testing.assert_array_equal(hdr, whdr, err_msg=f"{what}: headers {{k, t1, m, n_nan per item}}")
    assert values.shape == wvalues.shape, (what, values.shape, wvalues.shape)
    ok = values.view(np.uint64) == wvalues.view(np.uint64)
    assert ok.all(), (what, "(row, item, probability)", np.argwhere(~ok)[:5], values[~ok][:4], wvalues[~ok][:4])


def read_all(ctx):
    return ctx.bands_read(0, ctx.bands_count())


def assert_state(ctx, ref, what):
    for nm, want in ref.final.items():
        got = ctx.download(nm)
        assert got.dtype == want.dtype and (got.view(np.uint8) == want.view(np.uint8)).all(), (what, nm, "the observer changed a state plane")


# ---- 1. trajectory ----
@pytest.mark.parametrize("iv", [DAY, 3600])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_one_call_against_the_restatement(nx, ny, masked, iv):
    ref = reference(nx, ny)
    mask = mask_of(nx * ny) if masked else None
    want = expected(ref, iv, mask)
    assert len(want[0]) == NDAYS if iv == DAY else NDAYS < len(want[0]) < NDAYS * 24
    m = int(mask.sum()) if masked else nx * ny
    assert (want[0][:, 2::2] == m).all() and (want[0][:, 3::2] == 0).all() and (want[1][:, :, 0] < want[1][:, :, -1]).any()
    ctx, _ = make_ctx(nx, ny, False)
    ctx.bands_configure(NAMES, KINDS, PROBS, iv, 0, mask, NSTEPS)
    assert ctx.bands_count() == 0
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_rows(read_all(ctx), want, f"{nx} x {ny} masked={masked} iv={iv}")
    assert_state(ctx, ref, f"{nx} x {ny} masked={masked} iv={iv}")
    ctx.close()


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_pieces_with_the_observer_configured_in_the_middle_of_a_day(nx, ny):
    """Pieces of 1, 2, ... steps; the configuration comes in the middle of a day: the SUM of the day under way holds what was seen from
    then on, as the duration curves' does."""
    ref = reference(nx, ny)
    inside = [k for k in range(20, NSTEPS - 20) if ref.hdr[k - 1, 1] % DAY and ref.hdr[k, 1] % DAY]
    n1 = inside[len(inside) // 2]
    mask = mask_of(nx * ny)
    ctx, _ = make_ctx(nx, ny, False)
    ctx.run_steps(n1)
    ctx.bands_configure(NAMES, KINDS, PROBS, DAY, 0, mask, NSTEPS)
    for n in (1, 2, 37, NSTEPS - n1 - 40):
        ctx.run_steps(n)
    want = expected(ref, DAY, mask, first=n1)
    assert len(want[0]) == NDAYS - int(ref.hdr[n1, 1]) // DAY and want[0][0, 0] == int(ref.hdr[n1, 1]) // DAY
    assert_rows(read_all(ctx), want, f"{nx} x {ny} configured after {n1} steps, in pieces")
    assert_state(ctx, ref, f"{nx} x {ny} in pieces")
    ctx.close()


# ---- crafted values on a parameter plane, under a forcing of dry days ----
def dry_ctx(n, ndays=40):
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    forcing = combo_forcing(ndays=ndays)
    forcing["PREC"] = np.zeros_like(forcing["PREC"])
    forcing["TA"] = np.full_like(forcing["TA"], 12.0)
    ctx = create_svat(n, 1, params=hetero_params(n, seed=5), lateral=False)
    ctx.set_forcing_series(forcing)
    assert PLANE in ctx.index and PLANE not in ctx.pure_output_planes()
    return ctx


def one_day(ctx, values, probs, mask, what):
    """Upload `values`, step one (dry) day, and compare the row it closed with the restatement."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    rows = ctx.bands_count()
    ctx.upload(PLANE, values)
    ctx.run_steps(1)
    assert ctx.bands_count() == rows + 1, (what, "the step did not close a day")
    back = ctx.download(PLANE)
    assert (back.view(np.uint64) == values.view(np.uint64)).all(), (what, "the step wrote the parameter plane")
    hdr, got = ctx.bands_read(rows, 1)
    on = np.ones(values.size, dtype=bool) if mask is None else np.asarray(mask) != 0
    want, m, n_nan = quantiles_of(values[on], probs)
    assert hdr[0, 2:].tolist() == [m, n_nan], (what, hdr[0].tolist(), m, n_nan)
    assert (got[0, 0].view(np.uint64) == want.view(np.uint64)).all(), (what, got[0, 0], want)
    return want


@pytest.mark.parametrize("n", [1, 255, 256, 257, SELECT_GRID * 256 + 1])
def test_shape_boundaries_of_the_selection(n):
    """One column; a tile less one, a tile, a tile and one; and one column more than the striding grid has threads, so that one workgroup
    strides twice and the last tile holds a single key."""
    rng = np.random.default_rng(n)
    probs = (0.0, 1.0 / n, 0.25, 0.5, 0.75, 1.0 - 1.0 / n, 1.0)
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4)
    for day in range(3):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-4, 5, n)
        x[rng.random(n) < 0.1] = 0.0
        if day == 2:
            x[-1] = -1e300          # the extreme sits in the last, partial tile
        want = one_day(ctx, x, probs, None, f"n = {n}, day {day}")
        assert day != 2 or want[0] == -1e300
    ctx.close()


SELECT_UNROLL = 8     # roger_amd/csrc/rh_select.h: RH_SELECT_U of select_walk_tiles, the tiles a thread holds in flight per trip
SECOND_TRIP = SELECT_GRID * SELECT_UNROLL * 256 + 1


def assert_reaches_the_second_trip(n):
    """Host only: n columns give more tiles than one trip of the whole grid covers, and the last tile holds one key."""
    ntiles = -(-n // 256)
    assert ntiles > SELECT_GRID * SELECT_UNROLL and ntiles - 1 == SELECT_GRID * SELECT_UNROLL and n % 256 == 1, (n, ntiles, SELECT_GRID, SELECT_UNROLL)


def second_trip_columns(n):
    """(the column of tile 2048, a column of tile 256 + 255): workgroup 0's second trip, u = 0; workgroup 255's first trip, u = 1."""
    at = (SELECT_GRID + SELECT_GRID - 1) * 256 + 17
    assert at // 256 == 2 * SELECT_GRID - 1 and (n - 1) // 256 == SELECT_GRID * SELECT_UNROLL
    return n - 1, at


def test_second_trip_of_the_striding_loop():
    """The tile loop of k_bands_select is `for (t = blockIdx.x; t < ntiles; t += gridDim.x * U)` with U = 8 tiles in flight and a grid of
    at most 256 workgroups: one trip of the whole grid covers 256 x 8 = 2048 tiles of 256 keys, so the smallest n at which a workgroup
    makes a second trip is 2048 x 256 + 1 = 524 289 columns.  Tile 2048 then belongs to workgroup 0 on its second trip (u = 0), holds a
    single key, and u = 1 ... 7 of that trip lie beyond the last tile (the `i < n` guard); every other workgroup leaves the loop after one
    trip.  Not a workload size.  Memory: the context holds about 155 planes x 8 B x n = 0.65 GB, the bands one key plane of 4 MB.
    Day 0 puts the minimum into that last column, day 1 into a column of tile 256 + 255 (u = 1 of the first trip)."""
    n = SECOND_TRIP
    assert_reaches_the_second_trip(n)
    rng = np.random.default_rng(n)
    probs = (0.0, 1.0 / n, 0.25, 0.5, 0.75, 1.0 - 1.0 / n, 1.0)
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4)
    for day, at in enumerate(second_trip_columns(n)):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-4, 5, n)
        x[rng.random(n) < 0.1] = 0.0
        x[at] = -1e300
        want = one_day(ctx, x, probs, None, f"n = {n}, day {day}, the minimum in column {at}")
        assert want[0] == want[1] == -1e300 and want[2] > -1e300        # (p = 1 / n is rank 0 too)
    ctx.close()


# ---- the full width: 8 items x 8 probabilities ----
FULL_PLANES = ("theta_irr", "sand", "clay", "theta_6", "theta_27", "theta_4", "rew", "tew")
FULL_PROBS = (0.0, 0.03, 0.25, 0.5, 0.5625, 0.75, 0.97, 1.0)


def full_width_values(rng, n, day):
    """Eight different planes of crafted values for one day.  The first four planes are read by no routine of the step (theta_irr only for
    the irrigation demand, a pure output; sand, clay and theta_6 only by rh_params_soil at the setup), so they take adversarial values:
    both signs, -0.0, ties, infinities, NaN.  theta_27, theta_4, rew and tew are read by the crack depth and the evaporation stress, so
    they keep plausible, ordered ranges (theta_4 < theta_27, rew < tew), with ties."""
    wild = [rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n), np.round(rng.normal(size=n) * 4) / 8 + 0.375, rng.choice([-2.5, -0.0, 0.0, 1e-300, 7.0, np.inf, -np.inf], n),
            (np.float64(1.5).view(np.uint64) + rng.integers(0, 512, n).astype(np.uint64)).view(np.float64) * (-1.0) ** day]
    wild[0][rng.random(n) < 0.05] = np.nan
    tame = [0.12 + np.round(rng.random(n) * 64) / 800, 0.02 + np.round(rng.random(n) * 64) / 800, 2.0 + rng.permutation(n) * (6.0 / n), 10.0 + np.round(rng.random(n) * 200) / 10]
    return [np.ascontiguousarray(v, dtype=np.float64) for v in wild + tame]


def full_width_days(n, n_items, host, configure, seed):
    """Two dry days on a context with the bands (`configure(ctx, names, kinds)`) beside a context WITHOUT observers that gives the planes
    and the clock after every step to the restatement `host(kinds)`; items alternate SUM and LAST, so the second day's SUM rows hold both
    days.  Returns (ctx, the restatement); the caller reads, compares and closes."""
    rng = np.random.default_rng(seed)
    ctx, bare = dry_ctx(n), dry_ctx(n)
    names = FULL_PLANES[:n_items]
    kinds = [(SUM, LAST)[j % 2] for j in range(n_items)]
    for v in names:
        assert v in ctx.index and ctx.index[v] < ctx.planes_held and v not in ctx.pure_output_planes(), v
    configure(ctx, names, kinds)
    h = host(kinds)
    for day in range(2):
        values = full_width_values(rng, n, day)[:n_items]
        for c in (ctx, bare):
            for v, x in zip(names, values):
                c.upload(v, x)
            c.run_steps(1)
        s = bare.get_scalars()
        assert int(s.dt_secs) == DAY
        seen = [bare.download(v) for v in names]
        for v, x, got in zip(names, values, seen):
            assert (got.view(np.uint64) == x.view(np.uint64)).all(), (v, "the step wrote the plane: the crafted values were not what the observer saw")
        h.add(int(s.time) - int(s.dt_secs), int(s.time), seen)
    bare.close()
    return ctx, h


def assert_items_differ(values, what):
    """Host only: the expected rows of the items are pairwise different, so reading item j's prefix or key plane for item j' changes a bit."""
    ni = values.shape[1]
    for j in range(ni):
        for k in range(j + 1, ni):
            assert (values[:, j].view(np.uint64) != values[:, k].view(np.uint64)).any(), (what, "items", j, k, "have equal expected rows")


@pytest.mark.parametrize("n_probs", [1, 8])
@pytest.mark.parametrize("n_items", [1, 8])
def test_items_and_probabilities(n_items, n_probs):
    """1 and 8 items x 1 and 8 probabilities at 600 columns under test_hip_durations.py's mask: 64 (item, probability) pairs over the 4
    wavefronts of the pick, the 64 KiB LDS histogram, the clear loop over every item's bins."""
    n = 600
    probs = (0.5,) if n_probs == 1 else FULL_PROBS
    mask = mask_of(n)
    ctx, h = full_width_days(n, n_items, lambda kinds: HostBands(kinds, probs, n, mask, DAY, 0),
                             lambda c, names, kinds: c.bands_configure(names, kinds, probs, DAY, 0, mask, 4), seed=n_items * 10 + n_probs)
    want = h.rows()
    assert want[1].shape == (2, n_items, n_probs) and (want[0][:, 3] > 0).all(), "no NaN was counted"
    assert_items_differ(want[1], f"{n_items} items x {n_probs} probabilities")
    assert_rows(read_all(ctx), want, f"{n_items} items x {n_probs} probabilities")
    ctx.close()


def middle_probs(m):
    """0, the 1/m steps around the middle, 1."""
    m = max(int(m), 1)
    mid = [min(max(k / m, 0.0), 1.0) for k in (m // 2 - 1, m // 2, m // 2 + 1)]
    return (0.0,) + tuple(mid) + (1.0,)


def test_adversarial_keys():
    n = 300
    rng = np.random.default_rng(11)
    tiny, sub = np.finfo(np.float64).tiny, np.nextafter(0.0, 1.0)
    a = 0.3
    b = np.nextafter(a, 1.0)
    one_on = np.zeros(n, dtype=np.uint8)
    one_on[257] = 1
    last_digit = (np.float64(1.5).view(np.uint64) + rng.integers(0, 512, n).astype(np.uint64)).view(np.float64)   # equal but for the last 9 bits
    assert np.unique(last_digit.view(np.uint64) >> np.uint64(9)).size == 1 and np.unique(last_digit).size > 100
    zeros = np.zeros(n)
    zeros[::3] = -0.0
    specials = rng.choice([np.inf, -np.inf, sub, -sub, tiny / 4, -tiny / 4, tiny, 1.0, -1.0, 0.0], n)
    all_but_one_nan = np.full(n, np.nan)
    all_but_one_nan[131] = -2.5
    neg_nan = np.full(n, -np.nan)            # the sign bit of a NaN does not make it a value
    neg_nan[:10] = np.arange(10.0)
    cases = [("all equal", np.full(n, 0.125), None), ("negatives with positives", rng.normal(size=n), None),
             ("-0.0 among +0.0", zeros, None), ("infinities and subnormals", specials, None),
             ("all but one NaN", all_but_one_nan, None), ("all NaN", np.full(n, np.nan), None), ("NaN of either sign", neg_nan, None),
             ("a mask that leaves one column", rng.normal(size=n), one_on), ("every digit shared but the last", last_digit, None)]
    ctx = dry_ctx(n)
    for what, x, mask in cases:
        on = np.ones(n, dtype=bool) if mask is None else mask != 0
        m = int((~np.isnan(x[on])).sum())
        probs = middle_probs(m)
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, mask, 2)
        want = one_day(ctx, x, probs, mask, what)
        if what == "-0.0 among +0.0":
            assert (want.view(np.uint64) == 0).all()
        if what == "all NaN":
            hdr, got = ctx.bands_read(0, 1)
            assert hdr[0, 2:].tolist() == [0, n] and np.isnan(got).all()
        if what == "all but one NaN":
            assert (want == -2.5).all()
    # two values one unit in the last place apart: for each probability the split that puts the rank on the smaller and on the larger
    probs = (0.0, 0.25, 0.5, 0.75, 1.0)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 8)
    for p in probs[1:-1]:
        r = rank_of(p, n)
        for small in (r, r + 1):                       # `small` columns hold a: rank r is b, then a
            x = np.full(n, b)
            x[rng.permutation(n)[:small]] = a
            want = one_day(ctx, x, probs, None, f"ulp split {small} / {n - small}")
            assert want[probs.index(p)] == (a if small == r + 1 else b)
    ctx.close()


# ---- 4. ring ----
def test_ring_capacity_overwritten_rows_and_release():
    from roger_amd._native import NativeError

    n = 257
    rng = np.random.default_rng(5)
    ctx = dry_ctx(n)
    with pytest.raises(NativeError, match=r"rh_bands_read failed \(-3\)"):
        ctx.bands_read(0, 0)
    with pytest.raises(NativeError, match=r"rh_bands_count failed \(-3\)"):
        ctx.bands_count()
    probs = (0.1, 0.9)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2)
    days = [rng.normal(size=n) for _ in range(7)]
    want = np.array([quantiles_of(x, probs)[0] for x in days])
    got = []
    for k in range(0, 4, 2):                            # capacity 2, drained between calls of two steps
        for x in days[k:k + 2]:
            ctx.upload(PLANE, x)
            ctx.run_steps(1)
        hdr, values = ctx.bands_read(k, 2)
        assert hdr[:, 0].tolist() == [k, k + 1] and hdr[:, 1].tolist() == [(k + 1) * DAY, (k + 2) * DAY]
        got.append(values[:, 0])
    assert (np.concatenate(got).view(np.uint64) == want[:4].view(np.uint64)).all()
    for x in days[4:]:
        ctx.upload(PLANE, x)
        ctx.run_steps(1)
    assert ctx.bands_count() == 7
    with pytest.raises(NativeError, match=r"rh_bands_read failed \(-1\)") as e:
        ctx.bands_read(4, 3)
    assert "have been overwritten" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_read failed \(-1\)") as e:
        ctx.bands_read(6, 2)
    assert "have not been recorded" in str(e.value)
    hdr, values = ctx.bands_read(5, 2)                  # the ring's wrap
    assert (values[:, 0].view(np.uint64) == want[5:].view(np.uint64)).all() and hdr[:, 0].tolist() == [5, 6]
    ctx.bands_configure(())
    ctx.run_steps(2)
    with pytest.raises(NativeError, match=r"rh_bands_read failed \(-3\)"):
        ctx.bands_read(0, 0)
    ctx.close()


def test_refusals_leave_the_configuration_working():
    from roger_amd._native import NativeError
    from test_hip_points import float_planes

    ctx = dry_ctx(6)
    ints = [nm for nm, is_int in ctx.planes[: ctx.planes_held] if is_int]
    not_held = [nm for nm, _ in ctx.planes[ctx.planes_held:]]
    floats = float_planes(ctx)
    ok = dict(names=(PLANE, "q_ss"), kinds=(LAST, SUM), probs=(0.5,), interval=DAY, t_first=0, mask=None, capacity=4)
    ctx.bands_configure(**ok)
    bad = ((dict(names=(ints[0], "q_ss")), f"item 0: plane {ints[0]} is int32"), (dict(names=(PLANE, not_held[0])), f"item 1: plane id {ctx.index[not_held[0]]} "),
           (dict(names=floats[:9], kinds=(LAST,) * 9), "n_items = 9"), (dict(probs=tuple(np.linspace(0, 1, 9))), "n_probs = 9"), (dict(probs=()), "n_probs = 0"),
           (dict(probs=(0.5, 1.5)), "probability 1 = 1.5"), (dict(probs=(-0.25,)), "probability 0 = -0.25"), (dict(probs=(np.nan,)), "probability 0 = "),
           (dict(kinds=(LAST, 2)), "kind 2 of item 1"), (dict(interval=7200, t_first=7200), "interval_seconds = 7200"),
           (dict(t_first=600), "is not a multiple of the interval"), (dict(capacity=0), "capacity = 0"))
    for kw, text in bad:
        with pytest.raises(NativeError, match=r"rh_bands_configure failed \(-1\)") as err:
            ctx.bands_configure(**dict(ok, **kw))
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(ValueError, match="the mask has 5 values"):
        ctx.bands_configure(**dict(ok, mask=np.ones(5)))
    x = np.array([3.0, -1.0, 2.0, np.nan, 0.5, 7.0])
    ctx.upload(PLANE, x)
    ctx.run_steps(1)
    hdr, values = ctx.bands_read(0, 1)
    assert hdr[0, :4].tolist() == [0, DAY, 5, 1] and values[0, 0, 0] == 2.0 and values.shape == (1, 2, 1)
    # eight items and eight probabilities are accepted
    ctx.bands_configure(floats[:8], (LAST,) * 8, tuple(np.linspace(0, 1, 8)), 600, 0, None, 1)
    assert ctx.bands_count() == 0
    ctx.close()


# ---- 5. sparse stores ----
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_an_observed_pure_output_is_kept_by_the_sparse_kernel(nx, ny, monkeypatch):
    """q_ss is a pure output: with the sparse variant on, the KEEP kernel stores it for the observer; the rows equal the run without
    sparse stores (and both the restatement)."""
    want = expected(reference(nx, ny), 3600, None)
    rows = {}
    for sparse in (True, False):
        if not sparse:
            monkeypatch.setenv("RH_NO_SPARSE_STORES", "1")
        ctx, _ = make_ctx(nx, ny, False)
        assert "q_ss" in ctx.pure_output_planes()
        ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, None, NSTEPS)
        ctx.run_steps(NSTEPS)
        assert (ctx.sparse_steps() > 0) == sparse
        rows[sparse] = read_all(ctx)
        ctx.close()
    assert_rows(rows[True], rows[False], f"{nx} x {ny}: sparse against eager")
    assert_rows(rows[True], want, f"{nx} x {ny}: sparse against the restatement")
