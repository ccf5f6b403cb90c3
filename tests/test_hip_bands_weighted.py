"""GPU: likelihood-weighted ensemble bands (rh_bands_configure_weighted; k_bands and k_bands_select_w in roger_amd/csrc/rh_bands.h) against
the host restatement (tests/bands_weighted_reference.py: a stable sort, a cumulative sum of integer weights and the target formula):
every value by bits, every integer -- m, n_nan and the weight sum W -- exactly, the state planes untouched.

The trajectory, the grids and the crafted-value technique are tests/test_hip_bands.py's: the seeded heterogeneous SVAT columns at 257 x 1
and 40 x 25 over the 8 days / 150 steps of tests/test_hip_points.py's reference (shared with that module: computed once), and values
uploaded into the parameter plane theta_irr under a forcing of dry days, where every step closes a daily interval."""
import numpy as np
import pytest

from bands_reference import LAST, SUM
from bands_weighted_reference import HostWeightedBands, target_of, weighted_quantiles_of
from test_hip_bands import DAY, GRIDS, KINDS, NAMES, PLANE, PROBS, assert_rows, assert_state, dry_ctx, mask_of, read_all, reference
from test_hip_points import NDAYS, NSTEPS, make_ctx

pytestmark = pytest.mark.gpu


def weights_of(n, seed=17):
    """Seeded weights over 0 ... 65535, both ends among them, with tests/test_hip_bands.py's holes: a single zero, a whole zero wavefront
    and, on 40 x 25, a whole zero tile."""
    w = np.random.default_rng(seed).integers(0, 65536, n)
    w[:4] = (65535, 1, 65535, 2)
    return (w * mask_of(n)).astype(np.uint16)


def expected(ref, iv, w, first=0, nsteps=NSTEPS, probs=PROBS, t_first=0):
    h = HostWeightedBands(KINDS, probs, w.size, w, iv, t_first)
    for k in range(first, nsteps):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in NAMES])
    return h.rows()


def read_weighted(ctx, first=0):
    n = ctx.bands_count() - first
    return ctx.bands_read(first, n) + (ctx.bands_weight_sums(first, n),)


def assert_weighted_rows(got, want, what):
    assert_rows(got[:2], want[:2], what)
    assert got[2].dtype == np.int64
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: weight sums (row, item)")


# ---- 1. trajectory ----
@pytest.mark.parametrize("iv", [DAY, 3600])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_one_call_against_the_restatement(nx, ny, iv):
    ref = reference(nx, ny)
    w = weights_of(nx * ny)
    holes = mask_of(nx * ny) == 0
    assert holes.any() and (w[~holes] > 0).sum() > nx * ny // 2 and (nx * ny == 257 or holes[256:512].all())
    want = expected(ref, iv, w)
    assert len(want[0]) == NDAYS if iv == DAY else NDAYS < len(want[0]) < NDAYS * 24
    assert (want[0][:, 2::2] == int((w != 0).sum())).all() and (want[2] == int(w.astype(np.int64).sum())).all()
    ctx, _ = make_ctx(nx, ny, False)
    ctx.bands_configure(NAMES, KINDS, PROBS, iv, 0, None, NSTEPS, weights=w)
    assert ctx.bands_count() == 0
    ctx.run_steps(NSTEPS)
    assert ctx.sparse_steps() > 0
    assert_weighted_rows(read_weighted(ctx), want, f"{nx} x {ny} iv={iv}")
    assert_state(ctx, ref, f"{nx} x {ny} iv={iv}")
    ctx.close()


def inside_a_day(ref):
    inside = [k for k in range(20, NSTEPS - 20) if ref.hdr[k - 1, 1] % DAY and ref.hdr[k, 1] % DAY]
    return inside[len(inside) // 2]


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_pieces_with_the_observer_configured_in_the_middle_of_a_day(nx, ny):
    ref = reference(nx, ny)
    n1 = inside_a_day(ref)
    w = weights_of(nx * ny, seed=3)
    ctx, _ = make_ctx(nx, ny, False)
    ctx.run_steps(n1)
    ctx.bands_configure(NAMES, KINDS, PROBS, DAY, 0, None, NSTEPS, weights=w)
    for n in (1, 2, 37, NSTEPS - n1 - 40):
        ctx.run_steps(n)
    want = expected(ref, DAY, w, first=n1)
    assert len(want[0]) == NDAYS - int(ref.hdr[n1, 1]) // DAY
    assert_weighted_rows(read_weighted(ctx), want, f"{nx} x {ny} configured after {n1} steps, in pieces")
    assert_state(ctx, ref, f"{nx} x {ny} in pieces")
    ctx.close()


# ---- 2. weights 0 and 1: the plain configuration under the mask ----
def test_weights_0_and_1_record_the_rows_of_the_plain_configuration_under_the_mask():
    nx, ny = 40, 25
    ref = reference(nx, ny)
    w = mask_of(nx * ny).astype(np.uint16)
    rows = {}
    for weighted in (True, False):
        ctx, _ = make_ctx(nx, ny, False)
        if weighted:
            ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, None, NSTEPS, weights=w)
        else:
            ctx.bands_configure(NAMES, KINDS, PROBS, 3600, 0, w, NSTEPS)
        ctx.run_steps(NSTEPS)
        rows[weighted] = read_weighted(ctx) if weighted else read_all(ctx)
        assert_state(ctx, ref, f"weights 0 / 1, weighted={weighted}")
        ctx.close()
    assert len(rows[False][0]) > NDAYS
    assert_rows(rows[True][:2], rows[False], "weights in {0, 1} against mask = w")
    np.testing.assert_array_equal(rows[True][2], rows[False][0][:, 2::2], err_msg="W == m")


# ---- 3. crafted values on a parameter plane, under a forcing of dry days ----
def one_day(ctx, values, w, probs, what):
    """Upload `values`, step one (dry) day, and compare the row it closed -- header, values, weight sum -- with the restatement."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    rows = ctx.bands_count()
    ctx.upload(PLANE, values)
    ctx.run_steps(1)
    assert ctx.bands_count() == rows + 1, (what, "the step did not close a day")
    back = ctx.download(PLANE)
    assert (back.view(np.uint64) == values.view(np.uint64)).all(), (what, "the step wrote the parameter plane")
    (hdr, got), wsum = ctx.bands_read(rows, 1), ctx.bands_weight_sums(rows, 1)
    want, m, n_nan, W = weighted_quantiles_of(values, w, probs)
    assert hdr[0, 2:].tolist() == [m, n_nan] and wsum.tolist() == [[W]], (what, hdr[0].tolist(), wsum.tolist(), m, n_nan, W)
    assert (got[0, 0].view(np.uint64) == want.view(np.uint64)).all(), (what, got[0, 0], want)
    return want, m, n_nan, W


def dyadic_case(rng, n):
    """Distinct values, weights 1 ... 7 and the largest value's weight chosen so that W is a power of two: p = c / W is then exact for an
    integer c, and so is p * W.  (x, w, cumulative weights in the order of the values, W)."""
    x = rng.permutation(n) * 0.5 - n / 4.0
    w = rng.integers(1, 8, n)
    top = int(np.argmax(x))
    rest = int(w.sum() - w[top])
    W = 1 << rest.bit_length()
    w[top] = W - rest
    assert 1 <= w[top] <= 65535 and int(w.sum()) == W
    return x, w.astype(np.uint16), np.cumsum(w[np.argsort(x)]), W


@pytest.mark.parametrize("n", [257, 1000])
def test_crafted_values(n):
    rng = np.random.default_rng(n)
    ctx = dry_ctx(n)

    def configured(probs, w):
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, weights=w)

    # values that differ in the lowest 9 bits only: the last pass decides
    w = rng.integers(1, 65536, n).astype(np.uint16)
    x = (np.float64(1.5).view(np.uint64) + rng.integers(0, 512, n).astype(np.uint64)).view(np.float64)
    assert np.unique(x.view(np.uint64) >> np.uint64(9)).size == 1 and np.unique(x).size > 100
    probs = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
    configured(probs, w)
    want = one_day(ctx, x, w, probs, "every digit shared but the last")[0]
    assert np.unique(want).size >= 5

    # one column holds more than half of W: the answer for every p above its left cumulative share
    w = rng.integers(1, 40, n).astype(np.uint16)
    x = rng.normal(size=n)
    heavy = int(np.argsort(x)[n // 3])
    w[heavy] = 65535
    left = int(w[x < x[heavy]].astype(np.int64).sum())
    W = int(w.astype(np.int64).sum())
    assert 2 * 65535 > W
    probs = (0.0, left / W * 0.5, (left + 0.5) / W, 0.5, (left + 65535 - 0.5) / W, (left + 65535 + 0.5) / W, 1.0)
    configured(probs, w)
    want = one_day(ctx, x, w, probs, "one heavy column")[0]
    assert (want[2:5] == x[heavy]).all() and want[1] < x[heavy] < want[5]

    # equal values with different weights: three values, the weights of each add up
    x = rng.choice([-1.0, 0.0, 2.5], n)
    x[:3] = (-1.0, 0.0, 2.5)
    x[::7] = np.where(x[::7] == 0.0, -0.0, x[::7])
    w = rng.integers(1, 65536, n).astype(np.uint16)
    shares = np.cumsum([w[x == v].astype(np.int64).sum() for v in (-1.0, 0.0, 2.5)]) / w.astype(np.int64).sum()
    probs = (0.0, shares[0] * 0.999, shares[0] * 1.001, shares[1] * 0.999, shares[1] * 1.001, 1.0)
    configured(probs, w)
    want = one_day(ctx, x, w, probs, "equal values, different weights")[0]
    assert want.tolist() == [-1.0, -1.0, 0.0, 0.0, 2.5, 2.5] and not np.signbit(want[2:4]).any()

    # zero-weight columns hold the extremes and NaN: in neither m nor n_nan; NaN in weighted columns: in n_nan, not in W
    x = rng.normal(size=n)
    w = rng.integers(1, 65536, n).astype(np.uint16)
    out = rng.permutation(n)[:40]
    w[out] = 0
    x[out[:10]], x[out[10:20]], x[out[20:30]] = -np.inf, np.inf, np.nan
    x[out[30:]] = 1e300
    nan_in = np.setdiff1d(np.arange(n), out)[5:17]
    x[nan_in] = np.nan
    probs = (0.0, 0.5, 1.0)
    configured(probs, w)
    want, m, n_nan, W = one_day(ctx, x, w, probs, "zero weights on the extremes; NaN in weighted columns")
    assert (m, n_nan) == (n - 40 - 12, 12) and np.isfinite(want).all() and abs(want).max() < 10
    assert W == int(w.astype(np.int64).sum()) - int(w[nan_in].astype(np.int64).sum())

    # ceil(p W) lands exactly on a cumulative boundary, and one above it
    x, w, cw, W = dyadic_case(rng, n)
    b = n // 2
    probs = (0.0, float(cw[b]) / W, float(cw[b] + 1) / W, float(cw[0]) / W, float(cw[0] + 1) / W, 1.0)
    assert all(p * W == round(p * W) for p in probs)
    configured(probs, w)
    want = one_day(ctx, x, w, probs, "on a cumulative boundary and one above")[0]
    xs = np.sort(x)
    assert want.tolist() == [xs[0], xs[b], xs[b + 1], xs[0], xs[1], xs[-1]]

    # m == 0: every weighted column holds a NaN
    x = np.where(rng.random(n) < 0.5, 1.0, 2.0)
    w = np.zeros(n, dtype=np.uint16)
    w[[3, 64, n - 1]] = (5, 65535, 1)
    x[[3, 64, n - 1]] = np.nan
    configured(probs, w)
    want, m, n_nan, W = one_day(ctx, x, w, probs, "m == 0")
    assert (m, n_nan, W) == (0, 3, 0) and np.isnan(want).all()
    hdr, got = ctx.bands_read(0, 1)
    assert np.isnan(got).all() and hdr[0].tolist() == [hdr[0, 0], hdr[0, 1], 0, 3]
    ctx.close()


def prob_of_target(T, W):
    """A probability whose target ceil(p * W), by target_of's own arithmetic, is exactly T (1 <= T <= W)."""
    p = float(T) / float(W)
    while target_of(p, W) > T:
        p = float(np.nextafter(p, 0.0))
    assert target_of(p, W) == T, (T, W, p)
    return p


def test_second_trip_of_the_striding_loop():
    """tests/test_hip_bands.py's second-trip case for k_bands_select_w: n = 2048 x 256 + 1 = 524 289 columns is the smallest n at which a
    workgroup of the 256 (bands_weighted_grid gives 256 here: 2049 tiles need only 9 workgroups for the LDS bound) walks a second trip
    of 8 tiles; tile 2048 is workgroup 0's, holds a single key, and the seven tiles behind it lie beyond n.  Workgroup 0 sums nine tiles
    into its uint32 LDS bins.  Not a workload size; the context holds about 155 planes x 8 B x n = 0.65 GB, the bands a key plane of 4 MB
    and a weight plane of 1 MB.
    The last column has weight 65535, so it alone moves the cumulative weight across 65535 targets: with `before` the weight of the
    columns below it, the targets before + 1 and before + 65535 give its value, before and before + 65536 its neighbours'.  Day 0 puts
    the minimum there (before = 0), day 1 into a column of tile 256 + 255 (u = 1 of the first trip) with the last column's value
    somewhere in the middle."""
    from test_hip_bands import SECOND_TRIP, assert_reaches_the_second_trip, second_trip_columns

    n = SECOND_TRIP
    assert_reaches_the_second_trip(n)
    rng = np.random.default_rng(n)
    last, at = second_trip_columns(n)
    w = rng.integers(0, 65536, n)
    w[last], w[at] = 65535, 1
    w = w.astype(np.uint16)
    ctx = dry_ctx(n)
    for day in range(2):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-4, 5, n)
        x[at if day else last] = -1e300
        assert np.unique(x).size == n
        on = (w != 0) & (x < x[last])
        before, W = int(w[on].astype(np.int64).sum()), int(w.astype(np.int64).sum())
        below = x[on].max() if day else None
        above = x[(w != 0) & (x > x[last])].min()
        assert (before == 0) == (day == 0) and before + 65536 <= W
        probs = (0.0, prob_of_target(max(before, 1), W), prob_of_target(before + 1, W), prob_of_target(before + 65535, W), prob_of_target(before + 65536, W), 1.0)
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 2, weights=w)
        want, m, n_nan, Wd = one_day(ctx, x, w, probs, f"n = {n}, day {day}")
        assert (m, n_nan, Wd) == (int((w != 0).sum()), 0, W) and want[0] == -1e300
        assert want[1] == (below if day else x[last]) and want[2] == want[3] == x[last] and want[4] == above
    ctx.close()


@pytest.mark.parametrize("n_probs", [1, 8])
@pytest.mark.parametrize("n_items", [1, 8])
def test_items_and_probabilities(n_items, n_probs):
    """tests/test_hip_bands.py's full width for the weighted selection: 1 and 8 items x 1 and 8 probabilities at 600 columns, eight
    planes of different crafted values, SUM and LAST items over two dry days; header, values and weight sums against the restatement."""
    from test_hip_bands import FULL_PROBS, assert_items_differ, full_width_days

    n = 600
    probs = (0.5,) if n_probs == 1 else FULL_PROBS
    w = weights_of(n, seed=n_items + n_probs)
    ctx, h = full_width_days(n, n_items, lambda kinds: HostWeightedBands(kinds, probs, n, w, DAY, 0),
                             lambda c, names, kinds: c.bands_configure(names, kinds, probs, DAY, 0, None, 4, weights=w), seed=100 + n_items * 10 + n_probs)
    want = h.rows()
    assert want[1].shape == (2, n_items, n_probs) and want[2].shape == (2, n_items) and (want[0][:, 3] > 0).all(), "no NaN was counted"
    assert_items_differ(want[1], f"{n_items} items x {n_probs} probabilities, weighted")
    assert_weighted_rows(read_weighted(ctx), want, f"{n_items} items x {n_probs} probabilities, weighted")
    ctx.close()


# ---- 4. 64-bit sums ----
def test_a_bin_and_the_weight_sum_beyond_2_to_the_32():
    """70 000 columns of weight 65535 and two distinct values, 66 000 of the one: that value's digit bin holds 66 000 x 65535 > 2^32 in every
    pass (65 538 columns is the smallest number at which a 32-bit global counter goes wrong), and W = 70 000 x 65535 > 2^32."""
    n, many = 70000, 66000
    w = np.full(n, 65535, dtype=np.uint16)
    assert many * 65535 > 2 ** 32 and (many * 65535) % 2 ** 32 < (n - many) * 65535
    probs = (0.0, 0.5, 0.94, 0.95, 1.0)                   # many / n = 0.9428...
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=w)
    rng = np.random.default_rng(4)
    for a, b in ((0.25, 0.375), (0.375, 0.25)):        # the heavy value below, then above
        x = np.full(n, b)
        x[rng.permutation(n)[:many]] = a
        want, m, n_nan, W = one_day(ctx, x, w, probs, f"66 000 x {a}, 4 000 x {b}")
        assert (m, n_nan, W) == (n, 0, n * 65535) and W > 2 ** 32
        assert want.tolist() == ([a, a, a, b, b] if a < b else [b, a, a, a, a])
    ctx.close()


# ---- 5. ABI ----
def test_configurations_replace_each_other_and_refusals_leave_the_last_one_counting():
    from roger_amd._native import NativeError

    n = 300
    rng = np.random.default_rng(8)
    probs = (0.1, 0.5, 0.9)
    w = rng.integers(0, 65536, n).astype(np.uint16)
    w[::5] = 0
    ctx = dry_ctx(n)
    with pytest.raises(NativeError, match=r"rh_bands_weight_sums failed \(-3\)") as e:
        ctx.bands_weight_sums(0, 0)
    assert "rh_bands_configure_weighted has not been called" in str(e.value)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, w != 0, 4)                   # plain
    with pytest.raises(NativeError, match=r"rh_bands_weight_sums failed \(-3\)") as e:
        ctx.bands_weight_sums(0, 0)
    assert "configured without weights" in str(e.value) and "rh_bands_configure_weighted" in str(e.value)
    from test_hip_bands import one_day as plain_day

    plain_day(ctx, rng.normal(size=n), probs, w != 0, "plain, before")
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=w)          # weighted behind plain: a new series
    assert ctx.bands_count() == 0
    with pytest.raises(NativeError, match=r"rh_bands_zonal_read failed \(-3\)") as e:
        ctx.bands_zonal_read(0, 0)
    assert "configured with weights" in str(e.value) and "rh_bands_weight_sums" in str(e.value)
    one_day(ctx, rng.normal(size=n), w, probs, "weighted behind plain")
    # refused weighted calls: the configuration above keeps counting, and the binding keeps its shape
    for kw, text in ((dict(weights=np.zeros(n, dtype=np.uint16)), "no participating column (every weight is 0)"),
                     (dict(probs=(0.5, 1.5)), "probability 1 = 1.5"), (dict(capacity=0), "capacity = 0"), (dict(interval=7200), "interval_seconds = 7200")):
        args = dict(names=[PLANE, "q_ss"], kinds=[LAST, SUM], probs=(0.5,), interval=DAY, t_first=0, mask=None, capacity=4, weights=w)
        with pytest.raises(NativeError, match=r"rh_bands_configure_weighted failed \(-1\)") as e:
            ctx.bands_configure(**dict(args, **kw))
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="the weights have 299 values"):
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=w[:-1])
    with pytest.raises(ValueError, match="integers 0 ... 65535"):
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=np.full(n, 65536))
    with pytest.raises(ValueError, match="weights with zones is not built"):
        ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=w, zones=np.zeros(n, dtype=np.int32))
    one_day(ctx, rng.normal(size=n), w, probs, "after the refusals")
    assert ctx.bands_count() == 2 and ctx.bands_weight_sums(0, 2).shape == (2, 1)
    with pytest.raises(NativeError, match=r"rh_bands_weight_sums failed \(-1\)") as e:
        ctx.bands_weight_sums(1, 2)
    assert "have not been recorded" in str(e.value)
    # a mask on top is folded into the weights
    mask = rng.random(n) < 0.5
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, mask, 4, weights=w)
    one_day(ctx, rng.normal(size=n), np.where(mask, w, 0).astype(np.uint16), probs, "a mask folded in")
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, w != 0, 4)                   # and back to plain
    plain_day(ctx, rng.normal(size=n), probs, w != 0, "plain, behind weighted")
    with pytest.raises(NativeError, match=r"rh_bands_weight_sums failed \(-3\)"):
        ctx.bands_weight_sums(0, 1)
    ctx.bands_configure([PLANE], [LAST], probs, DAY, 0, None, 4, weights=w)
    ctx.bands_configure(())                                                          # release
    ctx.run_steps(2)
    for call in (lambda: ctx.bands_count(), lambda: ctx.bands_read(0, 0), lambda: ctx.bands_weight_sums(0, 0)):
        with pytest.raises(NativeError, match=r"failed \(-3\)"):
            call()
    ctx.close()


def test_state_and_restore_carry_a_weighted_run_through_the_middle_of_a_day():
    nx, ny = 257, 1
    ref = reference(nx, ny)
    n1 = inside_a_day(ref)
    w = weights_of(nx * ny, seed=29)
    want = expected(ref, DAY, w)
    ctx, _ = make_ctx(nx, ny, False)
    ctx.bands_configure(NAMES, KINDS, PROBS, DAY, 0, None, NSTEPS, weights=w)
    ctx.run_steps(n1)
    rows = ctx.bands_count()
    before, acc = read_weighted(ctx), ctx.bands_state()
    ctx.close()
    assert 0 < rows < NDAYS and acc.shape == (2, nx * ny) and not np.any(acc[:, w == 0])
    ctx, _ = make_ctx(nx, ny, False)                       # the continued run: the model's state by stepping, the observer's by restore
    ctx.run_steps(n1)
    ctx.bands_configure(NAMES, KINDS, PROBS, DAY, 0, None, NSTEPS, weights=w)
    ctx.bands_restore(acc, rows)
    assert ctx.bands_count() == rows
    ctx.run_steps(NSTEPS - n1)
    after = read_weighted(ctx, first=rows)
    assert_weighted_rows(tuple(np.concatenate([a, b]) for a, b in zip(before, after)), want, "rows before the restart followed by the rows behind it")
    assert_state(ctx, ref, "continued")
    ctx.close()
