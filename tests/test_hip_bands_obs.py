"""GPU: where the observation falls in the ensemble (rh_bands_observations / rh_bands_obs_read; k_bands_obs, k_bands_obs_row and
k_bands_obs_zonal in roger_amd/csrc/rh_bands.h) against the host restatement (tests/bands_obs_reference.py): every pair exactly, the
rows bit for bit what the same run records without observations, the state planes untouched -- plain, per zone and weighted.

The trajectory, the grids, the crafted-value technique and the stepping paths are those of tests/test_hip_bands.py, test_hip_bands_zonal.py,
test_hip_bands_weighted.py and test_hip_bands_paths.py: the seeded heterogeneous SVAT columns at 257 x 1 and 40 x 25 over 8 days / 150
steps, and values uploaded into the parameter plane theta_irr under a forcing of dry days, where every step closes a daily interval.
Observations are made from the rows the restatement records without them: a recorded quantile (a tie with at least one member), a value
beside one, NaN on some intervals, and a series that ends before the run does."""
import functools

import numpy as np
import pytest

from bands_obs_reference import HostObsBands, HostObsWeightedBands, HostObsZonalBands, inside_of, pair_of
from bands_reference import LAST, quantiles_of
from bands_weighted_reference import target_of, weighted_quantiles_of
from bands_zonal_reference import zonal_quantiles_of
from test_hip_bands import DAY, GRIDS, KINDS, NAMES, PLANE, PROBS, assert_state, dry_ctx
from test_hip_bands_paths import (ROUTED_KINDS, ROUTED_NAMES, ROUTED_WAYS, SELECTIONS, Selection, reference, restated, routed_record, routed_run)
from test_hip_points import NSTEPS, host_hooks, make_ctx

pytestmark = pytest.mark.gpu


class ObsSelection(Selection):
    """tests/test_hip_bands_paths.py's Selection with the restatements that record the pairs; the zonal one loses zone 1 to the mask (the
    zone stays in the list, without a column)."""

    def __init__(self, kind, n):
        super().__init__(kind, n)
        if kind == "zonal":
            self.zone = np.where(self.zone == 1, -1, self.zone).astype(np.int32)

    def host(self, kinds, iv, probs=PROBS):
        if self.kind == "plain":
            return HostObsBands(kinds, probs, self.n, self.mask, iv, 0)
        if self.kind == "zonal":
            return HostObsZonalBands(kinds, probs, self.n, self.zone, 3, iv, 0)
        return HostObsWeightedBands(kinds, probs, self.n, self.w, iv, 0)

    def totals(self, rows):
        """T_tot of every (row, item[, zone]): m, or W with weights."""
        if self.kind == "plain":
            return rows[0][:, 2::2]
        return rows[1][..., 0] if self.kind == "zonal" else rows[2]


def series_from(hdr, values, seed, drop=1):
    """Observations (item[, zone], intervals) from recorded rows -- values (rows, item[, zone], probability): per interval one of the
    recorded quantiles (a tie), for a third of them a value beside it, NaN on a tenth; 1.0 where no column took part; the series ends
    `drop` intervals before the rows do."""
    rng = np.random.default_rng(seed)
    k = hdr[:, 0]
    v = np.moveaxis(values, 0, -2)                      # (item[, zone], row, probability)
    pick = rng.integers(0, v.shape[-1], v.shape[:-1])
    o = np.take_along_axis(v, pick[..., None], -1)[..., 0]
    o = np.where(np.isnan(o), 1.0, o)
    o = np.where(rng.random(o.shape) < 0.33, o * (1.0 + 1e-3 * rng.normal(size=o.shape)), o)
    o[rng.random(o.shape) < 0.1] = np.nan
    length = int(k.max()) + 1 - drop
    obs = np.full(o.shape[:-1] + (length,), np.nan)
    obs[..., k[k < length]] = o[..., k < length]
    return np.ascontiguousarray(obs)


def assert_pairs(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=f"{what}: pairs (row, item[, zone], {{below, equal}})")


def assert_identity(values, totals, pairs, obs_rows, probs, what):
    """The two inequalities against the recorded quantiles, and `inside` against q_lo <= o <= q_hi; obs_rows (row, item[, zone]) the
    observation of every row, NaN: missing.  Returns the number of observed entries."""
    seen = 0
    for at in np.ndindex(pairs.shape[:-1]):
        below, equal = (int(c) for c in pairs[at])
        o, total = obs_rows[at], int(totals[at])
        if o != o:
            assert (below, equal) == (-1, -1), (what, at, below, equal)
            continue
        assert 0 <= below and 0 <= equal and below + equal <= total, (what, at, below, equal, total)
        if total == 0:
            assert (below, equal) == (0, 0), (what, at)
            continue
        seen += 1
        q = values[at]
        for i, p in enumerate(probs):
            T = target_of(p, total)
            assert (q[i] <= o) == (below + equal >= T) and (q[i] < o) == (below >= T), (what, at, p, q[i], o, below, equal, T)
        assert inside_of(below, equal, total, probs[1], probs[-2]) == (q[1] <= o <= q[-2]), (what, at)
    return seen


def obs_rows_of(obs, hdr, first_index=0):
    """The observation of every recorded row: (row, item[, zone])."""
    at = hdr[:, 0] + first_index
    ok = (at >= 0) & (at < obs.shape[-1])
    out = np.full(obs.shape[:-1] + (len(at),), np.nan)
    out[..., ok] = obs[..., at[ok]]
    return np.moveaxis(out, -1, 0)


@functools.lru_cache(maxsize=None)
def rows_without_observations(sel, nx, ny, iv):
    s = ObsSelection(sel, nx * ny)
    ctx, _ = make_ctx(nx, ny, False)
    s.configure(ctx, NAMES, KINDS, iv, NSTEPS)
    ctx.run_steps(NSTEPS)
    rows = s.read(ctx)
    ctx.close()
    return rows


def inside_a_day(ref):
    inside = [k for k in range(20, NSTEPS - 20) if ref.hdr[k - 1, 1] % DAY and ref.hdr[k, 1] % DAY]
    return inside[len(inside) // 2]


# ---- 1. trajectory ----
@pytest.mark.parametrize("iv", [DAY, 3600])
@pytest.mark.parametrize("pieces", [False, True], ids=["one_call", "pieces"])
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_trajectory(sel, nx, ny, pieces, iv):
    """In one call from the start, and in pieces with the observer and the observations configured in the middle of a day."""
    ref = reference(nx, ny, False)
    s = ObsSelection(sel, nx * ny)
    what = f"{sel} {nx} x {ny} iv={iv} pieces={pieces}"
    first = inside_a_day(ref) if pieces else 0
    bare = s.host(KINDS, iv)
    for k in range(first, NSTEPS):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        bare.add(t1 - dt, t1, [ref.planes[v][k] for v in NAMES])
    bare_rows = bare.rows()
    assert (bare.pair_rows() == -1).all() and len(bare_rows[0]) >= 3
    obs = series_from(bare_rows[0], s.values(bare_rows), seed=nx + iv % 7 + len(sel))
    assert obs.shape[:-1] == ((2, 3) if sel == "zonal" else (2,)) and np.isnan(obs).any() and obs.shape[-1] == int(bare_rows[0][-1, 0])
    h = s.host(KINDS, iv)
    h.observe(obs)
    for k in range(first, NSTEPS):
        t1, dt = int(ref.hdr[k, 1]), int(ref.hdr[k, 2])
        h.add(t1 - dt, t1, [ref.planes[v][k] for v in NAMES])
    want, pairs = h.rows(), h.pair_rows()
    assert (pairs[-1] == -1).all(), "the series ends before the run does"
    assert (pairs[..., 1] > 0).any() and (pairs[..., 0] > 0).any() and (sel != "zonal" or np.isin(pairs[:, :, 1], (0, -1)).all())
    ctx, _ = make_ctx(nx, ny, False)
    ctx.run_steps(first)
    s.configure(ctx, NAMES, KINDS, iv, NSTEPS)
    ctx.bands_observations(obs)
    for n in ((1, 2, 37, NSTEPS - first - 40) if pieces else (NSTEPS,)):
        ctx.run_steps(n)
    got = s.read(ctx)
    s.assert_rows(got, want, what)
    if not pieces:
        s.assert_rows(got, rows_without_observations(sel, nx, ny, iv), what + ": against the run without observations")
    got_pairs = ctx.bands_obs_read(0, ctx.bands_count())
    assert_pairs(got_pairs, pairs, what)
    seen = assert_identity(s.values(got), s.totals(got), got_pairs, obs_rows_of(obs, got[0]), PROBS, what)
    assert seen >= len(pairs) // 2, (what, seen)
    assert_state(ctx, ref, what)
    ctx.close()


# ---- 2. crafted values on a parameter plane, under a forcing of dry days ----
def crafted_days(rng, n):
    """(values, observation) per day: ties, both zeros, infinities, NaN columns, the extremes and beyond them, a missing observation."""
    few = rng.choice([-2.5, -0.0, 0.0, 1e-300, 7.0, 7.0, np.inf, -np.inf], n)
    few[:min(n, 8)] = [-2.5, -0.0, 0.0, 1e-300, 7.0, 7.0, np.inf, -np.inf][:min(n, 8)]
    smooth = rng.normal(size=n)
    holes = smooth.copy()
    holes[rng.random(n) < 0.2] = np.nan
    close = (np.float64(1.5).view(np.uint64) + rng.integers(0, 4, n).astype(np.uint64)).view(np.float64)
    return [(few, -0.0), (few, 0.0), (few, 7.0), (few, np.inf), (few, -np.inf), (few, np.nan), (few, -1e-320),
            (smooth, float(smooth.min())), (smooth, float(smooth.max())), (smooth, float(np.nextafter(smooth.min(), -np.inf))),
            (smooth, float(np.nextafter(smooth.max(), np.inf))), (holes, float(np.nanmedian(holes))), (np.full(n, np.nan), 0.5),
            (close, float(close[n // 2])), (close, float(np.nextafter(close.max(), 2.0))), (smooth, 0.0), (smooth, 0.1)]


def crafted_run(ctx, days, configure, read_row, n_series, lead, what):
    """Configure at the clock's day with a series that holds `lead` elements in front (first_index = lead) and ends two days early; step
    the days; every pair against the restatement, and the identity against the row's own quantiles.  n_series: 0, or the zones (every zone reads the same series)."""
    now = int(ctx.get_scalars().time)
    assert now % DAY == 0
    configure(now)
    series = np.concatenate([np.full(lead, 123.0), [o for _, o in days[:-2]]])
    ctx.bands_observations(np.broadcast_to(series, (1, n_series) + series.shape) if n_series else series[None, :], first_index=lead)
    for day, (x, o) in enumerate(days):
        x = np.ascontiguousarray(x, dtype=np.float64)
        ctx.upload(PLANE, x)
        ctx.run_steps(1)
        assert ctx.bands_count() == day + 1, (what, day, "the step did not close a day")
        read_row(day, x, o if day < len(days) - 2 else np.nan)


PROBS_C = (0.0, 0.05, 0.5, 0.95, 1.0)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_crafted_values(n):
    rng = np.random.default_rng(n)
    ctx = dry_ctx(n, ndays=64)
    days = crafted_days(rng, n)
    seen = []

    # plain, under a mask with a hole and (from 128 columns on) a whole empty wavefront
    mask = np.ones(n, dtype=np.uint8)
    mask[5] = 0
    if n >= 128:
        mask[64:128] = 0

    def plain_row(day, x, o):
        hdr, got = ctx.bands_read(day, 1)
        want, m, n_nan = quantiles_of(x[mask != 0], PROBS_C)
        assert hdr[0, 2:].tolist() == [m, n_nan] and (got[0, 0].view(np.uint64) == want.view(np.uint64)).all(), ("plain", n, day)
        pair = ctx.bands_obs_read(day, 1)
        assert pair.shape == (1, 1, 2) and tuple(pair[0, 0]) == pair_of(x[mask != 0], o), ("plain", n, day, o, pair, pair_of(x[mask != 0], o))
        seen.append(assert_identity(got[:, 0], np.array([m]), pair[:, 0], np.array([o]), PROBS_C, ("plain", n, day)))

    crafted_run(ctx, days, lambda now: ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, now, mask, 4), plain_row, 0, 0, "plain")

    # weighted: zero weights on a whole wavefront and, at 257 columns, in a second configuration on the whole first tile
    layouts = [rng.integers(1, 65536, n).astype(np.uint16)]
    layouts[0][[1, 2]] = (65535, 1)
    layouts[0][7] = 0
    if n >= 128:
        layouts[0][64:128] = 0
    if n == 257:
        layouts.append(np.where(np.arange(n) < 256, 0, 7).astype(np.uint16))
    for w in layouts:
        def weighted_row(day, x, o, w=w):
            hdr, got = ctx.bands_read(day, 1)
            want, m, n_nan, W = weighted_quantiles_of(x, w, PROBS_C)
            assert hdr[0, 2:].tolist() == [m, n_nan] and ctx.bands_weight_sums(day, 1).tolist() == [[W]], ("weighted", n, day)
            assert (got[0, 0].view(np.uint64) == want.view(np.uint64)).all(), ("weighted", n, day)
            pair = ctx.bands_obs_read(day, 1)
            assert tuple(pair[0, 0]) == pair_of(x, o, w), ("weighted", n, day, o, pair, pair_of(x, o, w))
            seen.append(assert_identity(got[:, 0], np.array([W]), pair[:, 0], np.array([o]), PROBS_C, ("weighted", n, day)))

        crafted_run(ctx, days, lambda now, w=w: ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, now, None, 4, weights=w), weighted_row,
                    0, 3, "weighted")

    # per zone: three interleaved zones, zone 1 without a column, the same series for every zone
    zone = (np.arange(n) % 3).astype(np.int32)
    zone[zone == 1] = -1
    zone[4] = -1

    def zonal_row(day, x, o):
        hdr, counts, got = ctx.bands_zonal_read(day, 1)
        want, wcounts = zonal_quantiles_of(x, zone, 3, PROBS_C)
        np.testing.assert_array_equal(counts[0, 0], wcounts)
        assert (got[0, 0].view(np.uint64) == want.view(np.uint64)).all(), ("zonal", n, day)
        pair = ctx.bands_obs_read(day, 1)
        assert pair.shape == (1, 1, 3, 2)
        for z in range(3):
            assert tuple(pair[0, 0, z]) == pair_of(x[zone == z], o), ("zonal", n, day, z, o, pair[0, 0, z])
        assert o != o or tuple(pair[0, 0, 1]) == (0, 0)
        seen.append(assert_identity(got[:, 0], counts[:, 0, :, 0], pair[:, 0], np.full((1, 3), o), PROBS_C, ("zonal", n, day)))

    crafted_run(ctx, days, lambda now: ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, now, None, 4, zones=zone, n_zones=3), zonal_row,
                3, 1, "zonal")
    assert sum(seen) >= 3 * (len(days) - 4), seen
    ctx.close()


def test_own_series_per_zone_and_item():
    """Two items, three zones, a series of its own for each: every (item, zone) block reads its own element."""
    n = 257
    rng = np.random.default_rng(6)
    zone = (np.arange(n) % 3).astype(np.int32)
    obs = rng.normal(size=(2, 3, 5))
    obs[1, 2, 1] = obs[0, 0, 3] = np.nan
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE, "sand"], [LAST, LAST], PROBS_C, DAY, 0, None, 8, zones=zone, n_zones=3)
    ctx.bands_observations(obs)
    xs = []
    for day in range(6):
        x = [np.round(rng.normal(size=n) * 4) / 4, np.round(rng.normal(size=n) * 2) / 2]
        obs_day = obs[:, :, day] if day < 5 else np.full((2, 3), np.nan)
        for j in range(2):
            at = int(np.flatnonzero(zone == 1)[day])
            if obs_day[j, 1] == obs_day[j, 1]:
                x[j][at] = obs_day[j, 1]                     # a tie in zone 1
        ctx.upload(PLANE, x[0])
        ctx.upload("sand", x[1])
        xs.append(x)
        ctx.run_steps(1)
    pairs = ctx.bands_obs_read(0, 6)
    assert pairs.shape == (6, 2, 3, 2) and (pairs[5] == -1).all() and (pairs[1, 1, 2] == -1).all() and (pairs[3, 0, 0] == -1).all()
    for day in range(5):
        for j in range(2):
            for z in range(3):
                assert tuple(pairs[day, j, z]) == pair_of(xs[day][j][zone == z], obs[j, z, day]), (day, j, z)
    assert (pairs[:5, :, 1, 1][~np.isnan(obs[:, 1, :].T)] >= 1).all()
    ctx.close()


# ---- 3. the ring ----
def test_ring_wrap_drained_in_between():
    n, cap, ndays = 300, 3, 8
    rng = np.random.default_rng(12)
    w = rng.integers(0, 4, n).astype(np.uint16)
    ctx = dry_ctx(n)
    ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, 0, None, cap, weights=w)
    obs = np.round(rng.normal(size=(1, ndays)) * 2) / 2
    obs[0, 4] = np.nan
    ctx.bands_observations(obs)
    got, want, read = [], [], 0
    for day in range(ndays):
        x = np.round(rng.normal(size=n) * 2) / 2
        ctx.upload(PLANE, x)
        ctx.run_steps(1)
        want.append(pair_of(x, obs[0, day], w))
        if day % 2 or day == ndays - 1:
            total = ctx.bands_count()
            got.append(ctx.bands_obs_read(read, total - read))
            read = total
    got = np.concatenate(got)
    assert_pairs(got, np.array(want, dtype=np.int64).reshape(ndays, 1, 2), "capacity 3, 8 rows")
    assert (got[4] == -1).all() and (got[..., 1] > 0).any()
    from roger_amd._native import NativeError

    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-1\)") as e:
        ctx.bands_obs_read(0, 2)
    assert "have been overwritten" in str(e.value)
    ctx.close()


# ---- 4. ABI ----
def test_refusals_sizes_and_reconfiguration():
    import ctypes as C

    from roger_amd._native import NativeError

    n = 300
    rng = np.random.default_rng(3)
    ctx = dry_ctx(n)
    obs = rng.normal(size=(1, 6))
    with pytest.raises(NativeError, match=r"rh_bands_observations failed \(-3\)") as e:
        ctx.bands_observations(obs)
    assert "rh_bands_configure has not been called" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-3\)") as e:
        ctx.bands_obs_read(0, 0)
    assert "rh_bands_configure has not been called" in str(e.value)
    ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, 0, None, 4)
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-3\)") as e:
        ctx.bands_obs_read(0, 0)
    assert "rh_bands_observations" in str(e.value) and "no observations are set" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_observations failed \(-1\)") as e:
        ctx.bands_observations(rng.normal(size=(1, 2, 6)))
    assert "n_series = 2" in str(e.value) and "without zones: 1 series per item" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_observations failed \(-1\)") as e:
        ctx.bands_observations(obs, first_index=-1)
    assert "first_index = -1" in str(e.value)
    with pytest.raises(ValueError, match="the bands 1 items"):
        ctx.bands_observations(rng.normal(size=(2, 6)))
    x = rng.normal(size=n)
    ctx.upload(PLANE, x)
    ctx.run_steps(1)                                       # a row before the observations: no pair
    ctx.bands_observations(obs)
    ctx.run_steps(1)
    pairs = ctx.bands_obs_read(0, 2)
    assert tuple(pairs[0, 0]) == (-1, -1) and tuple(pairs[1, 0]) == pair_of(x, obs[0, 1])
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-1\)") as e:
        ctx.bands_obs_read(1, 2)
    assert "have not been recorded" in str(e.value)
    buf = np.empty(8, dtype=np.int64)
    for bytes_ in (8, 24, 64):
        with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-1\)") as e:
            ctx._check(ctx._lib.rh_bands_obs_read(ctx._h, 0, 1, buf.ctypes.data_as(C.c_void_p), bytes_), "rh_bands_obs_read")
        assert "size mismatch (n_rows x n_items x n_series x 2 int64)" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-1\)") as e:
        ctx._check(ctx._lib.rh_bands_obs_read(ctx._h, 0, 1, None, 16), "rh_bands_obs_read")
    assert "size mismatch" in str(e.value)
    hdr_before = ctx.bands_read(0, 2)
    # a zonal configuration asks for a series per zone; reconfiguring drops the observations
    zone = (np.arange(n) % 2).astype(np.int32)
    ctx.bands_configure([PLANE], [LAST], PROBS_C, DAY, 0, None, 4, zones=zone, n_zones=2)
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-3\)") as e:
        ctx.bands_obs_read(0, 0)
    assert "no observations are set" in str(e.value)
    with pytest.raises(NativeError, match=r"rh_bands_observations failed \(-1\)") as e:
        ctx.bands_observations(obs)
    assert "n_series = 1" in str(e.value) and "n_zones = 2" in str(e.value)
    ctx.run_steps(1)
    assert ctx.bands_count() == 1
    ctx.bands_observations(np.stack([obs, obs + 1.0], axis=1), first_index=2)
    ctx.run_steps(1)
    k = int(ctx.bands_zonal_read(1, 1)[0][0, 0])
    pairs = ctx.bands_obs_read(0, 2)
    assert (pairs[0] == -1).all()
    for z in range(2):
        o = obs[0, k + 2] + z if k + 2 < 6 else np.nan
        assert tuple(pairs[1, 0, z]) == pair_of(x[zone == z], o), (z, k)
    ctx.bands_observations(None)                           # released: the bands go on, no pair is recorded or read
    ctx.run_steps(1)
    assert ctx.bands_count() == 3
    with pytest.raises(NativeError, match=r"rh_bands_obs_read failed \(-3\)"):
        ctx.bands_obs_read(0, 1)
    ctx.bands_configure(())
    with pytest.raises(NativeError, match=r"rh_bands_observations failed \(-3\)"):
        ctx.bands_observations(obs)
    assert len(hdr_before[0]) == 2
    ctx.close()


# ---- 5. one case per stepping path ----
def observed(s, kinds, iv, bare_rows, seed):
    obs = series_from(bare_rows[0], s.values(bare_rows), seed)
    h = s.host(kinds, iv)
    h.observe(obs)
    return obs, h


def test_lateral_flow_in_pieces():
    nx, ny, iv = 40, 25, 3600
    ref = reference(nx, ny, True)
    s = ObsSelection("weighted", nx * ny)
    obs, h = observed(s, KINDS, iv, restated(s.host(KINDS, iv), ref.hdr, ref.planes, NAMES), 5)
    want, pairs = restated(h, ref.hdr, ref.planes, NAMES), h.pair_rows()
    ctx, _ = make_ctx(nx, ny, True)
    s.configure(ctx, NAMES, KINDS, iv, NSTEPS)
    ctx.bands_observations(obs)
    for n in (1, 2, 37, NSTEPS - 40):
        ctx.run_steps(n)
    assert ctx.sparse_steps() > 0
    s.assert_rows(s.read(ctx), want, "lateral, pieces")
    assert_pairs(ctx.bands_obs_read(0, ctx.bands_count()), pairs, "lateral, pieces")
    assert (pairs[..., 1] > 0).any()
    assert_state(ctx, ref, "lateral, pieces")
    ctx.close()


@pytest.mark.parametrize("sel,path", [("plain", "routines"), ("zonal", "svat_step")])
def test_single_step_entry_points(sel, path):
    """The hooks on the host, a step at a time: first without observations for the series, then the same steps with them."""
    nx, ny, iv = 257, 1, 3600
    s = ObsSelection(sel, nx * ny)
    record = {}
    for observe in (False, True):
        ctx, forcing = make_ctx(nx, ny, False)
        s.configure(ctx, NAMES, KINDS, iv, 64)
        if observe:
            obs, h = observed(s, KINDS, iv, record["rows"], 9)
            ctx.bands_observations(obs)
        else:
            h = s.host(KINDS, iv)
        for _ in range(60):
            monthly = host_hooks(ctx, forcing)
            if path == "routines":
                ctx.call("rh_adaptive_dt")
                if monthly:
                    ctx.call("rh_params_surface")
                ctx.call("rh_step_core")
                ctx.call("rh_after_timestep")
            else:
                ctx.step(monthly)
            sc = ctx.get_scalars()
            h.add(sc.time - sc.dt_secs, sc.time, [ctx.download(v) for v in NAMES])
        record["rows"] = h.rows()
        assert len(record["rows"][0]) >= 3
        s.assert_rows(s.read(ctx), record["rows"], f"{path} observe={observe}")
        if observe:
            pairs = h.pair_rows()
            assert_pairs(ctx.bands_obs_read(0, ctx.bands_count()), pairs, path)
            assert (pairs >= 0).any() and (pairs[-1] == -1).all()
        ctx.close()


@pytest.mark.parametrize("sel,way", list(zip(SELECTIONS, ROUTED_WAYS)))
def test_routed_steps(sel, way, monkeypatch):
    iv = 3600
    rec = routed_record()
    s = ObsSelection(sel, rec.planes["S"].shape[1])
    bare = restated(s.host(ROUTED_KINDS, iv), rec.hdr, rec.planes, ROUTED_NAMES)
    obs, h = observed(s, ROUTED_KINDS, iv, bare, 21)
    want, pairs = restated(h, rec.hdr, rec.planes, ROUTED_NAMES), h.pair_rows()

    def configure(c):
        s.configure(c, ROUTED_NAMES, ROUTED_KINDS, iv, 256)
        c.bands_observations(obs)

    ctx = routed_run(way, configure, monkeypatch)
    s.assert_rows(s.read(ctx), want, f"routing context, {way}")
    assert_pairs(ctx.bands_obs_read(0, ctx.bands_count()), pairs, f"routing context, {way}")
    assert (pairs >= 0).any()
    ctx.close()
