// rh_bands.h -- ensemble bands (rh_bands_configure): after every step a variable is aggregated to an interval per column, and at every
// interval's end the exact quantiles ACROSS the columns -- the 5 % / 50 % / 95 % prediction band of a parameter study -- go into one row
// of a ring on the device.  A selection, not a reduction: integer counters over bit patterns, so a row is np.sort(...)[r] bit for bit.
// Part of the one translation unit roger_hip.hip, behind rh_durations.h.
//
// The clock is k_durations' (uniform over the grid, from D->S): t1 = S.time, t0 = t1 - S.dt_secs, iv the interval in seconds (86400, 3600
// or 600);
//   first   = t0 % iv == 0
//   closes  = t1 % iv == 0 && t1 - t0 <= iv     (a step longer than the interval never closes one)
//   k       = t1 / iv - 1 - t_first / iv
//   counted = closes && k >= 0                  (no upper bound on k)
// after_fused && D->skipped ends every launch as for every other observer.
//
// Items.  At most 8 float64 planes, each SUM or LAST; column i with mask[i] == 0 (a mask is optional) loads and stores nothing.  v the
// plane's value after the step:
//   SUM:   acc = first ? v : acc + v on every step (k_durations' rule, the same order of additions)
//   LAST:  nothing on a step that is not counted
// Interval value.  On a counted step s = (SUM ? acc : v) + 0.0 -- the addition turns -0.0 into +0.0, so equal zeros have one bit pattern
// and the result has no freedom left.  A NaN s is counted in n_nan and takes no further part; +-inf are ordinary values.  m is the
// number of masked-in columns whose s is not a NaN.
// Probabilities.  At most 8 probabilities p in [0, 1], shared by the items.  r = clamp((int64)ceil(p * (double)m) - 1, 0, m - 1) -- one
// double multiplication and one ceil, the same on host and device -- and the result is the r-th smallest s (from 0): np.sort(s)[r],
// the "inverted CDF" quantile; p = 0 is the minimum, p = 1 the maximum.  With m == 0 the row holds NaN.
// Ring.  One row per counted interval, row q at q mod bands_cap (the one ring rule of rh_observers.h): header int64 {k, t1} and per item
// {m, n_nan}; values (item, probability) float64.
//
// Keys.  k_bands (a workgroup per RH_BLOCK columns, after every step) does the SUM accumulation -- 24 B per SUM item and column; it ends
// after the scalar loads when the step is not counted and there is no SUM item -- and on a counted step stores the order-preserving
// key of s into the item's key plane: u = bits(s), key = u ^ (u >> 63 ? ~0 : 1 << 63); unsigned comparison of keys is < on the values.
// Validity is part of the key plane, not a plane of its own: a NaN s stores RH_SELECT_KEY_NAN (~0 - 1), and a masked-out column keeps
// RH_SELECT_KEY_MASKED (~0), which the configuration wrote once.  Both are the keys of NaN bit patterns, so no value's key equals them
// (the largest value's key, +inf's, is 0xfff0000000000000); the selection skips every key >= RH_SELECT_KEY_NAN and counts the first.
//
// Selection.  A radix selection on the keys, most significant digit first, for all (item, probability) pairs at once, in
// RH_SELECT_PASSES launches of k_bands_select<P> behind k_bands.  The host cannot know whether a step closes an interval (dt is the
// device's), so the launches follow every step and end after the scalar loads on a step that is not counted.
//   digits     11 bits: six passes over 11, 11, 11, 11, 11 and 9 bits.  8 bits would need eight passes.  A launch-bound grid (80 x 53
//              columns, 21 us per step) pays per launch, a large grid per pass over the keys (8 B per column): both favour fewer
//              passes, and 8 KiB of LDS per pair is there to be had -- a workgroup holds the 8 probabilities of ONE item (64 KiB) and
//              takes the items one after the other, each from its own key plane.
//   histogram  a workgroup strides over the tiles of RH_BLOCK keys (eight tiles in flight per thread) and counts the digit of every key
//              whose higher digits equal the pair's prefix into an LDS histogram (uint32, LDS atomics).  In pass 0 all probabilities
//              of an item share one histogram: there is no prefix yet.
//   merge      the workgroup adds its NON-ZERO bins to the global histogram bands_hist [item][probability][2048] with integer atomic
//              adds at device scope.  Integer adds commute: the sum does not depend on their order.  This is the one place where the
//              project's "no atomics" habit, which is about floating-point sums, does not apply.  Device-scope atomics on one cache
//              line are served one after the other (~ 25 ns each), so the grid is at most RH_SELECT_MAX_GRID
//              workgroups (one per CU) however many tiles there are, and after pass 0 nearly every bin is empty.
//   pick       the work of the workgroup that finishes last (k_step's tail pattern, one counter: the grid is small).  Its invariant
//              is kept: a thread's adds are RETURNING atomics whose results feed an LDS add in front of the workgroup's barrier, and
//              only behind that barrier does thread 0 count the workgroup done (a returning device-scope add on bands_done); the
//              last workgroup reads the histograms with device-scope loads.  A wavefront per pair scans the bins -- 64 at a time, all
//              loads requested first -- for the digit at which the cumulative count passes the remaining rank, appends it to the
//              pair's prefix and subtracts the count below it from the rank (bands_prefix, bands_rank: device memory, read by the
//              next launch).  Pass 0 also fixes m (the histogram's total), n_nan and r.  Then the workgroup clears the histograms
//              and the counter with device-scope stores.
//   row        after the last pass the prefix IS the key: inverted (key >> 63 ? key ^ 1 << 63 : ~key) it is the value.  Thread 0 writes
//              the header and advances bands_rows last.
// Cost.  A step that is not counted: as k_durations' (24 B per SUM item and column), and six launches that end after the scalar loads.
// A counted step: k_bands' 8 B store per item and column, and six passes x 8 B per item and column of key reads.
//
// Per zone (rh_bands_configure_zonal): the same rule for every zone of a zone map in one run -- block z of a row is, bit for bit, the row
// above under mask = (zone == z) -- selected by one workgroup per (zone, item) in its own LDS: k_bands_zonal at the end of this file.
//
// Likelihood-weighted (rh_bands_configure_weighted): the GLUE band -- column i counts as w_i identical members.  k_bands runs unchanged
// and k_bands_select_w<P> takes the place of the six k_bands_select<P>: behind k_bands_zonal in this file, the rule with it.
//
// Observations (rh_bands_observations): does the band contain the measurement?  Per counted interval, item (and zone) the int64 pair
// (below, equal) -- the members, or their weights, below and equal to the observation -- counted from the key planes in one more pass
// behind the selection: k_bands_obs, k_bands_obs_row and k_bands_obs_zonal at the end of this file, the rule with them.
#pragma once
#include "rh_select.h"   // the selection's pieces shared with rh_sas_bands.h: keys, passes, grids, the walks, the count, the pick, the pair

#define RH_BANDS_MAX_ITEMS 8
#define RH_BANDS_MAX_PROBS 8
#define RH_BANDS_SUM 0
#define RH_BANDS_LAST 1
#define RH_BANDS_MAX_ZONES 1024   // rh_bands_configure_zonal: a workgroup of k_bands_zonal per zone and item
static_assert(RH_BLOCK == RH_SELECT_BLOCK && RH_BANDS_MAX_PROBS == RH_SELECT_MAX_PROBS, "rh_select.h states the tile and the histograms of the selection");

struct BandsClock {
    bool first, counted;
    long long k, t1;
};
RH_DEV BandsClock bands_clock(const DevState *D) {
    const int64_t t1 = D->S.time, t0 = t1 - D->S.dt_secs, iv = D->bands_interval;
    BandsClock c;
    c.first = (t0 % iv) == 0;
    c.k = t1 / iv - 1 - D->bands_t_first / iv;
    c.counted = (t1 % iv) == 0 && t1 - t0 <= iv && c.k >= 0;
    c.t1 = t1;
    return c;
}

__global__ __launch_bounds__(RH_BLOCK) void k_bands(Arena a, DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted && !D->bands_nsum) return;   // (uniform over the grid)
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const unsigned char *mask = D->bands_mask;
    if (mask && !mask[i]) return;
    const size_t n = (size_t)a.n;
    const int ni = D->bands_nitems;
    for (int j = 0; j < ni; ++j) {
        const bool sum = D->bands_kinds[j] == RH_BANDS_SUM;
        if (!sum && !c.counted) continue;   // LAST: only the value at a counted interval's end
        double v;
        rh_ld(a, D->bands_planes[j], i, v);
        double s = v;
        if (sum) {
            double *p = D->bands_acc + (size_t)j * n + i;
            if (!c.first) s = *p + v;
            *p = s;
        }
        if (!c.counted) continue;
        s = s + 0.0;
        D->bands_keys[(size_t)j * n + i] = s != s ? RH_SELECT_KEY_NAN : bands_key_of(s);
    }
}

// The walk over the tiles, the digit count of a key and the pick step of a wavefront are rh_select.h's (select_walk_tiles, select_count,
// select_pick_step); the kernel is the shell around them: the clock, the merge, the completion pattern and the row.
template <int P>
__global__ __launch_bounds__(RH_BLOCK) void k_bands_select(Arena a, DevState *D, int after_fused) {
    constexpr int NB = BandsPass<P>::nb, NC = NB / 64;
    __shared__ unsigned hist[RH_BANDS_MAX_PROBS * RH_SELECT_NBINS];
    __shared__ unsigned nan_count, posted, is_last;
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;   // (uniform over the grid)
    const int ni = D->bands_nitems, np = D->bands_nprobs, nh = P == 0 ? 1 : np;
    const int64_t n = a.n;
    unsigned dep = 0;
    if (threadIdx.x == 0) posted = 0;
    for (int j = 0; j < ni; ++j) {
        for (int b = threadIdx.x; b < nh * NB; b += RH_BLOCK) hist[b] = 0;
        if (threadIdx.x == 0) nan_count = 0;
        __syncthreads();
        unsigned long long pre[RH_BANDS_MAX_PROBS];
#pragma unroll
        for (int q = 0; q < RH_BANDS_MAX_PROBS; ++q) pre[q] = (P > 0 && q < np) ? D->bands_prefix[j * RH_BANDS_MAX_PROBS + q] : 0ull;
        const unsigned long long *keys = D->bands_keys + (size_t)j * (size_t)n;
        unsigned mine = 0, mine_nan = 0;   // pass 0: the NaNs this thread met (the numbers are the histogram's total)
        select_walk_tiles<false>(keys, nullptr, n, [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<P>(key, w, np, pre, hist, mine, mine_nan); });
        if (P == 0 && mine_nan) atomicAdd(&nan_count, mine_nan);
        __syncthreads();
        unsigned *g = D->bands_hist + (size_t)j * RH_BANDS_MAX_PROBS * RH_SELECT_NBINS;
        for (int b = threadIdx.x; b < nh * NB; b += RH_BLOCK) {
            const unsigned cnt = hist[b];
            if (cnt) dep |= __hip_atomic_fetch_add(g + (b / NB) * RH_SELECT_NBINS + (b % NB), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 31;
        }
        if (P == 0 && threadIdx.x == 0 && nan_count)
            dep |= __hip_atomic_fetch_add(&D->bands_nan_count[j], nan_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 31;
        __syncthreads();   // (the next item clears the histogram)
    }
    // Completion: every thread's adds have returned before its LDS add (dep is 0: a count stays below 2^31), the barrier follows, and only
    // then is the workgroup counted done.
    atomicAdd(&posted, dep);
    __syncthreads();
    if (threadIdx.x == 0)
        is_last = __hip_atomic_fetch_add(&D->bands_done, 1u + posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!is_last) return;

    const int lane = threadIdx.x & 63;
    const long long row = D->bands_rows;
    const long long slot = row % D->bands_cap;
    for (int pair = threadIdx.x >> 6; pair < ni * np; pair += RH_BLOCK / 64) {   // (uniform over the wavefront)
        const int j = pair / np, q = pair - j * np, at = j * RH_BANDS_MAX_PROBS + q;
        const unsigned *h = D->bands_hist + (size_t)(j * RH_BANDS_MAX_PROBS + (P == 0 ? 0 : q)) * RH_SELECT_NBINS;
        unsigned v[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = __hip_atomic_load(h + k * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const SelectPick pk = select_pick_step<P>(v, D->bands_probs[q], &D->bands_prefix[at], &D->bands_rank[at]);
        const unsigned long long prefix = pk.prefix;
        const long long m = P == 0 ? pk.total : D->bands_m[j];
        if (lane == 0) {
            D->bands_prefix[at] = prefix;
            D->bands_rank[at] = pk.rank;
            if (P == 0 && q == 0) {
                D->bands_m[j] = m;
                D->bands_nan[j] = (long long)__hip_atomic_load(&D->bands_nan_count[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&D->bands_nan_count[j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (P == RH_SELECT_PASSES - 1) {
                D->bands[(size_t)slot * ni * np + j * np + q] = m ? bands_value_of(prefix) : __builtin_nan("");
            }
        }
    }
    __syncthreads();   // (in pass 0 the pairs of an item read one histogram)
    for (int b = threadIdx.x; b < ni * nh * NB; b += RH_BLOCK) {
        const int jq = b / NB;
        __hip_atomic_store(D->bands_hist + (size_t)((jq / nh) * RH_BANDS_MAX_PROBS + jq % nh) * RH_SELECT_NBINS + b % NB, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&D->bands_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (P == RH_SELECT_PASSES - 1) {
            long long *hd = D->bands_hdr + (size_t)slot * (2 + 2 * ni);
            hd[0] = c.k;
            hd[1] = c.t1;
            for (int j = 0; j < ni; ++j) {
                hd[2 + 2 * j] = D->bands_m[j];
                hd[3 + 2 * j] = D->bands_nan[j];
            }
            D->bands_rows = row + 1;
        }
    }
}

// ---- bands per zone (rh_bands_configure_zonal) ----
// The promise.  Block z of a row is, bit for bit, the row the plain configuration records with mask = (zone == z): np.sort(s)[clamp(ceil(p
// m) - 1, 0, m - 1)] over the zone's columns, with the + 0.0 rule and the NaN rule above.  k_bands runs unchanged (its byte mask is zone
// >= 0, written at the configuration), so the clock, the SUM accumulation and the key planes are the plain path's own.
// Column lists.  A stable counting sort on the host: bands_zone_off [n_zones + 1] and bands_zone_cols (int32 column indices, ascending
// within a zone), uploaded once.
// k_bands_zonal, ONE launch behind k_bands in place of the six k_bands_select: grid (n_zones, n_items).  A workgroup walks its zone's list
// (eight columns in flight per thread), gathers keys[j * n + col] and runs all RH_SELECT_PASSES digit passes itself: one LDS histogram per
// probability at the widths of BandsPass<P>; pass 0 is shared by the probabilities and yields m and n_nan; a wavefront per probability
// picks the digit (bands_pick); prefixes and ranks stay in LDS between the passes.  The later passes read the keys again: L2 serves them.
// LDS atomics only -- no device-scope atomic, no completion counter.  It writes its (item, zone) block of row bands_rows % bands_cap:
// counts {m, n_nan} and the values, NaN with m == 0.  k_bands_zonal_row<<<1, 1>>> behind it in the same stream writes {k, t1} and advances
// bands_rows: stream order stands where the plain path has its last-workgroup pattern.  Both end after the scalar loads on a step that
// is not counted.
// Load balance.  ONE workgroup walks a zone, however large: the largest zone sets the time of a counted step.  A map with one dominant
// zone belongs to the plain configuration's mask, whose selection strides over the whole device.
// Cost of a counted step: 8 B per item and participating column per pass gathered (six passes), 4 B per column of bands_zone_cols per pass,
// 2 launches.
template <int P>
RH_DEV void bands_zonal_pass(const unsigned long long *keys, const int *cols, long long beg, long long end, int np, const double *probs, unsigned *hist,
                             unsigned long long *s_prefix, long long *s_rank, long long *s_count, unsigned *s_nan) {
    constexpr int NB = BandsPass<P>::nb, NC = NB / 64;
    const int nh = P == 0 ? 1 : np;
    for (int b = threadIdx.x; b < nh * NB; b += RH_BLOCK) hist[b] = 0;
    if (P == 0 && threadIdx.x == 0) *s_nan = 0;
    __syncthreads();
    unsigned long long pre[RH_BANDS_MAX_PROBS];
#pragma unroll
    for (int q = 0; q < RH_BANDS_MAX_PROBS; ++q) pre[q] = (P > 0 && q < np) ? s_prefix[q] : 0ull;
    unsigned mine = 0, mine_nan = 0;   // pass 0: the NaNs this thread met (the numbers are the histogram's total)
    select_walk_list<false>(keys, nullptr, cols, beg, end, [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<P>(key, w, np, pre, hist, mine, mine_nan); });
    if (P == 0 && mine_nan) atomicAdd(s_nan, mine_nan);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < np; q += RH_BLOCK / 64) {   // (uniform over the wavefront)
        const unsigned *h = hist + (P == 0 ? 0 : q) * NB;
        unsigned v[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = h[k * 64 + lane];
        const SelectPick pk = select_pick_step<P>(v, probs[q], &s_prefix[q], &s_rank[q]);
        if (lane == 0) {
            s_prefix[q] = pk.prefix;
            s_rank[q] = pk.rank;
            if (P == 0 && q == 0) {
                s_count[0] = pk.total;
                s_count[1] = (long long)*s_nan;
            }
        }
    }
    __syncthreads();   // (the next pass clears the histograms and reads the prefixes)
}
__global__ __launch_bounds__(RH_BLOCK) void k_bands_zonal(DevState *D, long long n, int after_fused) {
    __shared__ unsigned hist[RH_BANDS_MAX_PROBS * RH_SELECT_NBINS];
    __shared__ unsigned long long s_prefix[RH_BANDS_MAX_PROBS];
    __shared__ long long s_rank[RH_BANDS_MAX_PROBS], s_count[2];
    __shared__ unsigned s_nan;
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;   // (uniform over the grid)
    const int z = blockIdx.x, j = blockIdx.y, nz = gridDim.x, ni = gridDim.y, np = D->bands_nprobs;
    const long long beg = D->bands_zone_off[z], end = D->bands_zone_off[z + 1];
    const unsigned long long *keys = D->bands_keys + (size_t)j * (size_t)n;
    const int *cols = D->bands_zone_cols;
    const double *probs = D->bands_probs;
    const size_t block = ((size_t)(D->bands_rows % D->bands_cap) * ni + j) * nz + z;
    double *out = D->bands + block * np;
    long long *counts = D->bands_counts + block * 2;
    bands_zonal_pass<0>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    const long long m = s_count[0];
    if (threadIdx.x == 0) {
        counts[0] = m;
        counts[1] = s_count[1];
    }
    if (m == 0) {   // (uniform over the workgroup)
        if ((int)threadIdx.x < np) out[threadIdx.x] = __builtin_nan("");
        return;
    }
    bands_zonal_pass<1>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    bands_zonal_pass<2>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    bands_zonal_pass<3>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    bands_zonal_pass<4>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    bands_zonal_pass<5>(keys, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, &s_nan);
    if ((int)threadIdx.x < np) {   // after the last pass the prefix IS the key
        out[threadIdx.x] = bands_value_of(s_prefix[threadIdx.x]);
    }
}
__global__ void k_bands_zonal_row(DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;
    const long long row = D->bands_rows;
    long long *hd = D->bands_hdr + 2 * (row % D->bands_cap);
    hd[0] = c.k;
    hd[1] = c.t1;
    D->bands_rows = row + 1;
}

// ---- likelihood-weighted bands (rh_bands_configure_weighted) ----
// The rule.  Everything is the plain bands' rule except what is named here: clock, SUM / LAST aggregation, s = (acc or v) + 0.0, NaN
// handling, keys.
// Weights.  Integer weights w_i, one uint16 per column, in 0 ... 65535: the type is the bound.  A column with w_i == 0 takes no part,
// exactly as a masked-out column: it loads and stores nothing in k_bands (whose byte mask is w != 0, written at the configuration, as
// the zonal path writes zone >= 0), it is in neither m nor n_nan, and its key stays RH_SELECT_KEY_MASKED.
// Counts.  m is the number of participating columns whose s is not a NaN, n_nan the number whose s is a NaN: column counts, as in the
// plain rule.  New: W = sum of w_i over the m columns, an int64.  W < 2^47, since n < 2^31, so (double)W is exact.
// Target and result.  For a probability p: T = clamp((int64)ceil(p * (double)W), 1, W) -- one double multiplication, one ceil, the same
// on host and device -- and the result is the smallest s with sum_{s_i <= s} w_i >= T.  In numpy:
//     o = np.argsort(s, kind="stable");  cw = np.cumsum(w[o].astype(np.int64));  value = s[o][np.searchsorted(cw, T, side="left")]
// equivalently np.sort(np.repeat(s, w))[T - 1].  p = 0 is the participants' minimum and p = 1 their maximum.  With m == 0 the row holds
// NaN and W = 0.
// Consequence.  With every weight in {0, 1}: T - 1 = clamp(ceil(p m) - 1, 0, m - 1), so the row is bit for bit the row of the plain
// configuration with mask = (w != 0), header and values, and W == m.  In the selection r = T - 1 takes the place of the rank
// (bands_rank_of(p, W) is T - 1): the pick is again "the digit at which the cumulative sum passes r", and r -= below.
//
// k_bands_select_w<P>: six launches, the digit widths of BandsPass<P>, the last-workgroup completion pattern of k_bands_select with its
// invariant.  What differs:
//   histogram  a key's bin gains w_i, not 1.  The weight plane (bands_weight, 2 B per column) is read in every pass, non-temporal, issued
//              with the key loads.  A zero weight needs no test: such a column's key is RH_SELECT_KEY_MASKED.
//   LDS bins   stay uint32 (64 KiB for eight probabilities).  A bin holds at most (columns the workgroup walks) x 65535, so a workgroup
//              walks at most RH_SELECT_W_MAX_TILES = 256 tiles of RH_BLOCK = 256 columns: 65536 x 65535 < 2^32.  bands_weighted_grid
//              derives the grid from that bound -- max(min(RH_SELECT_MAX_GRID, ntiles), ceil(ntiles / 256)) -- and is the one place that
//              does; beyond 16.7 x 10^6 columns the grid grows past one workgroup per CU.  (The tile loop gives workgroup b the tiles
//              t = b mod grid: ceil(ntiles / grid) of them at most.)
//   merge      into bands_whist, uint64 [item][probability][2048] (1 MiB), with returning 64-bit device-scope integer adds of the non-zero
//              bins (dep |= ret >> 63; a sum stays below 2^47).  The last workgroup clears it.
//   counts     m is no longer the histogram's total: pass 0 counts the keys below RH_SELECT_KEY_NAN per item in LDS beside nan_count, and
//              one returning device-scope add per workgroup and item takes it to bands_m_count.  W is the pass-0 histogram's total.
//   pick       select_pick_step over unsigned long long bins: k_bands_select and k_bands_zonal instantiate it over unsigned bins, with
//              32-bit lane arithmetic.
//   row        header {k, t1, m, n_nan per item} as in the plain path; W per item goes into a ring of its own, bands_wsum [cap][items]
//              int64, written with the header before bands_rows advances.
// No counter overflows for any configuration the configure call accepts (n < 2^31): LDS bins by the bound above, the global bins and W
// below 2^31 x 65535 < 2^47, m and n_nan below 2^31, bands_done at most 2^15 workgroups.  Integer atomics only.
// Cost of a counted step: the plain path's, plus 2 B per column, item and pass of weights, plus 64-bit merges (8 B a bin, not 4).
template <int P>
__global__ __launch_bounds__(RH_BLOCK) void k_bands_select_w(Arena a, DevState *D, int after_fused) {
    constexpr int NB = BandsPass<P>::nb, NC = NB / 64;
    __shared__ unsigned hist[RH_BANDS_MAX_PROBS * RH_SELECT_NBINS];
    __shared__ unsigned nan_count, num_count, posted, is_last;
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;   // (uniform over the grid)
    const int ni = D->bands_nitems, np = D->bands_nprobs, nh = P == 0 ? 1 : np;
    const int64_t n = a.n;
    const unsigned short *wts = D->bands_weight;
    unsigned dep = 0;
    if (threadIdx.x == 0) posted = 0;
    for (int j = 0; j < ni; ++j) {
        for (int b = threadIdx.x; b < nh * NB; b += RH_BLOCK) hist[b] = 0;
        if (threadIdx.x == 0) nan_count = num_count = 0;
        __syncthreads();
        unsigned long long pre[RH_BANDS_MAX_PROBS];
#pragma unroll
        for (int q = 0; q < RH_BANDS_MAX_PROBS; ++q) pre[q] = (P > 0 && q < np) ? D->bands_prefix[j * RH_BANDS_MAX_PROBS + q] : 0ull;
        const unsigned long long *keys = D->bands_keys + (size_t)j * (size_t)n;
        unsigned mine = 0, mine_nan = 0;   // pass 0: the numbers and the NaNs this thread met
        select_walk_tiles<true>(keys, wts, n, [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<P>(key, w, np, pre, hist, mine, mine_nan); });
        if (P == 0 && mine) atomicAdd(&num_count, mine);
        if (P == 0 && mine_nan) atomicAdd(&nan_count, mine_nan);
        __syncthreads();
        unsigned long long *g = D->bands_whist + (size_t)j * RH_BANDS_MAX_PROBS * RH_SELECT_NBINS;
        for (int b = threadIdx.x; b < nh * NB; b += RH_BLOCK) {
            const unsigned cnt = hist[b];
            if (cnt)
                dep |= (unsigned)(__hip_atomic_fetch_add(g + (b / NB) * RH_SELECT_NBINS + (b % NB), (unsigned long long)cnt, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT) >> 63);
        }
        if (P == 0 && threadIdx.x == 0) {
            if (nan_count) dep |= __hip_atomic_fetch_add(&D->bands_nan_count[j], nan_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 31;
            if (num_count) dep |= __hip_atomic_fetch_add(&D->bands_m_count[j], num_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 31;
        }
        __syncthreads();   // (the next item clears the histogram)
    }
    // Completion, as in k_bands_select: every thread's adds have returned before its LDS add (dep is 0: a sum stays below 2^47, a count
    // below 2^31), the barrier follows, and only then is the workgroup counted done.
    atomicAdd(&posted, dep);
    __syncthreads();
    if (threadIdx.x == 0)
        is_last = __hip_atomic_fetch_add(&D->bands_done, 1u + posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!is_last) return;

    const int lane = threadIdx.x & 63;
    const long long row = D->bands_rows;
    const long long slot = row % D->bands_cap;
    for (int pair = threadIdx.x >> 6; pair < ni * np; pair += RH_BLOCK / 64) {   // (uniform over the wavefront)
        const int j = pair / np, q = pair - j * np, at = j * RH_BANDS_MAX_PROBS + q;
        const unsigned long long *h = D->bands_whist + (size_t)(j * RH_BANDS_MAX_PROBS + (P == 0 ? 0 : q)) * RH_SELECT_NBINS;
        unsigned long long v[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = __hip_atomic_load(h + k * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const SelectPick pk = select_pick_step<P>(v, D->bands_probs[q], &D->bands_prefix[at], &D->bands_rank[at]);   // (pass 0: the rank is T - 1)
        const unsigned long long prefix = pk.prefix;
        if (lane == 0) {
            D->bands_prefix[at] = prefix;
            D->bands_rank[at] = pk.rank;
            if (P == 0 && q == 0) {
                D->bands_w[j] = pk.total;
                D->bands_m[j] = (long long)__hip_atomic_load(&D->bands_m_count[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                D->bands_nan[j] = (long long)__hip_atomic_load(&D->bands_nan_count[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&D->bands_m_count[j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&D->bands_nan_count[j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (P == RH_SELECT_PASSES - 1) {
                D->bands[(size_t)slot * ni * np + j * np + q] = D->bands_m[j] ? bands_value_of(prefix) : __builtin_nan("");
            }
        }
    }
    __syncthreads();   // (in pass 0 the pairs of an item read one histogram)
    for (int b = threadIdx.x; b < ni * nh * NB; b += RH_BLOCK) {
        const int jq = b / NB;
        __hip_atomic_store(D->bands_whist + (size_t)((jq / nh) * RH_BANDS_MAX_PROBS + jq % nh) * RH_SELECT_NBINS + b % NB, 0ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&D->bands_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (P == RH_SELECT_PASSES - 1) {
            long long *hd = D->bands_hdr + (size_t)slot * (2 + 2 * ni), *ws = D->bands_wsum + (size_t)slot * ni;
            hd[0] = c.k;
            hd[1] = c.t1;
            for (int j = 0; j < ni; ++j) {
                hd[2 + 2 * j] = D->bands_m[j];
                hd[3 + 2 * j] = D->bands_nan[j];
                ws[j] = D->bands_w[j];
            }
            D->bands_rows = row + 1;
        }
    }
}

// ---- where the observation falls (rh_bands_observations) ----
// The rule.  Everything is the bands' rule as it stands: clock, SUM / LAST aggregation, s = (acc or v) + 0.0, NaN handling, mask / zones /
// weights, ring numbering.  On top of it an item may carry observations: one float64 series per item without zones, one per zone with
// zones; NaN: missing.
// Indexing.  The series is indexed from the configuration's `start`, not from the first counted interval: for row interval number k the
// element is o = obs[k + bands_obs_first], bands_obs_first = (t_first - start) / frequency (the caller's); an index beyond the series
// means missing.
// The pair.  On a counted step, per item (and zone), an int64 pair (below, equal) goes into a ring beside the rows: o a NaN -- below =
// equal = -1; else o' = o + 0.0 and, over the participating columns whose s is a number,
//     below = sum c_i [s_i < o'],  equal = sum c_i [s_i == o'],  c_i = 1 (plain, zonal) or w_i (weighted);  m == 0: (0, 0).
// In numpy, x and wx the participants that are numbers: below = int(wx[x < o].sum()), equal = int(wx[x == o].sum()).  On the device an
// UNSIGNED comparison of the keys k_bands stored with key(o'): because of the + 0.0 on both sides it is the float comparison for every
// value that is not a NaN, +-0.0 and +-inf included.
// Consequences.  T_tot = m (plain, zonal) or W (weighted): 0 <= below, 0 <= equal, below + equal <= T_tot; for a recorded probability p
// with target T = clamp(ceil(p T_tot), 1, T_tot) and recorded quantile q:  q <= o <=> below + equal >= T,  q < o <=> below >= T.
//
// k_bands_obs (plain and weighted): grid (min(RH_SELECT_MAX_GRID, ntiles), items) behind the selection's last pass.  A workgroup strides
// over the tiles of its item's key plane as k_bands_select does (eight tiles in flight per thread); a thread adds 1, or bands_weight[i],
// into two int64 registers; keys >= RH_SELECT_KEY_NAN are skipped (a zero weight needs no test: that key is RH_SELECT_KEY_MASKED).  The
// wavefronts reduce by shuffles, the four of a workgroup through LDS, and thread 0 stores the workgroup's pair into bands_obs_part
// [item][workgroup][2]: plain stores, no atomics, no last-workgroup pattern.  A missing o ends the workgroup after the scalar loads.
// k_bands_obs_row: grid (items), one wavefront; adds the partials and writes the pair at the slot of the row just recorded -- the
// selection's last pass has advanced bands_rows, so that is (bands_rows - 1) mod bands_cap.  Stream order stands where the plain path has
// its completion counter.
// k_bands_obs_zonal: grid (zones, items) behind k_bands_zonal_row; a workgroup walks its zone's column list as bands_zonal_pass does,
// reduces likewise and writes its pair itself.
// All three end after the scalar loads on a step that is not counted, and under after_fused && D->skipped.
// No sum overflows: a thread, a workgroup and an item add at most n < 2^31 columns of weight <= 65535 -- below 2^47, as W.
// Cost of a counted step with observations: one more pass of 8 B (+ 2 B with weights) per item and column, on top of the selection's
// six, and two launches (zonal: one launch, 8 B + 4 B per participating column gathered).
// the observation of (item j, series z) for the interval the clock closes; NaN: missing, or beyond the series
RH_DEV double bands_obs_of(const DevState *D, const BandsClock &c, int j, int z, int nseries) {
    const long long at = c.k + D->bands_obs_first, len = D->bands_obs_n;
    return at >= 0 && at < len ? D->bands_obs[((size_t)j * nseries + z) * (size_t)len + (size_t)at] : __builtin_nan("");
}
// key(o + 0.0): the key expression of k_bands (o is not a NaN)
RH_DEV unsigned long long bands_obs_key(double o) {
    return bands_key_of(o + 0.0);
}
// (the pair of a key, the workgroup's sums and the sum of the partials are select_pair_add, select_pair_reduce and select_pair_partials of
// rh_select.h)
__global__ __launch_bounds__(RH_BLOCK) void k_bands_obs(Arena a, DevState *D, int after_fused) {
    __shared__ long long s_part[RH_BLOCK / 64][2];
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;   // (uniform over the grid)
    const int j = blockIdx.y;
    const double o = bands_obs_of(D, c, j, 0, 1);
    if (o != o) return;   // (uniform over the item's workgroups: k_bands_obs_row writes -1, -1 and reads no partial)
    const unsigned long long ko = bands_obs_key(o);
    const int64_t n = a.n;
    const unsigned long long *keys = D->bands_keys + (size_t)j * (size_t)n;
    const unsigned short *wts = D->bands_weight;   // (null: every participating column counts 1; uniform, tested once outside the walk)
    long long below = 0, equal = 0;   // (below 2^47: at most n < 2^31 columns of weight <= 65535)
    const auto add = [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_pair_add(key, w, ko, below, equal); };
    if (wts)
        select_walk_tiles<true>(keys, wts, n, add);
    else
        select_walk_tiles<false>(keys, wts, n, add);
    select_pair_reduce(below, equal, s_part);
    if (threadIdx.x == 0) {
        long long *part = D->bands_obs_part + ((size_t)j * gridDim.x + blockIdx.x) * 2;
        part[0] = below;
        part[1] = equal;
    }
}
__global__ __launch_bounds__(64) void k_bands_obs_row(DevState *D, int nparts, int after_fused) {
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;
    const int j = blockIdx.x, ni = gridDim.x;
    const double o = bands_obs_of(D, c, j, 0, 1);
    long long below = -1, equal = -1;
    if (o == o) select_pair_partials(D->bands_obs_part + (size_t)j * nparts * 2, nparts, below, equal);   // (uniform over the wavefront)
    if (threadIdx.x == 0) {
        long long *out = D->bands_obs_ring + ((size_t)((D->bands_rows - 1) % D->bands_cap) * ni + j) * 2;
        out[0] = below;
        out[1] = equal;
    }
}
__global__ __launch_bounds__(RH_BLOCK) void k_bands_obs_zonal(DevState *D, long long n, int after_fused) {
    __shared__ long long s_part[RH_BLOCK / 64][2];
    if (after_fused && D->skipped) return;
    const BandsClock c = bands_clock(D);
    if (!c.counted) return;   // (uniform over the grid)
    const int z = blockIdx.x, j = blockIdx.y, nz = gridDim.x, ni = gridDim.y;
    long long *out = D->bands_obs_ring + (((size_t)((D->bands_rows - 1) % D->bands_cap) * ni + j) * nz + z) * 2;
    const double o = bands_obs_of(D, c, j, z, nz);
    if (o != o) {   // (uniform over the workgroup)
        if (threadIdx.x == 0) out[0] = out[1] = -1;
        return;
    }
    const unsigned long long ko = bands_obs_key(o);
    const long long beg = D->bands_zone_off[z], end = D->bands_zone_off[z + 1];
    const unsigned long long *keys = D->bands_keys + (size_t)j * (size_t)n;
    const int *cols = D->bands_zone_cols;
    long long below = 0, equal = 0;   // (at most n < 2^31)
    select_walk_list<false>(keys, nullptr, cols, beg, end, [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_pair_add(key, w, ko, below, equal); });
    select_pair_reduce(below, equal, s_part);
    if (threadIdx.x == 0) {
        out[0] = below;
        out[1] = equal;
    }
}
