// rh_sas_bands.h -- transport bands (rh_sas_bands_*, include/roger_hip_sas.h): the exact quantiles ACROSS the columns of a window value of
// the offline transport model, per sample window -- the 5 % / 50 % / 95 % band of the simulated delta-18O of a SAS parameter study around
// the bottle samples -- and where the observation falls in it.  A selection, not a reduction: integer counters over bit patterns, so a
// row is np.sort(np.repeat(s, w))[T - 1] bit for bit.  Included by rh_sas.hip only; the numpy twin is tests/sas_bands_reference.py.
//
// THE RULE
// Windows and clock.  The host owns the clock, exactly as for rh_sas_scores_*: window k is the days [first_day[k], last_day[k]] of the
// context's count of recorded days; windows are in increasing order and do not overlap.  A day outside every window launches nothing,
// and so does a day inside a window whose first day was never recorded.
// Items.  At most 8 items (value, weight, kind), kind BULK, MEAN or LAST with the codes and the meaning of rh_sas_scores.h; value a
// width-1 float64 result of the step, weight a daily flux input (BULK only).  Per column and day num and den follow k_sas_scores: they
// restart from +0.0 on the window's first day; the day is ELIGIBLE iff wd > 0 && v == v (BULK: wd the day's weight, MEAN: wd = 1.0);
// num = num + fl(v * wd), den = den + wd, one IEEE operation each (the library is built with -ffp-contract=off).
// Window value.  On the closing day  BULK / MEAN: s = den > 0 ? num / den : NaN;  LAST: s = v.  Then s = s + 0.0, so -0.0 becomes +0.0 and
// equal zeros have one bit pattern.  A NaN s is counted in n_nan and takes no further part; +-inf are ordinary values.
// Participation.  An optional byte mask and an optional uint16 weight w_i in 0 ... 65535 (GLUE likelihoods); without a weight plane
// w_i = 1.  A column with mask == 0 or w_i == 0 loads and stores nothing.
// Counts.  m: the participating columns with a number; n_nan: those with a NaN; W = sum of w_i over the m columns, an int64 that is
// exact as a double.
// Quantiles.  At most 8 probabilities p in [0, 1], shared by the items.  T = clamp((int64)ceil(p * (double)W), 1, W); the result is the
// smallest s with sum_{s_i <= s} w_i >= T, the bits of np.sort(np.repeat(s, w))[T - 1] -- the weighted rule of rh_bands.h, which with all
// weights 1 is the plain rule np.sort(s)[clamp(ceil(p m) - 1, 0, m - 1)].  With m == 0 the values are NaN and W = 0.
// Observations (optional; per item one float64 series of length K, NaN: missing).  On the closing day the int64 pair (below, equal): the
// weights of the members below and equal to o + 0.0, by the UNSIGNED comparison of the stored keys with key(o + 0.0) as in rh_bands.h
// ("where the observation falls"); a missing o gives (-1, -1); m == 0 gives (0, 0).
// Result.  No ring: the host knows K.  rows [K][item][probability] float64 (NaN until the window closes), hdr [K][item]{m, n_nan, W}
// int64 (0), obs_pair [K][item][2] int64 (-1, written so at configure: the host stores the pair of a missing observation itself).  The
// host holds closed [K], as the scores do.
//
// THE LAUNCHES.  All on the context's stream, ordered by kernel boundaries: no completion counter, no spin, no returning atomic.
//   k_sas_bands_day   one thread per column: num / den; on the closing day the key of s into the item's key plane.  Validity is part of
//                     the key plane: a NaN s stores KEY_NAN, a column that does not participate keeps KEY_MASKED, written once at
//                     configure.  Launched on every day of an open window if some item is BULK / MEAN, else on closing days only.
//   closing day:      k_sas_bands_hist<P>, k_sas_bands_pick<P> for P = 0 ... 5 (digits of 11, 11, 11, 11, 11 and 9 bits, most significant
//                     first), then with an observation that is not NaN k_sas_bands_obs, k_sas_bands_obs_row: 13 launches, 15 with
//                     observations.
// No counter overflows for any configuration the configure call accepts (n < 2^31): an LDS bin by bands_weighted_grid's bound (rh_select.h:
// 256 tiles x 256 columns x 65535 < 2^32), the global bins, W and the pairs below 2^31 x 65535 < 2^47, m and n_nan below 2^31.
// Bytes per column.  The day kernel as rh_sas_scores.h counts them (a BULK item 48 B on a non-closing day, 32 B on a window's first), and
// 8 B more for the key on a closing day.  The selection: six passes x (8 B key + 2 B weight) per item and column; with observations one
// pass more.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rh_select.h"
#include "roger_hip_sas.h"

#define SAS_BANDS_HDR 3        // m, n_nan, W
static_assert(RH_SAS_BANDS_MAX_PROBS == RH_SELECT_MAX_PROBS && SAS_BANDS_HDR == RH_SELECT_HDR, "rh_select.h states the histograms of the selection");

struct SasBandsDev {
    const double *val[RH_SAS_BANDS_MAX_ITEMS];   // the width-1 value
    const double *wgt[RH_SAS_BANDS_MAX_ITEMS];   // first row of the DAILY weight; null: none
    int kind[RH_SAS_BANDS_MAX_ITEMS];
    double probs[RH_SAS_BANDS_MAX_PROBS];
    int n_items, n_probs;
    int64_t n, n_samples;
    const unsigned char *mask;                   // [n] or null
    const unsigned short *weight;                // [n] or null: every participating column counts 1
    const double *obs;                           // [item][sample] or null
    double *acc;                                 // [item][2][n]: num, den
    unsigned long long *keys;                    // [item][n]
    unsigned long long *hist;                    // [item][probability][2048], zero between two passes
    unsigned *m_count, *nan_count;               // [item], zero between two closing days
    unsigned long long *prefix;                  // [item][8]: the digits picked so far
    long long *rank;                             // [item][8]: the rank that remains below the prefix
    long long *m, *nan, *w;                      // [item]: fixed by pass 0
    long long *obs_part;                         // [item][workgroup][2]
    double *rows;                                // [sample][item][probability]
    long long *hdr;                              // [sample][item][3]
    long long *obs_pair;                         // [sample][item][2]
};

__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_day(const SasBandsDev *__restrict__ P, int first, int closes, int64_t day_off) {
    const int64_t i = (int64_t)blockIdx.x * RH_SELECT_BLOCK + threadIdx.x;
    const size_t n = (size_t)P->n;
    if (i >= P->n) return;
    if (P->mask && !P->mask[i]) return;
    if (P->weight && !P->weight[i]) return;
    const int ni = P->n_items;
    for (int j = 0; j < ni; ++j) {
        const int kind = P->kind[j];
        if (kind == RH_SAS_SCORES_LAST && !closes) continue;
        const double v = P->val[j][i];
        double s = v;
        if (kind != RH_SAS_SCORES_LAST) {
            double *p = P->acc + (size_t)j * 2 * n + (size_t)i;
            const double wd = kind == RH_SAS_SCORES_BULK ? P->wgt[j][day_off + i] : 1.0;
            double num = 0.0, den = 0.0;
            if (!first) {
                num = p[0];
                den = p[n];
            }
            const bool eligible = wd > 0.0 && v == v;
            if (eligible) {
                const double t = v * wd;   // rounded before it is added
                num = num + t;
                den = den + wd;
            }
            if (first || eligible) {
                p[0] = num;
                p[n] = den;
            }
            if (!closes) continue;
            s = den > 0.0 ? num / den : __builtin_nan("");
        }
        s = s + 0.0;
        P->keys[(size_t)j * n + (size_t)i] = s != s ? RH_SELECT_KEY_NAN : bands_key_of(s);
    }
}

// Pass PASS, the histograms: grid bands_weighted_grid(n).  A workgroup takes the items one after the other: select_walk_tiles and
// select_count of rh_select.h fill an LDS histogram per probability -- with a weight plane a key counts its weight, else 1 -- then its
// NON-ZERO bins go to the global uint64 histogram with device-scope integer adds whose results nobody takes: integer adds commute, the
// sum does not depend on their order, and only k_sas_bands_pick<PASS>, the next kernel in the stream, reads it.
template <int PASS>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_hist(const SasBandsDev *__restrict__ P) {
    constexpr int NB = BandsPass<PASS>::nb;
    __shared__ unsigned hist[RH_SAS_BANDS_MAX_PROBS * RH_SELECT_NBINS];
    __shared__ unsigned nan_count, num_count;
    const int ni = P->n_items, np = P->n_probs, nh = PASS == 0 ? 1 : np;
    const int64_t n = P->n;
    const unsigned short *wts = P->weight;   // (uniform: tested once per workgroup and item, outside the loop over the keys)
    for (int j = 0; j < ni; ++j) {
        for (int b = threadIdx.x; b < nh * NB; b += RH_SELECT_BLOCK) hist[b] = 0;
        if (threadIdx.x == 0) nan_count = num_count = 0;
        __syncthreads();
        unsigned long long pre[RH_SAS_BANDS_MAX_PROBS];
#pragma unroll
        for (int q = 0; q < RH_SAS_BANDS_MAX_PROBS; ++q) pre[q] = (PASS > 0 && q < np) ? P->prefix[j * RH_SAS_BANDS_MAX_PROBS + q] : 0ull;
        const unsigned long long *keys = P->keys + (size_t)j * (size_t)n;
        unsigned mine = 0, mine_nan = 0;   // pass 0: the numbers and the NaNs this thread met
        const auto count = [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<PASS>(key, w, np, pre, hist, mine, mine_nan); };
        if (wts)
            select_walk_tiles<true>(keys, wts, n, count);
        else
            select_walk_tiles<false>(keys, wts, n, count);
        if (PASS == 0 && mine) atomicAdd(&num_count, mine);
        if (PASS == 0 && mine_nan) atomicAdd(&nan_count, mine_nan);
        __syncthreads();
        unsigned long long *g = P->hist + (size_t)j * RH_SAS_BANDS_MAX_PROBS * RH_SELECT_NBINS;
        for (int b = threadIdx.x; b < nh * NB; b += RH_SELECT_BLOCK) {
            const unsigned cnt = hist[b];
            if (cnt) (void)__hip_atomic_fetch_add(g + (b / NB) * RH_SELECT_NBINS + (b % NB), (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (PASS == 0 && threadIdx.x == 0) {
            if (nan_count) (void)__hip_atomic_fetch_add(&P->nan_count[j], nan_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (num_count) (void)__hip_atomic_fetch_add(&P->m_count[j], num_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();   // (the next item clears the histogram)
    }
}

// Pass PASS, the pick: ONE workgroup behind k_sas_bands_hist<PASS>.  A wavefront per (item, probability) pair reads the pair's bins -- 64
// at a time, all loads requested first -- finds the digit at which the cumulative weight passes the remaining rank, appends it to the
// pair's prefix and subtracts the weight below it from the rank.  Pass 0 fixes m, n_nan, W and T - 1.  Behind a workgroup barrier the
// bins that were read are cleared.  After the last pass the prefix IS the key: row k of the result.
template <int PASS>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_pick(const SasBandsDev *__restrict__ P, int64_t k) {
    constexpr int NB = BandsPass<PASS>::nb, NC = NB / 64;
    const int ni = P->n_items, np = P->n_probs, nh = PASS == 0 ? 1 : np;
    const int lane = threadIdx.x & 63;
    for (int pair = threadIdx.x >> 6; pair < ni * np; pair += RH_SELECT_BLOCK / 64) {   // (uniform over the wavefront)
        const int j = pair / np, q = pair - j * np, at = j * RH_SAS_BANDS_MAX_PROBS + q;
        const unsigned long long *h = P->hist + (size_t)(j * RH_SAS_BANDS_MAX_PROBS + (PASS == 0 ? 0 : q)) * RH_SELECT_NBINS;
        unsigned long long v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = h[c * 64 + lane];
        const SelectPick pk = select_pick_step<PASS>(v, P->probs[q], &P->prefix[at], &P->rank[at]);   // (pass 0: the rank is T - 1)
        const unsigned long long prefix = pk.prefix;
        if (lane == 0) {
            P->prefix[at] = prefix;
            P->rank[at] = pk.rank;
            if (PASS == 0 && q == 0) {
                P->w[j] = pk.total;
                P->m[j] = (long long)P->m_count[j];
                P->nan[j] = (long long)P->nan_count[j];
                P->m_count[j] = 0u;
                P->nan_count[j] = 0u;
            }
            if (PASS == RH_SELECT_PASSES - 1) {
                const long long m = P->m[j];
                P->rows[((size_t)k * ni + j) * np + q] = m ? bands_value_of(prefix) : __builtin_nan("");
                if (q == 0) {
                    long long *hd = P->hdr + ((size_t)k * ni + j) * SAS_BANDS_HDR;
                    hd[0] = m;
                    hd[1] = P->nan[j];
                    hd[2] = P->w[j];
                }
            }
        }
    }
    __syncthreads();   // (in pass 0 the pairs of an item read one histogram)
    for (int b = threadIdx.x; b < ni * nh * NB; b += RH_SELECT_BLOCK) {
        const int jq = b / NB;
        P->hist[(size_t)((jq / nh) * RH_SAS_BANDS_MAX_PROBS + jq % nh) * RH_SELECT_NBINS + b % NB] = 0ull;
    }
}

// ---- where the observation falls ----
// k_sas_bands_obs: grid (select_obs_grid(n), items) behind the last pick.  A workgroup strides over the tiles of its item's key plane as
// k_sas_bands_hist does; a thread adds 1, or the column's weight, into two int64 registers; keys >= KEY_NAN are skipped (a zero weight
// needs no test: that key is KEY_MASKED).  The wavefronts reduce by shuffles, the four of a workgroup through LDS, and thread 0 stores the
// workgroup's pair into obs_part: plain stores, no atomics.  k_sas_bands_obs_row: grid (items), one wavefront; adds the partials in a
// fixed order into obs_pair[k].  An item whose observation of window k is missing ends both after the scalar loads: its pair stays
// (-1, -1).
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_obs(const SasBandsDev *__restrict__ P, int64_t k) {
    __shared__ long long s_part[RH_SELECT_BLOCK / 64][2];
    const int j = blockIdx.y;
    const double o = P->obs[(size_t)j * (size_t)P->n_samples + (size_t)k];
    if (o != o) return;   // (uniform over the item's workgroups)
    const unsigned long long ko = bands_key_of(o + 0.0);
    const int64_t n = P->n;
    const unsigned long long *keys = P->keys + (size_t)j * (size_t)n;
    const unsigned short *wts = P->weight;   // (uniform: tested once, outside the walk)
    long long below = 0, equal = 0;   // (below 2^47: at most n < 2^31 columns of weight <= 65535)
    const auto add = [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_pair_add(key, w, ko, below, equal); };
    if (wts)
        select_walk_tiles<true>(keys, wts, n, add);
    else
        select_walk_tiles<false>(keys, wts, n, add);
    select_pair_reduce(below, equal, s_part);
    if (threadIdx.x == 0) {
        long long *part = P->obs_part + ((size_t)j * gridDim.x + blockIdx.x) * 2;
        part[0] = below;
        part[1] = equal;
    }
}
__global__ __launch_bounds__(64) void k_sas_bands_obs_row(const SasBandsDev *__restrict__ P, int64_t k, int nparts) {
    const int j = blockIdx.x, ni = gridDim.x;
    const double o = P->obs[(size_t)j * (size_t)P->n_samples + (size_t)k];
    if (o != o) return;   // (uniform over the wavefront)
    long long below, equal;
    select_pair_partials(P->obs_part + (size_t)j * nparts * 2, nparts, below, equal);
    if (threadIdx.x == 0) {
        long long *out = P->obs_pair + ((size_t)k * ni + j) * 2;
        out[0] = below;
        out[1] = equal;
    }
}
