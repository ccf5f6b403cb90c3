// rh_sas_bands_zonal.h -- transport bands per zone (rh_sas_bands_configure_zonal, include/roger_hip_sas.h): the exact quantiles of
// rh_sas_bands.h for every zone of a zone map in one run -- the lysimeters of a SAS parameter study, the land uses or sub-catchments of a
// catchment map -- each zone with its own observations.  Included by rh_sas.hip only, behind rh_sas_bands.h; the numpy twin is
// tests/sas_bands_zonal_reference.py.
//
// THE PROMISE (the whole specification).  Block (item, zone z) of window k is bit for bit what rh_sas_bands_configure records for that item
// with mask = (zone == z) & mask, the same weights, probabilities and windows and obs = obs[item][z]: rows [k][item][z][probability], hdr
// [k][item][z]{m, n_nan, W}, obs_pair [k][item][z]{below, equal}.  Everything in THE RULE of rh_sas_bands.h holds per zone: the clock and the
// windows, BULK / MEAN / LAST, s + 0.0, a NaN counted in n_nan and taking no further part, +-inf as values, T = clamp((int64)ceil(p *
// (double)W), 1, W) and the smallest s whose cumulative weight reaches T.  A zone with m == 0 gives NaN rows, W = 0 and, with an observation
// that is not missing, the pair (0, 0); a missing observation gives (-1, -1).  A column with zone == -1, mask == 0 or weight 0 loads and
// stores nothing and is in no zone's counts.
//
// THE LAUNCHES.  k_sas_bands_day runs unchanged: at configure the host folds zone >= 0 into the byte mask it tests.  Column lists: a stable
// counting sort on the host over the PARTICIPATING columns only (zone >= 0, mask != 0, weight != 0): zone_off [n_zones + 1] and zone_cols
// (int32 column indices, ascending within a zone), uploaded once.  On a closing day, behind k_sas_bands_day, in stream order:
//   k_sas_bands_zonal<WEIGHTED>  grid (n_zones, n_items), in place of the twelve k_sas_bands_hist<P> / k_sas_bands_pick<P>.  A workgroup
//                     walks its zone's list, eight columns in flight per thread, gathers keys[j * n + col] and, WEIGHTED, weight[col], and
//                     runs all six digit passes of BandsPass<P> itself: uint32 LDS histograms [probability][2048], pass 0 shared by the
//                     probabilities and yielding m, n_nan and W; a wavefront per probability widens the bins to 64 bit and picks the
//                     digit over 64-bit cumulative sums (select_pick_step); prefixes and ranks stay in LDS between the passes.  The later passes read
//                     the keys again: L2 serves them.  It writes its block of rows[k] and hdr[k].
//   k_sas_bands_obs_zonal  grid (n_zones, n_items), only when observations are configured and window k has one.  A workgroup whose
//                     observation is NaN ends after its scalar loads: the pair stays (-1, -1), written at configure.  Otherwise it walks
//                     the list and adds 1 or w_i into two int64 registers by the unsigned comparison with key(o + 0.0), reduces by
//                     shuffles and through LDS and stores the pair.
// A closing day is 1 + 1 (+ 1) launches instead of 13 (15).  LDS atomics only: no device-scope atomic, no completion counter, no spin; stream
// order stands where the plain path has its kernel boundaries.
//
// THE LDS BOUND, enforced at configure.  A uint32 bin holds at most (participating columns of the zone) x 65535, so with a weight plane a
// zone has at most RH_SELECT_W_MAX_TILES x RH_SELECT_BLOCK = 65536 participating columns (65536 x 65535 < 2^32, rh_select.h asserts it);
// a larger zone is refused and belongs to the plain configuration's mask.  Without weights any zone size below 2^31 is exact.
// LOAD BALANCE.  ONE workgroup walks a zone, however large: the largest zone sets the closing day's time.  A map with one dominant zone
// belongs to the plain configuration's mask, whose selection strides over the whole device.
// Bytes on a closing day, per item and participating column: six passes x (4 B list entry + 8 B key gathered + 2 B weight gathered); with
// observations one pass more.
#pragma once
#include "rh_sas_bands.h"

#define SAS_BANDS_ZONAL_MAX_WEIGHTED ((long long)RH_SELECT_W_MAX_TILES * RH_SELECT_BLOCK)   // participating columns of a weighted zone

struct SasBandsZonalDev {
    const long long *zone_off;   // [n_zones + 1]
    const int *zone_cols;        // the participating columns, ascending within a zone
};

// Pass PASS of one (zone, item) workgroup over the list entries [beg, end): the histograms, then the pick.  s_cnt: {numbers, NaNs} of
// pass 0; s_count: {m, n_nan, W} fixed by pass 0.
template <int PASS, bool WEIGHTED>
RH_SELECT_DEV void sas_bands_zonal_pass(const unsigned long long *keys, const unsigned short *wts, const int *cols, long long beg, long long end, int np,
                                        const double *probs, unsigned *hist, unsigned long long *s_prefix, long long *s_rank, long long *s_count, unsigned *s_cnt) {
    constexpr int NB = BandsPass<PASS>::nb, NC = NB / 64;
    const int nh = PASS == 0 ? 1 : np;
    for (int b = threadIdx.x; b < nh * NB; b += RH_SELECT_BLOCK) hist[b] = 0;
    if (PASS == 0 && threadIdx.x == 0) s_cnt[0] = s_cnt[1] = 0;
    __syncthreads();
    unsigned long long pre[RH_SAS_BANDS_MAX_PROBS];
#pragma unroll
    for (int q = 0; q < RH_SAS_BANDS_MAX_PROBS; ++q) pre[q] = (PASS > 0 && q < np) ? s_prefix[q] : 0ull;
    unsigned mine = 0, mine_nan = 0;   // pass 0: the numbers and the NaNs this thread met
    select_walk_list<WEIGHTED>(keys, wts, cols, beg, end, [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<PASS>(key, w, np, pre, hist, mine, mine_nan); });
    if (PASS == 0 && mine) atomicAdd(&s_cnt[0], mine);
    if (PASS == 0 && mine_nan) atomicAdd(&s_cnt[1], mine_nan);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < np; q += RH_SELECT_BLOCK / 64) {   // (uniform over the wavefront)
        const unsigned *h = hist + (PASS == 0 ? 0 : q) * NB;
        unsigned long long v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = (unsigned long long)h[c * 64 + lane];
        const SelectPick pk = select_pick_step<PASS>(v, probs[q], &s_prefix[q], &s_rank[q]);   // (pass 0: the rank is T - 1)
        if (lane == 0) {
            s_prefix[q] = pk.prefix;
            s_rank[q] = pk.rank;
            if (PASS == 0 && q == 0) {
                s_count[0] = (long long)s_cnt[0];
                s_count[1] = (long long)s_cnt[1];
                s_count[2] = pk.total;
            }
        }
    }
    __syncthreads();   // (the next pass clears the histograms and reads the prefixes)
}

template <bool WEIGHTED>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_zonal(const SasBandsDev *__restrict__ P, SasBandsZonalDev Z, int64_t k) {
    __shared__ unsigned hist[RH_SAS_BANDS_MAX_PROBS * RH_SELECT_NBINS];
    __shared__ unsigned long long s_prefix[RH_SAS_BANDS_MAX_PROBS];
    __shared__ long long s_rank[RH_SAS_BANDS_MAX_PROBS], s_count[SAS_BANDS_HDR];
    __shared__ unsigned s_cnt[2];
    const int z = blockIdx.x, j = blockIdx.y, nz = gridDim.x, ni = gridDim.y, np = P->n_probs;
    const long long beg = Z.zone_off[z], end = Z.zone_off[z + 1];
    const unsigned long long *keys = P->keys + (size_t)j * (size_t)P->n;
    const unsigned short *wts = P->weight;
    const int *cols = Z.zone_cols;
    const double *probs = P->probs;
    const size_t block = ((size_t)k * ni + j) * nz + z;
    double *out = P->rows + block * np;
    long long *hd = P->hdr + block * SAS_BANDS_HDR;
    sas_bands_zonal_pass<0, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    const long long m = s_count[0];
    if (threadIdx.x == 0) {
        hd[0] = m;
        hd[1] = s_count[1];
        hd[2] = s_count[2];
    }
    if (m == 0) {   // (uniform over the workgroup)
        if ((int)threadIdx.x < np) out[threadIdx.x] = __builtin_nan("");
        return;
    }
    sas_bands_zonal_pass<1, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    sas_bands_zonal_pass<2, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    sas_bands_zonal_pass<3, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    sas_bands_zonal_pass<4, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    sas_bands_zonal_pass<5, WEIGHTED>(keys, wts, cols, beg, end, np, probs, hist, s_prefix, s_rank, s_count, s_cnt);
    if ((int)threadIdx.x < np) out[threadIdx.x] = bands_value_of(s_prefix[threadIdx.x]);   // after the last pass the prefix IS the key
}

// where the observation falls, per zone: obs is [item][zone][sample]
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_obs_zonal(const SasBandsDev *__restrict__ P, SasBandsZonalDev Z, int64_t k) {
    __shared__ long long s_part[RH_SELECT_BLOCK / 64][2];
    const int z = blockIdx.x, j = blockIdx.y, nz = gridDim.x, ni = gridDim.y;
    const double o = P->obs[((size_t)j * nz + z) * (size_t)P->n_samples + (size_t)k];
    if (o != o) return;   // (uniform over the workgroup)
    const unsigned long long ko = bands_key_of(o + 0.0);
    const long long beg = Z.zone_off[z], end = Z.zone_off[z + 1];
    const unsigned long long *keys = P->keys + (size_t)j * (size_t)P->n;
    const unsigned short *wts = P->weight;   // (uniform: tested once, outside the walk)
    const int *cols = Z.zone_cols;
    long long below = 0, equal = 0;   // (below 2^47: fewer than 2^31 columns of weight <= 65535)
    const auto add = [&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_pair_add(key, w, ko, below, equal); };
    if (wts)
        select_walk_list<true>(keys, wts, cols, beg, end, add);
    else
        select_walk_list<false>(keys, wts, cols, beg, end, add);
    select_pair_reduce(below, equal, s_part);
    if (threadIdx.x == 0) {
        long long *out = P->obs_pair + (((size_t)k * ni + j) * nz + z) * 2;
        out[0] = below;
        out[1] = equal;
    }
}
