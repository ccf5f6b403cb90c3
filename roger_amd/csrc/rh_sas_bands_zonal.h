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
//                     the keys again: L2 serves them.  It writes its block of rows[k] and hdr[k].  The pass body is select_lds_pass<P> /
//                     select_lds_block of rh_select.h, which k_sas_age_bands (rh_sas_age_bands.h) runs over a contiguous run.
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

// One (zone, item) workgroup: the whole selection in its own LDS (select_lds_block of rh_select.h) over the zone's list entries.
template <bool WEIGHTED>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_bands_zonal(const SasBandsDev *__restrict__ P, SasBandsZonalDev Z, int64_t k) {
    RH_SELECT_LDS(L);
    const int z = blockIdx.x, j = blockIdx.y, nz = gridDim.x, ni = gridDim.y, np = P->n_probs;
    const long long beg = Z.zone_off[z], end = Z.zone_off[z + 1];
    const unsigned long long *keys = P->keys + (size_t)j * (size_t)P->n;
    const unsigned short *wts = P->weight;
    const int *cols = Z.zone_cols;
    const size_t block = ((size_t)k * ni + j) * nz + z;
    select_lds_block([&](auto body) RH_SELECT_BODY { select_walk_list<WEIGHTED>(keys, wts, cols, beg, end, body); }, np, P->probs, L, P->rows + block * np,
                     P->hdr + block * SAS_BANDS_HDR);
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
