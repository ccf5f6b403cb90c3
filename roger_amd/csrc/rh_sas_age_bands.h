// rh_sas_age_bands.h -- transport bands by age (rh_sas_age_bands_*, include/roger_hip_sas.h): the exact quantiles of rh_sas_bands.h ACROSS
// the columns for every age class of an age-resolved array -- the 5 - 50 - 95 % band of the travel time distribution TT_q_ss(T) or of the
// storage by age sa_s(T) over the behavioural sets of a SAS parameter study -- without downloading the (n, ages) array.  rh_sas.hip includes
// it for the constants and rh_sas_age_launch; rh_sas_age.hip defines RH_SAS_AGE_UNIT and holds the kernels.  The numpy twin is
// tests/sas_age_bands_reference.py.
//
// THE RULE (one promise, the whole specification).  Block (item j, age class a) of window k -- rows [k][j][a][probability], hdr
// [k][j][a]{m, n_nan, W} -- is bit for bit what THE RULE of rh_sas_bands.h gives for the width-1 values A_j[:, a] under the same mask,
// weights and probabilities, with kind LAST:
//   s = v + 0.0 (so -0.0 becomes +0.0);
//   a NaN element is counted in THAT age class's n_nan and takes no further part; +-inf are ordinary values;
//   a column with mask == 0 or weight 0 loads and stores nothing;
//   T = clamp((int64)ceil(p * (double)W), 1, W), and the result is the smallest s with sum_{s_i <= s} w_i >= T;
//   m == 0 gives NaN rows and W = 0.
// m, n_nan and W are per age class: NaN patterns differ along the age axis.
// Clock and windows are SasWindows, as for the scores and the bands, with an own count of recorded days from 0 at configure.  The ABI takes
// an item kind so that window means can follow; only RH_SAS_SCORES_LAST with weight -1 is accepted today, and work is enqueued on the
// closing day of an open window only.  (BULK / MEAN need an (n, W) accumulator and a per-element den per item.)
//
// THE LAUNCHES.  At configure the host builds part_cols [n_part], the participating columns in ascending order, and the compacted weights
// wts_c [n_part] (wts_c[i] = weights[part_cols[i]]), and uploads both once.  On a closing day, per item, one after another on the
// context's stream, so that ONE key plane of Wmax x n_part x 8 B serves all items:
//   k_sas_age_keys     grid (ceil(n_part / 64), ceil(W_j / 64)), 256 threads: a transpose through LDS, tile 64 columns x 64 age classes,
//                      rows padded by one key against bank conflicts.  Reads A[part_cols[i]][a] with lanes along the age axis, which is
//                      contiguous in memory; writes keys[a][i] with lanes along i: unit stride on both sides.  The key is KEY_NAN for a NaN,
//                      else bands_key_of(v + 0.0).  Both edges are guarded: W_j and n_part need not be multiples of 64.
//   k_sas_age_bands<WEIGHTED>   grid (W_j), 256 threads: workgroup a walks the contiguous run keys[a][0 ... n_part) (select_walk_run, eight
//                      loads in flight per thread, the weight at the same index of wts_c) and runs all six digit passes in its own LDS
//                      (select_lds_block of rh_select.h, the pass body k_sas_bands_zonal runs); writes its block of rows[k] and hdr[k].
// LDS atomics only: no device-scope atomic, no completion counter, no spin; stream order orders the launches.
//
// THE LDS BOUND, enforced at configure.  A uint32 bin holds at most n_part x 65535, so with a weight plane at most RH_SELECT_W_MAX_TILES x
// RH_SELECT_BLOCK = 65536 cells take part (rh_select.h asserts 65536 x 65535 < 2^32).  Without weights any n < 2^31 is exact.
// LOAD BALANCE.  ONE workgroup walks an age class: a closing day's time grows with n_part, and W_j workgroups are in flight.
// Bytes on a closing day, per item, participating column and age class: 8 B read and 8 B written by the transpose, six passes x (8 B key
// + 2 B weight) by the selection (a run of 10^5 keys is 0.8 MB: the later passes are served by the caches).
//
// PER ZONE (rh_sas_age_bands_configure_zonal; the numpy twin is tests/sas_age_bands_zonal_reference.py).  One more promise: block (item j,
// zone z, age class a) -- rows [k][j][z][a][probability], hdr [k][j][z][a]{m, n_nan, W}, the zone axis in front of the age axis -- is bit for
// bit what the plain configuration records for item j and age class a with mask = (zone == z) & mask.  A column with zone == -1, mask == 0
// or weight 0 is in no zone's counts.  The host orders part_cols and wts_c by zone with a stable counting sort (ascending within a zone)
// and uploads zone_off [n_zones + 1], so that k_sas_age_keys, unchanged, writes a key plane whose row a holds zone z's keys as the
// contiguous run [zone_off[z], zone_off[z + 1]).  Per item at most three launches (SasAgeZones lists the zones of each):
//   k_sas_age_bands_zonal<WEIGHTED>   grid (W_j, long zones), 256 threads: the zones of more than SAS_AGE_SHORT_ZONE = 256 participating
//                      cells; select_walk_run over the zone's run and select_lds_block, as k_sas_age_bands: a shell, nothing restated.
//   k_sas_age_bands_small<WEIGHTED>   grid (W_j, short zones), 256 threads: the zones of 1 ... 256 cells.  A zone map multiplies the runs by
//                      up to 1024 and the six passes cost six clears of up to 64 KiB of LDS and six picks however short the run is; here a
//                      thread holds ONE key and weight (beyond the run's end KEY_MASKED and 0, so that such a thread counts in no
//                      reduction and is no candidate), both go to LDS, and behind one barrier c_t = sum of w_j over the run's members with
//                      key_j <= key_t, read as broadcasts (uint32: 256 x 65535 < 2^32).  m, n_nan and W by a workgroup reduction; per
//                      probability T - 1 = bands_rank_of(p, W) and the result is the minimum key over the threads with c_t >= T -- a
//                      shuffle minimum per wavefront, LDS across the four -- turned back by bands_value_of.  No histogram, no digit
//                      pass, 3376 B of LDS; the same promise and the same bits as the six passes.
// An empty zone is in neither list: its blocks keep the NaN rows and zero headers configure wrote.  THE BOUND is per zone: with a weight
// plane a ZONE of more than 65536 participating cells is refused; the total may be larger, which the plain configuration refuses.
#pragma once
#include <hip/hip_runtime.h>

#include "rh_select.h"

#define SAS_AGE_TILE 64                                                                     // columns and age classes of a transpose tile
#define SAS_AGE_BANDS_MAX_WEIGHTED ((long long)RH_SELECT_W_MAX_TILES * RH_SELECT_BLOCK)   // participating cells under a weight plane
static_assert(RH_SELECT_BLOCK % SAS_AGE_TILE == 0, "a wavefront of the transpose is one row of a tile");

// One item's two launches on `stream`: the transpose into keys [W][n_part], then the selection of the W age classes into the item's blocks
// rows [W][np] and hdr [W][3] of the window; wts_c null: every participating column counts 1.  Defined in rh_sas_age.hip, the translation
// unit that holds the kernels below and is linked behind every other unit (LINK_LAST of roger_amd/build.py).  Why: with these kernels
// inside rh_sas.hip, `bench.py --model sas` with nothing configured lay above the parent's range in two sessions; in a unit of their own
// it lay within it in both alternation orders (DESIGN.md 3.9.3 gives the figures and what the control runs do and do not show).
void rh_sas_age_launch(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys,
                       const unsigned short *wts_c, const double *probs, int np, double *rows, long long *hdr);

// Per zone: what the two kernels of a zonal configuration are told.  zone_off [n_zones + 1] into part_cols / wts_c / a row of the key plane,
// which are in zone order; the zones of 1 ... SAS_AGE_SHORT_ZONE participating cells and the longer ones (an empty zone is in neither list:
// its blocks keep what configure wrote).
struct SasAgeZones {
    const long long *zone_off;
    const int *short_zones, *long_zones;
    int n_short, n_long;
};
#ifndef SAS_AGE_SHORT_ZONE   // (tools/sas_age_bands_time.py builds a variant with 0: every zone through the six passes, to price the second path)
#define SAS_AGE_SHORT_ZONE RH_SELECT_BLOCK   // by construction, not tuned: one key per thread of k_sas_age_bands_small
#endif
static_assert(SAS_AGE_SHORT_ZONE <= RH_SELECT_BLOCK, "k_sas_age_bands_small holds one key per thread");
// One item's launches of a zonal configuration on `stream`: the transpose, unchanged, with part_cols in zone order; k_sas_age_bands_zonal
// where there are long zones, k_sas_age_bands_small where there are short ones; rows [n_zones][W][np] and hdr [n_zones][W][3] are the item's
// blocks of the window.
void rh_sas_age_launch_zonal(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys,
                             const unsigned short *wts_c, const SasAgeZones &Z, const double *probs, int np, double *rows, long long *hdr);

#ifdef RH_SAS_AGE_UNIT
// keys[a][i] = key(A[part_cols[i]][a] + 0.0) for i < n_part, a < W
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_keys(const double *__restrict__ A, int W, const int *__restrict__ part_cols, long long n_part,
                                                                  unsigned long long *__restrict__ keys) {
    __shared__ unsigned long long tile[SAS_AGE_TILE][SAS_AGE_TILE + 1];
    constexpr int ROWS = RH_SELECT_BLOCK / SAS_AGE_TILE;   // rows of a tile per trip
    const long long i0 = (long long)blockIdx.x * SAS_AGE_TILE;
    const int a0 = (int)blockIdx.y * SAS_AGE_TILE, lane = threadIdx.x % SAS_AGE_TILE, row = threadIdx.x / SAS_AGE_TILE;
#pragma unroll
    for (int t = 0; t < SAS_AGE_TILE / ROWS; ++t) {   // column i0 + r, lanes along the age axis
        const int r = row + t * ROWS;
        const long long i = i0 + r;
        const int a = a0 + lane;
        if (i < n_part && a < W) {
            const double s = A[(size_t)part_cols[i] * (size_t)W + (size_t)a] + 0.0;
            tile[r][lane] = s != s ? RH_SELECT_KEY_NAN : bands_key_of(s);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < SAS_AGE_TILE / ROWS; ++t) {   // age class a0 + r, lanes along the columns
        const int r = row + t * ROWS;
        const long long i = i0 + lane;
        const int a = a0 + r;
        if (a < W && i < n_part) keys[(size_t)a * (size_t)n_part + (size_t)i] = tile[lane][r];
    }
}

// workgroup a: the selection over keys[a][0 ... n_part); rows and hdr are the item's blocks of window k, [W][n_probs] and [W][3]
template <bool WEIGHTED>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_bands(const unsigned long long *__restrict__ keys, const unsigned short *__restrict__ wts_c,
                                                                   long long n_part, const double *__restrict__ probs, int np, double *__restrict__ rows,
                                                                   long long *__restrict__ hdr) {
    RH_SELECT_LDS(L);
    const size_t a = blockIdx.x;
    const unsigned long long *run = keys + a * (size_t)n_part;
    select_lds_block([&](auto body) RH_SELECT_BODY { select_walk_run<WEIGHTED>(run, wts_c, n_part, body); }, np, probs, L, rows + a * (size_t)np,
                     hdr + a * RH_SELECT_HDR);
}

// ---- per zone (rh_sas_age_bands_configure_zonal): one run of the key plane per (age class, zone) ----
// workgroup (a, l): the selection over the run keys[a][zone_off[z] ... zone_off[z + 1]) of zone z = long_zones[l]; rows and hdr are the
// item's blocks of window k, [n_zones][W][n_probs] and [n_zones][W][3], W = gridDim.x
template <bool WEIGHTED>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_bands_zonal(const unsigned long long *__restrict__ keys, const unsigned short *__restrict__ wts_c,
                                                                         long long n_part, SasAgeZones Z, const double *__restrict__ probs, int np,
                                                                         double *__restrict__ rows, long long *__restrict__ hdr) {
    RH_SELECT_LDS(L);
    const size_t a = blockIdx.x, z = (size_t)Z.long_zones[blockIdx.y], block = z * gridDim.x + a;
    const long long beg = Z.zone_off[z], len = Z.zone_off[z + 1] - beg;
    const unsigned long long *run = keys + a * (size_t)n_part + (size_t)beg;
    const unsigned short *wts = WEIGHTED ? wts_c + beg : nullptr;
    select_lds_block([&](auto body) RH_SELECT_BODY { select_walk_run<WEIGHTED>(run, wts, len, body); }, np, probs, L, rows + block * (size_t)np,
                     hdr + block * RH_SELECT_HDR);
}

// the sum of x over the workgroup, in every thread: shuffles within a wavefront, LDS across the RH_SELECT_BLOCK / 64 of them
RH_SELECT_DEV unsigned sas_age_block_sum(unsigned x, unsigned *s_part) {
    for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    x = 0;
#pragma unroll
    for (int w = 0; w < RH_SELECT_BLOCK / 64; ++w) x += s_part[w];
    return x;
}

// workgroup (a, l): zone z = short_zones[l] has 1 ... RH_SELECT_BLOCK participating cells, so a thread holds ONE key of the run and the
// selection needs no histogram and no digit pass: c_t, the weight of the members at or below thread t's key, is formed from the run in LDS
// (every lane of a read asks for the same address: a broadcast), and the result of a probability is the smallest key with c_t >= T.  The
// same promise and the same bits as select_lds_block: T - 1 is bands_rank_of(p, W), the value is bands_value_of(key).
template <bool WEIGHTED>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_bands_small(const unsigned long long *__restrict__ keys, const unsigned short *__restrict__ wts_c,
                                                                         long long n_part, SasAgeZones Z, const double *__restrict__ probs, int np,
                                                                         double *__restrict__ rows, long long *__restrict__ hdr) {
    __shared__ unsigned long long s_key[RH_SELECT_BLOCK], s_min[RH_SELECT_MAX_PROBS][RH_SELECT_BLOCK / 64];
    __shared__ unsigned s_w[RH_SELECT_BLOCK], s_part[3][RH_SELECT_BLOCK / 64];
    const size_t a = blockIdx.x, z = (size_t)Z.short_zones[blockIdx.y], block = z * gridDim.x + a;
    const long long beg = Z.zone_off[z];
    const int len = (int)(Z.zone_off[z + 1] - beg), t = (int)threadIdx.x;   // 1 ... RH_SELECT_BLOCK
    const bool in = t < len;
    const unsigned long long key = in ? keys[a * (size_t)n_part + (size_t)(beg + t)] : RH_SELECT_KEY_MASKED;
    const unsigned w = in ? (WEIGHTED ? (unsigned)wts_c[beg + t] : 1u) : 0u;
    s_key[t] = key;
    s_w[t] = w;
    __syncthreads();
    const bool number = key < RH_SELECT_KEY_NAN;
    unsigned c = 0;   // at most RH_SELECT_BLOCK x 65535 < 2^32
#pragma unroll 4
    for (int j = 0; j < len; ++j) {   // (the run's members only; the padding beyond its end is for the three reductions below)
        const unsigned long long kj = s_key[j];
        c += (kj <= key && kj < RH_SELECT_KEY_NAN) ? s_w[j] : 0u;
    }
    const unsigned m = sas_age_block_sum(number ? 1u : 0u, s_part[0]), n_nan = sas_age_block_sum(key == RH_SELECT_KEY_NAN ? 1u : 0u, s_part[1]),
                   total = sas_age_block_sum(number ? w : 0u, s_part[2]);
    if (t == 0) {
        hdr[block * RH_SELECT_HDR] = (long long)m;
        hdr[block * RH_SELECT_HDR + 1] = (long long)n_nan;
        hdr[block * RH_SELECT_HDR + 2] = (long long)total;
    }
    double *out = rows + block * (size_t)np;
    if (m == 0) {   // (uniform over the workgroup)
        if (t < np) out[t] = __builtin_nan("");
        return;
    }
    for (int q = 0; q < np; ++q) {
        const long long r = bands_rank_of(probs[q], (long long)total);   // T - 1
        unsigned long long best = (number && (long long)c > r) ? key : RH_SELECT_KEY_MASKED;
        for (int off = 32; off; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off);
            best = other < best ? other : best;
        }
        if ((t & 63) == 0) s_min[q][t >> 6] = best;
    }
    __syncthreads();
    if (t < np) {
        unsigned long long best = s_min[t][0];
#pragma unroll
        for (int wv = 1; wv < RH_SELECT_BLOCK / 64; ++wv) best = s_min[t][wv] < best ? s_min[t][wv] : best;
        out[t] = bands_value_of(best);
    }
}

static void sas_age_launch_keys(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys) {
    const dim3 tiles((unsigned)((n_part + SAS_AGE_TILE - 1) / SAS_AGE_TILE), (unsigned)((W + SAS_AGE_TILE - 1) / SAS_AGE_TILE));
    hipLaunchKernelGGL(k_sas_age_keys, tiles, dim3(RH_SELECT_BLOCK), 0, stream, A, W, part_cols, n_part, keys);
}

void rh_sas_age_launch(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys,
                       const unsigned short *wts_c, const double *probs, int np, double *rows, long long *hdr) {
    sas_age_launch_keys(stream, A, W, part_cols, n_part, keys);
    if (wts_c)
        hipLaunchKernelGGL(k_sas_age_bands<true>, dim3((unsigned)W), dim3(RH_SELECT_BLOCK), 0, stream, (const unsigned long long *)keys, wts_c, n_part, probs, np,
                           rows, hdr);
    else
        hipLaunchKernelGGL(k_sas_age_bands<false>, dim3((unsigned)W), dim3(RH_SELECT_BLOCK), 0, stream, (const unsigned long long *)keys, wts_c, n_part, probs, np,
                           rows, hdr);
}

template <bool WEIGHTED>
static void sas_age_launch_zones(hipStream_t stream, int W, long long n_part, const unsigned long long *keys, const unsigned short *wts_c, const SasAgeZones &Z,
                                 const double *probs, int np, double *rows, long long *hdr) {
    if (Z.n_long)
        hipLaunchKernelGGL(k_sas_age_bands_zonal<WEIGHTED>, dim3((unsigned)W, (unsigned)Z.n_long), dim3(RH_SELECT_BLOCK), 0, stream, keys, wts_c, n_part, Z, probs,
                           np, rows, hdr);
    if (Z.n_short)
        hipLaunchKernelGGL(k_sas_age_bands_small<WEIGHTED>, dim3((unsigned)W, (unsigned)Z.n_short), dim3(RH_SELECT_BLOCK), 0, stream, keys, wts_c, n_part, Z, probs,
                           np, rows, hdr);
}

void rh_sas_age_launch_zonal(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys,
                             const unsigned short *wts_c, const SasAgeZones &Z, const double *probs, int np, double *rows, long long *hdr) {
    sas_age_launch_keys(stream, A, W, part_cols, n_part, keys);
    if (wts_c)
        sas_age_launch_zones<true>(stream, W, n_part, keys, wts_c, Z, probs, np, rows, hdr);
    else
        sas_age_launch_zones<false>(stream, W, n_part, keys, wts_c, Z, probs, np, rows, hdr);
}
#endif   // RH_SAS_AGE_UNIT
