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

void rh_sas_age_launch(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys,
                       const unsigned short *wts_c, const double *probs, int np, double *rows, long long *hdr) {
    const dim3 tiles((unsigned)((n_part + SAS_AGE_TILE - 1) / SAS_AGE_TILE), (unsigned)((W + SAS_AGE_TILE - 1) / SAS_AGE_TILE));
    hipLaunchKernelGGL(k_sas_age_keys, tiles, dim3(RH_SELECT_BLOCK), 0, stream, A, W, part_cols, n_part, keys);
    if (wts_c)
        hipLaunchKernelGGL(k_sas_age_bands<true>, dim3((unsigned)W), dim3(RH_SELECT_BLOCK), 0, stream, (const unsigned long long *)keys, wts_c, n_part, probs, np,
                           rows, hdr);
    else
        hipLaunchKernelGGL(k_sas_age_bands<false>, dim3((unsigned)W), dim3(RH_SELECT_BLOCK), 0, stream, (const unsigned long long *)keys, wts_c, n_part, probs, np,
                           rows, hdr);
}
#endif   // RH_SAS_AGE_UNIT
