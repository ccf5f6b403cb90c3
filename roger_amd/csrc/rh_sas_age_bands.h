// rh_sas_age_bands.h -- transport bands by age (rh_sas_age_bands_*, include/roger_hip_sas.h): the exact quantiles of rh_sas_bands.h ACROSS
// the columns for every age class of an age-resolved array -- the 5 - 50 - 95 % band of the travel time distribution TT_q_ss(T) or of the
// storage by age sa_s(T) over the behavioural sets of a SAS parameter study -- without downloading the (n, ages) array.  rh_sas.hip includes
// it for the constants and the rh_sas_age_launch_* functions; rh_sas_age.hip defines RH_SAS_AGE_UNIT and holds the kernels.  The numpy twin is
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
// Clock and windows are SasWindows, as for the scores and the bands, with an own count of recorded days from 0 at configure.  These calls
// record a SNAPSHOT and stay LAST-only: only RH_SAS_SCORES_LAST with weight -1 is accepted, and work is enqueued on the closing day of an
// open window only.  The window means (BULK / MEAN) are an observer of their own, rh_sas_age_window_bands_*: WINDOW MEANS below.
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
//
// WINDOW MEANS (rh_sas_age_window_bands_*; the numpy twin is tests/sas_age_window_bands_reference.py).  One more promise and nothing
// restated: block (item j, [zone z,] age class a) of window k is bit for bit what THE RULE of rh_sas_bands.h records for the width-1 values
// A_j[:, a] with the same item weight and kind -- BULK by a daily flux input, or MEAN -- under the same mask, weights, probabilities and
// windows; with zones, mask = (zone == z) & mask.  Per participating column, age class and recorded day of an open window: wd is the
// column's value in row `day` of the daily weight (BULK) or 1.0 (MEAN); eligible iff wd > 0 && v == v; num = num + fl(v * wd), den = den + wd,
// one IEEE operation each; both restart from +0.0 on the window's first day, eligible or not; on the closing day
// s = den > 0 ? num / den : NaN, then s + 0.0; a NaN s is counted in that block's n_nan.  den is per ELEMENT: a NaN in one age class on one
// day must not touch its neighbours.  The observer has its own SasWindows (accumulate = true), key plane, participating set and result: it
// may be configured beside the snapshot observer.  Per item acc = num [n_part][W_j], den [n_part][W_j] in participating order (zone order
// under zones), the age axis contiguous as in the source rows, indexed in size_t (n_part x W passes 2^31 at 10^7 x 1001), zero at configure.
//   k_sas_age_acc<BULK>           every day of an open window that does not close it: grid (ceil(n_part / 4)), 256 threads, a wavefront per
//                      column, lanes along the age axis: source, num and den are unit stride and the column's wd is read once.  An
//                      eligible element moves 8 B source + 16 B read + 16 B written; a first day reads no accumulator; wd <= 0 touches
//                      nothing, except that a first day stores the zeros without loading the source; an ineligible element of another day
//                      stores nothing.
//   k_sas_age_keys_window<BULK>   the closing day: k_sas_age_keys' transpose with the same tile, padding and guards, whose load side does
//                      the day's update in registers and forms s and the key; no accumulator is stored, the next window restarts.  24 B
//                      read (8 B on a one-day window) and 8 B written per element.
// Behind it the selection launches above, as they are (rh_sas_age_launch_select).  Stream order orders everything.
#pragma once
#include <hip/hip_runtime.h>

#include "rh_select.h"

#define SAS_AGE_TILE 64                                                                     // columns and age classes of a transpose tile
#define SAS_AGE_BANDS_MAX_WEIGHTED ((long long)RH_SELECT_W_MAX_TILES * RH_SELECT_BLOCK)   // participating cells under a weight plane
static_assert(RH_SELECT_BLOCK % SAS_AGE_TILE == 0, "a wavefront of the transpose is one row of a tile");

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

// The launches of one item on `stream`, each stated once; both observers (the snapshot's sas_age_bands_enqueue and the window means'
// sas_age_window_bands_enqueue of rh_sas_observers.h) fill a key plane and then call the ONE selection.  Defined in rh_sas_age.hip, the
// translation unit that holds the kernels below and is linked behind every other unit (LINK_LAST of roger_amd/build.py).  Why: with these
// kernels inside rh_sas.hip, `bench.py --model sas` with nothing configured lay above the parent's range in two sessions; in a unit of
// their own it lay within it in both alternation orders (DESIGN.md 3.9.3 gives the figures and what the control runs do and do not show).
//   rh_sas_age_launch_keys     the snapshot's transpose of A into keys [W][n_part] (part_cols in zone order under zones)
//   rh_sas_age_launch_select   the selection of the W age classes of a key plane into the item's blocks of the window: Z null, rows [W][np]
//                              and hdr [W][3] by k_sas_age_bands; else rows [n_zones][W][np] and hdr [n_zones][W][3] by
//                              k_sas_age_bands_zonal where there are long zones and k_sas_age_bands_small where there are short ones.
//                              wts_c null: every participating column counts 1
//   rh_sas_age_launch_window   a day of an open window of the window means (below): k_sas_age_acc, or on the closing day
//                              k_sas_age_keys_window into keys; wrow the day's row of the daily weight (BULK) or null (MEAN)
void rh_sas_age_launch_keys(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys);
void rh_sas_age_launch_select(hipStream_t stream, int W, long long n_part, const unsigned long long *keys, const unsigned short *wts_c, const SasAgeZones *Z,
                              const double *probs, int np, double *rows, long long *hdr);
void rh_sas_age_launch_window(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, const double *wrow, bool first, bool closes,
                              double *num, double *den, unsigned long long *keys);

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

// ---- window means (rh_sas_age_window_bands_*): num and den per participating column and age class, [n_part][W] each ----
// One update of an element, the words of k_sas_bands_day: eligible iff wd > 0 && v == v (the caller has tested wd); the product is rounded
// before it is added (-ffp-contract=off).
RH_SELECT_DEV bool sas_age_acc_add(double v, double wd, double &num, double &den) {
    const bool eligible = v == v;
    if (eligible) {
        const double t = v * wd;
        num = num + t;
        den = den + wd;
    }
    return eligible;
}

// A day of an open window that does not close it.  A wavefront per participating column i, lanes along the age axis: the source row
// A[part_cols[i]][...], num[i][...] and den[i][...] are unit stride, and the column's wd is read once.  wd <= 0 (or NaN): nothing is
// touched, unless the day is the window's first -- then the zeros are stored and the source is not loaded.  A first day reads no accumulator;
// an element that is not eligible on another day stores nothing.
template <bool BULK>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_acc(const double *__restrict__ A, int W, const int *__restrict__ part_cols, long long n_part,
                                                                 const double *__restrict__ wrow, int first, double *__restrict__ num,
                                                                 double *__restrict__ den) {
    const long long i = (long long)blockIdx.x * (RH_SELECT_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= n_part) return;   // (uniform over the wavefront)
    const int lane = threadIdx.x & 63, col = part_cols[i];
    const double wd = BULK ? wrow[col] : 1.0;
    const size_t at = (size_t)i * (size_t)W;
    double *pn = num + at, *pd = den + at;
    if (!(wd > 0.0)) {
        if (first)
            for (int a = lane; a < W; a += 64) pn[a] = pd[a] = 0.0;
        return;
    }
    const double *src = A + (size_t)col * (size_t)W;
#pragma unroll 4
    for (int a = lane; a < W; a += 64) {
        double n_ = 0.0, d_ = 0.0;
        if (!first) {
            n_ = pn[a];
            d_ = pd[a];
        }
        const bool eligible = sas_age_acc_add(src[a], wd, n_, d_);
        if (first || eligible) {
            pn[a] = n_;
            pd[a] = d_;
        }
    }
}

// The closing day: k_sas_age_keys' transpose -- the same tile, padding and guards on both edges -- whose load side does the day's update in
// registers, forms s = den > 0 ? num / den : NaN, then s + 0.0, and the key.  A row of a tile is a column and a wavefront, so wd is uniform
// over it.  No accumulator is stored: the next window restarts.
template <bool BULK>
__global__ __launch_bounds__(RH_SELECT_BLOCK) void k_sas_age_keys_window(const double *__restrict__ A, int W, const int *__restrict__ part_cols, long long n_part,
                                                                         const double *__restrict__ wrow, int first, const double *__restrict__ num,
                                                                         const double *__restrict__ den, unsigned long long *__restrict__ keys) {
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
            const int col = part_cols[i];
            const double wd = BULK ? wrow[col] : 1.0;
            const size_t at = (size_t)i * (size_t)W + (size_t)a;
            double n_ = 0.0, d_ = 0.0;
            if (!first) {
                n_ = num[at];
                d_ = den[at];
            }
            if (wd > 0.0) (void)sas_age_acc_add(A[(size_t)col * (size_t)W + (size_t)a], wd, n_, d_);
            const double s = (d_ > 0.0 ? n_ / d_ : __builtin_nan("")) + 0.0;
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

static dim3 sas_age_tiles(int W, long long n_part) {
    return dim3((unsigned)((n_part + SAS_AGE_TILE - 1) / SAS_AGE_TILE), (unsigned)((W + SAS_AGE_TILE - 1) / SAS_AGE_TILE));
}

void rh_sas_age_launch_keys(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, unsigned long long *keys) {
    hipLaunchKernelGGL(k_sas_age_keys, sas_age_tiles(W, n_part), dim3(RH_SELECT_BLOCK), 0, stream, A, W, part_cols, n_part, keys);
}

template <bool WEIGHTED>
static void sas_age_launch_select(hipStream_t stream, int W, long long n_part, const unsigned long long *keys, const unsigned short *wts_c, const SasAgeZones *Z,
                                  const double *probs, int np, double *rows, long long *hdr) {
    if (!Z)
        hipLaunchKernelGGL(k_sas_age_bands<WEIGHTED>, dim3((unsigned)W), dim3(RH_SELECT_BLOCK), 0, stream, keys, wts_c, n_part, probs, np, rows, hdr);
    if (Z && Z->n_long)
        hipLaunchKernelGGL(k_sas_age_bands_zonal<WEIGHTED>, dim3((unsigned)W, (unsigned)Z->n_long), dim3(RH_SELECT_BLOCK), 0, stream, keys, wts_c, n_part, *Z, probs,
                           np, rows, hdr);
    if (Z && Z->n_short)
        hipLaunchKernelGGL(k_sas_age_bands_small<WEIGHTED>, dim3((unsigned)W, (unsigned)Z->n_short), dim3(RH_SELECT_BLOCK), 0, stream, keys, wts_c, n_part, *Z, probs,
                           np, rows, hdr);
}

void rh_sas_age_launch_select(hipStream_t stream, int W, long long n_part, const unsigned long long *keys, const unsigned short *wts_c, const SasAgeZones *Z,
                              const double *probs, int np, double *rows, long long *hdr) {
    if (wts_c)
        sas_age_launch_select<true>(stream, W, n_part, keys, wts_c, Z, probs, np, rows, hdr);
    else
        sas_age_launch_select<false>(stream, W, n_part, keys, wts_c, Z, probs, np, rows, hdr);
}

template <bool BULK>
static void sas_age_launch_window(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, const double *wrow, bool first, bool closes,
                                  double *num, double *den, unsigned long long *keys) {
    if (closes)
        hipLaunchKernelGGL(k_sas_age_keys_window<BULK>, sas_age_tiles(W, n_part), dim3(RH_SELECT_BLOCK), 0, stream, A, W, part_cols, n_part, wrow, first ? 1 : 0,
                           (const double *)num, (const double *)den, keys);
    else
        hipLaunchKernelGGL(k_sas_age_acc<BULK>, dim3((unsigned)((n_part + RH_SELECT_BLOCK / 64 - 1) / (RH_SELECT_BLOCK / 64))), dim3(RH_SELECT_BLOCK), 0, stream, A, W,
                           part_cols, n_part, wrow, first ? 1 : 0, num, den);
}

void rh_sas_age_launch_window(hipStream_t stream, const double *A, int W, const int *part_cols, long long n_part, const double *wrow, bool first, bool closes,
                              double *num, double *den, unsigned long long *keys) {
    if (wrow)
        sas_age_launch_window<true>(stream, A, W, part_cols, n_part, wrow, first, closes, num, den, keys);
    else
        sas_age_launch_window<false>(stream, A, W, part_cols, n_part, wrow, first, closes, num, den, keys);
}
#endif   // RH_SAS_AGE_UNIT
