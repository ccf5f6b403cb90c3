// rh_sas_totals.h -- catchment totals of the SAS context (rh_sas_totals_*, include/roger_hip_sas.h): the kernels that reduce one row, and
// what the host tells them.  Included by rh_sas.hip only; the day kernels know nothing of it.
//
// An item is (array, weight).  Its block of a row is [wsum, count, sum, min, max] for a width-1 array and [wsum, count, sum[0 ... W)]
// for an age-resolved one; which cells count, and the ORDER of every sum, are stated in the header.  Two kinds of launch:
//
//   k_sas_totals_tiles / k_sas_totals_finish   every item's five width-1 statistics (for an age item: wsum and count only).  Lanes run
//       along cells: the wavefront tree with strides 32 ... 1, (w0 + w1) + (w2 + w3) per tile of 256 cells, the tiles' partials as
//       plain stores into part [item][stat][tile]; the finish kernel -- one workgroup per item -- strides them over 256 accumulators
//       in increasing order and takes the same two levels.  This is the order of k_totals_tiles / k_totals_finish (rh_control.h).
//       SAS_TOTALS_CHUNK items' values and weights are loaded before the first of them is reduced.
//   k_sas_totals_ages                          one age item, one level: a workgroup per (run of 256 consecutive cells, chunk of up to
//       256 ages).  Lanes run along the AGE axis, which is contiguous: every global load is unit stride and no sum crosses lanes.
//       A thread adds its age class of the run's cells left to right, starting from +0.0; the run's mask bytes and weights are
//       staged in LDS once, a cell that is not eligible is skipped by a wave-uniform branch (its row is not loaded) and contributes
//       +0.0, SAS_TOTALS_BATCH rows are in flight ahead of the ordered adds.  Level 1 (FIRST) reads the array with non-temporal
//       loads -- it is read once -- applies weight and NaN rule and writes partials [run][age]; the further levels are the same kernel
//       on the partials, plain sums, until one run is left, which lands in the ring's row.
//       (A running sum that starts at +0.0 is never -0.0, so adding a skipped cell's +0.0 and skipping the add are the same bits.)
//
// Scratch, sized at configure: part is items x 5 x tiles float64 (10^6 cells, 32 items: 5 MB); the age levels share two buffers of
// runs x Wmax and ceil(runs / 256) x Wmax float64 -- at 10^6 cells x 1000 ages 31 MB + 0.13 MB -- that the age items use one after
// another (the stream orders them).  No floating-point atomics, no counter on the device: row number and ring slot are the host's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "roger_hip_sas.h"

#define SAS_TOTALS_BLOCK 256
#define SAS_TOTALS_RUN 256     // cells per run of the age rule
#define SAS_TOTALS_NSTAT 5     // wsum, count, sum, min, max
#define SAS_TOTALS_CHUNK 4     // items loaded before the first is reduced (k_sas_totals_tiles)
#define SAS_TOTALS_BATCH 8     // rows in flight per thread (k_sas_totals_ages)

struct SasTotalsDev {
    const double *val[RH_SAS_TOTALS_MAX_ITEMS];     // width-1 value (a DAILY input: its first row); null: an age item
    const double *wgt[RH_SAS_TOTALS_MAX_ITEMS];     // first row of the DAILY weight; null: none
    int64_t off[RH_SAS_TOTALS_MAX_ITEMS];           // first element of the item's block in a row
    unsigned char val_daily[RH_SAS_TOTALS_MAX_ITEMS];
    int n_items, ntiles;
    int64_t n;
    const unsigned char *mask;                      // [n] or null
    double *part;                                   // [item][stat][tile]
};

__device__ __forceinline__ double sas_totals_identity(int stat) {
    return stat < 3 ? 0.0 : (stat == 3 ? __builtin_huge_val() : -__builtin_huge_val());
}
__device__ __forceinline__ double sas_totals_op(int stat, double x, double y) { return stat < 3 ? x + y : (stat == 3 ? fmin(x, y) : fmax(x, y)); }
template <int STAT>
__device__ __forceinline__ double sas_totals_wave(double x) {
    for (int off = 32; off; off >>= 1) x = sas_totals_op(STAT, x, __shfl_xor(x, off));
    return x;
}
// (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double sas_totals_four(int stat, const double *p) {
    return sas_totals_op(stat, sas_totals_op(stat, p[0], p[1]), sas_totals_op(stat, p[2], p[3]));
}

// day_off: (day mod forcing_days) * n, or -1 for "no daily row": an item with a weight or a DAILY value then has no eligible cell
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_totals_tiles(const SasTotalsDev *__restrict__ P, int64_t day_off) {
    __shared__ double part[RH_SAS_TOTALS_MAX_ITEMS * SAS_TOTALS_NSTAT][SAS_TOTALS_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * SAS_TOTALS_BLOCK + threadIdx.x;
    const int ni = P->n_items, wave = threadIdx.x >> 6;
    const unsigned char *mask = P->mask;
    const bool inside = i < P->n && (!mask || __builtin_nontemporal_load(mask + i) != 0);
    for (int j0 = 0; j0 < ni; j0 += SAS_TOTALS_CHUNK) {
        double v[SAS_TOTALS_CHUNK], w[SAS_TOTALS_CHUNK];
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_CHUNK; ++k) {
            v[k] = 0.0;
            w[k] = 0.0;      // (not eligible)
            const int j = j0 + k;
            if (j >= ni || !inside) continue;
            const double *pv = P->val[j], *pw = P->wgt[j];
            const bool daily = P->val_daily[j] != 0;
            if ((pw || daily) && day_off < 0) continue;
            w[k] = pw ? __builtin_nontemporal_load(pw + day_off + i) : 1.0;
            if (pv) v[k] = __builtin_nontemporal_load(pv + (daily ? day_off : 0) + i);
        }
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_CHUNK; ++k) {
            const int j = j0 + k;
            if (j >= ni) break;
            const bool counted = w[k] > 0.0 && v[k] == v[k];          // (a NaN weight is not > 0)
            const double t = P->wgt[j] ? v[k] * w[k] : v[k];          // rounded before it is added (-ffp-contract=off)
            const double ws = sas_totals_wave<0>(counted ? w[k] : 0.0);
            const double cn = sas_totals_wave<1>(counted ? 1.0 : 0.0);
            const double sm = sas_totals_wave<2>(counted ? t : 0.0);
            const double lo = sas_totals_wave<3>(counted ? v[k] : sas_totals_identity(3));
            const double hi = sas_totals_wave<4>(counted ? v[k] : sas_totals_identity(4));
            if ((threadIdx.x & 63) == 0) {
                double(*q)[SAS_TOTALS_BLOCK / 64] = part + j * SAS_TOTALS_NSTAT;
                q[0][wave] = ws;
                q[1][wave] = cn;
                q[2][wave] = sm;
                q[3][wave] = lo;
                q[4][wave] = hi;
            }
        }
    }
    __syncthreads();
    const int ntiles = P->ntiles;
    for (int q = threadIdx.x; q < ni * SAS_TOTALS_NSTAT; q += SAS_TOTALS_BLOCK)
        P->part[(size_t)q * ntiles + blockIdx.x] = sas_totals_four(q % SAS_TOTALS_NSTAT, part[q]);
}

// one workgroup per item: the tiles' partials into the item's block of the row
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_totals_finish(const SasTotalsDev *__restrict__ P, double *__restrict__ row) {
    __shared__ double part[SAS_TOTALS_NSTAT][SAS_TOTALS_BLOCK / 64];
    const int j = (int)blockIdx.x, ntiles = P->ntiles;
    const double *src = P->part + (size_t)j * SAS_TOTALS_NSTAT * ntiles;
    constexpr int PT = 4;   // rounds of partials loaded before the first is added: a thread's loads are independent, its adds ordered
    double x[SAS_TOTALS_NSTAT];
#pragma unroll
    for (int s = 0; s < SAS_TOTALS_NSTAT; ++s) x[s] = sas_totals_identity(s);
    for (int t0 = threadIdx.x; t0 < ntiles; t0 += PT * SAS_TOTALS_BLOCK) {
        double v[SAS_TOTALS_NSTAT][PT];
#pragma unroll
        for (int s = 0; s < SAS_TOTALS_NSTAT; ++s)
#pragma unroll
            for (int k = 0; k < PT; ++k) {
                const int t = t0 + k * SAS_TOTALS_BLOCK;
                v[s][k] = t < ntiles ? src[(size_t)s * ntiles + t] : 0.0;
            }
#pragma unroll
        for (int k = 0; k < PT; ++k)   // in increasing tile order
            if (t0 + k * SAS_TOTALS_BLOCK < ntiles) {
#pragma unroll
                for (int s = 0; s < SAS_TOTALS_NSTAT; ++s) x[s] = sas_totals_op(s, x[s], v[s][k]);
            }
    }
    const double r0 = sas_totals_wave<0>(x[0]), r1 = sas_totals_wave<1>(x[1]), r2 = sas_totals_wave<2>(x[2]);
    const double r3 = sas_totals_wave<3>(x[3]), r4 = sas_totals_wave<4>(x[4]);
    if ((threadIdx.x & 63) == 0) {
        const int wave = threadIdx.x >> 6;
        part[0][wave] = r0;
        part[1][wave] = r1;
        part[2][wave] = r2;
        part[3][wave] = r3;
        part[4][wave] = r4;
    }
    __syncthreads();
    const int nstat = P->val[j] ? SAS_TOTALS_NSTAT : 2;   // an age item: wsum and count, its sums follow from k_sas_totals_ages
    if ((int)threadIdx.x < nstat) row[P->off[j] + threadIdx.x] = sas_totals_four((int)threadIdx.x, part[threadIdx.x]);
}

// One level of the age rule.  src is (n, W); run b = blockIdx.x holds the cells [256 b, 256 b + 256); thread -> age class
// blockIdx.y * blockDim.x + threadIdx.x; dst[b * W + age] = the run's sum.  FIRST: src is the array itself, `mask` ([n] or null) and `wgt`
// (the day's row of the weight or null) select the cells, `live` == 0 makes every cell ineligible (day < 0 with a weight).
template <bool FIRST>
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_totals_ages(const double *__restrict__ src, int64_t n, int W,
                                                                      const unsigned char *__restrict__ mask, const double *__restrict__ wgt,
                                                                      int live, double *__restrict__ dst) {
    __shared__ double s_w[SAS_TOTALS_RUN];
    __shared__ int s_e[SAS_TOTALS_RUN];
    const int64_t c0 = (int64_t)blockIdx.x * SAS_TOTALS_RUN;
    const int m = (int)(n - c0 < SAS_TOTALS_RUN ? n - c0 : SAS_TOTALS_RUN);
    const int a = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    const bool act = a < W;
    if (FIRST) {
        for (int k = threadIdx.x; k < SAS_TOTALS_RUN; k += blockDim.x) {
            bool e = k < m && live && (!mask || mask[c0 + k] != 0);
            double w = 1.0;
            if (e && wgt) {
                w = wgt[c0 + k];
                e = w > 0.0;
            }
            s_e[k] = e ? 1 : 0;
            s_w[k] = e ? w : 1.0;   // (a skipped cell's term is +0.0 * 1.0)
        }
        __syncthreads();
    }
    const double *p = src + (size_t)c0 * (size_t)W + (size_t)(act ? a : 0);
    double acc = 0.0;
    for (int k0 = 0; k0 < m; k0 += SAS_TOTALS_BATCH) {
        double v[SAS_TOTALS_BATCH];
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {
            const int kk = k0 + k;
            v[k] = 0.0;
            if (kk >= m) continue;
            if (FIRST) {
                if (__builtin_amdgcn_readfirstlane(s_e[kk]) && act) v[k] = __builtin_nontemporal_load(p + (size_t)kk * (size_t)W);
            } else if (act) {
                v[k] = p[(size_t)kk * (size_t)W];
            }
        }
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {   // left to right
            const int kk = k0 + k;
            if (kk >= m) continue;
            double t = v[k];
            if (FIRST) {
                if (t != t) t = 0.0;                     // a NaN element contributes +0.0 (the reference's nansum)
                else if (wgt) t = t * s_w[kk];           // rounded before it is added
            }
            acc = acc + t;
        }
    }
    if (act) dst[(size_t)blockIdx.x * (size_t)W + (size_t)a] = acc;
}
