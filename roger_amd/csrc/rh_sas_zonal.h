// rh_sas_zonal.h -- zonal totals of the SAS context (rh_sas_zonal_*, include/roger_hip_sas.h): every zone of a zone map in ONE pass that
// loads each row of an age-resolved array once.  Included by rh_sas.hip only, behind rh_sas_totals.h, whose items, statistics, identity,
// operations and wavefront tree it uses; the day kernels know nothing of it.
//
// Row block z is, bit for bit, what rh_sas_totals_* records with mask = (zone == z).  A (tile of 256 cells, zone) pair that exists is a
// SLOT; the pairs that do not exist are left out, and leaving them out changes no bit:
//   width 1     the rule of rh_zonal.h with five statistics: a slot gets its wavefront trees and (w0 op w1) op (w2 op w3); a zone has 256
//               accumulators, accumulator t takes the slots of the tiles with tile mod 256 == t in increasing tile order, then the same
//               two levels.  The partial of a pair that does not exist would be a tree of identities, which is the identity; an
//               accumulator that starts at +0.0 / +inf / -inf is never -0.0 and never NaN (min, max), so taking the identity changes no
//               bit (the argument in the header of rh_zonal.h).
//   width W > 1 per age class.  A run of the age rule is 256 consecutive cells, which is a tile, so the slots are the same slots.  Level 1:
//               the cells of z in the run are added left to right from +0.0 (a cell that is not eligible, a NaN element: +0.0).  The
//               dense rule then sums 256 consecutive partials left to right, 256 of those, and so on; a run, or a group of runs, without
//               a cell of z has the partial +0.0.  A running sum that starts at +0.0 is never -0.0, so adding that +0.0 or skipping it
//               are the same bits, and so is an extra level +0.0 + x.  Hence ONE walk over the zone's slots in increasing run order with
//               nested accumulators: a2 takes the slot partials, is added into a3 and cleared when run / 256 changes, a3 into a4 when
//               run / 65536 changes, both flushed at the end (n_cells < 2^31: the dense rule has at most four levels).
//
//   k_sas_zonal_tiles / k_sas_zonal_finish   k_zonal_tiles / k_zonal_finish (rh_zonal.h) with the value, weight and eligibility handling
//       of k_sas_totals_tiles: a workgroup per tile, a round per zone the tile holds (wave-uniform ids from the index), SAS_TOTALS_CHUNK
//       items loaded before the first is reduced, the slots' partials as plain stores into part [slot][item][stat]; one workgroup per
//       zone finishes.
//   k_sas_zonal_ages          one age item, level 1: a workgroup per (tile, chunk of up to 256 ages), lanes along the age axis.  The index
//       holds the tile's cells GROUPED BY SLOT (a stable grouping: increasing cell order within a slot); the workgroup stages that list
//       with the item's eligibility and weights in LDS once and walks it, so every eligible row is loaded once -- non-temporal, unit
//       stride -- whatever the number of zones in the tile.  A skip is a wave-uniform branch and loads nothing; SAS_TOTALS_BATCH rows
//       are in flight ahead of the ordered adds, across slot borders; where the slot changes the sum is stored to part [slot][age] and
//       starts again from +0.0.
//   k_sas_zonal_ages_finish   a workgroup per (zone, chunk of ages): the nested walk above, into the ring's row.  A zone without a cell
//       gets +0.0.
// Scratch, sized at configure: slots x items x 5 float64; ONE level-1 buffer of slots x Wmax float64 that the age items use one after
// another (the stream orders them).  No floating-point atomics, no counter on the device: row number and tags are the host's.
#pragma once
#include <algorithm>
#include <vector>

#include "rh_sas_totals.h"

struct SasZonalDev {
    const double *val[RH_SAS_TOTALS_MAX_ITEMS];     // as SasTotalsDev
    const double *wgt[RH_SAS_TOTALS_MAX_ITEMS];
    int64_t off[RH_SAS_TOTALS_MAX_ITEMS];           // first element of the item's block in a ZONE's part of a row
    unsigned char val_daily[RH_SAS_TOTALS_MAX_ITEMS];
    int n_items;
    int64_t n, zone_elems;                          // float64 per zone in a row
    const int *zone, *tile_ptr, *tile_zone, *acc_ptr, *acc_slot;   // the index (sas_zonal_index)
    double *part;                                   // [slot][item][stat]
};

// The index over a zone map, in one int32 buffer.  zone[n]; tile b holds the zones tile_zone[tile_ptr[b] ... tile_ptr[b + 1]), ascending:
// that position is the pair's slot.  Width 1: accumulator t of zone z takes acc_slot[acc_ptr[z * 256 + t] ... acc_ptr[z * 256 + t + 1]),
// in increasing tile order.  Age rule: zone z walks run_slot[run_ptr[z] ... run_ptr[z + 1]) in increasing run order, slot s lies in run
// slot_tile[s]; the cells of slot s, grouped, are cell[cell_ptr[s] ... cell_ptr[s + 1]): low byte the cell's place in its tile, the next
// byte the slot's place in its tile.
enum { SZ_ZONE, SZ_TILE_PTR, SZ_TILE_ZONE, SZ_ACC_PTR, SZ_ACC_SLOT, SZ_RUN_PTR, SZ_RUN_SLOT, SZ_SLOT_TILE, SZ_CELL_PTR, SZ_CELL, SZ_PARTS };
static int64_t sas_zonal_index(const int32_t *zone, int64_t n, int n_zones, std::vector<int> &buf, int64_t off[SZ_PARTS]) {
    const int64_t ntiles = (n + SAS_TOTALS_BLOCK - 1) / SAS_TOTALS_BLOCK;
    std::vector<int> tile_ptr((size_t)ntiles + 1, 0), tile_zone, slot_tile, cell_ptr(1, 0), cell, present;
    for (int64_t b = 0; b < ntiles; ++b) {
        const int64_t c0 = b * SAS_TOTALS_BLOCK, c1 = std::min<int64_t>(n, c0 + SAS_TOTALS_BLOCK);
        present.clear();   // the tile's cells inside a zone, by zone; stable: increasing cell order within the slot
        for (int64_t i = c0; i < c1; ++i)
            if (zone[i] >= 0) present.push_back((int)(i - c0));
        std::stable_sort(present.begin(), present.end(), [&](int x, int y) { return zone[c0 + x] < zone[c0 + y]; });
        for (size_t k = 0, r = 0; k < present.size(); ++k) {
            cell.push_back(present[k] | ((int)r << 8));
            if (k + 1 == present.size() || zone[c0 + present[k + 1]] != zone[c0 + present[k]]) {
                tile_zone.push_back(zone[c0 + present[k]]);
                slot_tile.push_back((int)b);
                cell_ptr.push_back((int)cell.size());
                ++r;
            }
        }
        tile_ptr[(size_t)b + 1] = (int)tile_zone.size();
    }
    const int64_t S = (int64_t)tile_zone.size();
    std::vector<int> acc_ptr((size_t)n_zones * SAS_TOTALS_BLOCK + 1, 0), acc_slot((size_t)S), run_ptr((size_t)n_zones + 1, 0), run_slot((size_t)S);
    for (int64_t s = 0; s < S; ++s) {
        ++acc_ptr[(size_t)tile_zone[s] * SAS_TOTALS_BLOCK + slot_tile[s] % SAS_TOTALS_BLOCK + 1];
        ++run_ptr[(size_t)tile_zone[s] + 1];
    }
    for (size_t k = 1; k < acc_ptr.size(); ++k) acc_ptr[k] += acc_ptr[k - 1];
    for (size_t k = 1; k < run_ptr.size(); ++k) run_ptr[k] += run_ptr[k - 1];
    std::vector<int> fill(acc_ptr.begin(), acc_ptr.end() - 1), rfill(run_ptr.begin(), run_ptr.end() - 1);
    for (int64_t s = 0; s < S; ++s) {   // slots ascend with their tiles: increasing tile order within every list
        acc_slot[(size_t)fill[(size_t)tile_zone[s] * SAS_TOTALS_BLOCK + slot_tile[s] % SAS_TOTALS_BLOCK]++] = (int)s;
        run_slot[(size_t)rfill[(size_t)tile_zone[s]]++] = (int)s;
    }
    const std::vector<int> *parts[SZ_PARTS] = {nullptr, &tile_ptr, &tile_zone, &acc_ptr, &acc_slot, &run_ptr, &run_slot, &slot_tile, &cell_ptr, &cell};
    buf.assign(zone, zone + n);
    off[SZ_ZONE] = 0;
    for (int k = 1; k < SZ_PARTS; ++k) {
        off[k] = (int64_t)buf.size();
        buf.insert(buf.end(), parts[k]->begin(), parts[k]->end());
    }
    return S;
}

// One workgroup per tile: for every zone the tile holds the five trees of every item, into part [slot][item][stat].  The LDS staging is
// double-buffered as in k_zonal_tiles, so a zone costs one barrier.  day_off: as k_sas_totals_tiles.
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_zonal_tiles(const SasZonalDev *__restrict__ P, int64_t day_off) {
    __shared__ double part[2][SAS_TOTALS_CHUNK * SAS_TOTALS_NSTAT][SAS_TOTALS_BLOCK / 64];
    const int s0 = P->tile_ptr[blockIdx.x], s1 = P->tile_ptr[blockIdx.x + 1];
    if (s0 == s1) return;   // (no cell of any zone in this tile: nothing to load)
    const int64_t i = (int64_t)blockIdx.x * SAS_TOTALS_BLOCK + threadIdx.x;
    const int ni = P->n_items, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mine = i < P->n ? __builtin_nontemporal_load(P->zone + i) : -1;
    int round = 0;
    for (int j0 = 0; j0 < ni; j0 += SAS_TOTALS_CHUNK) {
        const int nk = ni - j0 < SAS_TOTALS_CHUNK ? ni - j0 : SAS_TOTALS_CHUNK;
        double v[SAS_TOTALS_CHUNK], w[SAS_TOTALS_CHUNK], t[SAS_TOTALS_CHUNK];
        bool counted[SAS_TOTALS_CHUNK];
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_CHUNK; ++k) {
            v[k] = 0.0;
            w[k] = 0.0;      // (not eligible)
            if (k >= nk || mine < 0) continue;
            const int j = j0 + k;
            const double *pv = P->val[j], *pw = P->wgt[j];
            const bool daily = P->val_daily[j] != 0;
            if ((pw || daily) && day_off < 0) continue;
            w[k] = pw ? __builtin_nontemporal_load(pw + day_off + i) : 1.0;
            if (pv) v[k] = __builtin_nontemporal_load(pv + (daily ? day_off : 0) + i);
        }
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_CHUNK; ++k) {
            counted[k] = w[k] > 0.0 && v[k] == v[k];                                   // (a NaN weight is not > 0)
            t[k] = (k < nk && P->wgt[j0 + k]) ? v[k] * w[k] : v[k];                    // rounded before it is added (-ffp-contract=off)
        }
        for (int s = s0; s < s1; ++s, ++round) {
            const int z = P->tile_zone[s];
            const bool in = mine == z;
            double(*buf)[SAS_TOTALS_BLOCK / 64] = part[round & 1];
            if (__ballot(in)) {
#pragma unroll
                for (int k = 0; k < SAS_TOTALS_CHUNK; ++k) {
                    if (k >= nk) break;
                    const bool c = in && counted[k];
                    const double ws = sas_totals_wave<0>(c ? w[k] : 0.0);
                    const double cn = sas_totals_wave<1>(c ? 1.0 : 0.0);
                    const double sm = sas_totals_wave<2>(c ? t[k] : 0.0);
                    const double lo = sas_totals_wave<3>(c ? v[k] : sas_totals_identity(3));
                    const double hi = sas_totals_wave<4>(c ? v[k] : sas_totals_identity(4));
                    if (lane == 0) {
                        double(*q)[SAS_TOTALS_BLOCK / 64] = buf + k * SAS_TOTALS_NSTAT;
                        q[0][wave] = ws;
                        q[1][wave] = cn;
                        q[2][wave] = sm;
                        q[3][wave] = lo;
                        q[4][wave] = hi;
                    }
                }
            } else if (lane < nk * SAS_TOTALS_NSTAT) {   // no cell of z in this wavefront: the tree of identities is the identity
                buf[lane][wave] = sas_totals_identity(lane % SAS_TOTALS_NSTAT);
            }
            __syncthreads();
            if ((int)threadIdx.x < nk * SAS_TOTALS_NSTAT)
                P->part[((size_t)s * ni + j0) * SAS_TOTALS_NSTAT + threadIdx.x] = sas_totals_four((int)threadIdx.x % SAS_TOTALS_NSTAT, buf[threadIdx.x]);
        }
    }
}

// One workgroup per zone: thread t is accumulator t -- it walks its slots in increasing tile order -- then the two levels, into the zone's
// part of the row.  Four slots x five statistics are loaded before the first is used: a thread's loads are independent, its operations
// ordered.
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_zonal_finish(const SasZonalDev *__restrict__ P, double *__restrict__ row) {
    __shared__ double part[RH_SAS_TOTALS_MAX_ITEMS * SAS_TOTALS_NSTAT][SAS_TOTALS_BLOCK / 64];
    const int z = (int)blockIdx.x, ni = P->n_items;
    const int p0 = P->acc_ptr[z * SAS_TOTALS_BLOCK + threadIdx.x], p1 = P->acc_ptr[z * SAS_TOTALS_BLOCK + threadIdx.x + 1];
    constexpr int PT = 4;
    for (int j = 0; j < ni; ++j) {
        double x[SAS_TOTALS_NSTAT];
#pragma unroll
        for (int st = 0; st < SAS_TOTALS_NSTAT; ++st) x[st] = sas_totals_identity(st);
        for (int p = p0; p < p1; p += PT) {
            double v[PT][SAS_TOTALS_NSTAT];
#pragma unroll
            for (int k = 0; k < PT; ++k) {
                const int s = p + k < p1 ? P->acc_slot[p + k] : -1;
#pragma unroll
                for (int st = 0; st < SAS_TOTALS_NSTAT; ++st) v[k][st] = s >= 0 ? P->part[((size_t)s * ni + j) * SAS_TOTALS_NSTAT + st] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < PT; ++k)   // in increasing tile order
                if (p + k < p1) {
#pragma unroll
                    for (int st = 0; st < SAS_TOTALS_NSTAT; ++st) x[st] = sas_totals_op(st, x[st], v[k][st]);
                }
        }
        const double r0 = sas_totals_wave<0>(x[0]), r1 = sas_totals_wave<1>(x[1]), r2 = sas_totals_wave<2>(x[2]);
        const double r3 = sas_totals_wave<3>(x[3]), r4 = sas_totals_wave<4>(x[4]);
        if ((threadIdx.x & 63) == 0) {
            double(*q)[SAS_TOTALS_BLOCK / 64] = part + j * SAS_TOTALS_NSTAT;
            const int wave = threadIdx.x >> 6;
            q[0][wave] = r0;
            q[1][wave] = r1;
            q[2][wave] = r2;
            q[3][wave] = r3;
            q[4][wave] = r4;
        }
    }
    __syncthreads();
    double *dst = row + (size_t)z * (size_t)P->zone_elems;
    for (int q = threadIdx.x; q < ni * SAS_TOTALS_NSTAT; q += SAS_TOTALS_BLOCK) {
        const int j = q / SAS_TOTALS_NSTAT, st = q % SAS_TOTALS_NSTAT;
        if (st < (P->val[j] ? SAS_TOTALS_NSTAT : 2)) dst[P->off[j] + st] = sas_totals_four(st, part[q]);   // an age item: wsum and count
    }
}

// Level 1 of the age rule for every slot of tile blockIdx.x.  src is (n, W); thread -> age class blockIdx.y * blockDim.x + threadIdx.x;
// dst[slot * W + age] = the sum over the slot's cells.  wgt: the day's row of the weight or null; `live` == 0 makes every cell
// ineligible (day < 0 with a weight).
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_zonal_ages(const double *__restrict__ src, int W, const int *__restrict__ tile_ptr,
                                                                     const int *__restrict__ cell_ptr, const int *__restrict__ cell,
                                                                     const double *__restrict__ wgt, int live, double *__restrict__ dst) {
    __shared__ double s_w[SAS_TOTALS_RUN];
    __shared__ int s_e[SAS_TOTALS_RUN], s_cell[SAS_TOTALS_RUN], s_slot[SAS_TOTALS_RUN];
    const int s0 = tile_ptr[blockIdx.x], s1 = tile_ptr[blockIdx.x + 1];
    if (s0 == s1) return;
    const int g0 = cell_ptr[s0], m = cell_ptr[s1] - g0;   // the tile's cells inside a zone: 1 ... 256
    const int64_t c0 = (int64_t)blockIdx.x * SAS_TOTALS_RUN;
    for (int k = threadIdx.x; k < m; k += blockDim.x) {
        const int g = cell[g0 + k], c = g & 255;
        bool e = live != 0;
        double w = 1.0;
        if (e && wgt) {
            w = wgt[c0 + c];
            e = w > 0.0;
        }
        s_cell[k] = c;
        s_slot[k] = g >> 8;
        s_e[k] = e ? 1 : 0;
        s_w[k] = e ? w : 1.0;   // (a skipped cell's term is +0.0 * 1.0)
    }
    __syncthreads();
    const int a = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    const bool act = a < W;
    const double *p = src + (size_t)c0 * (size_t)W + (size_t)(act ? a : 0);
    double acc = 0.0;
    for (int k0 = 0; k0 < m; k0 += SAS_TOTALS_BATCH) {
        double v[SAS_TOTALS_BATCH];
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {
            const int kk = k0 + k;
            v[k] = 0.0;
            if (kk >= m) continue;
            if (__builtin_amdgcn_readfirstlane(s_e[kk]) && act)
                v[k] = __builtin_nontemporal_load(p + (size_t)__builtin_amdgcn_readfirstlane(s_cell[kk]) * (size_t)W);
        }
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {   // left to right within the slot
            const int kk = k0 + k;
            if (kk >= m) continue;
            double t = v[k];
            if (t != t) t = 0.0;                     // a NaN element contributes +0.0 (the reference's nansum)
            else if (wgt) t = t * s_w[kk];           // rounded before it is added
            acc = acc + t;
            const int sl = __builtin_amdgcn_readfirstlane(s_slot[kk]);
            if (kk + 1 == m || __builtin_amdgcn_readfirstlane(s_slot[kk + 1]) != sl) {   // the slot's last cell
                if (act) dst[(size_t)(s0 + sl) * (size_t)W + (size_t)a] = acc;
                acc = 0.0;
            }
        }
    }
}

// The further levels of the age rule for zone blockIdx.x, in one walk over its slots (the nested accumulators of the header):
// row[zone * zone_elems + age]; `row` points at the item's sums in zone 0's part.
__global__ __launch_bounds__(SAS_TOTALS_BLOCK) void k_sas_zonal_ages_finish(const double *__restrict__ part, int W, const int *__restrict__ run_ptr,
                                                                            const int *__restrict__ run_slot, const int *__restrict__ slot_tile,
                                                                            double *__restrict__ row, int64_t zone_elems) {
    const int z = (int)blockIdx.x, a = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    const bool act = a < W;
    const int p0 = run_ptr[z], p1 = run_ptr[z + 1];
    const double *p = part + (size_t)(act ? a : 0);
    double a2 = 0.0, a3 = 0.0, a4 = 0.0;
    int prev = -1;
    for (int q0 = p0; q0 < p1; q0 += SAS_TOTALS_BATCH) {
        double v[SAS_TOTALS_BATCH];
        int run[SAS_TOTALS_BATCH];
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {
            v[k] = 0.0;
            run[k] = 0;
            if (q0 + k >= p1) continue;
            const int s = run_slot[q0 + k];
            run[k] = slot_tile[s];
            if (act) v[k] = p[(size_t)s * (size_t)W];
        }
#pragma unroll
        for (int k = 0; k < SAS_TOTALS_BATCH; ++k) {   // in increasing run order
            if (q0 + k >= p1) continue;
            const int r = run[k];
            if (prev >= 0 && (r >> 8) != (prev >> 8)) {
                a3 = a3 + a2;
                a2 = 0.0;
                if ((r >> 16) != (prev >> 16)) {
                    a4 = a4 + a3;
                    a3 = 0.0;
                }
            }
            a2 = a2 + v[k];
            prev = r;
        }
    }
    a3 = a3 + a2;
    a4 = a4 + a3;
    if (act) row[(size_t)z * (size_t)zone_elems + (size_t)a] = a4;
}
