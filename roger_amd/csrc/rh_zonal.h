// rh_zonal.h -- zonal totals (rh_zonal_configure): after a step, the sum, minimum and maximum of up to 32 planes for EVERY zone of a zone
// map (sub-catchments, land uses, soil classes), one row of a ring per step, in ONE pass over the planes.  Part of the one translation
// unit roger_hip.hip, behind rh_control.h (totals_identity, totals_op, totals_wave).
//
// The ORDER is the catchment totals' (rh_control.h, k_totals_tiles / k_totals_finish), applied to the mask `zone == z`:
//   a wavefront:  the tree over its 64 lanes with strides 32 ... 1; a lane whose column is not in z (or beyond n) holds the identity
//                 (+0.0, +inf, -inf)
//   a workgroup:  (w0 op w1) op (w2 op w3) of its four wavefronts, through LDS
//   the grid:     256 accumulators per zone; accumulator t starts at the identity and takes, in increasing tile order, the partials of
//                 the tiles with tile mod 256 == t THAT HOLD A COLUMN OF z; the 256 accumulators then take the two levels above
// The dense rule of rh_totals_* would also take the partials of the tiles without a column of z.  Such a partial is a tree of identities,
// which is the identity, and taking it changes no bit of an accumulator:
//   sum: the accumulator starts at +0.0, and x + y is -0.0 only where both are -0.0, so an accumulator is never -0.0; for every other
//        x (NaN and the infinities included) x + +0.0 == x, bit for bit;
//   min, max: fmin / fmax return the other operand when one is NaN, the accumulator starts at +inf / -inf, so it is never NaN, and
//        fmin(x, +inf) == x, fmax(x, -inf) == x.
// So row z equals tree_totals(values, zone == z) (roger_amd/totals.py, tests/totals_reference.py) in every bit of the sums, while a tile
// costs work for the zones it holds only.  No floating-point atomics; the (tile, zone) partials are plain stores.
//
// The row counter and the header: workgroup 0 of k_zonal_tiles writes the header of row zonal_rows and then zonal_rows + 1; no other
// workgroup of that launch reads the counter.  Every workgroup of k_zonal_finish (one per zone) reads the counter the tile launch in
// front of it on the stream left -- its row is zonal_rows - 1 -- and none writes it.  No workgroup reads a word that a workgroup of its
// own launch advances.
#pragma once

#define RH_ZONAL_CHUNK 8   // planes loaded before the first of them is reduced, as RH_TOTALS_CHUNK
// One workgroup per tile of 256 columns: for every zone the tile holds (ascending, wave-uniform ids from the index) the three trees of
// every plane, into zonal_part [slot][plane][stat].  The LDS staging is double-buffered, so a zone costs one barrier: the writers of
// round r + 2 have passed the barrier of round r + 1, which every reader of round r reached after its reads.
__global__ __launch_bounds__(RH_BLOCK) void k_zonal_tiles(Arena a, DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    __shared__ double part[2][RH_ZONAL_CHUNK * 3][RH_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    const int nv = D->zonal_nplanes, wave = threadIdx.x >> 6;
    const bool inside = i < a.n;
    const int mine = inside ? __builtin_nontemporal_load(D->zonal_zone + i) : -1;
    const int s0 = D->zonal_tile_ptr[blockIdx.x], s1 = D->zonal_tile_ptr[blockIdx.x + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const rh_scalars &S = D->S;
        const long long row = D->zonal_rows;
        long long *h = D->zonal_hdr + 3 * (row % D->zonal_cap);
        h[0] = S.itt;
        h[1] = S.time;
        h[2] = S.dt_secs;
        D->zonal_rows = row + 1;
    }
    if (s0 == s1) return;   // (no column of any zone in this tile: nothing to load)
    int round = 0;
    for (int j0 = 0; j0 < nv; j0 += RH_ZONAL_CHUNK) {
        const int nk = nv - j0 < RH_ZONAL_CHUNK ? nv - j0 : RH_ZONAL_CHUNK;
        double v[RH_ZONAL_CHUNK];
#pragma unroll
        for (int k = 0; k < RH_ZONAL_CHUNK; ++k) {
            v[k] = 0.0;
            if (inside && k < nk) rh_ld(a, D->zonal_planes[j0 + k], i, v[k]);
        }
        for (int s = s0; s < s1; ++s, ++round) {
            const int z = D->zonal_tile_zone[s];
            const bool counted = mine == z;
            double(*buf)[RH_BLOCK / 64] = part[round & 1];
            if (__ballot(counted)) {
#pragma unroll
                for (int k = 0; k < RH_ZONAL_CHUNK; ++k) {
                    if (k >= nk) break;
                    const double sum = totals_wave<0>(counted ? v[k] : totals_identity(0));
                    const double lo = totals_wave<1>(counted ? v[k] : totals_identity(1));
                    const double hi = totals_wave<2>(counted ? v[k] : totals_identity(2));
                    if ((threadIdx.x & 63) == 0) {
                        buf[k * 3 + 0][wave] = sum;
                        buf[k * 3 + 1][wave] = lo;
                        buf[k * 3 + 2][wave] = hi;
                    }
                }
            } else if ((threadIdx.x & 63) < nk * 3) {   // no column of z in this wavefront: the tree of identities is the identity
                buf[threadIdx.x & 63][wave] = totals_identity((int)(threadIdx.x & 63) % 3);
            }
            __syncthreads();
            if ((int)threadIdx.x < nk * 3) {
                const int q = threadIdx.x, stat = q % 3;
                D->zonal_part[((size_t)s * nv + j0) * 3 + q] = totals_op(stat, totals_op(stat, buf[q][0], buf[q][1]), totals_op(stat, buf[q][2], buf[q][3]));
            }
        }
    }
}
// One workgroup per zone: thread t is accumulator t -- it walks its slots in increasing tile order -- then the two levels, into row
// zonal_rows - 1 (see above), values (zone, plane, {sum, min, max}).  Four planes x three statistics x four slots are loaded before the
// first is used, as in k_totals_finish: the loads of a thread are independent, only its operations are ordered.
__global__ __launch_bounds__(RH_BLOCK) void k_zonal_finish(DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    __shared__ double part[RH_POINTS_MAX_PLANES * 3][RH_BLOCK / 64];
    const int z = blockIdx.x, nv = D->zonal_nplanes, nq = nv * 3;
    const long long slot = (D->zonal_rows - 1) % D->zonal_cap;
    const int p0 = D->zonal_acc_ptr[z * RH_BLOCK + threadIdx.x], p1 = D->zonal_acc_ptr[z * RH_BLOCK + threadIdx.x + 1];
    constexpr int PJ = 4, PT = 4;
    for (int j0 = 0; j0 < nv; j0 += PJ) {
        double x[PJ][3];
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int st = 0; st < 3; ++st) x[j][st] = totals_identity(st);
        for (int p = p0; p < p1; p += PT) {
            double v[PT][PJ][3];
#pragma unroll
            for (int k = 0; k < PT; ++k) {
                const int s = p + k < p1 ? D->zonal_acc_slot[p + k] : -1;
#pragma unroll
                for (int j = 0; j < PJ; ++j)
#pragma unroll
                    for (int st = 0; st < 3; ++st)
                        v[k][j][st] = (s >= 0 && j0 + j < nv) ? D->zonal_part[((size_t)s * nv + j0 + j) * 3 + st] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < PT; ++k)   // in increasing tile order
                if (p + k < p1) {
#pragma unroll
                    for (int j = 0; j < PJ; ++j)
#pragma unroll
                        for (int st = 0; st < 3; ++st) x[j][st] = totals_op(st, x[j][st], v[k][j][st]);
                }
        }
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
            if (j0 + j >= nv) break;
            const double s = totals_wave<0>(x[j][0]), lo = totals_wave<1>(x[j][1]), hi = totals_wave<2>(x[j][2]);
            if ((threadIdx.x & 63) == 0) {
                part[(j0 + j) * 3 + 0][threadIdx.x >> 6] = s;
                part[(j0 + j) * 3 + 1][threadIdx.x >> 6] = lo;
                part[(j0 + j) * 3 + 2][threadIdx.x >> 6] = hi;
            }
        }
    }
    __syncthreads();
    double *dst = D->zonal + ((size_t)slot * D->zonal_nzones + z) * nq;
    for (int q = threadIdx.x; q < nq; q += RH_BLOCK) {
        const int stat = q % 3;
        dst[q] = totals_op(stat, totals_op(stat, part[q][0], part[q][1]), totals_op(stat, part[q][2], part[q][3]));
    }
}
