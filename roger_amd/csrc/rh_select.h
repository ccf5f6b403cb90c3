// rh_select.h -- the pure pieces of the radix selection on order-preserving keys that the ensemble bands of the SVAT / oneD step
// (rh_bands.h, in roger_hip.hip) and the bands of the offline transport model (rh_sas_bands.h, in rh_sas.hip) share: the key of a double
// and its inverse, the digits of the six passes, the rank of a probability, the grid whose workgroups cannot overflow a uint32 LDS bin,
// and the pick of a wavefront over 64-bit bins.  Functions of their arguments only: no kernel, no device state, no memory access.
#pragma once
#include <hip/hip_runtime.h>

#define RH_SELECT_DEV __device__ __forceinline__
#define RH_SELECT_BLOCK 256         // keys of a tile, threads of a workgroup
#define RH_SELECT_MAX_GRID 256      // workgroups of a pass (one per CU), unless the LDS bound asks for more
#define RH_SELECT_W_MAX_TILES 256   // tiles one workgroup may walk with weights up to 65535 in uint32 LDS bins
#define RH_SELECT_KEY_MASKED (~0ull)
#define RH_SELECT_KEY_NAN (~0ull - 1ull)

// pass P of the selection: digit bits [shift, shift + width) of the key; the bits above them are the prefix
template <int P>
struct BandsPass {
    static constexpr int shift = P < 5 ? 53 - 11 * P : 0, width = P < 5 ? 11 : 9, nb = 1 << width, high = shift + width;
};
// The order-preserving key of a value that is not a NaN: unsigned comparison of keys is < on the values.  Both reserved keys above are
// keys of NaN bit patterns, so no value's key equals them (the largest, +inf's, is 0xfff0000000000000).
RH_SELECT_DEV unsigned long long bands_key_of(double s) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    return u ^ ((u >> 63) ? ~0ull : 1ull << 63);
}
// ... and the value of a key
RH_SELECT_DEV double bands_value_of(unsigned long long key) {
    const unsigned long long u = (key >> 63) ? key ^ (1ull << 63) : ~key;
    return __longlong_as_double((long long)u);
}
// the rank of probability p among m values (with weights: T - 1 among W members): one double multiplication, one ceil
RH_SELECT_DEV long long bands_rank_of(double p, long long m) {
    long long r = (long long)ceil(p * (double)m) - 1;
    r = r > m - 1 ? m - 1 : r;
    return r < 0 ? 0 : r;
}
// A uint32 LDS bin holds at most (columns the workgroup walks) x 65535: max(min(MAX_GRID, ntiles), ceil(ntiles / W_MAX_TILES)) workgroups,
// workgroup b taking the tiles t = b mod grid -- ceil(ntiles / grid) of them at most.
static_assert((unsigned long long)RH_SELECT_W_MAX_TILES * RH_SELECT_BLOCK * 65535ull < (1ull << 32), "a uint32 LDS bin holds a workgroup's weights");
static inline unsigned bands_weighted_grid(long long n) {
    const long long ntiles = (n + RH_SELECT_BLOCK - 1) / RH_SELECT_BLOCK, few = ntiles < RH_SELECT_MAX_GRID ? ntiles : RH_SELECT_MAX_GRID,
                    bound = (ntiles + RH_SELECT_W_MAX_TILES - 1) / RH_SELECT_W_MAX_TILES;
    return (unsigned)(few > bound ? few : bound);
}
RH_SELECT_DEV unsigned long long bands_wave_scan64(unsigned long long x) {   // inclusive, over the 64 lanes
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}
// The pick of one wavefront over 64-bit bins (sums of weights, below 2^47): bin k * 64 + lane of a histogram in v[k]; the digit at which
// the cumulative sum passes the rank r, and the sum below it.  (No bin passes it only where the histogram is empty: digit 0, below 0.)
template <int NC>
RH_SELECT_DEV void bands_pick64(const unsigned long long (&v)[NC], long long r, int &digit, long long &below) {
    long long base = 0;
    bool found = false;
    digit = 0;
    below = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const unsigned long long incl = bands_wave_scan64(v[k]);
        const long long chunk = (long long)__shfl(incl, 63);
        if (!found && base + chunk > r) {
            const unsigned long long hit = __ballot(base + (long long)incl > r);
            const int l = __ffsll((long long)hit) - 1;
            digit = k * 64 + l;
            below = base + (long long)__shfl(incl - v[k], l);
            found = true;
        }
        base += chunk;
    }
}
