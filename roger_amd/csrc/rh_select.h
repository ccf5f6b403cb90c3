// rh_select.h -- the pieces of the radix selection on order-preserving keys that the ensemble bands of the SVAT / oneD step (rh_bands.h, in
// roger_hip.hip) and the bands of the offline transport model (rh_sas_bands.h, rh_sas_bands_zonal.h and rh_sas_age_bands.h, in rh_sas.hip)
// share, each stated once: the key of a double and its inverse, the digits of the six passes, the rank of a probability, the grids, the
// three walks over the keys, the digit count of a key, the pick of a wavefront over the bins, the whole selection of one workgroup in its
// own LDS (a zone, an age class), and the pair (below, equal) of an observation.  No kernel, no
// DevState / SasBandsDev: device functions that take pointers.  What differs between the kernels -- the clocks, the merge into global
// bins, the completion pattern, where prefix and rank live, the ring and row writes -- is theirs.
#pragma once
#include <hip/hip_runtime.h>

#define RH_SELECT_DEV __device__ __forceinline__
#define RH_SELECT_BODY __attribute__((always_inline))   // on the lambda a walk calls per key: U call sites, one loop body
#define RH_SELECT_BLOCK 256         // keys of a tile, threads of a workgroup
#define RH_SELECT_U 8               // tiles (list entries) a thread holds in flight per trip
#define RH_SELECT_MAX_GRID 256      // workgroups of a pass (one per CU), unless the LDS bound asks for more
#define RH_SELECT_W_MAX_TILES 256   // tiles one workgroup may walk with weights up to 65535 in uint32 LDS bins
#define RH_SELECT_MAX_PROBS 8       // probabilities of an item: LDS histograms of a workgroup
#define RH_SELECT_NBINS 2048        // 11-bit digits: bins of a histogram in memory
#define RH_SELECT_PASSES 6
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
// the workgroups per item of the pass that counts an observation's pair: min(MAX_GRID, max(1, ntiles))
static inline unsigned select_obs_grid(long long n) {
    const long long ntiles = (n + RH_SELECT_BLOCK - 1) / RH_SELECT_BLOCK;
    return (unsigned)(ntiles < RH_SELECT_MAX_GRID ? (ntiles < 1 ? 1 : ntiles) : RH_SELECT_MAX_GRID);
}

// ---- the walks: body(key, w) for every key of the workgroup's share, U loads requested before the first use ----
// A key plane of n keys: tile t of RH_SELECT_BLOCK keys belongs to workgroup t mod grid; non-temporal loads.  WEIGHTED: the 2-byte weight
// plane is read with the keys; else w is the constant 1.  Beyond n the key is KEY_MASKED (and the weight 0).
template <bool WEIGHTED, class Body>
RH_SELECT_DEV void select_walk_tiles(const unsigned long long *keys, const unsigned short *wts, long long n, Body body) {
    constexpr int U = RH_SELECT_U;
    const long long ntiles = (n + RH_SELECT_BLOCK - 1) / RH_SELECT_BLOCK;
    for (long long t = blockIdx.x; t < ntiles; t += (long long)gridDim.x * U) {
        unsigned long long key[U];
        unsigned w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i = (t + (long long)u * gridDim.x) * RH_SELECT_BLOCK + threadIdx.x;   // (beyond the last tile: beyond n)
            key[u] = i < n ? __builtin_nontemporal_load(keys + i) : RH_SELECT_KEY_MASKED;
            w[u] = WEIGHTED ? (i < n ? (unsigned)__builtin_nontemporal_load(wts + i) : 0u) : 1u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) body(key[u], w[u]);
    }
}
// The entries [beg, end) of a column list, walked by ONE workgroup: cols[at], then the gathers keys[col] and, WEIGHTED, wts[col]; plain
// loads.  Beyond end the key is KEY_MASKED (and the weight 0).
template <bool WEIGHTED, class Body>
RH_SELECT_DEV void select_walk_list(const unsigned long long *keys, const unsigned short *wts, const int *cols, long long beg, long long end, Body body) {
    constexpr int U = RH_SELECT_U;
    for (long long base = beg; base < end; base += (long long)RH_SELECT_BLOCK * U) {
        int col[U];
        unsigned long long key[U];
        unsigned w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long at = base + (long long)u * RH_SELECT_BLOCK + threadIdx.x;
            col[u] = at < end ? cols[at] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            key[u] = col[u] >= 0 ? keys[col[u]] : RH_SELECT_KEY_MASKED;
            w[u] = WEIGHTED ? (col[u] >= 0 ? (unsigned)wts[col[u]] : 0u) : 1u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) body(key[u], w[u]);
    }
}
// A contiguous run of n keys, walked by ONE workgroup: keys[at] and, WEIGHTED, the weight at the SAME index wts[at]; plain loads.  Beyond
// the run's end the key is KEY_MASKED (and the weight 0).
template <bool WEIGHTED, class Body>
RH_SELECT_DEV void select_walk_run(const unsigned long long *keys, const unsigned short *wts, long long n, Body body) {
    constexpr int U = RH_SELECT_U;
    for (long long base = 0; base < n; base += (long long)RH_SELECT_BLOCK * U) {
        unsigned long long key[U];
        unsigned w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long at = base + (long long)u * RH_SELECT_BLOCK + threadIdx.x;
            key[u] = at < n ? keys[at] : RH_SELECT_KEY_MASKED;
            w[u] = WEIGHTED ? (at < n ? (unsigned)wts[at] : 0u) : 1u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) body(key[u], w[u]);
    }
}

// ---- the count: one key into the workgroup's LDS histograms (uint32, LDS atomics) ----
// Keys >= KEY_NAN take no part; pass 0 counts the NaN and the numbers this thread met in registers (one LDS add per thread behind the
// walk is the caller's).  Pass 0 has one histogram for all probabilities -- there is no prefix yet; a later pass adds w into the
// histogram of every probability q < np whose prefix pre[q] the key's higher digits equal.
template <int PASS>
RH_SELECT_DEV void select_count(unsigned long long key, unsigned w, int np, const unsigned long long (&pre)[RH_SELECT_MAX_PROBS], unsigned *hist,
                                unsigned &mine, unsigned &mine_nan) {
    using PS = BandsPass<PASS>;
    if (key >= RH_SELECT_KEY_NAN) {
        if (PASS == 0 && key == RH_SELECT_KEY_NAN) ++mine_nan;
        return;
    }
    const unsigned d = (unsigned)(key >> PS::shift) & (unsigned)(PS::nb - 1);
    if (PASS == 0) {
        ++mine;
        atomicAdd(&hist[d], w);
    } else {
#pragma unroll
        for (int q = 0; q < RH_SELECT_MAX_PROBS; ++q)
            if (q < np && (key >> (PS::high & 63)) == pre[q]) atomicAdd(&hist[q * PS::nb + d], w);
    }
}

// ---- the pick of one wavefront: bin k * 64 + lane of a histogram in v[k]; T the bins' type (uint32 counts, or uint64 sums of weights
// below 2^47), and the lane arithmetic of the scan is T's ----
template <class T>
RH_SELECT_DEV T bands_wave_scan(T x) {   // inclusive, over the 64 lanes
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}
// the digit at which the cumulative sum passes the rank r, and the sum below it.  (No bin passes it only where the histogram is empty:
// digit 0, below 0.)
template <int NC, class T>
RH_SELECT_DEV void bands_pick(const T (&v)[NC], long long r, int &digit, long long &below) {
    long long base = 0;
    bool found = false;
    digit = 0;
    below = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const T incl = bands_wave_scan(v[k]);
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
// One pass of one (item, probability) pair, the bins in registers.  Pass 0 forms the histogram's total and from it the rank of p; a later
// pass reads the rank and the prefix where the pass before stored them (device memory or LDS), the prefix only behind the pick.  The
// digit picked is appended to the prefix, the sum below it leaves the rank; storing both is the caller's.
struct SelectPick {
    unsigned long long prefix;
    long long rank, total;   // total: pass 0 only
};
template <int PASS, class T>
RH_SELECT_DEV SelectPick select_pick_step(const T (&v)[BandsPass<PASS>::nb / 64], double p, const unsigned long long *prefix, const long long *rank) {
    constexpr int NC = BandsPass<PASS>::nb / 64;
    long long total = 0, r;
    if (PASS == 0) {
        T tot = 0;
#pragma unroll
        for (int k = 0; k < NC; ++k) tot += v[k];
        for (int off = 32; off; off >>= 1) tot += __shfl_xor(tot, off);
        total = (long long)tot;
        r = bands_rank_of(p, total);
    } else {
        r = *rank;
    }
    long long below;
    int digit;
    bands_pick<NC>(v, r, digit, below);
    return {(PASS == 0 ? 0ull : *prefix << BandsPass<PASS>::width) | (unsigned long long)digit, r - below, total};
}

// ---- the whole selection by ONE workgroup in its own LDS (a zone of rh_sas_bands_zonal.h, an age class of rh_sas_age_bands.h) ----
// uint32 histograms [probability][2048], pass 0 shared by the probabilities; the prefixes and the ranks that remain between the passes;
// count {m, n_nan, W} fixed by pass 0; cnt {numbers, NaNs} of pass 0.  With weights the workgroup's share holds at most
// RH_SELECT_W_MAX_TILES x RH_SELECT_BLOCK keys (the static_assert above): the caller's configure call enforces it.
#define RH_SELECT_HDR 3   // m, n_nan, W
struct SelectLds {
    unsigned *hist;
    unsigned long long *prefix;
    long long *rank, *count;
    unsigned *cnt;
};
#define RH_SELECT_LDS(L)                                                         \
    __shared__ unsigned L##_hist[RH_SELECT_MAX_PROBS * RH_SELECT_NBINS];         \
    __shared__ unsigned long long L##_prefix[RH_SELECT_MAX_PROBS];               \
    __shared__ long long L##_rank[RH_SELECT_MAX_PROBS], L##_count[RH_SELECT_HDR]; \
    __shared__ unsigned L##_cnt[2];                                              \
    const SelectLds L = {L##_hist, L##_prefix, L##_rank, L##_count, L##_cnt}
// Pass PASS: walk(body) calls body(key, w) for every key of the workgroup's share (one of the walks above); the histograms, then a
// wavefront per probability widens the bins to 64 bit and picks the digit.
template <int PASS, class Walk>
RH_SELECT_DEV void select_lds_pass(Walk walk, int np, const double *probs, const SelectLds &L) {
    constexpr int NB = BandsPass<PASS>::nb, NC = NB / 64;
    const int nh = PASS == 0 ? 1 : np;
    for (int b = threadIdx.x; b < nh * NB; b += RH_SELECT_BLOCK) L.hist[b] = 0;
    if (PASS == 0 && threadIdx.x == 0) L.cnt[0] = L.cnt[1] = 0;
    __syncthreads();
    unsigned long long pre[RH_SELECT_MAX_PROBS];
#pragma unroll
    for (int q = 0; q < RH_SELECT_MAX_PROBS; ++q) pre[q] = (PASS > 0 && q < np) ? L.prefix[q] : 0ull;
    unsigned mine = 0, mine_nan = 0;   // pass 0: the numbers and the NaNs this thread met
    unsigned *hist = L.hist;
    walk([&](unsigned long long key, unsigned w) RH_SELECT_BODY { select_count<PASS>(key, w, np, pre, hist, mine, mine_nan); });
    if (PASS == 0 && mine) atomicAdd(&L.cnt[0], mine);
    if (PASS == 0 && mine_nan) atomicAdd(&L.cnt[1], mine_nan);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < np; q += RH_SELECT_BLOCK / 64) {   // (uniform over the wavefront)
        const unsigned *h = L.hist + (PASS == 0 ? 0 : q) * NB;
        unsigned long long v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = (unsigned long long)h[c * 64 + lane];
        const SelectPick pk = select_pick_step<PASS>(v, probs[q], &L.prefix[q], &L.rank[q]);   // (pass 0: the rank is T - 1)
        if (lane == 0) {
            L.prefix[q] = pk.prefix;
            L.rank[q] = pk.rank;
            if (PASS == 0 && q == 0) {
                L.count[0] = (long long)L.cnt[0];
                L.count[1] = (long long)L.cnt[1];
                L.count[2] = pk.total;
            }
        }
    }
    __syncthreads();   // (the next pass clears the histograms and reads the prefixes)
}
// All six passes: hd {m, n_nan, W} and the np values of out, NaN where m == 0.
template <class Walk>
RH_SELECT_DEV void select_lds_block(Walk walk, int np, const double *probs, const SelectLds &L, double *out, long long *hd) {
    select_lds_pass<0>(walk, np, probs, L);
    const long long m = L.count[0];
    if (threadIdx.x == 0) {
        hd[0] = m;
        hd[1] = L.count[1];
        hd[2] = L.count[2];
    }
    if (m == 0) {   // (uniform over the workgroup)
        if ((int)threadIdx.x < np) out[threadIdx.x] = __builtin_nan("");
        return;
    }
    select_lds_pass<1>(walk, np, probs, L);
    select_lds_pass<2>(walk, np, probs, L);
    select_lds_pass<3>(walk, np, probs, L);
    select_lds_pass<4>(walk, np, probs, L);
    select_lds_pass<5>(walk, np, probs, L);
    if ((int)threadIdx.x < np) out[threadIdx.x] = bands_value_of(L.prefix[threadIdx.x]);   // after the last pass the prefix IS the key
}

// ---- the pair of an observation with key ko: the weights of the keys below and equal to it (below 2^47) ----
RH_SELECT_DEV void select_pair_add(unsigned long long key, unsigned w, unsigned long long ko, long long &below, long long &equal) {
    if (key >= RH_SELECT_KEY_NAN) return;
    below += key < ko ? (long long)w : 0ll;
    equal += key == ko ? (long long)w : 0ll;
}
RH_SELECT_DEV void select_pair_wave(long long &below, long long &equal) {   // every lane holds the wavefront's sums
    for (int off = 32; off; off >>= 1) {
        below += __shfl_xor(below, off);
        equal += __shfl_xor(equal, off);
    }
}
// the workgroup's sums: shuffles within a wavefront, LDS across the RH_SELECT_BLOCK / 64 of them; thread 0 holds the result
RH_SELECT_DEV void select_pair_reduce(long long &below, long long &equal, long long (*s_part)[2]) {
    select_pair_wave(below, equal);
    if ((threadIdx.x & 63) == 0) {
        s_part[threadIdx.x >> 6][0] = below;
        s_part[threadIdx.x >> 6][1] = equal;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        below = equal = 0;
        for (int w = 0; w < RH_SELECT_BLOCK / 64; ++w) {
            below += s_part[w][0];
            equal += s_part[w][1];
        }
    }
}
// the sums of nparts workgroups' pairs, by one wavefront, in a fixed order
RH_SELECT_DEV void select_pair_partials(const long long *part, int nparts, long long &below, long long &equal) {
    below = equal = 0;
    for (int b = threadIdx.x; b < nparts; b += 64) {
        below += part[2 * b];
        equal += part[2 * b + 1];
    }
    select_pair_wave(below, equal);
}
