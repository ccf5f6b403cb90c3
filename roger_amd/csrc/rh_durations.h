// rh_durations.h -- duration curves (rh_durations_configure): after every step a variable is aggregated to an interval per column, and
// at every interval's end the interval value is counted into a per-column histogram over edges shared by all columns, with the exact
// extremes and the run lengths of a threshold spell, all of which stay on the device.  Part of the one translation unit roger_hip.hip,
// behind rh_events.h.
//
// The clock (uniform over the grid, from D->S as k_scores reads it): t1 = S.time, t0 = t1 - S.dt_secs, iv the interval in seconds
// (86400, 3600 or 600);
//   first   = t0 % iv == 0
//   closes  = t1 % iv == 0 && t1 - t0 <= iv     (a step longer than the interval never closes one: such intervals were never started)
//   k       = t1 / iv - 1 - t_first / iv
//   counted = closes && k >= 0                  (no upper bound on k)
// after_fused && D->skipped ends the launch as for every other observer.  The kernel reads no per-context word that it also writes, so
// no workgroup reads anything another workgroup of its launch advances; a column's words belong to that column: plain loads and stores,
// no atomics.
//
// Column i with mask[i] == 0 (a mask is optional) loads and stores nothing.  Per item j (at most 16), v the plane's value after the step:
//   SUM:   acc = first ? v : acc + v on every step (k_diag's rate rule, the same order of additions); the interval value s = acc.
//          An interval that the configuration found under way sums what was seen from then on -- the rule of an accumulator slot
//          first touched inside its interval.
//   LAST:  nothing on a step that is not counted; on a counted step s = v, and its acc plane stays +0.0 in memory.
// On a counted step, with the item's m edges e_0 < ... < e_{m-1} (finite, strictly ascending, 0 <= m <= 63):
//   bin      s != s ? m + 1 (the NaN bin) : b = #{q : e_q <= s} -- a value on an edge goes to the upper bin, -inf to bin 0, +inf to bin m,
//            -0.0 on an edge 0.0 goes up; count[j][bin][i] += 1 (uint32)
//   extremes mn = s < mn ? s : mn,  mx = s > mx ? s : mx, from +inf / -inf; a NaN compares false and is skipped, of equal zeros the
//            first one seen stays
//   spell    only with a threshold thr (not NaN) and a side:  in = side == BELOW ? s < thr : s >= thr  (a NaN s: false);
//            run = in ? run + 1 : 0;  in && run == 1: n_spells += 1;  longest = max(longest, run)  (uint32 each)
// Spells run over consecutive COUNTED intervals: an hourly or ten-minute interval under a longer step is never started -- it is neither
// counted nor does it break a run.
//
// Storage.  counts [sum of the items' m + 2 bins][n] uint32, item j's bins from bin_off[j], the columns contiguous within a bin: the
// lanes of a wavefront that fall into the same bin share their sectors.  vals [item][{acc, mn, mx}][n] float64, spells
// [item][{run, longest, n_spells}][n] uint32.  Cleared at the configuration, mn / mx to +inf / -inf.
// The edges.  On a counted step the workgroup stages every item's edges in LDS once, 64 doubles per item (16 x 64 x 8 = 8 KiB), NaN
// behind the item's own: `e <= s` is false for a NaN e, so the count over 63 places is the count over the item's m.  b comes from a
// binary search of six probes (32, 16, 8, 4, 2, 1 -- a fixed trip, a select per probe, no branch).
// Cost.  A step that is neither counted nor has a SUM item ends after the scalar loads.  A step that is not counted moves 24 B per SUM
// item and column (the accumulators' shape) and nothing else.  A counted step moves per item and column the value (8 B), acc (16 B,
// SUM), one counter (8 B), mn and mx (16 B read, a store only where one changes) and, with a spell, 12 B read and up to 12 B written.
#pragma once

#define RH_DURATIONS_MAX_ITEMS 16
#define RH_DURATIONS_MAX_EDGES 63
#define RH_DURATIONS_SUM 0
#define RH_DURATIONS_LAST 1
#define RH_DURATIONS_BELOW 0
#define RH_DURATIONS_AT_OR_ABOVE 1
__global__ __launch_bounds__(RH_BLOCK) void k_durations(Arena a, DevState *D, int after_fused) {
    __shared__ double edges[RH_DURATIONS_MAX_ITEMS * 64];
    if (after_fused && D->skipped) return;
    const int64_t t1 = D->S.time, t0 = t1 - D->S.dt_secs, iv = D->durations_interval;
    const bool first = (t0 % iv) == 0;
    const bool closes = (t1 % iv) == 0 && t1 - t0 <= iv;
    const int64_t k = t1 / iv - 1 - D->durations_t_first / iv;
    const bool counted = closes && k >= 0;
    if (!counted && !D->durations_nsum) return;   // (uniform over the grid)
    const int ni = D->durations_nitems;
    if (counted) {   // (uniform: every thread of the workgroup reaches the barrier)
        const double *e = D->durations_edges;
        for (int q = threadIdx.x; q < ni * 64; q += RH_BLOCK) {
            const int j = q >> 6, r = q & 63;
            edges[q] = r < D->durations_nedges[j] ? e[D->durations_edge_off[j] + r] : __builtin_nan("");
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const unsigned char *mask = D->durations_mask;
    if (mask && !mask[i]) return;
    const size_t n = (size_t)a.n;
    for (int j = 0; j < ni; ++j) {
        const bool sum = D->durations_kinds[j] == RH_DURATIONS_SUM;
        if (!sum && !counted) continue;   // LAST: only the value at a counted interval's end
        double v;
        rh_ld(a, D->durations_planes[j], i, v);
        double *p = D->durations_vals + (size_t)j * 3 * n + i;
        double s = v;
        if (sum) {
            if (!first) s = p[0] + v;
            p[0] = s;
        }
        if (!counted) continue;
        const double *E = edges + 64 * j;
        int b = 0;
#pragma unroll
        for (int w = 32; w; w >>= 1) b += E[b + w - 1] <= s ? w : 0;
        if (s != s) b = D->durations_nedges[j] + 1;
        unsigned *c = D->durations_counts + ((size_t)D->durations_bin_off[j] + b) * n + i;
        *c = *c + 1u;
        const double mn = p[n], mx = p[2 * n];
        if (s < mn) p[n] = s;
        if (s > mx) p[2 * n] = s;
        const double thr = D->durations_thr[j];
        if (thr == thr) {
            unsigned *q = D->durations_spells + (size_t)j * 3 * n + i;
            const bool in = D->durations_sides[j] == RH_DURATIONS_BELOW ? s < thr : s >= thr;
            const unsigned run = in ? q[0] + 1u : 0u;
            q[0] = run;
            if (run > q[n]) q[n] = run;
            if (run == 1u) q[2 * n] = q[2 * n] + 1u;
        }
    }
}
