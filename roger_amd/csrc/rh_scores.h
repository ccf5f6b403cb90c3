// rh_scores.h -- scores against observed series (rh_scores_configure): after every step a variable is aggregated to the observation
// interval per column, and at every interval's end the result is compared with the observation of the column's series and added into
// four per-column moments that stay on the device.  Part of the one translation unit roger_hip.hip, behind rh_control.h (k_diag).
//
// The clock (uniform over the grid, from D->S as k_diag reads it): t1 = S.time, t0 = t1 - S.dt_secs, iv the interval in seconds;
//   first  = t0 % iv == 0
//   closes = t1 % iv == 0 && t1 - t0 <= iv      (a step longer than the interval never closes one: such intervals were never started)
//   k      = t1 / iv - 1 - t_first / iv,  scored only when 0 <= k < n_intervals
// The kernel reads no per-context word that it also writes, so no workgroup reads anything another workgroup of its launch advances.
//
// Column i has s = series[i] (no map: s = 0); s < 0 loads and stores nothing.  Per item j, v the plane's value after the step:
//   SUM:   acc = first ? v : acc + v on every step (k_diag's rate rule, the same order of additions)
//   LAST:  nothing on a non-closing step; on a closing step acc = v, and its acc plane stays +0.0 in memory
//   on a scored closing step o = obs[(j * n_series + s) * n_intervals + k]; if o == o (not NaN), each +, -, * one IEEE operation in
//   this order (the library is built with -ffp-contract=off):
//       m1 += acc;   m2 += acc * acc;   m3 += acc * o;   d = acc - o;  m4 += d * d
//   A NaN acc goes in as it is: only a missing observation skips.
// scores [item][5][n] float64 holds {acc, m1, m2, m3, m4}, cleared to +0.0, indexed base + m * n + i like the accumulators, plain loads
// and stores, no atomics.  Thread 0 of workgroup 0 stores closed[k] = 1 on a scored closing step (a byte nobody reads on the device).
// A non-closing step moves 24 B per SUM item and column (the accumulators' shape), a scored closing step 80 B more per item.
#pragma once

#define RH_SCORES_MAX_ITEMS 16
#define RH_SCORES_SUM 0
#define RH_SCORES_LAST 1
__global__ __launch_bounds__(RH_BLOCK) void k_scores(Arena a, DevState *D, int after_fused) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n || (after_fused && D->skipped)) return;
    const int64_t t1 = D->S.time, t0 = t1 - D->S.dt_secs, iv = D->scores_interval;
    const bool first = (t0 % iv) == 0;
    const bool closes = (t1 % iv) == 0 && t1 - t0 <= iv;
    const int64_t k = t1 / iv - 1 - D->scores_t_first / iv, nk = D->scores_nintervals;
    const bool scored = closes && k >= 0 && k < nk;
    if (i == 0 && scored) D->scores_closed[k] = 1;
    const int ns = D->scores_nseries, ni = D->scores_nitems;
    const int s = D->scores_series ? D->scores_series[i] : 0;
    if (s < 0) return;
    const double *obs = D->scores_obs;
    const size_t n = (size_t)a.n;
    for (int j = 0; j < ni; ++j) {
        const bool sum = D->scores_kinds[j] == RH_SCORES_SUM;
        if (!sum && !scored) continue;   // LAST: only the value at the interval's end counts, and only where it is compared
        double v;
        rh_ld(a, D->scores_planes[j], i, v);
        double *p = D->scores + (size_t)j * 5 * n + i;
        double acc = v;
        if (sum) {
            if (!first) acc = p[0] + v;
            p[0] = acc;
        }
        if (!scored) continue;
        // one series: the same element for every column -- one element per wavefront
        const double o = ns == 1 ? obs[(size_t)j * nk + k] : obs[((size_t)j * ns + s) * nk + k];
        if (o == o) {
            const double m1 = p[n] + acc;
            const double sq = acc * acc;
            const double m2 = p[2 * n] + sq;
            const double so = acc * o;
            const double m3 = p[3 * n] + so;
            const double d = acc - o;
            const double dd = d * d;
            const double m4 = p[4 * n] + dd;
            p[n] = m1;
            p[2 * n] = m2;
            p[3 * n] = m3;
            p[4 * n] = m4;
        }
    }
}
