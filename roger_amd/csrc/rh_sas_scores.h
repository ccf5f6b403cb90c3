// rh_sas_scores.h -- scores of the SAS context against observed tracer samples (rh_sas_scores_*, include/roger_hip_sas.h): the kernel
// that scores one day, and what the host tells it.  Included by rh_sas.hip only; the day kernels know nothing of it.
//
// A sample is a bulk sample over a window of days [first_day[k], last_day[k]]; what is compared with it is the flux-weighted mean of
// the simulated concentration over the window, sum(q C) / sum(q).  The clock is the HOST's: it counts the scored days, decides which
// window a day lies in and launches k_sas_scores behind the day's kernel with
//   k        the window's index,  first: the day is the window's first,  closes: the day is its last,
//   day_off  (row of the daily inputs) * n: where the day's weights stand.
// A day outside every window, or inside a window whose first day was never scored, launches nothing: the device holds no counter and
// no clock, it reads no word that it also writes for another thread.
//
// Column i has s = series[i] (no map: s = 0); s < 0 loads and stores nothing.  Per item j = (value, weight, kind), v = value[i] after
// the day, each +, -, *, / one IEEE operation in the order written (the library is built with -ffp-contract=off):
//   BULK:  wd = weight[day_off + i]          MEAN:  wd = 1.0
//       on the window's first day num and den restart from +0.0 (their planes are not loaded);
//       the day is ELIGIBLE if wd > 0 and v == v (a NaN weight is not > 0):  num = num + fl(v * wd);  den = den + wd
//       a day that is not eligible leaves both as they are
//   LAST:  nothing before the closing day
//   on the closing day, o = obs[(j * n_series + s) * K + k]:
//       BULK / MEAN: the sample is COUNTED if o == o and den > 0, sim = num / den
//       LAST:        the sample is COUNTED if o == o and v == v,  sim = v
//       a counted sample:  n += 1.0;  m1 += sim;  m2 += sim * sim;  m3 += sim * o;  d = sim - o;  m4 += d * d;  so += o;  soo += o * o
// The simulated concentration is NaN on a day without flux, so the number of counted samples differs between columns of one series:
// n, so = sum o and soo = sum o^2 are per-column planes beside the four moments of k_scores (rh_scores.h).
// scores [item][9][n] float64 holds {num, den, n, m1, m2, m3, m4, so, soo}, cleared to +0.0, indexed base + m * n + i, plain loads and
// stores, no atomics.  With one series the observation is the same element for every column: one element per wavefront.
//
// Bytes per item and column.  A non-closing day of a BULK item: 8 (v) + 8 (wd) + 16 (num, den loaded) + 16 (stored) = 48 B; MEAN
// saves the weight's 8; the window's first day saves the 16 loaded; a day that is not eligible, and is not the first, stores nothing.
// A LAST item moves nothing on a non-closing day.  A closing day adds, where the sample is counted, 7 planes loaded and stored:
// 112 B more (a LAST item: 8 + 112).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "roger_hip_sas.h"

#define SAS_SCORES_BLOCK 256
#define SAS_SCORES_NMOM 9      // num, den, n, m1, m2, m3, m4, so, soo

struct SasScoresDev {
    const double *val[RH_SAS_SCORES_MAX_ITEMS];     // the width-1 value
    const double *wgt[RH_SAS_SCORES_MAX_ITEMS];     // first row of the DAILY weight; null: none
    int kind[RH_SAS_SCORES_MAX_ITEMS];
    int n_items, n_series;
    int64_t n, n_samples;
    const int32_t *series;                          // [n] or null
    const double *obs;                              // [item][series][sample]
    double *scores;                                 // [item][9][n]
};

__global__ __launch_bounds__(SAS_SCORES_BLOCK) void k_sas_scores(const SasScoresDev *__restrict__ P, int64_t k, int first, int closes,
                                                                 int64_t day_off) {
    const int64_t i = (int64_t)blockIdx.x * SAS_SCORES_BLOCK + threadIdx.x;
    const size_t n = (size_t)P->n;
    if (i >= P->n) return;
    const int s = P->series ? P->series[i] : 0;
    if (s < 0) return;
    const int ni = P->n_items, ns = P->n_series;
    const size_t K = (size_t)P->n_samples;
    const double *obs = P->obs;
    for (int j = 0; j < ni; ++j) {
        const int kind = P->kind[j];
        if (kind == RH_SAS_SCORES_LAST && !closes) continue;
        const double v = P->val[j][i];
        double *p = P->scores + (size_t)j * SAS_SCORES_NMOM * n + (size_t)i;
        double sim = v;
        bool counted = v == v;
        if (kind != RH_SAS_SCORES_LAST) {
            const double wd = kind == RH_SAS_SCORES_BULK ? P->wgt[j][day_off + i] : 1.0;
            double num = 0.0, den = 0.0;
            if (!first) {
                num = p[0];
                den = p[n];
            }
            const bool eligible = wd > 0.0 && v == v;
            if (eligible) {
                const double t = v * wd;   // rounded before it is added
                num = num + t;
                den = den + wd;
            }
            if (first || eligible) {
                p[0] = num;
                p[n] = den;
            }
            if (!closes) continue;
            counted = den > 0.0;
            sim = num / den;
        }
        // one series: the same element for every column -- one element per wavefront
        const double o = ns == 1 ? obs[(size_t)j * K + (size_t)k] : obs[((size_t)j * ns + s) * K + (size_t)k];
        if (counted && o == o) {
            const double cn = p[2 * n] + 1.0;
            const double m1 = p[3 * n] + sim;
            const double sq = sim * sim;
            const double m2 = p[4 * n] + sq;
            const double sx = sim * o;
            const double m3 = p[5 * n] + sx;
            const double d = sim - o;
            const double dd = d * d;
            const double m4 = p[6 * n] + dd;
            const double so = p[7 * n] + o;
            const double oo = o * o;
            const double soo = p[8 * n] + oo;
            p[2 * n] = cn;
            p[3 * n] = m1;
            p[4 * n] = m2;
            p[5 * n] = m3;
            p[6 * n] = m4;
            p[7 * n] = so;
            p[8 * n] = soo;
        }
    }
}
