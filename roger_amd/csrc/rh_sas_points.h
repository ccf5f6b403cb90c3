// rh_sas_points.h -- time series at observation columns of the SAS context (rh_sas_points_*, include/roger_hip_sas.h): the kernel that
// records one row, and what the host tells it.  Included by rh_sas.hip only; the day kernels know nothing of it.
//
// A row holds, for every configured array in configured order, the configured cells in configured order, `width` doubles each -- 1 for a
// per-cell scalar, ages for tt_* / mtt_* / sa_* / msa_*, ages + 1 for TT_* -- with the age axis contiguous:
//   row[off[j] + k * width[j] + a] = array_j[cells[k] * width[j] + a]
// k_sas_points is that gather and nothing else, launched on the context's stream behind a completed day: every value is the bits
// rh_sas_download would return.  An array's K * width values are one flat index space cut into workgroups of SAS_POINTS_BLOCK
// threads: consecutive lanes read consecutive ages of a column (unit stride, a new column every `width` lanes) and, where width is 1,
// consecutive lanes are consecutive cells, so the scalars of 256 cells share one workgroup.  Stores are unit stride throughout.
// first_block[] cuts the grid by array: everything a workgroup looks up from it is uniform.  Row number and ring slot are the
// host's (it enqueues every row): the destination arrives as an argument, there is no counter on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "roger_hip_sas.h"

#define SAS_POINTS_BLOCK 256

struct SasPointsDev {
    const double *src[RH_SAS_POINTS_MAX_ARRAYS];
    int64_t off[RH_SAS_POINTS_MAX_ARRAYS];               // first element of the array's block in a row
    int first_block[RH_SAS_POINTS_MAX_ARRAYS + 1];       // workgroups [first_block[j], first_block[j + 1]) gather array j
    int width[RH_SAS_POINTS_MAX_ARRAYS];
    int n_arrays, n_cells;
    int64_t cells[RH_SAS_POINTS_MAX_CELLS];
};

__global__ __launch_bounds__(SAS_POINTS_BLOCK) void k_sas_points(const SasPointsDev *__restrict__ P, double *__restrict__ row) {
    const int b = (int)blockIdx.x;
    int j = 0;
    while (j + 1 < P->n_arrays && b >= P->first_block[j + 1]) ++j;
    const unsigned w = (unsigned)P->width[j];
    const unsigned e = (unsigned)(b - P->first_block[j]) * SAS_POINTS_BLOCK + threadIdx.x;   // (at most 256 cells x 4096 ages = 2^20)
    if (e >= (unsigned)P->n_cells * w) return;
    const unsigned k = e / w, a = e - k * w;
    row[P->off[j] + e] = P->src[j][P->cells[k] * (int64_t)w + a];
}
