// rh_sas.hip -- the C ABI of the SAS / oxygen-18 transport step for gfx950 (kernels: rh_sas_kernels.h, rh_sas_solvers_impl.h)
// (include/roger_hip_sas.h).
//
// One workgroup per soil column.  The age axis is laid out blocked over the workgroup: thread t
// owns the E consecutive age classes [t * E, (t + 1) * E) of every age vector in registers, so the
// whole day -- 2 inflows, 5 outgoing fluxes with `substeps` sub-steps each, storage concentrations,
// age statistics, ageing -- runs on one read and one write of the four state vectors
// (sa_rz, msa_rz, sa_ss, msa_ss): 8 * ages * 8 bytes per column and day.  The arithmetic is
// dominated by the power-law SAS function, 5 * substeps * (ages + 1) `pow` per column and day
// (3 * 10^4 at ages = 1000), which makes this kernel fp64-ALU bound, not HBM bound.
//
// Every formula below is a per-element restatement of the reference's array expressions (file:line
// in the comments; roger/core/transport.py unless said otherwise) with the reference's operation
// order; no FMA contraction (-ffp-contract=off).  Two deliberate differences, both at rounding
// level: prefix sums are block scans instead of sequential `cumsum`s, sums over ages are tree
// reductions instead of numpy's pairwise sums.  The scan is built so that what the algorithm is
// sensitive to still holds exactly: cumulative values are non-decreasing for non-negative input and
// an empty age class contributes an exact 0 to every difference of cumulative values.
#include <hip/hip_runtime.h>
#include <cstdio>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rh_host.h"
#include "roger_hip.h"
#include "roger_hip_sas.h"
#include "rh_sas_dev.h"
#include "rh_sas_points.h"
#include "rh_sas_totals.h"
#include "rh_sas_zonal.h"
#include "rh_sas_scores.h"
#include "rh_sas_bands.h"
#include "rh_sas_bands_zonal.h"

#include <algorithm>
#include <memory>

static const char *const SAS_NAMES[] = {
#define RH_SAS_ARRAY(name, kind, when) #name,
#include "rh_sas_arrays.def"
#undef RH_SAS_ARRAY
};
static const unsigned char SAS_KIND[] = {
#define RH_SAS_ARRAY(name, kind, when) K_##kind,
#include "rh_sas_arrays.def"
#undef RH_SAS_ARRAY
};
static const unsigned char SAS_WHEN[] = {
#define RH_SAS_ARRAY(name, kind, when) W_##when,
#include "rh_sas_arrays.def"
#undef RH_SAS_ARRAY
};

__global__ void k_selftest_div(const double *a, const double *d, double *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = udiv(a[i], udiv_prepare(d[i]));
}
__global__ void k_selftest_pow(const double *x, const double *k, double *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const PowConsts C = load_pow_consts(SAS_LOG_T);
    if (i >= n) return;
    // the same dispatch as the power-law branch of calc_tt_family: exponents 0.5 / 1.5 / 1 through the square root
    if (k[i] == 0.5) out[i] = sqrt_unit(x[i]);
    else if (k[i] == 1.5) out[i] = x[i] * sqrt_unit(x[i]);
    else if (k[i] == 1.0) out[i] = x[i];
    else if (k[i] == 0.2) {   // the fifth-root path with its range check
        int e2;
        const double y = pow_fifth(x[i], &e2);
        out[i] = (e2 < -126) ? sas_pow_ratio(C, x[i], 1.0, 0.0, k[i]) : y;
    } else out[i] = sas_pow_ratio(C, x[i], 1.0, 0.0, k[i]);
}

// ---------------------------------------------------------------------------------------------
// host side: context and C ABI
// ---------------------------------------------------------------------------------------------
// A ring of `cap` rows of row_elems float64 on the device, row r at r mod cap, and the rows' tags in a host ring of the same capacity:
// what the points, the totals and the zonal totals record into.  The host enqueues every row, so it counts them.  cap 0: the observer is off.
struct SasRing {
    DevBuf<double> ring;
    std::unique_ptr<int64_t[]> tags;
    int64_t cap = 0, row_elems = 0, rows = 0;
    bool on() const { return cap != 0; }
    double *next_row() const { return ring + (size_t)(rows % cap) * (size_t)row_elems; }
    void enqueued(int64_t tag) { tags[(size_t)(rows++ % cap)] = tag; }   // (the launches into next_row() are in the stream)
    hipError_t release() {
        tags.reset();
        cap = row_elems = rows = 0;
        return ring.release();
    }
};

struct rh_sas_ctx {
    Stream stream;                   // first member: destroyed last, after everything that was enqueued on it has been released
    rh_sas_config cfg = {};
    DevBuf<void> arr[SA_COUNT];      // the arrays of rh_sas_arrays.def this configuration holds
    int64_t elems[SA_COUNT] = {};
    DevBuf<int> unsupported;
    bool timing = false;
    EventPool events;                // pairs (start, stop) around the day's launch
    // time series at observation columns (rh_sas_points_configure): the ring (off: no k_sas_points launch) and what the kernel is told
    SasRing points;
    DevBuf<SasPointsDev> points_cfg;
    int points_blocks = 0;           // workgroups of one row's launch
    // catchment totals (rh_sas_totals_configure): the ring (off: no launches); the width-1 partials, the two level buffers of the age
    // rule (rh_sas_totals.h), the mask on the device, and the host's copy of what the kernels are told
    SasRing totals;
    DevBuf<double> totals_part, totals_lvl[2];
    DevBuf<SasTotalsDev> totals_cfg;
    DevBuf<unsigned char> totals_mask;
    SasTotalsDev totals_host = {};
    int totals_width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *totals_src[RH_SAS_TOTALS_MAX_ITEMS] = {};   // the age items' arrays
    int64_t totals_ncells = 0;
    // zonal totals (rh_sas_zonal_configure): the ring (off: no launches); the slots' width-1 partials, the ONE level-1 buffer of the age
    // rule, the index over the zone map (rh_sas_zonal.h) and where its parts start
    SasRing zonal;
    DevBuf<double> zonal_part, zonal_lvl;
    DevBuf<SasZonalDev> zonal_cfg;
    DevBuf<int> zonal_index;
    SasZonalDev zonal_host = {};
    int zonal_nzones = 0;
    int zonal_width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *zonal_src[RH_SAS_TOTALS_MAX_ITEMS] = {};
    int64_t zonal_at[SZ_PARTS] = {};
    int64_t zonal_ntiles = 0;
    std::vector<int64_t> zonal_ncells;   // cells of every zone
    // scores against observed samples (rh_sas_scores_configure): the moments, the observations and the series map on the device; the
    // windows, the day count, the window the count stands in or before, and the closed flags are the host's (rh_sas_scores.h)
    DevBuf<double> scores_buf, scores_obs;
    DevBuf<int32_t> scores_series;
    DevBuf<SasScoresDev> scores_cfg;
    std::vector<int64_t> scores_first, scores_last;
    std::vector<unsigned char> scores_closed;
    int scores_items = 0;            // 0: not configured, no launches
    bool scores_accumulate = false;  // an item is BULK or MEAN: the days before a window's last are launched too
    int64_t scores_days = 0, scores_k = 0, scores_open = -1;
    // transport bands (rh_sas_bands_configure): num / den, the key planes, the global histograms, the selection's few words (prefixes,
    // ranks, counts: SasBandsWords), the result and what the kernels are told on the device; the windows, the day count, the window the
    // count stands in or before, the closed flags and the observations' copy are the host's (rh_sas_bands.h)
    DevBuf<double> bands_acc, bands_rows, bands_obs;
    DevBuf<unsigned long long> bands_keys, bands_hist;
    DevBuf<long long> bands_words, bands_hdr, bands_pair, bands_part;
    DevBuf<unsigned char> bands_mask;
    DevBuf<unsigned short> bands_weight;
    DevBuf<SasBandsDev> bands_cfg;
    std::vector<int64_t> bands_first, bands_last;
    std::vector<unsigned char> bands_closed;
    std::vector<double> bands_obs_host;   // [item][sample]; empty: no observations
    int bands_items = 0, bands_probs = 0;   // 0: not configured, no launches
    bool bands_accumulate = false;          // an item is BULK or MEAN: the days before a window's last are launched too
    int64_t bands_days = 0, bands_k = 0, bands_open = -1;
    // ... per zone (rh_sas_bands_configure_zonal, rh_sas_bands_zonal.h): the result gains the zone axis behind the item's, the observations'
    // copy is [item][zone][sample]; the zones' column lists
    int bands_zones = 0;                    // 0: the plain configuration (k_sas_bands_hist / _pick); else k_sas_bands_zonal on (zones, items)
    DevBuf<long long> bands_zone_off;
    DevBuf<int> bands_zone_cols;
    std::string err;
};
static std::string g_sas_create_err;

static int sfail(rh_sas_ctx *ctx, int code, const std::string &msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_sas_create_err = msg;
    return code;
}
#define SHIPCHK(ctx, call)                                                                                      \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) return sfail(ctx, RH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

static int64_t sas_elems(const rh_sas_config &c, int a) {
    const int when = SAS_WHEN[a];
    if (when == W_STATS && !c.age_statistics) return 0;
    if (when == W_DIAG && !c.keep_distributions) return 0;
    if (when == W_ANION && c.tracer == RH_SAS_TRACER_OXYGEN18) return 0;
    switch (SAS_KIND[a]) {
    case K_AGE: return c.n_cells * c.ages;
    case K_NAGE: return c.n_cells * (c.ages + 1);
    case K_CELL: return c.n_cells;
    case K_DAILY: return c.n_cells * c.forcing_days;
    case K_PARAM: return c.n_cells * 8;
    case K_MASK: return c.n_cells;
    }
    return 0;
}

// ---- what the observers' calls further down share; the rules of a ring itself are rh_host.h's ----
static int sas_check_capacity(rh_sas_ctx *ctx, const std::string &who, int64_t capacity) {
    const std::string why = ring_capacity_refusal(who, capacity, 0);   // (every configure call bounds its ring's bytes itself)
    return why.empty() ? RH_OK : sfail(ctx, RH_ERR_ARG, why);
}
// RH_ERR_STATE for the function `who` unless `configure` has switched its observer on
static int sas_on(rh_sas_ctx *ctx, bool on, const char *who, const char *configure) {
    return on ? RH_OK : sfail(ctx, RH_ERR_STATE, std::string(who) + ": " + configure + " has not been called");
}
// rows [first_row, first_row + n_rows) of a ring that is on and their tags to the host, for the function `who`.  Synchronises.
static int sas_ring_read(rh_sas_ctx *ctx, const char *who, const SasRing &r, int64_t first_row, int64_t n_rows, int64_t *tags, double *values,
                         size_t value_bytes) {
    const size_t nv = (size_t)r.row_elems;
    const std::string why = ring_range_refusal(who, first_row, n_rows, r.rows, r.cap);
    if (!why.empty()) return sfail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!tags || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return sfail(ctx, RH_ERR_ARG, std::string(who) + ": size mismatch (n_rows x row_elems float64)");
    const int rc = ring_pieces(first_row, n_rows, r.cap, [&](int64_t done, int64_t slot, int64_t m) -> int {
        SHIPCHK(ctx, hipMemcpyAsync(values + (size_t)done * nv, r.ring + (size_t)slot * nv, (size_t)m * nv * sizeof(double), hipMemcpyDeviceToHost,
                                    ctx->stream));
        std::copy(r.tags.get() + slot, r.tags.get() + slot + m, tags + done);
        return RH_OK;
    });
    return rc ? rc : rh_sas_sync(ctx);
}

// pass P of the transport bands' selection (rh_sas_bands.h): the histograms over the key planes, then the pick of one workgroup
template <int P>
static void sas_bands_pass(rh_sas_ctx *ctx, unsigned grid, int64_t k) {
    const SasBandsDev *cfg = ctx->bands_cfg.get();
    hipLaunchKernelGGL(k_sas_bands_hist<P>, dim3(grid), dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg);
    hipLaunchKernelGGL(k_sas_bands_pick<P>, dim3(1), dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg, k);
}

extern "C" {

void rh_sas_default_config(rh_sas_config *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_cells = 1;
    cfg->ages = 1000;         // benchmarks/SVATOXYGEN18_benchmark.py:28-44
    cfg->substeps = 1;        // settings.sas_solver_substeps default, roger/settings.py:120
    cfg->forcing_days = 1;
    cfg->vsmow = 2005.2e-6;   // roger/settings.py:76-78
    cfg->d18O_min = -20;
    cfg->d18O_max = 0;
}

const char *rh_sas_last_error(const rh_sas_ctx *ctx) { return ctx ? ctx->err.c_str() : g_sas_create_err.c_str(); }
int rh_sas_num_arrays(void) { return SA_COUNT; }
const char *rh_sas_array_name(int a) { return (a >= 0 && a < SA_COUNT) ? SAS_NAMES[a] : nullptr; }
int rh_sas_array_is_int(int a) { return (a >= 0 && a < SA_COUNT) ? (SAS_KIND[a] == K_MASK) : -1; }
int rh_sas_array_index(const char *name) {
    if (!name) return -1;
    for (int a = 0; a < SA_COUNT; ++a)
        if (std::strcmp(SAS_NAMES[a], name) == 0) return a;
    return -1;
}
int64_t rh_sas_array_elems(const rh_sas_ctx *ctx, int a) { return (ctx && a >= 0 && a < SA_COUNT) ? ctx->elems[a] : 0; }

int rh_sas_create(const rh_sas_config *cfg, rh_sas_ctx **out) {
    if (!cfg || !out) return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: null argument");
    if (cfg->n_cells <= 0 || cfg->n_cells > 0x7fffffffLL) return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: n_cells out of range");
    if (cfg->ages < 2 || cfg->ages + 1 > RH_SAS_MAX_NAGES)
        return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: ages must be in [2, RH_SAS_MAX_NAGES - 1]");
    if (cfg->substeps < 1 || cfg->forcing_days < 1) return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: substeps and forcing_days must be >= 1");
    if (cfg->tracer < RH_SAS_TRACER_OXYGEN18 || cfg->tracer > RH_SAS_TRACER_VIRTUAL)
        return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: tracer must be RH_SAS_TRACER_OXYGEN18, _BROMIDE, _CHLORIDE or _VIRTUAL");
    if (cfg->solver < RH_SAS_SOLVER_DETERMINISTIC || cfg->solver > RH_SAS_SOLVER_RK4)
        return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: solver must be RH_SAS_SOLVER_DETERMINISTIC, _EULER or _RK4");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return sfail(nullptr, RH_ERR_NODEVICE, "rh_sas_create: no HIP device visible (this backend has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: device ordinal out of range");
    SHIPCHK(nullptr, hipSetDevice(cfg->device));
    rh_sas_ctx *ctx = new (std::nothrow) rh_sas_ctx();
    if (!ctx) return sfail(nullptr, RH_ERR_ARG, "rh_sas_create: out of host memory");
    ctx->cfg = *cfg;
    auto bail = [&](hipError_t e, const char *what) {
        std::string msg = std::string(what) + ": " + hipGetErrorString(e);
        rh_sas_destroy(ctx);
        return sfail(nullptr, RH_ERR_HIP, msg);
    };
    hipError_t e;
    if ((e = ctx->stream.create()) != hipSuccess) return bail(e, "hipStreamCreate");
    for (int a = 0; a < SA_COUNT; ++a) {
        const int64_t ne = sas_elems(*cfg, a);
        if (!ne) continue;
        const size_t bytes = (size_t)ne * (SAS_KIND[a] == K_MASK ? sizeof(int32_t) : sizeof(double));
        if ((e = ctx->arr[a].alloc(bytes)) != hipSuccess) return bail(e, "hipMalloc(SAS array)");
        if ((e = hipMemsetAsync(ctx->arr[a], 0, bytes, ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
        ctx->elems[a] = ne;
    }
    if ((e = ctx->unsupported.alloc(sizeof(int))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemsetAsync(ctx->unsupported, 0, sizeof(int), ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
    {   // maskCatch defaults to 1 (roger/variables.py)
        std::vector<int32_t> ones((size_t)cfg->n_cells, 1);
        if ((e = hipMemcpyAsync(ctx->arr[SA_maskCatch], ones.data(), ones.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
            return bail(e, "hipMemcpy(maskCatch)");
        if (cfg->tracer != RH_SAS_TRACER_OXYGEN18) {   // alpha_transp, alpha_q: initial=1 (roger/variables.py:5377-5405)
            std::vector<double> one((size_t)cfg->n_cells, 1.0);
            for (int a : {SA_alpha_transp, SA_alpha_q})
                if ((e = hipMemcpyAsync(ctx->arr[a], one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
                    return bail(e, "hipMemcpy(alpha)");
        }
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    }
    *out = ctx;
    return RH_OK;
}

void rh_sas_destroy(rh_sas_ctx *ctx) {
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
}

int rh_sas_set_stream(rh_sas_ctx *ctx, void *hip_stream) {
    if (!ctx) return RH_ERR_ARG;
    SHIPCHK(ctx, ctx->stream.adopt((hipStream_t)hip_stream));
    return RH_OK;
}

int rh_sas_sync(rh_sas_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    int bad = 0;
    SHIPCHK(ctx, hipMemcpyAsync(&bad, ctx->unsupported, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad & 2)   // (the invariant blk_cumsum's top value rests on, checked by every day's kernel before it stores: ADVICE r3)
        return sfail(ctx, RH_ERR_STATE, "internal: an age class above ages - 1 (register padding of the age axis) holds water after a day's fluxes");
    if (bad)
        return sfail(ctx, RH_ERR_STATE,
                     "a column's sas_params select a code that is none of the reference's SAS families (1, 2, 3, 31-37, 4, 51, 52, 6, 61, 62)");
    return RH_OK;
}

static int sas_check(rh_sas_ctx *ctx, int a, size_t bytes, const void *host, const char *who) {
    if (!ctx) return RH_ERR_ARG;
    if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": unknown array id");
    if (!ctx->arr[a]) return sfail(ctx, RH_ERR_STATE, std::string(who) + ": array " + SAS_NAMES[a] + " is not held by this context (age_statistics / keep_distributions)");
    const size_t want = (size_t)ctx->elems[a] * (SAS_KIND[a] == K_MASK ? sizeof(int32_t) : sizeof(double));
    if (bytes != want) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": size mismatch for array " + SAS_NAMES[a]);
    if (!host) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": null host pointer");
    return RH_OK;
}

int rh_sas_upload(rh_sas_ctx *ctx, int a, const void *host, size_t bytes) {
    const int rc = sas_check(ctx, a, bytes, host, "rh_sas_upload");
    if (rc) return rc;
    SHIPCHK(ctx, hipMemcpyAsync(ctx->arr[a], host, bytes, hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

int rh_sas_download(rh_sas_ctx *ctx, int a, void *host, size_t bytes) {
    const int rc = sas_check(ctx, a, bytes, host, "rh_sas_download");
    if (rc) return rc;
    SHIPCHK(ctx, hipMemcpyAsync(host, ctx->arr[a], bytes, hipMemcpyDeviceToHost, ctx->stream));
    return rh_sas_sync(ctx);
}

static int sas_check_cells(rh_sas_ctx *ctx, int a, int64_t first, int64_t cnt, size_t bytes, const void *host, const char *who,
                           size_t *offset) {
    if (!ctx) return RH_ERR_ARG;
    if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": unknown array id");
    if (!ctx->arr[a]) return sfail(ctx, RH_ERR_STATE, std::string(who) + ": array " + SAS_NAMES[a] + " is not held by this context");
    if (SAS_KIND[a] == K_DAILY) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": daily inputs are (forcing_days, n_cells); use the whole-array call");
    if (first < 0 || cnt <= 0 || first + cnt > ctx->cfg.n_cells) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": cell range out of bounds");
    const size_t row = (size_t)(ctx->elems[a] / ctx->cfg.n_cells) * (SAS_KIND[a] == K_MASK ? sizeof(int32_t) : sizeof(double));
    if (bytes != row * (size_t)cnt) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": size mismatch for array " + SAS_NAMES[a]);
    if (!host) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": null host pointer");
    *offset = row * (size_t)first;
    return RH_OK;
}

int rh_sas_upload_cells(rh_sas_ctx *ctx, int a, int64_t first_cell, int64_t n_cells, const void *host, size_t bytes) {
    size_t off;
    const int rc = sas_check_cells(ctx, a, first_cell, n_cells, bytes, host, "rh_sas_upload_cells", &off);
    if (rc) return rc;
    SHIPCHK(ctx, hipMemcpyAsync((char *)ctx->arr[a].get() + off, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

int rh_sas_download_cells(rh_sas_ctx *ctx, int a, int64_t first_cell, int64_t n_cells, void *host, size_t bytes) {
    size_t off;
    const int rc = sas_check_cells(ctx, a, first_cell, n_cells, bytes, host, "rh_sas_download_cells", &off);
    if (rc) return rc;
    SHIPCHK(ctx, hipMemcpyAsync(host, (const char *)ctx->arr[a].get() + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return rh_sas_sync(ctx);
}

int rh_sas_set_daily_from_device(rh_sas_ctx *ctx, int a, int64_t day_row, const double *dev_src) {
    if (!ctx) return RH_ERR_ARG;
    if (a < 0 || a >= SA_COUNT || SAS_KIND[a] != K_DAILY) return sfail(ctx, RH_ERR_ARG, "rh_sas_set_daily_from_device: not a daily input array");
    if (day_row < 0 || day_row >= ctx->cfg.forcing_days || !dev_src) return sfail(ctx, RH_ERR_ARG, "rh_sas_set_daily_from_device: bad row or null source");
    SHIPCHK(ctx, hipMemcpyAsync((double *)ctx->arr[a].get() + day_row * ctx->cfg.n_cells, dev_src, (size_t)ctx->cfg.n_cells * sizeof(double),
                                hipMemcpyDeviceToDevice, ctx->stream));
    return RH_OK;
}

void *rh_sas_array_device_ptr(rh_sas_ctx *ctx, int a) { return (ctx && a >= 0 && a < SA_COUNT) ? ctx->arr[a].get() : nullptr; }

int rh_sas_stages(rh_sas_ctx *ctx, int64_t day, int stages) {
    if (!ctx) return RH_ERR_ARG;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_stages: negative day");
    if ((stages & ~(RH_SAS_ALL | RH_SAS_RESCALE)) || !stages) return sfail(ctx, RH_ERR_ARG, "rh_sas_stages: bad stage mask");
    const rh_sas_config &c = ctx->cfg;
    if ((stages & RH_SAS_STORAGE) && c.age_statistics && !c.keep_distributions &&
        (!(stages & RH_SAS_TRANSP) || !(stages & RH_SAS_Q_SS)))
        return sfail(ctx, RH_ERR_STATE,
                     "rh_sas_stages: age statistics need the transpiration and percolation stages in the same launch, or keep_distributions");
    SasArgs args;
    args.n = c.n_cells;
    args.day_off = (day % c.forcing_days) * c.n_cells;
    args.ages = c.ages;
    args.substeps = c.substeps;
    args.stages = stages;
    args.stats = c.age_statistics ? 1 : 0;
    args.diag = c.keep_distributions ? 1 : 0;
    args.tracer = c.tracer;
    args.vsmow = c.vsmow;
    args.dmin = c.d18O_min;
    args.dmax = c.d18O_max;
    args.unsupported = ctx->unsupported;
    for (int a = 0; a < SA_COUNT; ++a) args.a[a] = ctx->arr[a];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (ctx->timing) {
        SHIPCHK(ctx, ctx->events.next_pair(&ev0, &ev1));
        ctx->events.taken();
        SHIPCHK(ctx, hipEventRecord(ev0, ctx->stream));
    }
    if (c.solver != RH_SAS_SOLVER_DETERMINISTIC && (stages & RH_SAS_ALL)) {
        // the explicit solvers evaluate all fluxes of a sub-step on one state: the day cannot be cut into stages
        if (stages != RH_SAS_ALL)
            return sfail(ctx, RH_ERR_ARG, "rh_sas_stages: with an explicit solver the day runs in one launch (RH_SAS_ALL); only RH_SAS_RESCALE may run on its own");
        const bool anion = c.tracer != RH_SAS_TRACER_OXYGEN18;
        const int rc = c.solver == RH_SAS_SOLVER_RK4 ? (anion ? rh_sas_launch_rk4_anion : rh_sas_launch_rk4_iso)(ctx->stream, args)
                                                     : (anion ? rh_sas_launch_euler_anion : rh_sas_launch_euler_iso)(ctx->stream, args);
        if (rc) return sfail(ctx, rc, "rh_sas_stages: unknown solver");
        SHIPCHK(ctx, hipGetLastError());
        if (ctx->timing) SHIPCHK(ctx, hipEventRecord(ev1, ctx->stream));
        return RH_OK;
    }
    // smallest workgroup whose blocked layout covers the ages + 1 edges (rh_sas_kernels.h; the isotope and the anion kernels are
    // translation units of their own, rh_sas_det_iso.hip / rh_sas_det_anion.hip)
#ifdef RH_SAS_PHASES
    static unsigned long long *d_phases = nullptr;
    if (!d_phases) (void)hipMalloc((void **)&d_phases, 32 * sizeof(unsigned long long));
    (void)hipMemsetAsync(d_phases, 0, 32 * sizeof(unsigned long long), ctx->stream);
    args.phases = d_phases;
#endif
    const int lrc = (ctx->cfg.tracer != RH_SAS_TRACER_OXYGEN18 ? rh_sas_launch_det_anion : rh_sas_launch_det_iso)(ctx->stream, args, (unsigned)ctx->cfg.n_cells, c.ages + 1);
#ifdef RH_SAS_PHASES
    {
        unsigned long long h[32];
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipMemcpy(h, d_phases, sizeof(h), hipMemcpyDeviceToHost);
        unsigned long long tot = 0;
        for (int k = 0; k < 16; ++k) tot += h[k];
        std::fprintf(stderr, "sas phases, cycles per column (day %lld):", (long long)day);
        for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %d:%.0f", k, (double)h[k] / (double)ctx->cfg.n_cells);
        std::fprintf(stderr, "  total %.0f\n", (double)tot / (double)ctx->cfg.n_cells);
    }
#endif
    if (lrc) return sfail(ctx, lrc, "rh_sas_stages: the age axis does not fit the kernel shapes of this build");
    SHIPCHK(ctx, hipGetLastError());
    if (ctx->timing) SHIPCHK(ctx, hipEventRecord(ev1, ctx->stream));
    return RH_OK;
}

// ---- time series at observation columns (include/roger_hip_sas.h) ----
// one row behind what the stream holds so far: the gather into the ring's next slot, the tag beside it
static int sas_points_enqueue(rh_sas_ctx *ctx, int64_t tag) {
    hipLaunchKernelGGL(k_sas_points, dim3((unsigned)ctx->points_blocks), dim3(SAS_POINTS_BLOCK), 0, ctx->stream, ctx->points_cfg.get(),
                       ctx->points.next_row());
    SHIPCHK(ctx, hipGetLastError());
    ctx->points.enqueued(tag);
    return RH_OK;
}

static int sas_totals_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day);
static int sas_zonal_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day);
static int sas_scores_enqueue(rh_sas_ctx *ctx, int64_t day);
static int sas_bands_enqueue(rh_sas_ctx *ctx, int64_t day);

// a whole day and, with points, totals, zonal totals, scores or bands configured, their rows, the day's scoring and its band work
static int sas_day(rh_sas_ctx *ctx, int64_t day) {
    int rc = rh_sas_stages(ctx, day, RH_SAS_ALL);
    if (!rc && ctx->points.on()) rc = sas_points_enqueue(ctx, day);
    if (!rc && ctx->totals.on()) rc = sas_totals_enqueue(ctx, day, day);
    if (!rc && ctx->zonal.on()) rc = sas_zonal_enqueue(ctx, day, day);
    if (!rc && ctx->scores_items) rc = sas_scores_enqueue(ctx, day);
    if (!rc && ctx->bands_items) rc = sas_bands_enqueue(ctx, day);
    return rc;
}

int rh_sas_step(rh_sas_ctx *ctx, int64_t day) {
    if (!ctx) return RH_ERR_ARG;
    return sas_day(ctx, day);
}

int rh_sas_run_days(rh_sas_ctx *ctx, int64_t day0, int64_t ndays) {
    if (!ctx) return RH_ERR_ARG;
    if (ndays < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_run_days: negative ndays");
    for (int64_t d = 0; d < ndays; ++d) {
        const int rc = sas_day(ctx, day0 + d);
        if (rc) return rc;
    }
    return RH_OK;
}

int rh_sas_points_configure(rh_sas_ctx *ctx, const int64_t *cells, int n_cells, const int *arrays, int n_arrays, int64_t capacity) {
    const std::string who = "rh_sas_points_configure: ";
    if (!ctx) return RH_ERR_ARG;
    if (n_cells < 0 || n_cells > RH_SAS_POINTS_MAX_CELLS)
        return sfail(ctx, RH_ERR_ARG, who + "n_cells = " + std::to_string(n_cells) + " (0 ... " + std::to_string(RH_SAS_POINTS_MAX_CELLS) + ")");
    if (n_arrays < 0 || n_arrays > RH_SAS_POINTS_MAX_ARRAYS)
        return sfail(ctx, RH_ERR_ARG, who + "n_arrays = " + std::to_string(n_arrays) + " (0 ... " + std::to_string(RH_SAS_POINTS_MAX_ARRAYS) + ")");
    const bool off = n_cells == 0 || n_arrays == 0;
    SasPointsDev P = {};
    int64_t row_elems = 0;
    if (!off) {
        if (!cells || !arrays) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
        if (int rc = sas_check_capacity(ctx, who, capacity)) return rc;
        for (int j = 0; j < n_arrays; ++j) {
            const int a = arrays[j];
            if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown array id " + std::to_string(a));
            const std::string name = std::string("array ") + SAS_NAMES[a];
            if (std::find(arrays, arrays + j, a) != arrays + j) return sfail(ctx, RH_ERR_ARG, who + name + " is given twice");
            if (SAS_KIND[a] == K_MASK) return sfail(ctx, RH_ERR_ARG, who + name + " is int32 (float64 arrays only)");
            if (SAS_KIND[a] == K_DAILY || SAS_KIND[a] == K_PARAM)
                return sfail(ctx, RH_ERR_ARG, who + name + " is an input of the step, not a per-cell result (daily inputs and sas_params_* are not recorded)");
            if (!ctx->arr[a])
                return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
            P.src[j] = (const double *)ctx->arr[a].get();
            P.width[j] = (int)(ctx->elems[a] / ctx->cfg.n_cells);
            P.off[j] = row_elems;
            P.first_block[j + 1] = P.first_block[j] + (n_cells * P.width[j] + SAS_POINTS_BLOCK - 1) / SAS_POINTS_BLOCK;
            row_elems += (int64_t)n_cells * P.width[j];
        }
        std::vector<int64_t> seen(cells, cells + n_cells);
        std::sort(seen.begin(), seen.end());
        for (int c = 0; c < n_cells; ++c) {
            if (cells[c] < 0 || cells[c] >= ctx->cfg.n_cells)
                return sfail(ctx, RH_ERR_ARG, who + "cell " + std::to_string(cells[c]) + " is outside [0, " + std::to_string(ctx->cfg.n_cells) + ")");
            if (c && seen[c] == seen[c - 1]) return sfail(ctx, RH_ERR_ARG, who + "cell " + std::to_string(seen[c]) + " is given twice");
            P.cells[c] = cells[c];
        }
        P.n_arrays = n_arrays;
        P.n_cells = n_cells;
        if (capacity > ((int64_t)1 << 31) / (row_elems * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + "capacity = " + std::to_string(capacity) + " rows of " + std::to_string(row_elems) +
                                              " float64 are a ring above 2 GiB");
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, ctx->points.release());
    SHIPCHK(ctx, ctx->points_cfg.release());
    ctx->points_blocks = 0;
    if (off) return RH_OK;
    std::unique_ptr<int64_t[]> tags(new (std::nothrow) int64_t[(size_t)capacity]);
    if (!tags) return sfail(ctx, RH_ERR_ARG, who + "out of host memory for the tags of " + std::to_string(capacity) + " rows");
    SHIPCHK(ctx, ctx->points.ring.alloc((size_t)capacity * (size_t)row_elems * sizeof(double)));
    SHIPCHK(ctx, ctx->points_cfg.alloc(sizeof(SasPointsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->points_cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the source is a local)
    ctx->points.tags = std::move(tags);
    ctx->points_blocks = P.first_block[n_arrays];
    ctx->points.row_elems = row_elems;
    ctx->points.cap = capacity;
    return RH_OK;
}

static int sas_points_on(rh_sas_ctx *ctx, const char *who) {
    return ctx ? sas_on(ctx, ctx->points.on(), who, "rh_sas_points_configure") : RH_ERR_ARG;
}

int rh_sas_points_record(rh_sas_ctx *ctx, int64_t tag) {
    if (int rc = sas_points_on(ctx, "rh_sas_points_record")) return rc;
    return sas_points_enqueue(ctx, tag);
}

int rh_sas_points_count(rh_sas_ctx *ctx, int64_t *rows_total) {
    if (int rc = sas_points_on(ctx, "rh_sas_points_count")) return rc;
    if (!rows_total) return sfail(ctx, RH_ERR_ARG, "rh_sas_points_count: null pointer");
    *rows_total = ctx->points.rows;
    return RH_OK;
}

int rh_sas_points_row_elems(const rh_sas_ctx *ctx, int64_t *elems) {
    if (int rc = sas_points_on(const_cast<rh_sas_ctx *>(ctx), "rh_sas_points_row_elems")) return rc;
    if (!elems) return RH_ERR_ARG;
    *elems = ctx->points.row_elems;
    return RH_OK;
}

int rh_sas_points_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    if (int rc = sas_points_on(ctx, "rh_sas_points_read")) return rc;
    return sas_ring_read(ctx, "rh_sas_points_read", ctx->points, first_row, n_rows, tags, values, value_bytes);
}

// ---- catchment totals (include/roger_hip_sas.h; kernels and orders: rh_sas_totals.h) ----
// one row behind what the stream holds so far: the width-1 statistics of every item, then the age items one after another
static int sas_totals_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    const int64_t n = ctx->cfg.n_cells;
    const int64_t day_off = day < 0 ? -1 : (day % ctx->cfg.forcing_days) * n;
    const SasTotalsDev &P = ctx->totals_host;
    double *row = ctx->totals.next_row();
    hipLaunchKernelGGL(k_sas_totals_tiles, dim3((unsigned)P.ntiles), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, ctx->totals_cfg.get(), day_off);
    hipLaunchKernelGGL(k_sas_totals_finish, dim3((unsigned)P.n_items), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, ctx->totals_cfg.get(), row);
    for (int j = 0; j < P.n_items; ++j) {
        const int W = ctx->totals_width[j];
        if (W == 1) continue;
        const unsigned bs = (unsigned)std::min(SAS_TOTALS_BLOCK, (W + 63) / 64 * 64);
        const unsigned chunks = ((unsigned)W + bs - 1) / bs;
        const double *src = ctx->totals_src[j];
        int64_t m = n;
        for (int lvl = 0;; ++lvl) {
            const int64_t runs = (m + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
            double *dst = runs == 1 ? row + P.off[j] + 2 : ctx->totals_lvl[lvl & 1].get();
            if (lvl == 0)
                hipLaunchKernelGGL(k_sas_totals_ages<true>, dim3((unsigned)runs, chunks), dim3(bs), 0, ctx->stream, src, m, W, P.mask,
                                   P.wgt[j] ? P.wgt[j] + std::max<int64_t>(day_off, 0) : nullptr, (P.wgt[j] && day_off < 0) ? 0 : 1, dst);
            else
                hipLaunchKernelGGL(k_sas_totals_ages<false>, dim3((unsigned)runs, chunks), dim3(bs), 0, ctx->stream, src, m, W,
                                   (const unsigned char *)nullptr, (const double *)nullptr, 1, dst);
            if (runs == 1) break;
            src = dst;
            m = runs;
        }
    }
    SHIPCHK(ctx, hipGetLastError());
    ctx->totals.enqueued(tag);
    return RH_OK;
}

// What the items of rh_sas_totals_configure and rh_sas_zonal_configure are: ids checked, the arrays and weights on the device, the widths
// and the blocks' places in a row (a zone's part of it).  `who` opens the message of a refusal.
static int sas_totals_items(rh_sas_ctx *ctx, const std::string &who, const rh_sas_totals_item *items, int n_items, const double **val,
                            const double **wgt, int64_t *off, unsigned char *val_daily, int *width, const double **srcs, int64_t *row_elems,
                            int *wmax) {
    const int64_t n = ctx->cfg.n_cells;
    for (int j = 0; j < n_items; ++j) {
        const int a = items[j].array, w = items[j].weight;
        if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown array id " + std::to_string(a));
        if (w < -1 || w >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown weight id " + std::to_string(w));
        const std::string name = std::string("array ") + SAS_NAMES[a];
        for (int k = 0; k < j; ++k)
            if (items[k].array == a && items[k].weight == w) return sfail(ctx, RH_ERR_ARG, who + name + " is given twice with the same weight");
        if (SAS_KIND[a] == K_MASK) return sfail(ctx, RH_ERR_ARG, who + name + " is int32 (float64 arrays only)");
        if (SAS_KIND[a] == K_PARAM) return sfail(ctx, RH_ERR_ARG, who + name + " is a parameter block of the step (sas_params_* are not reduced)");
        if (w >= 0 && (SAS_KIND[w] != K_DAILY || w == SA_C_in))
            return sfail(ctx, RH_ERR_ARG, who + "weight " + SAS_NAMES[w] + " is not a daily flux input (inf_mat_rz ... cpr_rz)");
        if (!ctx->arr[a])
            return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
        const double *base = (const double *)ctx->arr[a].get();
        width[j] = SAS_KIND[a] == K_DAILY ? 1 : (int)(ctx->elems[a] / n);
        val[j] = width[j] == 1 ? base : nullptr;
        srcs[j] = width[j] == 1 ? nullptr : base;
        val_daily[j] = SAS_KIND[a] == K_DAILY;
        wgt[j] = w >= 0 ? (const double *)ctx->arr[w].get() : nullptr;
        off[j] = *row_elems;
        *row_elems += width[j] == 1 ? SAS_TOTALS_NSTAT : 2 + width[j];
        if (width[j] > 1) *wmax = std::max(*wmax, width[j]);
    }
    return RH_OK;
}

int rh_sas_totals_configure(rh_sas_ctx *ctx, const unsigned char *mask, const rh_sas_totals_item *items, int n_items, int64_t capacity) {
    const std::string who = "rh_sas_totals_configure: ";
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_SAS_TOTALS_MAX_ITEMS)
        return sfail(ctx, RH_ERR_ARG, who + "n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SAS_TOTALS_MAX_ITEMS) + ")");
    const int64_t n = ctx->cfg.n_cells;
    SasTotalsDev P = {};
    int width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *srcs[RH_SAS_TOTALS_MAX_ITEMS] = {};
    int64_t row_elems = 0, ncells = n;
    int wmax = 0;
    if (n_items) {
        if (!items) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
        if (int rc = sas_check_capacity(ctx, who, capacity)) return rc;
        if (int rc = sas_totals_items(ctx, who, items, n_items, P.val, P.wgt, P.off, P.val_daily, width, srcs, &row_elems, &wmax)) return rc;
        if (mask) {
            ncells = 0;
            for (int64_t c = 0; c < n; ++c) ncells += mask[c] != 0;
            if (!ncells) return sfail(ctx, RH_ERR_ARG, who + "the mask holds no cell");
        }
        if (capacity > ((int64_t)1 << 31) / (row_elems * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + "capacity = " + std::to_string(capacity) + " rows of " + std::to_string(row_elems) +
                                              " float64 are a ring above 2 GiB");
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, ctx->totals.release());
    SHIPCHK(ctx, ctx->totals_part.release());
    SHIPCHK(ctx, ctx->totals_lvl[0].release());
    SHIPCHK(ctx, ctx->totals_lvl[1].release());
    SHIPCHK(ctx, ctx->totals_cfg.release());
    SHIPCHK(ctx, ctx->totals_mask.release());
    ctx->totals_ncells = 0;
    if (!n_items) return RH_OK;
    std::unique_ptr<int64_t[]> tags(new (std::nothrow) int64_t[(size_t)capacity]);
    if (!tags) return sfail(ctx, RH_ERR_ARG, who + "out of host memory for the tags of " + std::to_string(capacity) + " rows");
    const int64_t ntiles = (n + SAS_TOTALS_BLOCK - 1) / SAS_TOTALS_BLOCK, runs1 = (n + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
    const int64_t runs2 = (runs1 + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
    SHIPCHK(ctx, ctx->totals.ring.alloc((size_t)capacity * (size_t)row_elems * sizeof(double)));
    SHIPCHK(ctx, ctx->totals_part.alloc((size_t)n_items * SAS_TOTALS_NSTAT * (size_t)ntiles * sizeof(double)));
    if (wmax && runs1 > 1) {
        SHIPCHK(ctx, ctx->totals_lvl[0].alloc((size_t)runs1 * (size_t)wmax * sizeof(double)));
        SHIPCHK(ctx, ctx->totals_lvl[1].alloc((size_t)runs2 * (size_t)wmax * sizeof(double)));
    }
    if (mask) {
        SHIPCHK(ctx, ctx->totals_mask.alloc((size_t)n));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->totals_mask, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    P.n_items = n_items;
    P.ntiles = (int)ntiles;
    P.n = n;
    P.mask = ctx->totals_mask.get();
    P.part = ctx->totals_part.get();
    SHIPCHK(ctx, ctx->totals_cfg.alloc(sizeof(SasTotalsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->totals_cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and a local)
    ctx->totals_host = P;
    std::copy(width, width + RH_SAS_TOTALS_MAX_ITEMS, ctx->totals_width);
    std::copy(srcs, srcs + RH_SAS_TOTALS_MAX_ITEMS, ctx->totals_src);
    ctx->totals.tags = std::move(tags);
    ctx->totals.row_elems = row_elems;
    ctx->totals_ncells = ncells;
    ctx->totals.cap = capacity;
    return RH_OK;
}

static int sas_totals_on(rh_sas_ctx *ctx, const char *who) {
    return ctx ? sas_on(ctx, ctx->totals.on(), who, "rh_sas_totals_configure") : RH_ERR_ARG;
}

int rh_sas_totals_record(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    if (int rc = sas_totals_on(ctx, "rh_sas_totals_record")) return rc;
    return sas_totals_enqueue(ctx, tag, day);
}

int rh_sas_totals_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (int rc = sas_totals_on(ctx, "rh_sas_totals_count")) return rc;
    if (!rows_total || !ncells) return sfail(ctx, RH_ERR_ARG, "rh_sas_totals_count: null pointer");
    *rows_total = ctx->totals.rows;
    *ncells = ctx->totals_ncells;
    return RH_OK;
}

int rh_sas_totals_row_elems(const rh_sas_ctx *ctx, int64_t *elems) {
    if (int rc = sas_totals_on(const_cast<rh_sas_ctx *>(ctx), "rh_sas_totals_row_elems")) return rc;
    if (!elems) return RH_ERR_ARG;
    *elems = ctx->totals.row_elems;
    return RH_OK;
}

int rh_sas_totals_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    if (int rc = sas_totals_on(ctx, "rh_sas_totals_read")) return rc;
    return sas_ring_read(ctx, "rh_sas_totals_read", ctx->totals, first_row, n_rows, tags, values, value_bytes);
}

// ---- zonal totals (include/roger_hip_sas.h; kernels, index and orders: rh_sas_zonal.h) ----
// one row behind what the stream holds so far: every item's width-1 statistics for every zone, then the age items one after another
static int sas_zonal_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    const int64_t n = ctx->cfg.n_cells;
    const int64_t day_off = day < 0 ? -1 : (day % ctx->cfg.forcing_days) * n;
    const SasZonalDev &P = ctx->zonal_host;
    const int *ix = ctx->zonal_index.get();
    const int64_t *at = ctx->zonal_at;
    double *row = ctx->zonal.next_row();
    const unsigned ntiles = (unsigned)ctx->zonal_ntiles, nz = (unsigned)ctx->zonal_nzones;
    hipLaunchKernelGGL(k_sas_zonal_tiles, dim3(ntiles), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, ctx->zonal_cfg.get(), day_off);
    hipLaunchKernelGGL(k_sas_zonal_finish, dim3(nz), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, ctx->zonal_cfg.get(), row);
    for (int j = 0; j < P.n_items; ++j) {
        const int W = ctx->zonal_width[j];
        if (W == 1) continue;
        const unsigned bs = (unsigned)std::min(SAS_TOTALS_BLOCK, (W + 63) / 64 * 64);
        const unsigned chunks = ((unsigned)W + bs - 1) / bs;
        hipLaunchKernelGGL(k_sas_zonal_ages, dim3(ntiles, chunks), dim3(bs), 0, ctx->stream, ctx->zonal_src[j], W, ix + at[SZ_TILE_PTR],
                           ix + at[SZ_CELL_PTR], ix + at[SZ_CELL], P.wgt[j] ? P.wgt[j] + std::max<int64_t>(day_off, 0) : nullptr,
                           (P.wgt[j] && day_off < 0) ? 0 : 1, ctx->zonal_lvl.get());
        hipLaunchKernelGGL(k_sas_zonal_ages_finish, dim3(nz, chunks), dim3(bs), 0, ctx->stream, (const double *)ctx->zonal_lvl.get(), W,
                           ix + at[SZ_RUN_PTR], ix + at[SZ_RUN_SLOT], ix + at[SZ_SLOT_TILE], row + P.off[j] + 2, P.zone_elems);
    }
    SHIPCHK(ctx, hipGetLastError());
    ctx->zonal.enqueued(tag);
    return RH_OK;
}

int rh_sas_zonal_configure(rh_sas_ctx *ctx, const int32_t *zone, int n_zones, const rh_sas_totals_item *items, int n_items, int64_t capacity) {
    const std::string who = "rh_sas_zonal_configure: ";
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_SAS_TOTALS_MAX_ITEMS)
        return sfail(ctx, RH_ERR_ARG, who + "n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SAS_TOTALS_MAX_ITEMS) + ")");
    const int64_t n = ctx->cfg.n_cells;
    SasZonalDev P = {};
    int width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *srcs[RH_SAS_TOTALS_MAX_ITEMS] = {};
    int64_t zone_elems = 0, at[SZ_PARTS] = {}, S = 0;
    int wmax = 0;
    std::vector<int64_t> ncells;
    std::vector<int> index;
    if (n_items) {
        if (!items || !zone) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
        if (n_zones < 1 || n_zones > RH_SAS_ZONAL_MAX_ZONES)
            return sfail(ctx, RH_ERR_ARG, who + "n_zones = " + std::to_string(n_zones) + " (1 ... " + std::to_string(RH_SAS_ZONAL_MAX_ZONES) + ")");
        if (int rc = sas_check_capacity(ctx, who, capacity)) return rc;
        if (int rc = sas_totals_items(ctx, who, items, n_items, P.val, P.wgt, P.off, P.val_daily, width, srcs, &zone_elems, &wmax)) return rc;
        ncells.assign((size_t)n_zones, 0);
        int64_t inside = 0;
        for (int64_t c = 0; c < n; ++c) {
            if (zone[c] < -1 || zone[c] >= n_zones)
                return sfail(ctx, RH_ERR_ARG, who + "zone id " + std::to_string(zone[c]) + " of cell " + std::to_string(c) +
                                                  " (-1: outside, else 0 ... " + std::to_string(n_zones - 1) + ")");
            if (zone[c] >= 0) {
                ++ncells[(size_t)zone[c]];
                ++inside;
            }
        }
        if (!inside) return sfail(ctx, RH_ERR_ARG, who + "the map holds no cell in any zone (0 of " + std::to_string(n) + " cells)");
        if (capacity > ((int64_t)1 << 31) / (zone_elems * n_zones * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + "capacity = " + std::to_string(capacity) + " rows of " + std::to_string(n_zones) + " zones x " +
                                              std::to_string(zone_elems) + " float64 are a ring above 2 GiB");
        S = sas_zonal_index(zone, n, n_zones, index, at);
        if (wmax && S > ((int64_t)1 << 31) / ((int64_t)wmax * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + std::to_string(S) + " (tile, zone) slots x " + std::to_string(wmax) +
                                              " float64 are a level-1 buffer above 2 GiB");
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, ctx->zonal.release());
    SHIPCHK(ctx, ctx->zonal_part.release());
    SHIPCHK(ctx, ctx->zonal_lvl.release());
    SHIPCHK(ctx, ctx->zonal_cfg.release());
    SHIPCHK(ctx, ctx->zonal_index.release());
    ctx->zonal_nzones = 0;
    ctx->zonal_ntiles = 0;
    ctx->zonal_ncells.clear();
    if (!n_items) return RH_OK;
    std::unique_ptr<int64_t[]> tags(new (std::nothrow) int64_t[(size_t)capacity]);
    if (!tags) return sfail(ctx, RH_ERR_ARG, who + "out of host memory for the tags of " + std::to_string(capacity) + " rows");
    const int64_t row_elems = zone_elems * n_zones;
    SHIPCHK(ctx, ctx->zonal.ring.alloc((size_t)capacity * (size_t)row_elems * sizeof(double)));
    SHIPCHK(ctx, ctx->zonal_part.alloc((size_t)S * (size_t)n_items * SAS_TOTALS_NSTAT * sizeof(double)));
    if (wmax) SHIPCHK(ctx, ctx->zonal_lvl.alloc((size_t)S * (size_t)wmax * sizeof(double)));
    SHIPCHK(ctx, ctx->zonal_index.alloc(index.size() * sizeof(int)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->zonal_index, index.data(), index.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const int *ix = ctx->zonal_index.get();
    P.n_items = n_items;
    P.n = n;
    P.zone_elems = zone_elems;
    P.zone = ix + at[SZ_ZONE];
    P.tile_ptr = ix + at[SZ_TILE_PTR];
    P.tile_zone = ix + at[SZ_TILE_ZONE];
    P.acc_ptr = ix + at[SZ_ACC_PTR];
    P.acc_slot = ix + at[SZ_ACC_SLOT];
    P.part = ctx->zonal_part.get();
    SHIPCHK(ctx, ctx->zonal_cfg.alloc(sizeof(SasZonalDev)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->zonal_cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are locals)
    ctx->zonal_host = P;
    std::copy(width, width + RH_SAS_TOTALS_MAX_ITEMS, ctx->zonal_width);
    std::copy(srcs, srcs + RH_SAS_TOTALS_MAX_ITEMS, ctx->zonal_src);
    std::copy(at, at + SZ_PARTS, ctx->zonal_at);
    ctx->zonal.tags = std::move(tags);
    ctx->zonal.row_elems = row_elems;
    ctx->zonal_ntiles = (n + SAS_TOTALS_BLOCK - 1) / SAS_TOTALS_BLOCK;
    ctx->zonal_ncells = std::move(ncells);
    ctx->zonal_nzones = n_zones;
    ctx->zonal.cap = capacity;
    return RH_OK;
}

static int sas_zonal_on(rh_sas_ctx *ctx, const char *who) {
    return ctx ? sas_on(ctx, ctx->zonal.on(), who, "rh_sas_zonal_configure") : RH_ERR_ARG;
}

int rh_sas_zonal_record(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    if (int rc = sas_zonal_on(ctx, "rh_sas_zonal_record")) return rc;
    return sas_zonal_enqueue(ctx, tag, day);
}

int rh_sas_zonal_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (int rc = sas_zonal_on(ctx, "rh_sas_zonal_count")) return rc;
    if (!rows_total || !ncells) return sfail(ctx, RH_ERR_ARG, "rh_sas_zonal_count: null pointer");
    *rows_total = ctx->zonal.rows;
    std::copy(ctx->zonal_ncells.begin(), ctx->zonal_ncells.end(), ncells);
    return RH_OK;
}

int rh_sas_zonal_row_elems(const rh_sas_ctx *ctx, int64_t *elems) {
    if (int rc = sas_zonal_on(const_cast<rh_sas_ctx *>(ctx), "rh_sas_zonal_row_elems")) return rc;
    if (!elems) return RH_ERR_ARG;
    *elems = ctx->zonal.row_elems;
    return RH_OK;
}

int rh_sas_zonal_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    if (int rc = sas_zonal_on(ctx, "rh_sas_zonal_read")) return rc;
    return sas_ring_read(ctx, "rh_sas_zonal_read", ctx->zonal, first_row, n_rows, tags, values, value_bytes);
}

// ---- scores against observed samples (include/roger_hip_sas.h; the kernel and the rule: rh_sas_scores.h) ----
// the next day of the count, behind what the stream holds so far: which window it lies in is decided here, the kernel is told
static int sas_scores_enqueue(rh_sas_ctx *ctx, int64_t day) {
    const int64_t t = ctx->scores_days++, K = (int64_t)ctx->scores_first.size(), n = ctx->cfg.n_cells;
    int64_t &k = ctx->scores_k;
    while (k < K && ctx->scores_last[(size_t)k] < t) ++k;   // (windows that passed without being open)
    if (k >= K || t < ctx->scores_first[(size_t)k]) return RH_OK;
    const bool first = t == ctx->scores_first[(size_t)k], closes = t == ctx->scores_last[(size_t)k];
    if (first) ctx->scores_open = k;
    if (ctx->scores_open != k) return RH_OK;                // (its first day was never scored)
    if (closes || ctx->scores_accumulate) {
        hipLaunchKernelGGL(k_sas_scores, dim3((unsigned)((n + SAS_SCORES_BLOCK - 1) / SAS_SCORES_BLOCK)), dim3(SAS_SCORES_BLOCK), 0, ctx->stream,
                           ctx->scores_cfg.get(), k, first ? 1 : 0, closes ? 1 : 0, (day % ctx->cfg.forcing_days) * n);
        SHIPCHK(ctx, hipGetLastError());
    }
    if (closes) {
        ctx->scores_closed[(size_t)k] = 1;
        ctx->scores_open = -1;
        ++k;
    }
    return RH_OK;
}

int rh_sas_scores_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const int32_t *series, int n_series,
                            const double *obs, const int64_t *first_day, const int64_t *last_day, int64_t n_samples) {
    const std::string who = "rh_sas_scores_configure: ";
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_SAS_SCORES_MAX_ITEMS)
        return sfail(ctx, RH_ERR_ARG, who + "n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SAS_SCORES_MAX_ITEMS) + ")");
    const int64_t n = ctx->cfg.n_cells;
    SasScoresDev P = {};
    bool accumulate = false;
    if (n_items) {
        if (!items || !obs || !first_day || !last_day) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
        if (n_series < 1 || n_series > RH_SAS_SCORES_MAX_SERIES)
            return sfail(ctx, RH_ERR_ARG, who + "n_series = " + std::to_string(n_series) + " (1 ... " + std::to_string(RH_SAS_SCORES_MAX_SERIES) + ")");
        if (n_samples < 1 || n_samples > (int64_t)1 << 31)
            return sfail(ctx, RH_ERR_ARG, who + "n_samples = " + std::to_string(n_samples) + " (at least one, at most 2^31)");
        static const char *const KIND[] = {"BULK", "MEAN", "LAST"};
        for (int j = 0; j < n_items; ++j) {
            const int a = items[j].value, w = items[j].weight, kind = items[j].kind;
            if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown array id " + std::to_string(a));
            if (w < -1 || w >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown weight id " + std::to_string(w));
            const std::string name = std::string("array ") + SAS_NAMES[a];
            if (kind < RH_SAS_SCORES_BULK || kind > RH_SAS_SCORES_LAST)
                return sfail(ctx, RH_ERR_ARG, who + "kind " + std::to_string(kind) + " of " + name + " (0: BULK, 1: MEAN, 2: LAST)");
            for (int q = 0; q < j; ++q)
                if (items[q].value == a && items[q].weight == w && items[q].kind == kind)
                    return sfail(ctx, RH_ERR_ARG, who + name + " is given twice with the same weight and kind");
            if (SAS_KIND[a] == K_MASK) return sfail(ctx, RH_ERR_ARG, who + name + " is int32 (float64 arrays only)");
            if (SAS_KIND[a] == K_PARAM) return sfail(ctx, RH_ERR_ARG, who + name + " is a parameter block of the step (sas_params_* are not scored)");
            if (SAS_KIND[a] == K_DAILY) return sfail(ctx, RH_ERR_ARG, who + name + " is a daily input of the step, not a result (daily inputs are weights here)");
            if (SAS_KIND[a] != K_CELL) return sfail(ctx, RH_ERR_ARG, who + name + " is age-resolved (a sample is compared with one value per cell)");
            if (w >= 0 && (SAS_KIND[w] != K_DAILY || w == SA_C_in))
                return sfail(ctx, RH_ERR_ARG, who + "weight " + SAS_NAMES[w] + " is not a daily flux input (inf_mat_rz ... cpr_rz)");
            if (kind == RH_SAS_SCORES_BULK && w < 0) return sfail(ctx, RH_ERR_ARG, who + name + " is BULK and has no weight");
            if (kind != RH_SAS_SCORES_BULK && w >= 0)
                return sfail(ctx, RH_ERR_ARG, who + name + " is " + KIND[kind] + " and has the weight " + SAS_NAMES[w] + " (only BULK takes one)");
            if (!ctx->arr[a])
                return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
            P.val[j] = (const double *)ctx->arr[a].get();
            P.wgt[j] = w >= 0 ? (const double *)ctx->arr[w].get() : nullptr;
            P.kind[j] = kind;
            accumulate = accumulate || kind != RH_SAS_SCORES_LAST;
        }
        if (series) {
            int64_t scored = 0;
            for (int64_t c = 0; c < n; ++c) {
                if (series[c] >= n_series)
                    return sfail(ctx, RH_ERR_ARG, who + "series " + std::to_string(series[c]) + " of cell " + std::to_string(c) +
                                                      " (< 0: not scored, else 0 ... " + std::to_string(n_series - 1) + ")");
                scored += series[c] >= 0;
            }
            if (!scored) return sfail(ctx, RH_ERR_ARG, who + "the series map scores no cell (0 of " + std::to_string(n) + " cells)");
        }
        for (int64_t k = 0; k < n_samples; ++k) {
            if (first_day[k] > last_day[k])
                return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " is [" + std::to_string(first_day[k]) + ", " +
                                                  std::to_string(last_day[k]) + "]: its last day lies before its first");
            if (k && first_day[k] <= last_day[k - 1])
                return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " starts on day " + std::to_string(first_day[k]) + ", window " +
                                                  std::to_string(k - 1) + " ends on day " + std::to_string(last_day[k - 1]) +
                                                  " (windows are in increasing order and do not overlap)");
        }
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that add into the old moments)
    SHIPCHK(ctx, ctx->scores_buf.release());
    SHIPCHK(ctx, ctx->scores_obs.release());
    SHIPCHK(ctx, ctx->scores_series.release());
    SHIPCHK(ctx, ctx->scores_cfg.release());
    ctx->scores_first.clear();
    ctx->scores_last.clear();
    ctx->scores_closed.clear();
    ctx->scores_items = 0;
    ctx->scores_accumulate = false;
    ctx->scores_days = ctx->scores_k = 0;
    ctx->scores_open = -1;
    if (!n_items) return RH_OK;
    const size_t mb = (size_t)n_items * SAS_SCORES_NMOM * (size_t)n * sizeof(double);
    const size_t ob = (size_t)n_items * (size_t)n_series * (size_t)n_samples * sizeof(double);
    SHIPCHK(ctx, ctx->scores_buf.alloc(mb));
    SHIPCHK(ctx, hipMemsetAsync(ctx->scores_buf, 0, mb, ctx->stream));
    SHIPCHK(ctx, ctx->scores_obs.alloc(ob));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->scores_obs, obs, ob, hipMemcpyHostToDevice, ctx->stream));
    if (series) {
        SHIPCHK(ctx, ctx->scores_series.alloc((size_t)n * sizeof(int32_t)));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->scores_series, series, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    P.n_items = n_items;
    P.n_series = n_series;
    P.n = n;
    P.n_samples = n_samples;
    P.series = ctx->scores_series.get();
    P.obs = ctx->scores_obs.get();
    P.scores = ctx->scores_buf.get();
    SHIPCHK(ctx, ctx->scores_cfg.alloc(sizeof(SasScoresDev)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->scores_cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and a local)
    ctx->scores_first.assign(first_day, first_day + n_samples);
    ctx->scores_last.assign(last_day, last_day + n_samples);
    ctx->scores_closed.assign((size_t)n_samples, 0);
    ctx->scores_accumulate = accumulate;
    ctx->scores_items = n_items;
    return RH_OK;
}

static int sas_scores_on(rh_sas_ctx *ctx, const char *who) {
    return ctx ? sas_on(ctx, ctx->scores_items != 0, who, "rh_sas_scores_configure") : RH_ERR_ARG;
}

int rh_sas_scores_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_scores_on(ctx, "rh_sas_scores_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_scores_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_scores_enqueue(ctx, day);
}

int rh_sas_scores_read(rh_sas_ctx *ctx, double *moments, size_t moment_bytes, unsigned char *closed, size_t closed_bytes,
                       int64_t *days_scored) {
    if (int rc = sas_scores_on(ctx, "rh_sas_scores_read")) return rc;
    if (!moments || !closed || moment_bytes != (size_t)ctx->scores_items * SAS_SCORES_NMOM * (size_t)ctx->cfg.n_cells * sizeof(double) ||
        closed_bytes != ctx->scores_closed.size())
        return sfail(ctx, RH_ERR_ARG, "rh_sas_scores_read: size mismatch (n_items x 9 x n_cells float64, n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(moments, ctx->scores_buf, moment_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(ctx->scores_closed.begin(), ctx->scores_closed.end(), closed);
    if (days_scored) *days_scored = ctx->scores_days;
    return rh_sas_sync(ctx);
}

// ---- transport bands (include/roger_hip_sas.h; the kernels and the rule: rh_sas_bands.h) ----
// the selection's words on the device, one allocation of int64: where each part starts
enum SasBandsWords {
    SBW_PREFIX = 0,
    SBW_RANK = SBW_PREFIX + RH_SAS_BANDS_MAX_ITEMS * RH_SAS_BANDS_MAX_PROBS,
    SBW_M = SBW_RANK + RH_SAS_BANDS_MAX_ITEMS * RH_SAS_BANDS_MAX_PROBS,
    SBW_NAN = SBW_M + RH_SAS_BANDS_MAX_ITEMS,
    SBW_W = SBW_NAN + RH_SAS_BANDS_MAX_ITEMS,
    SBW_M_COUNT = SBW_W + RH_SAS_BANDS_MAX_ITEMS,                 // uint32 [items]
    SBW_NAN_COUNT = SBW_M_COUNT + RH_SAS_BANDS_MAX_ITEMS / 2,     // uint32 [items]
    SBW_WORDS = SBW_NAN_COUNT + RH_SAS_BANDS_MAX_ITEMS / 2
};
// the next day of the count, behind what the stream holds so far: the clock of sas_scores_enqueue; on a closing day the six passes of the
// selection follow the day's kernel, and the two kernels of the observations where window k has one
static int sas_bands_enqueue(rh_sas_ctx *ctx, int64_t day) {
    const int64_t t = ctx->bands_days++, K = (int64_t)ctx->bands_first.size(), n = ctx->cfg.n_cells;
    int64_t &k = ctx->bands_k;
    while (k < K && ctx->bands_last[(size_t)k] < t) ++k;   // (windows that passed without being open)
    if (k >= K || t < ctx->bands_first[(size_t)k]) return RH_OK;
    const bool first = t == ctx->bands_first[(size_t)k], closes = t == ctx->bands_last[(size_t)k];
    if (first) ctx->bands_open = k;
    if (ctx->bands_open != k) return RH_OK;                // (its first day was never recorded)
    const SasBandsDev *cfg = ctx->bands_cfg.get();
    if (closes || ctx->bands_accumulate)
        hipLaunchKernelGGL(k_sas_bands_day, dim3((unsigned)((n + SAS_BANDS_BLOCK - 1) / SAS_BANDS_BLOCK)), dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg,
                           first ? 1 : 0, closes ? 1 : 0, (day % ctx->cfg.forcing_days) * n);
    if (closes && ctx->bands_zones) {   // per zone: one launch in place of the twelve, one more where window k has an observation
        const size_t nz = (size_t)ctx->bands_zones;
        const SasBandsZonalDev Z = {ctx->bands_zone_off.get(), ctx->bands_zone_cols.get()};
        const dim3 grid((unsigned)nz, (unsigned)ctx->bands_items);
        if (ctx->bands_weight)
            hipLaunchKernelGGL(k_sas_bands_zonal<true>, grid, dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg, Z, k);
        else
            hipLaunchKernelGGL(k_sas_bands_zonal<false>, grid, dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg, Z, k);
        bool observed = false;
        for (size_t jz = 0; jz < (size_t)ctx->bands_items * nz && !ctx->bands_obs_host.empty() && !observed; ++jz) {
            const double o = ctx->bands_obs_host[jz * (size_t)K + (size_t)k];
            observed = o == o;
        }
        if (observed) hipLaunchKernelGGL(k_sas_bands_obs_zonal, grid, dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg, Z, k);
        ctx->bands_closed[(size_t)k] = 1;
        ctx->bands_open = -1;
        ++k;
    } else if (closes) {
        const unsigned grid = bands_weighted_grid((long long)n);
        sas_bands_pass<0>(ctx, grid, k);
        sas_bands_pass<1>(ctx, grid, k);
        sas_bands_pass<2>(ctx, grid, k);
        sas_bands_pass<3>(ctx, grid, k);
        sas_bands_pass<4>(ctx, grid, k);
        sas_bands_pass<5>(ctx, grid, k);
        bool observed = false;
        for (int j = 0; j < ctx->bands_items && !ctx->bands_obs_host.empty(); ++j) {
            const double o = ctx->bands_obs_host[(size_t)j * (size_t)K + (size_t)k];
            observed = observed || o == o;
        }
        if (observed) {   // (an item without one ends after the scalar loads: its pair stays (-1, -1), as configure wrote it)
            const unsigned parts = sas_bands_obs_grid((long long)n);
            hipLaunchKernelGGL(k_sas_bands_obs, dim3(parts, (unsigned)ctx->bands_items), dim3(SAS_BANDS_BLOCK), 0, ctx->stream, cfg, k);
            hipLaunchKernelGGL(k_sas_bands_obs_row, dim3((unsigned)ctx->bands_items), dim3(64), 0, ctx->stream, cfg, k, (int)parts);
        }
        ctx->bands_closed[(size_t)k] = 1;
        ctx->bands_open = -1;
        ++k;
    }
    SHIPCHK(ctx, hipGetLastError());
    return RH_OK;
}

// rh_sas_bands_configure (zone == nullptr, n_zones == 0) and rh_sas_bands_configure_zonal, for the function `name`: with zones the result and
// the observations gain the zone axis behind the item's, the byte mask becomes (zone >= 0) & mask, and the zones' column lists are built
static int sas_bands_configure(rh_sas_ctx *ctx, const char *name, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                               const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights, const double *obs,
                               const int64_t *first_day, const int64_t *last_day, int64_t n_samples) {
    const std::string who = std::string(name) + ": ";
    const bool zonal = n_zones != 0;
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_SAS_BANDS_MAX_ITEMS)
        return sfail(ctx, RH_ERR_ARG, who + "n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SAS_BANDS_MAX_ITEMS) + ")");
    const int64_t n = ctx->cfg.n_cells;
    SasBandsDev P = {};
    bool accumulate = false;
    std::vector<unsigned char> folded;          // per zone: (zone >= 0) & mask
    std::vector<long long> zone_off;            // per zone: [n_zones + 1] into ...
    std::vector<int> zone_cols;                 // ... the participating columns, ascending within a zone
    if (n_items) {
        if (!items || !probs || !first_day || !last_day || (zonal && !zone)) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
        if (n_probs < 1 || n_probs > RH_SAS_BANDS_MAX_PROBS)
            return sfail(ctx, RH_ERR_ARG, who + "n_probs = " + std::to_string(n_probs) + " (1 ... " + std::to_string(RH_SAS_BANDS_MAX_PROBS) + ")");
        for (int q = 0; q < n_probs; ++q) {
            if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
                return sfail(ctx, RH_ERR_ARG, who + "probability " + std::to_string(q) + " is " + std::to_string(probs[q]) + " (within [0, 1])");
            P.probs[q] = probs[q];
        }
        if (zonal && (n_samples < 1 || n_samples > ((int64_t)1 << 31) / ((int64_t)n_items * n_zones * n_probs * (int64_t)sizeof(double))))
            return sfail(ctx, RH_ERR_ARG, who + "n_samples = " + std::to_string(n_samples) + " (at least one; rows of " + std::to_string(n_items) + " x " +
                                              std::to_string(n_zones) + " x " + std::to_string(n_probs) + " float64 within 2 GiB)");
        if (n_samples < 1 || n_samples > ((int64_t)1 << 31) / ((int64_t)n_items * n_probs * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + "n_samples = " + std::to_string(n_samples) + " (at least one; rows of " + std::to_string(n_items) + " x " +
                                              std::to_string(n_probs) + " float64 within 2 GiB)");
        static const char *const KIND[] = {"BULK", "MEAN", "LAST"};
        for (int j = 0; j < n_items; ++j) {
            const int a = items[j].value, w = items[j].weight, kind = items[j].kind;
            if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown array id " + std::to_string(a));
            if (w < -1 || w >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown weight id " + std::to_string(w));
            const std::string name = std::string("array ") + SAS_NAMES[a];
            if (kind < RH_SAS_SCORES_BULK || kind > RH_SAS_SCORES_LAST)
                return sfail(ctx, RH_ERR_ARG, who + "kind " + std::to_string(kind) + " of " + name + " (0: BULK, 1: MEAN, 2: LAST)");
            for (int q = 0; q < j; ++q)
                if (items[q].value == a && items[q].weight == w && items[q].kind == kind)
                    return sfail(ctx, RH_ERR_ARG, who + name + " is given twice with the same weight and kind");
            if (SAS_KIND[a] == K_MASK) return sfail(ctx, RH_ERR_ARG, who + name + " is int32 (float64 arrays only)");
            if (SAS_KIND[a] == K_PARAM) return sfail(ctx, RH_ERR_ARG, who + name + " is a parameter block of the step (sas_params_* have no band)");
            if (SAS_KIND[a] == K_DAILY) return sfail(ctx, RH_ERR_ARG, who + name + " is a daily input of the step, not a result (daily inputs are weights here)");
            if (SAS_KIND[a] != K_CELL) return sfail(ctx, RH_ERR_ARG, who + name + " is age-resolved (a band is over one value per cell)");
            if (w >= 0 && (SAS_KIND[w] != K_DAILY || w == SA_C_in))
                return sfail(ctx, RH_ERR_ARG, who + "weight " + SAS_NAMES[w] + " is not a daily flux input (inf_mat_rz ... cpr_rz)");
            if (kind == RH_SAS_SCORES_BULK && w < 0) return sfail(ctx, RH_ERR_ARG, who + name + " is BULK and has no weight");
            if (kind != RH_SAS_SCORES_BULK && w >= 0)
                return sfail(ctx, RH_ERR_ARG, who + name + " is " + KIND[kind] + " and has the weight " + SAS_NAMES[w] + " (only BULK takes one)");
            if (!ctx->arr[a])
                return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
            P.val[j] = (const double *)ctx->arr[a].get();
            P.wgt[j] = w >= 0 ? (const double *)ctx->arr[w].get() : nullptr;
            P.kind[j] = kind;
            accumulate = accumulate || kind != RH_SAS_SCORES_LAST;
        }
        if (zonal) {   // the zones' sizes, the bound of a weighted zone, then the stable counting sort over the participating columns
            zone_off.assign((size_t)n_zones + 1, 0);
            folded.assign((size_t)n, 0);
            for (int64_t c = 0; c < n; ++c) {
                if (zone[c] < -1 || zone[c] >= n_zones)
                    return sfail(ctx, RH_ERR_ARG, who + "zone[" + std::to_string(c) + "] = " + std::to_string(zone[c]) + " (-1: outside every zone, else 0 ... " +
                                                      std::to_string(n_zones - 1) + ")");
                folded[(size_t)c] = zone[c] >= 0 && (!mask || mask[c]);
                if (folded[(size_t)c] && (!weights || weights[c])) ++zone_off[(size_t)zone[c] + 1];
            }
            for (int z = 0; z < n_zones && weights; ++z)
                if (zone_off[(size_t)z + 1] > SAS_BANDS_ZONAL_MAX_WEIGHTED)
                    return sfail(ctx, RH_ERR_ARG, who + "zone " + std::to_string(z) + " has " + std::to_string(zone_off[(size_t)z + 1]) +
                                                      " participating cells under a weight plane (at most " + std::to_string(SAS_BANDS_ZONAL_MAX_WEIGHTED) +
                                                      ": a uint32 LDS bin holds a zone's weights; a larger zone belongs to the mask of rh_sas_bands_configure)");
            for (int z = 0; z < n_zones; ++z) zone_off[(size_t)z + 1] += zone_off[(size_t)z];
            zone_cols.resize((size_t)zone_off[(size_t)n_zones]);
            std::vector<long long> at(zone_off.begin(), zone_off.end() - 1);
            for (int64_t c = 0; c < n; ++c)
                if (folded[(size_t)c] && (!weights || weights[c])) zone_cols[(size_t)at[(size_t)zone[c]]++] = (int)c;
            mask = folded.data();
        }
        if (mask || weights) {
            int64_t part = 0;
            for (int64_t c = 0; c < n; ++c) part += (!mask || mask[c]) && (!weights || weights[c]);
            if (!part)
                return sfail(ctx, RH_ERR_ARG, who + "no cell takes part (0 of " + std::to_string(n) + " cells have mask != 0 and a weight > 0)");
        }
        for (int64_t k = 0; k < n_samples; ++k) {
            if (first_day[k] > last_day[k])
                return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " is [" + std::to_string(first_day[k]) + ", " +
                                                  std::to_string(last_day[k]) + "]: its last day lies before its first");
            if (k && first_day[k] <= last_day[k - 1])
                return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " starts on day " + std::to_string(first_day[k]) + ", window " +
                                                  std::to_string(k - 1) + " ends on day " + std::to_string(last_day[k - 1]) +
                                                  " (windows are in increasing order and do not overlap)");
        }
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old result)
    for (DevBuf<double> *b : {&ctx->bands_acc, &ctx->bands_rows, &ctx->bands_obs}) SHIPCHK(ctx, b->release());
    for (DevBuf<unsigned long long> *b : {&ctx->bands_keys, &ctx->bands_hist}) SHIPCHK(ctx, b->release());
    for (DevBuf<long long> *b : {&ctx->bands_words, &ctx->bands_hdr, &ctx->bands_pair, &ctx->bands_part}) SHIPCHK(ctx, b->release());
    SHIPCHK(ctx, ctx->bands_mask.release());
    SHIPCHK(ctx, ctx->bands_weight.release());
    SHIPCHK(ctx, ctx->bands_cfg.release());
    SHIPCHK(ctx, ctx->bands_zone_off.release());
    SHIPCHK(ctx, ctx->bands_zone_cols.release());
    ctx->bands_zones = 0;
    ctx->bands_first.clear();
    ctx->bands_last.clear();
    ctx->bands_closed.clear();
    ctx->bands_obs_host.clear();
    ctx->bands_items = ctx->bands_probs = 0;
    ctx->bands_accumulate = false;
    ctx->bands_days = ctx->bands_k = 0;
    ctx->bands_open = -1;
    if (!n_items) return RH_OK;
    const size_t K = (size_t)n_samples, ni = (size_t)n_items, np = (size_t)n_probs, nb = zonal ? (size_t)n_zones : 1;   // nb: blocks per item
    const size_t acc_b = ni * 2 * (size_t)n * sizeof(double), key_b = ni * (size_t)n * sizeof(unsigned long long);
    const size_t hist_b = ni * RH_SAS_BANDS_MAX_PROBS * SAS_BANDS_NBINS * sizeof(unsigned long long);
    const size_t row_b = K * ni * nb * np * sizeof(double), hdr_b = K * ni * nb * SAS_BANDS_HDR * sizeof(long long), pair_b = K * ni * nb * 2 * sizeof(long long);
    SHIPCHK(ctx, ctx->bands_acc.alloc(acc_b));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_acc, 0, acc_b, ctx->stream));
    SHIPCHK(ctx, ctx->bands_keys.alloc(key_b));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_keys, 0xff, key_b, ctx->stream));   // RH_SELECT_KEY_MASKED: every byte set
    SHIPCHK(ctx, ctx->bands_hist.alloc(hist_b));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_hist, 0, hist_b, ctx->stream));
    SHIPCHK(ctx, ctx->bands_words.alloc(SBW_WORDS * sizeof(long long)));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_words, 0, SBW_WORDS * sizeof(long long), ctx->stream));
    const std::vector<double> nans(K * ni * nb * np, std::nan(""));
    SHIPCHK(ctx, ctx->bands_rows.alloc(row_b));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_rows, nans.data(), row_b, hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, ctx->bands_hdr.alloc(hdr_b));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_hdr, 0, hdr_b, ctx->stream));
    SHIPCHK(ctx, ctx->bands_pair.alloc(pair_b));
    SHIPCHK(ctx, hipMemsetAsync(ctx->bands_pair, 0xff, pair_b, ctx->stream));   // (-1, -1): every byte set
    if (mask) {
        SHIPCHK(ctx, ctx->bands_mask.alloc((size_t)n));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_mask, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    if (weights) {
        SHIPCHK(ctx, ctx->bands_weight.alloc((size_t)n * sizeof(unsigned short)));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_weight, weights, (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice, ctx->stream));
    }
    if (obs) {
        SHIPCHK(ctx, ctx->bands_obs.alloc(ni * nb * K * sizeof(double)));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_obs, obs, ni * nb * K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (!zonal) SHIPCHK(ctx, ctx->bands_part.alloc(ni * sas_bands_obs_grid((long long)n) * 2 * sizeof(long long)));
    }
    if (zonal) {
        SHIPCHK(ctx, ctx->bands_zone_off.alloc(zone_off.size() * sizeof(long long)));
        SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_zone_off, zone_off.data(), zone_off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        SHIPCHK(ctx, ctx->bands_zone_cols.alloc((zone_cols.size() + 1) * sizeof(int)));   // (+ 1: never an empty allocation)
        SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_zone_cols, zone_cols.data(), zone_cols.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    long long *words = ctx->bands_words.get();
    P.n_items = n_items;
    P.n_probs = n_probs;
    P.n = n;
    P.n_samples = n_samples;
    P.mask = ctx->bands_mask.get();
    P.weight = ctx->bands_weight.get();
    P.obs = ctx->bands_obs.get();
    P.acc = ctx->bands_acc.get();
    P.keys = ctx->bands_keys.get();
    P.hist = ctx->bands_hist.get();
    P.prefix = (unsigned long long *)(words + SBW_PREFIX);
    P.rank = words + SBW_RANK;
    P.m = words + SBW_M;
    P.nan = words + SBW_NAN;
    P.w = words + SBW_W;
    P.m_count = (unsigned *)(words + SBW_M_COUNT);
    P.nan_count = (unsigned *)(words + SBW_NAN_COUNT);
    P.obs_part = ctx->bands_part.get();
    P.rows = ctx->bands_rows.get();
    P.hdr = ctx->bands_hdr.get();
    P.obs_pair = ctx->bands_pair.get();
    SHIPCHK(ctx, ctx->bands_cfg.alloc(sizeof(SasBandsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(ctx->bands_cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and locals)
    ctx->bands_first.assign(first_day, first_day + n_samples);
    ctx->bands_last.assign(last_day, last_day + n_samples);
    ctx->bands_closed.assign(K, 0);
    if (obs) ctx->bands_obs_host.assign(obs, obs + ni * nb * K);
    ctx->bands_accumulate = accumulate;
    ctx->bands_probs = n_probs;
    ctx->bands_items = n_items;
    ctx->bands_zones = zonal ? n_zones : 0;
    return RH_OK;
}

int rh_sas_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                           const unsigned char *mask, const uint16_t *weights, const double *obs, const int64_t *first_day,
                           const int64_t *last_day, int64_t n_samples) {
    return sas_bands_configure(ctx, "rh_sas_bands_configure", items, n_items, probs, n_probs, nullptr, 0, mask, weights, obs, first_day, last_day, n_samples);
}

int rh_sas_bands_configure_zonal(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                                 const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights, const double *obs,
                                 const int64_t *first_day, const int64_t *last_day, int64_t n_samples) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items && (n_zones < 1 || n_zones > RH_SAS_BANDS_MAX_ZONES))
        return sfail(ctx, RH_ERR_ARG, "rh_sas_bands_configure_zonal: n_zones = " + std::to_string(n_zones) + " (1 ... " + std::to_string(RH_SAS_BANDS_MAX_ZONES) + ")");
    return sas_bands_configure(ctx, "rh_sas_bands_configure_zonal", items, n_items, probs, n_probs, zone, n_items ? n_zones : 0, mask, weights, obs, first_day,
                               last_day, n_samples);
}

static int sas_bands_on(rh_sas_ctx *ctx, const char *who) {
    return ctx ? sas_on(ctx, ctx->bands_items != 0, who, "rh_sas_bands_configure") : RH_ERR_ARG;
}

int rh_sas_bands_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_bands_on(ctx, "rh_sas_bands_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_bands_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_bands_enqueue(ctx, day);
}

int rh_sas_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair, size_t pair_bytes,
                      unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    if (int rc = sas_bands_on(ctx, "rh_sas_bands_read")) return rc;
    if (ctx->bands_zones) return sfail(ctx, RH_ERR_STATE, "rh_sas_bands_read: the bands are configured per zone (read them with rh_sas_bands_zonal_read)");
    const size_t K = ctx->bands_closed.size(), ni = (size_t)ctx->bands_items, np = (size_t)ctx->bands_probs;
    if (!rows || !hdr || !obs_pair || !closed || row_bytes != K * ni * np * sizeof(double) || hdr_bytes != K * ni * SAS_BANDS_HDR * sizeof(int64_t) ||
        pair_bytes != K * ni * 2 * sizeof(int64_t) || closed_bytes != K)
        return sfail(ctx, RH_ERR_ARG, "rh_sas_bands_read: size mismatch (n_samples x n_items x n_probs float64, n_samples x n_items x 3 and x 2 int64, "
                                      "n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(rows, ctx->bands_rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(hdr, ctx->bands_hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(obs_pair, ctx->bands_pair, pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(ctx->bands_closed.begin(), ctx->bands_closed.end(), closed);
    if (days_recorded) *days_recorded = ctx->bands_days;
    return rh_sas_sync(ctx);
}

int rh_sas_bands_zonal_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair, size_t pair_bytes,
                            unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = sas_on(ctx, ctx->bands_items != 0 && ctx->bands_zones != 0, "rh_sas_bands_zonal_read", "rh_sas_bands_configure_zonal")) return rc;
    const size_t K = ctx->bands_closed.size(), blocks = (size_t)ctx->bands_items * (size_t)ctx->bands_zones, np = (size_t)ctx->bands_probs;
    if (!rows || !hdr || !obs_pair || !closed || row_bytes != K * blocks * np * sizeof(double) || hdr_bytes != K * blocks * SAS_BANDS_HDR * sizeof(int64_t) ||
        pair_bytes != K * blocks * 2 * sizeof(int64_t) || closed_bytes != K)
        return sfail(ctx, RH_ERR_ARG, "rh_sas_bands_zonal_read: size mismatch (n_samples x n_items x n_zones x n_probs float64, n_samples x n_items x n_zones "
                                      "x 3 and x 2 int64, n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(rows, ctx->bands_rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(hdr, ctx->bands_hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(obs_pair, ctx->bands_pair, pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(ctx->bands_closed.begin(), ctx->bands_closed.end(), closed);
    if (days_recorded) *days_recorded = ctx->bands_days;
    return rh_sas_sync(ctx);
}

static int selftest2(const double *x, const double *k, double *out, int64_t n, int which);
int rh_sas_selftest_pow(const double *x, const double *k, double *out, int64_t n) { return selftest2(x, k, out, n, 0); }
int rh_sas_selftest_div(const double *a, const double *d, double *out, int64_t n) { return selftest2(a, d, out, n, 1); }
static int selftest2(const double *x, const double *k, double *out, int64_t n, int which) {
    if (!x || !k || !out || n <= 0) return RH_ERR_ARG;
    double *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)n * 3 * sizeof(double)) != hipSuccess) return RH_ERR_HIP;
    int rc = RH_OK;
    if (hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, k, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = RH_ERR_HIP;
    if (rc == RH_OK) {
        if (which == 0)
            hipLaunchKernelGGL(k_selftest_pow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, d + n, d + 2 * n, n);
        else
            hipLaunchKernelGGL(k_selftest_div, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, d + n, d + 2 * n, n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = RH_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
}

int rh_sas_enable_timing(rh_sas_ctx *ctx, int on) {
    if (!ctx) return RH_ERR_ARG;
    ctx->timing = on != 0;
    ctx->events.restart();
    return RH_OK;
}

int rh_sas_timing_summary(rh_sas_ctx *ctx, double *total_ms, int64_t *launches) {
    if (!ctx || !total_ms || !launches) return RH_ERR_ARG;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    SHIPCHK(ctx, ctx->events.total_ms(total_ms));
    *launches = (int64_t)ctx->events.launches();
    return RH_OK;
}

}  // extern "C"
