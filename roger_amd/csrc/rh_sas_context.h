// rh_sas_context.h -- the transport context (rh_sas_ctx) and what every host file of it uses: the array tables, a ring of rows (SasRing),
// the window clock (SasWindows), one struct per observer, sfail / SHIPCHK and the rules that the observers' calls share.  Part of the one
// translation unit rh_sas.hip, behind the kernel headers; host code only.
#pragma once

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

// What every observer's release() returns: the first error of the releases it made, all of which have run by then.
static hipError_t first_error(std::initializer_list<hipError_t> errors) {
    for (hipError_t e : errors)
        if (e != hipSuccess) return e;
    return hipSuccess;
}

// A ring of `cap` rows of row_elems float64 on the device, row r at r mod cap, and the rows' tags in a host ring of the same capacity:
// what the points, the totals and the zonal totals record into.  The host enqueues every row, so it counts them.  cap 0: the observer is off.
struct SasRing {
    DevBuf<double> ring;
    std::unique_ptr<int64_t[]> tags;
    int64_t cap = 0, row_elems = 0, rows = 0;
    bool on() const { return cap != 0; }
    double *next_row() const { return ring + (size_t)(rows % cap) * (size_t)row_elems; }
    void enqueued(int64_t tag) { tags[(size_t)(rows++ % cap)] = tag; }   // (the launches into next_row() are in the stream)
    // the last statement of a configure call, behind sas_ring_alloc and everything else that can fail
    void start(int64_t capacity) { cap = capacity; }
    hipError_t release() {
        tags.reset();
        cap = row_elems = rows = 0;
        return ring.release();
    }
};

// The windows of days that the scores and the bands compare over, and the clock that walks them: the windows, the day count, the window
// the count stands in or before, the closed flags (rh_sas_scores.h, "The day count" of roger_hip_sas.h).  All of it is the host's.
struct SasWindows {
    std::vector<int64_t> first, last;
    std::vector<unsigned char> closed;
    bool accumulate = false;   // an item is BULK or MEAN: the days before a window's last are launched too
    int64_t days = 0, k = 0, open = -1;
    // what a day is: `launch` the day's kernel for window k with these flags, or nothing
    struct Tick { bool launch; int64_t k; bool first, closes; };
    bool on() const { return !first.empty(); }
    void set(const int64_t *first_day, const int64_t *last_day, int64_t n_samples, bool accumulate_) {
        *this = SasWindows();
        first.assign(first_day, first_day + n_samples);
        last.assign(last_day, last_day + n_samples);
        closed.assign((size_t)n_samples, 0);
        accumulate = accumulate_;
    }
    // the next day of the count: which window it lies in is decided here, the kernel is told.  A closing day closes its window here
    // and nowhere else.
    Tick tick() {
        Tick now = {false, 0, false, false};
        const int64_t t = days++, K = (int64_t)first.size();
        while (k < K && last[(size_t)k] < t) ++k;   // (windows that passed without being open)
        if (k >= K || t < first[(size_t)k]) return now;
        if (t == first[(size_t)k]) open = k;
        if (open != k) return now;                  // (its first day was never recorded)
        now.k = k;
        now.first = t == first[(size_t)k];
        now.closes = t == last[(size_t)k];
        now.launch = now.closes || accumulate;
        if (now.closes) {
            closed[(size_t)k] = 1;
            open = -1;
            ++k;
        }
        return now;
    }
};

// ---- one struct per observer: its buffers on the device, the host's copies, on() and release().  release() frees every buffer,
// returns the first error and leaves the observer off with every host field at its initial value: the assignment at its end resets
// whatever the struct holds, so a member added later cannot stay live behind a released neighbour. ----

// time series at observation columns (rh_sas_points_configure): the ring (off: no k_sas_points launch) and what the kernel is told
struct SasPoints {
    static constexpr const char *configure = "rh_sas_points_configure";
    SasRing ring;
    DevBuf<SasPointsDev> cfg;
    int blocks = 0;   // workgroups of one row's launch
    bool on() const { return ring.on(); }
    hipError_t release() {
        const hipError_t e = first_error({ring.release(), cfg.release()});
        *this = SasPoints();
        return e;
    }
};

// catchment totals (rh_sas_totals_configure): the ring (off: no launches); the width-1 partials, the two level buffers of the age
// rule (rh_sas_totals.h), the mask on the device, and the host's copy of what the kernels are told
struct SasTotals {
    static constexpr const char *configure = "rh_sas_totals_configure";
    SasRing ring;
    DevBuf<double> part, lvl[2];
    DevBuf<SasTotalsDev> cfg;
    DevBuf<unsigned char> mask;
    SasTotalsDev host = {};
    int width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *src[RH_SAS_TOTALS_MAX_ITEMS] = {};   // the age items' arrays
    int64_t ncells = 0;
    bool on() const { return ring.on(); }
    hipError_t release() {
        const hipError_t e = first_error({ring.release(), part.release(), lvl[0].release(), lvl[1].release(), cfg.release(), mask.release()});
        *this = SasTotals();
        return e;
    }
};

// zonal totals (rh_sas_zonal_configure): the ring (off: no launches); the slots' width-1 partials, the ONE level-1 buffer of the age
// rule, the index over the zone map (rh_sas_zonal.h) and where its parts start
struct SasZonal {
    static constexpr const char *configure = "rh_sas_zonal_configure";
    SasRing ring;
    DevBuf<double> part, lvl;
    DevBuf<SasZonalDev> cfg;
    DevBuf<int> index;
    SasZonalDev host = {};
    int nzones = 0;
    int width[RH_SAS_TOTALS_MAX_ITEMS] = {};
    const double *src[RH_SAS_TOTALS_MAX_ITEMS] = {};
    int64_t at[SZ_PARTS] = {};
    int64_t ntiles = 0;
    std::vector<int64_t> ncells;   // cells of every zone
    bool on() const { return ring.on(); }
    hipError_t release() {
        const hipError_t e = first_error({ring.release(), part.release(), lvl.release(), cfg.release(), index.release()});
        *this = SasZonal();
        return e;
    }
};

// scores against observed samples (rh_sas_scores_configure): the moments, the observations and the series map on the device; the
// windows and their clock are the host's.  On while it has windows.
struct SasScores {
    static constexpr const char *configure = "rh_sas_scores_configure";
    DevBuf<double> buf, obs;
    DevBuf<int32_t> series;
    DevBuf<SasScoresDev> cfg;
    SasWindows win;
    int n_items = 0;
    bool on() const { return win.on(); }
    hipError_t release() {
        const hipError_t e = first_error({buf.release(), obs.release(), series.release(), cfg.release()});
        *this = SasScores();
        return e;
    }
};

// transport bands (rh_sas_bands_configure): num / den, the key planes, the global histograms, the selection's few words (prefixes,
// ranks, counts: SasBandsWords), the result and what the kernels are told on the device; the windows, their clock and the observations'
// copy are the host's (rh_sas_bands.h).  On while it has windows.
struct SasBands {
    static constexpr const char *configure = "rh_sas_bands_configure";
    DevBuf<double> acc, rows, obs;
    DevBuf<unsigned long long> keys, hist;
    DevBuf<long long> words, hdr, pair, part;
    DevBuf<unsigned char> mask;
    DevBuf<unsigned short> weight;
    DevBuf<SasBandsDev> cfg;
    SasWindows win;
    std::vector<double> obs_host;   // [item][sample]; empty: no observations
    int n_items = 0, n_probs = 0;
    // ... per zone (rh_sas_bands_configure_zonal, rh_sas_bands_zonal.h): the result gains the zone axis behind the item's, the observations'
    // copy is [item][zone][sample]; the zones' column lists
    int zones = 0;                  // 0: the plain configuration (k_sas_bands_hist / _pick); else k_sas_bands_zonal on (zones, items)
    DevBuf<long long> zone_off;
    DevBuf<int> zone_cols;
    bool on() const { return win.on(); }
    // window k has an observation in one of the (item[, zone]) blocks of its result
    bool observed(int64_t k) const {
        const size_t K = win.first.size(), blocks = (size_t)n_items * (size_t)(zones ? zones : 1);
        for (size_t b = 0; b < blocks && !obs_host.empty(); ++b) {
            const double o = obs_host[b * K + (size_t)k];
            if (o == o) return true;
        }
        return false;
    }
    hipError_t release() {
        const hipError_t e = first_error({acc.release(), rows.release(), obs.release(), keys.release(), hist.release(), words.release(), hdr.release(),
                                          pair.release(), part.release(), mask.release(), weight.release(), cfg.release(), zone_off.release(),
                                          zone_cols.release()});
        *this = SasBands();
        return e;
    }
};

// transport bands by age (rh_sas_age_bands_configure, rh_sas_age_bands.h): ONE key plane [Wmax][n_part] that the items share, the
// participating columns and their compacted weights, the probabilities and the result on the device; the items' arrays and widths, the
// windows and their clock are the host's.  On while it has windows.
struct SasAgeBands {
    static constexpr const char *configure = "rh_sas_age_bands_configure";
    DevBuf<double> rows, probs;
    DevBuf<long long> hdr;
    DevBuf<unsigned long long> keys;
    DevBuf<int> part_cols;
    DevBuf<unsigned short> wts_c;   // null: every participating column counts 1
    SasWindows win;
    const double *src[RH_SAS_AGE_BANDS_MAX_ITEMS] = {};
    int width[RH_SAS_AGE_BANDS_MAX_ITEMS] = {};
    int n_items = 0, n_probs = 0;
    int64_t n_part = 0, ages_total = 0;   // ages_total: the sum of the items' widths
    // ... per zone (rh_sas_age_bands_configure_zonal): part_cols and wts_c are in zone order, the result gains the zone axis behind the
    // item's and in front of the age axis; where each zone's run starts and the lists of the short and of the long zones
    int zones = 0;                        // 0: the plain configuration (k_sas_age_bands); else k_sas_age_bands_zonal / _small
    DevBuf<long long> zone_off;
    DevBuf<int> zone_lists;               // [n_short] short zones, then [n_long] long ones
    int n_short = 0, n_long = 0;
    SasAgeZones dev_zones() const { return {zone_off.get(), zone_lists.get(), zone_lists.get() + n_short, n_short, n_long}; }
    bool on() const { return win.on(); }
    hipError_t release() {
        const hipError_t e = first_error({rows.release(), probs.release(), hdr.release(), keys.release(), part_cols.release(), wts_c.release(),
                                          zone_off.release(), zone_lists.release()});
        *this = SasAgeBands();
        return e;
    }
};

// window means of the bands by age (rh_sas_age_window_bands_configure, rh_sas_age_bands.h): everything the snapshot observer holds -- a key
// plane, a participating set, a result and a clock, all of its OWN, since both may be configured -- and per item num [n_part][W_j] and
// den [n_part][W_j] in ONE allocation, zero at configure, the first row of the item's daily weight (BULK; null: MEAN)
struct SasAgeWindowBands : SasAgeBands {
    static constexpr const char *configure = "rh_sas_age_window_bands_configure";
    DevBuf<double> acc;
    size_t acc_off[RH_SAS_AGE_BANDS_MAX_ITEMS] = {};     // where item j's num starts; its den follows n_part x W_j later
    const double *wgt[RH_SAS_AGE_BANDS_MAX_ITEMS] = {};
    hipError_t release() {
        const hipError_t e = first_error({SasAgeBands::release(), acc.release()});
        *this = SasAgeWindowBands();
        return e;
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
    SasPoints points;
    SasTotals totals;
    SasZonal zonal;
    SasScores scores;
    SasBands bands;
    SasAgeBands age_bands;
    SasAgeWindowBands age_window_bands;
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

// ---- what the observers' calls share; the rules of a ring itself are rh_host.h's ----
static int sas_check_capacity(rh_sas_ctx *ctx, const std::string &who, int64_t capacity) {
    const std::string why = ring_capacity_refusal(who, capacity, 0);   // (every configure call bounds its ring's bytes itself)
    return why.empty() ? RH_OK : sfail(ctx, RH_ERR_ARG, why);
}
// RH_ERR_STATE for the function `who` unless `configure` has switched its observer on
static int sas_on(rh_sas_ctx *ctx, bool on, const char *who, const char *configure) {
    return on ? RH_OK : sfail(ctx, RH_ERR_STATE, std::string(who) + ": " + configure + " has not been called");
}
// ... for the observer `obs` of a context that may be null
template <class O>
static int sas_on(rh_sas_ctx *ctx, O rh_sas_ctx::*obs, const char *who) {
    return ctx ? sas_on(ctx, (ctx->*obs).on(), who, O::configure) : RH_ERR_ARG;
}

// -- a ring's configure call: the bound before anything is released, the allocation behind the release; SasRing::start() ends the call --
// capacity rows of row_elems float64 stay within 2 GiB; `row` says what a row is made of
static int sas_ring_bound(rh_sas_ctx *ctx, const std::string &who, int64_t capacity, int64_t row_elems, const std::string &row) {
    if (capacity > ((int64_t)1 << 31) / (row_elems * (int64_t)sizeof(double)))
        return sfail(ctx, RH_ERR_ARG, who + "capacity = " + std::to_string(capacity) + " rows of " + row + " float64 are a ring above 2 GiB");
    return RH_OK;
}
// the tags and the buffer of a released ring, which stays off
static int sas_ring_alloc(rh_sas_ctx *ctx, const std::string &who, SasRing &r, int64_t capacity, int64_t row_elems) {
    std::unique_ptr<int64_t[]> tags(new (std::nothrow) int64_t[(size_t)capacity]);
    if (!tags) return sfail(ctx, RH_ERR_ARG, who + "out of host memory for the tags of " + std::to_string(capacity) + " rows");
    SHIPCHK(ctx, r.ring.alloc((size_t)capacity * (size_t)row_elems * sizeof(double)));
    r.tags = std::move(tags);
    r.row_elems = row_elems;
    return RH_OK;
}

// -- a ring's other calls, for the function `who` of the observer `obs` --
// the rows recorded so far; `other`: the call's second result pointer, where it has one
template <class O>
static int sas_ring_count(rh_sas_ctx *ctx, O rh_sas_ctx::*obs, const char *who, int64_t *rows_total, const void *other) {
    if (int rc = sas_on(ctx, obs, who)) return rc;
    if (!rows_total || !other) return sfail(ctx, RH_ERR_ARG, std::string(who) + ": null pointer");
    *rows_total = (ctx->*obs).ring.rows;
    return RH_OK;
}
template <class O>
static int sas_ring_row_elems(const rh_sas_ctx *ctx, O rh_sas_ctx::*obs, const char *who, int64_t *elems) {
    if (int rc = sas_on(const_cast<rh_sas_ctx *>(ctx), obs, who)) return rc;
    if (!elems) return RH_ERR_ARG;
    *elems = (ctx->*obs).ring.row_elems;
    return RH_OK;
}
// rows [first_row, first_row + n_rows) and their tags to the host.  Synchronises.
template <class O>
static int sas_ring_read(rh_sas_ctx *ctx, O rh_sas_ctx::*obs, const char *who, int64_t first_row, int64_t n_rows, int64_t *tags, double *values,
                         size_t value_bytes) {
    if (int rc = sas_on(ctx, obs, who)) return rc;
    const SasRing &r = (ctx->*obs).ring;
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

// The weight of a (value, weight, kind) item whose ids and kind are known ones: a daily flux input, which BULK has and no other kind does.
// The one statement of it, for the scores, the bands and the window means of the bands by age; `name` is "array <value>".
static int sas_window_weight(rh_sas_ctx *ctx, const std::string &who, const std::string &name, int w, int kind) {
    static const char *const KIND[] = {"BULK", "MEAN", "LAST"};
    if (w >= 0 && (SAS_KIND[w] != K_DAILY || w == SA_C_in))
        return sfail(ctx, RH_ERR_ARG, who + "weight " + SAS_NAMES[w] + " is not a daily flux input (inf_mat_rz ... cpr_rz)");
    if (kind == RH_SAS_SCORES_BULK && w < 0) return sfail(ctx, RH_ERR_ARG, who + name + " is BULK and has no weight");
    if (kind != RH_SAS_SCORES_BULK && w >= 0)
        return sfail(ctx, RH_ERR_ARG, who + name + " is " + KIND[kind] + " and has the weight " + SAS_NAMES[w] + " (only BULK takes one)");
    return RH_OK;
}

// What the (value, weight, kind) items of rh_sas_scores_configure and of the two bands calls are: ids and kinds checked, the arrays and
// weights on the device, and whether any item accumulates over its window.  `who` opens the message of a refusal; `params_are` says what
// sas_params_* are to the caller ("are not scored"), `one_value` why an age-resolved array is none of its items.
static int sas_window_items(rh_sas_ctx *ctx, const std::string &who, const rh_sas_scores_item *items, int n_items, const char *params_are,
                            const char *one_value, const double **val, const double **wgt, int *kinds, bool *accumulate) {
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
        if (SAS_KIND[a] == K_PARAM) return sfail(ctx, RH_ERR_ARG, who + name + " is a parameter block of the step (sas_params_* " + params_are + ")");
        if (SAS_KIND[a] == K_DAILY) return sfail(ctx, RH_ERR_ARG, who + name + " is a daily input of the step, not a result (daily inputs are weights here)");
        if (SAS_KIND[a] != K_CELL) return sfail(ctx, RH_ERR_ARG, who + name + " is age-resolved (" + one_value + ")");
        if (int rc = sas_window_weight(ctx, who, name, w, kind)) return rc;
        if (!ctx->arr[a])
            return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
        val[j] = (const double *)ctx->arr[a].get();
        wgt[j] = w >= 0 ? (const double *)ctx->arr[w].get() : nullptr;
        kinds[j] = kind;
        *accumulate = *accumulate || kind != RH_SAS_SCORES_LAST;
    }
    return RH_OK;
}

// The windows of the same calls: each ends no earlier than it starts, and they come in increasing order without overlap.
static int sas_check_windows(rh_sas_ctx *ctx, const std::string &who, const int64_t *first_day, const int64_t *last_day, int64_t n_samples) {
    for (int64_t k = 0; k < n_samples; ++k) {
        if (first_day[k] > last_day[k])
            return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " is [" + std::to_string(first_day[k]) + ", " +
                                              std::to_string(last_day[k]) + "]: its last day lies before its first");
        if (k && first_day[k] <= last_day[k - 1])
            return sfail(ctx, RH_ERR_ARG, who + "window " + std::to_string(k) + " starts on day " + std::to_string(first_day[k]) + ", window " +
                                              std::to_string(k - 1) + " ends on day " + std::to_string(last_day[k - 1]) +
                                              " (windows are in increasing order and do not overlap)");
    }
    return RH_OK;
}
