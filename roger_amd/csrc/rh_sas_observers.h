// rh_sas_observers.h -- what follows every day of the transport model: the time series at observation columns (rh_sas_points_*), the
// catchment totals (rh_sas_totals_*), the zonal totals (rh_sas_zonal_*), the scores against observed samples (rh_sas_scores_*) and the
// transport bands, plain and per zone (rh_sas_bands_*), by age (rh_sas_age_bands_*) and the window means by age
// (rh_sas_age_window_bands_*).  Each has its launch sequence (sas_*_enqueue, which the day calls), its configure
// call and its reads.  Part of the one translation unit rh_sas.hip, behind rh_sas_context.h; the entry points get their C linkage from
// their declarations in roger_hip_sas.h.
#pragma once

// ---- time series at observation columns (include/roger_hip_sas.h) ----
// one row behind what the stream holds so far: the gather into the ring's next slot, the tag beside it
static int sas_points_enqueue(rh_sas_ctx *ctx, int64_t tag) {
    SasPoints &S = ctx->points;
    hipLaunchKernelGGL(k_sas_points, dim3((unsigned)S.blocks), dim3(SAS_POINTS_BLOCK), 0, ctx->stream, S.cfg.get(), S.ring.next_row());
    SHIPCHK(ctx, hipGetLastError());
    S.ring.enqueued(tag);
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
        if (int rc = sas_ring_bound(ctx, who, capacity, row_elems, std::to_string(row_elems))) return rc;
    }
    SasPoints &S = ctx->points;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, S.release());
    if (off) return RH_OK;
    if (int rc = sas_ring_alloc(ctx, who, S.ring, capacity, row_elems)) return rc;
    SHIPCHK(ctx, S.cfg.alloc(sizeof(SasPointsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(S.cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the source is a local)
    S.blocks = P.first_block[n_arrays];
    S.ring.start(capacity);
    return RH_OK;
}

int rh_sas_points_record(rh_sas_ctx *ctx, int64_t tag) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::points, "rh_sas_points_record")) return rc;
    return sas_points_enqueue(ctx, tag);
}
int rh_sas_points_count(rh_sas_ctx *ctx, int64_t *rows_total) { return sas_ring_count(ctx, &rh_sas_ctx::points, "rh_sas_points_count", rows_total, rows_total); }
int rh_sas_points_row_elems(const rh_sas_ctx *ctx, int64_t *elems) { return sas_ring_row_elems(ctx, &rh_sas_ctx::points, "rh_sas_points_row_elems", elems); }
int rh_sas_points_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    return sas_ring_read(ctx, &rh_sas_ctx::points, "rh_sas_points_read", first_row, n_rows, tags, values, value_bytes);
}

// ---- catchment totals (include/roger_hip_sas.h; kernels and orders: rh_sas_totals.h) ----
// one row behind what the stream holds so far: the width-1 statistics of every item, then the age items one after another
static int sas_totals_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    SasTotals &S = ctx->totals;
    const int64_t n = ctx->cfg.n_cells;
    const int64_t day_off = day < 0 ? -1 : (day % ctx->cfg.forcing_days) * n;
    const SasTotalsDev &P = S.host;
    double *row = S.ring.next_row();
    hipLaunchKernelGGL(k_sas_totals_tiles, dim3((unsigned)P.ntiles), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, S.cfg.get(), day_off);
    hipLaunchKernelGGL(k_sas_totals_finish, dim3((unsigned)P.n_items), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, S.cfg.get(), row);
    for (int j = 0; j < P.n_items; ++j) {
        const int W = S.width[j];
        if (W == 1) continue;
        const unsigned bs = (unsigned)std::min(SAS_TOTALS_BLOCK, (W + 63) / 64 * 64);
        const unsigned chunks = ((unsigned)W + bs - 1) / bs;
        const double *src = S.src[j];
        int64_t m = n;
        for (int lvl = 0;; ++lvl) {
            const int64_t runs = (m + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
            double *dst = runs == 1 ? row + P.off[j] + 2 : S.lvl[lvl & 1].get();
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
    S.ring.enqueued(tag);
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
        if (int rc = sas_ring_bound(ctx, who, capacity, row_elems, std::to_string(row_elems))) return rc;
    }
    SasTotals &S = ctx->totals;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, S.release());
    if (!n_items) return RH_OK;
    if (int rc = sas_ring_alloc(ctx, who, S.ring, capacity, row_elems)) return rc;
    const int64_t ntiles = (n + SAS_TOTALS_BLOCK - 1) / SAS_TOTALS_BLOCK, runs1 = (n + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
    const int64_t runs2 = (runs1 + SAS_TOTALS_RUN - 1) / SAS_TOTALS_RUN;
    SHIPCHK(ctx, S.part.alloc((size_t)n_items * SAS_TOTALS_NSTAT * (size_t)ntiles * sizeof(double)));
    if (wmax && runs1 > 1) {
        SHIPCHK(ctx, S.lvl[0].alloc((size_t)runs1 * (size_t)wmax * sizeof(double)));
        SHIPCHK(ctx, S.lvl[1].alloc((size_t)runs2 * (size_t)wmax * sizeof(double)));
    }
    if (mask) {
        SHIPCHK(ctx, S.mask.alloc((size_t)n));
        SHIPCHK(ctx, hipMemcpyAsync(S.mask, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    P.n_items = n_items;
    P.ntiles = (int)ntiles;
    P.n = n;
    P.mask = S.mask.get();
    P.part = S.part.get();
    SHIPCHK(ctx, S.cfg.alloc(sizeof(SasTotalsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(S.cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and a local)
    S.host = P;
    std::copy(width, width + RH_SAS_TOTALS_MAX_ITEMS, S.width);
    std::copy(srcs, srcs + RH_SAS_TOTALS_MAX_ITEMS, S.src);
    S.ncells = ncells;
    S.ring.start(capacity);
    return RH_OK;
}

int rh_sas_totals_record(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::totals, "rh_sas_totals_record")) return rc;
    return sas_totals_enqueue(ctx, tag, day);
}
int rh_sas_totals_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (int rc = sas_ring_count(ctx, &rh_sas_ctx::totals, "rh_sas_totals_count", rows_total, ncells)) return rc;
    *ncells = ctx->totals.ncells;
    return RH_OK;
}
int rh_sas_totals_row_elems(const rh_sas_ctx *ctx, int64_t *elems) { return sas_ring_row_elems(ctx, &rh_sas_ctx::totals, "rh_sas_totals_row_elems", elems); }
int rh_sas_totals_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    return sas_ring_read(ctx, &rh_sas_ctx::totals, "rh_sas_totals_read", first_row, n_rows, tags, values, value_bytes);
}

// ---- zonal totals (include/roger_hip_sas.h; kernels, index and orders: rh_sas_zonal.h) ----
// one row behind what the stream holds so far: every item's width-1 statistics for every zone, then the age items one after another
static int sas_zonal_enqueue(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    SasZonal &S = ctx->zonal;
    const int64_t n = ctx->cfg.n_cells;
    const int64_t day_off = day < 0 ? -1 : (day % ctx->cfg.forcing_days) * n;
    const SasZonalDev &P = S.host;
    const int *ix = S.index.get();
    const int64_t *at = S.at;
    double *row = S.ring.next_row();
    const unsigned ntiles = (unsigned)S.ntiles, nz = (unsigned)S.nzones;
    hipLaunchKernelGGL(k_sas_zonal_tiles, dim3(ntiles), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, S.cfg.get(), day_off);
    hipLaunchKernelGGL(k_sas_zonal_finish, dim3(nz), dim3(SAS_TOTALS_BLOCK), 0, ctx->stream, S.cfg.get(), row);
    for (int j = 0; j < P.n_items; ++j) {
        const int W = S.width[j];
        if (W == 1) continue;
        const unsigned bs = (unsigned)std::min(SAS_TOTALS_BLOCK, (W + 63) / 64 * 64);
        const unsigned chunks = ((unsigned)W + bs - 1) / bs;
        hipLaunchKernelGGL(k_sas_zonal_ages, dim3(ntiles, chunks), dim3(bs), 0, ctx->stream, S.src[j], W, ix + at[SZ_TILE_PTR],
                           ix + at[SZ_CELL_PTR], ix + at[SZ_CELL], P.wgt[j] ? P.wgt[j] + std::max<int64_t>(day_off, 0) : nullptr,
                           (P.wgt[j] && day_off < 0) ? 0 : 1, S.lvl.get());
        hipLaunchKernelGGL(k_sas_zonal_ages_finish, dim3(nz, chunks), dim3(bs), 0, ctx->stream, (const double *)S.lvl.get(), W,
                           ix + at[SZ_RUN_PTR], ix + at[SZ_RUN_SLOT], ix + at[SZ_SLOT_TILE], row + P.off[j] + 2, P.zone_elems);
    }
    SHIPCHK(ctx, hipGetLastError());
    S.ring.enqueued(tag);
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
    int64_t zone_elems = 0, at[SZ_PARTS] = {}, S1 = 0;
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
        if (int rc = sas_ring_bound(ctx, who, capacity, zone_elems * n_zones, std::to_string(n_zones) + " zones x " + std::to_string(zone_elems)))
            return rc;
        S1 = sas_zonal_index(zone, n, n_zones, index, at);
        if (wmax && S1 > ((int64_t)1 << 31) / ((int64_t)wmax * (int64_t)sizeof(double)))
            return sfail(ctx, RH_ERR_ARG, who + std::to_string(S1) + " (tile, zone) slots x " + std::to_string(wmax) +
                                              " float64 are a level-1 buffer above 2 GiB");
    }
    SasZonal &S = ctx->zonal;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    SHIPCHK(ctx, S.release());
    if (!n_items) return RH_OK;
    if (int rc = sas_ring_alloc(ctx, who, S.ring, capacity, zone_elems * n_zones)) return rc;
    SHIPCHK(ctx, S.part.alloc((size_t)S1 * (size_t)n_items * SAS_TOTALS_NSTAT * sizeof(double)));
    if (wmax) SHIPCHK(ctx, S.lvl.alloc((size_t)S1 * (size_t)wmax * sizeof(double)));
    SHIPCHK(ctx, S.index.alloc(index.size() * sizeof(int)));
    SHIPCHK(ctx, hipMemcpyAsync(S.index, index.data(), index.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const int *ix = S.index.get();
    P.n_items = n_items;
    P.n = n;
    P.zone_elems = zone_elems;
    P.zone = ix + at[SZ_ZONE];
    P.tile_ptr = ix + at[SZ_TILE_PTR];
    P.tile_zone = ix + at[SZ_TILE_ZONE];
    P.acc_ptr = ix + at[SZ_ACC_PTR];
    P.acc_slot = ix + at[SZ_ACC_SLOT];
    P.part = S.part.get();
    SHIPCHK(ctx, S.cfg.alloc(sizeof(SasZonalDev)));
    SHIPCHK(ctx, hipMemcpyAsync(S.cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are locals)
    S.host = P;
    std::copy(width, width + RH_SAS_TOTALS_MAX_ITEMS, S.width);
    std::copy(srcs, srcs + RH_SAS_TOTALS_MAX_ITEMS, S.src);
    std::copy(at, at + SZ_PARTS, S.at);
    S.ntiles = (n + SAS_TOTALS_BLOCK - 1) / SAS_TOTALS_BLOCK;
    S.ncells = std::move(ncells);
    S.nzones = n_zones;
    S.ring.start(capacity);
    return RH_OK;
}

int rh_sas_zonal_record(rh_sas_ctx *ctx, int64_t tag, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::zonal, "rh_sas_zonal_record")) return rc;
    return sas_zonal_enqueue(ctx, tag, day);
}
int rh_sas_zonal_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (int rc = sas_ring_count(ctx, &rh_sas_ctx::zonal, "rh_sas_zonal_count", rows_total, ncells)) return rc;
    std::copy(ctx->zonal.ncells.begin(), ctx->zonal.ncells.end(), ncells);
    return RH_OK;
}
int rh_sas_zonal_row_elems(const rh_sas_ctx *ctx, int64_t *elems) { return sas_ring_row_elems(ctx, &rh_sas_ctx::zonal, "rh_sas_zonal_row_elems", elems); }
int rh_sas_zonal_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes) {
    return sas_ring_read(ctx, &rh_sas_ctx::zonal, "rh_sas_zonal_read", first_row, n_rows, tags, values, value_bytes);
}

// ---- scores against observed samples (include/roger_hip_sas.h; the kernel and the rule: rh_sas_scores.h) ----
// the next day of the count, behind what the stream holds so far
static int sas_scores_enqueue(rh_sas_ctx *ctx, int64_t day) {
    SasScores &S = ctx->scores;
    const SasWindows::Tick now = S.win.tick();
    if (!now.launch) return RH_OK;
    const int64_t n = ctx->cfg.n_cells;
    hipLaunchKernelGGL(k_sas_scores, dim3((unsigned)((n + SAS_SCORES_BLOCK - 1) / SAS_SCORES_BLOCK)), dim3(SAS_SCORES_BLOCK), 0, ctx->stream,
                       S.cfg.get(), now.k, now.first ? 1 : 0, now.closes ? 1 : 0, (day % ctx->cfg.forcing_days) * n);
    SHIPCHK(ctx, hipGetLastError());
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
        if (int rc = sas_window_items(ctx, who, items, n_items, "are not scored", "a sample is compared with one value per cell", P.val, P.wgt, P.kind,
                                      &accumulate))
            return rc;
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
        if (int rc = sas_check_windows(ctx, who, first_day, last_day, n_samples)) return rc;
    }
    SasScores &S = ctx->scores;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that add into the old moments)
    SHIPCHK(ctx, S.release());
    if (!n_items) return RH_OK;
    const size_t mb = (size_t)n_items * SAS_SCORES_NMOM * (size_t)n * sizeof(double);
    const size_t ob = (size_t)n_items * (size_t)n_series * (size_t)n_samples * sizeof(double);
    SHIPCHK(ctx, S.buf.alloc(mb));
    SHIPCHK(ctx, hipMemsetAsync(S.buf, 0, mb, ctx->stream));
    SHIPCHK(ctx, S.obs.alloc(ob));
    SHIPCHK(ctx, hipMemcpyAsync(S.obs, obs, ob, hipMemcpyHostToDevice, ctx->stream));
    if (series) {
        SHIPCHK(ctx, S.series.alloc((size_t)n * sizeof(int32_t)));
        SHIPCHK(ctx, hipMemcpyAsync(S.series, series, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    P.n_items = n_items;
    P.n_series = n_series;
    P.n = n;
    P.n_samples = n_samples;
    P.series = S.series.get();
    P.obs = S.obs.get();
    P.scores = S.buf.get();
    SHIPCHK(ctx, S.cfg.alloc(sizeof(SasScoresDev)));
    SHIPCHK(ctx, hipMemcpyAsync(S.cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and a local)
    S.n_items = n_items;
    S.win.set(first_day, last_day, n_samples, accumulate);
    return RH_OK;
}

int rh_sas_scores_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::scores, "rh_sas_scores_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_scores_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_scores_enqueue(ctx, day);
}

int rh_sas_scores_read(rh_sas_ctx *ctx, double *moments, size_t moment_bytes, unsigned char *closed, size_t closed_bytes,
                       int64_t *days_scored) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::scores, "rh_sas_scores_read")) return rc;
    const SasScores &S = ctx->scores;
    if (!moments || !closed || moment_bytes != (size_t)S.n_items * SAS_SCORES_NMOM * (size_t)ctx->cfg.n_cells * sizeof(double) ||
        closed_bytes != S.win.closed.size())
        return sfail(ctx, RH_ERR_ARG, "rh_sas_scores_read: size mismatch (n_items x 9 x n_cells float64, n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(moments, S.buf, moment_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(S.win.closed.begin(), S.win.closed.end(), closed);
    if (days_scored) *days_scored = S.win.days;
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

// pass P of the transport bands' selection (rh_sas_bands.h): the histograms over the key planes, then the pick of one workgroup
template <int P>
static void sas_bands_pass(rh_sas_ctx *ctx, unsigned grid, int64_t k) {
    const SasBandsDev *cfg = ctx->bands.cfg.get();
    hipLaunchKernelGGL(k_sas_bands_hist<P>, dim3(grid), dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg);
    hipLaunchKernelGGL(k_sas_bands_pick<P>, dim3(1), dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg, k);
}
template <int... P>   // ... and the passes P..., in order
static void sas_bands_passes(rh_sas_ctx *ctx, unsigned grid, int64_t k, std::integer_sequence<int, P...>) {
    (sas_bands_pass<P>(ctx, grid, k), ...);
}

// the next day of the count, behind what the stream holds so far: the day's kernel; on a closing day the selection follows it -- per zone
// one launch, else the six passes -- and the kernels of the observations where window k has one
static int sas_bands_enqueue(rh_sas_ctx *ctx, int64_t day) {
    SasBands &S = ctx->bands;
    const SasWindows::Tick now = S.win.tick();
    if (!now.launch) return RH_OK;
    const int64_t n = ctx->cfg.n_cells, k = now.k;
    const SasBandsDev *cfg = S.cfg.get();
    hipLaunchKernelGGL(k_sas_bands_day, dim3((unsigned)((n + RH_SELECT_BLOCK - 1) / RH_SELECT_BLOCK)), dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg,
                       now.first ? 1 : 0, now.closes ? 1 : 0, (day % ctx->cfg.forcing_days) * n);
    if (now.closes && S.zones) {   // per zone: one launch in place of the twelve, one more where window k has an observation
        const SasBandsZonalDev Z = {S.zone_off.get(), S.zone_cols.get()};
        const dim3 grid((unsigned)S.zones, (unsigned)S.n_items);
        if (S.weight)
            hipLaunchKernelGGL(k_sas_bands_zonal<true>, grid, dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg, Z, k);
        else
            hipLaunchKernelGGL(k_sas_bands_zonal<false>, grid, dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg, Z, k);
        if (S.observed(k)) hipLaunchKernelGGL(k_sas_bands_obs_zonal, grid, dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg, Z, k);
    } else if (now.closes) {
        sas_bands_passes(ctx, bands_weighted_grid((long long)n), k, std::make_integer_sequence<int, RH_SELECT_PASSES>{});
        if (S.observed(k)) {   // (an item without one ends after the scalar loads: its pair stays (-1, -1), as configure wrote it)
            const unsigned parts = select_obs_grid((long long)n);
            hipLaunchKernelGGL(k_sas_bands_obs, dim3(parts, (unsigned)S.n_items), dim3(RH_SELECT_BLOCK), 0, ctx->stream, cfg, k);
            hipLaunchKernelGGL(k_sas_bands_obs_row, dim3((unsigned)S.n_items), dim3(64), 0, ctx->stream, cfg, k, (int)parts);
        }
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
        if (int rc = sas_window_items(ctx, who, items, n_items, "have no band", "a band is over one value per cell", P.val, P.wgt, P.kind, &accumulate))
            return rc;
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
        if (int rc = sas_check_windows(ctx, who, first_day, last_day, n_samples)) return rc;
    }
    SasBands &S = ctx->bands;
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old result)
    SHIPCHK(ctx, S.release());
    if (!n_items) return RH_OK;
    const size_t K = (size_t)n_samples, ni = (size_t)n_items, np = (size_t)n_probs, nb = zonal ? (size_t)n_zones : 1;   // nb: blocks per item
    const size_t acc_b = ni * 2 * (size_t)n * sizeof(double), key_b = ni * (size_t)n * sizeof(unsigned long long);
    const size_t hist_b = ni * RH_SAS_BANDS_MAX_PROBS * RH_SELECT_NBINS * sizeof(unsigned long long);
    const size_t row_b = K * ni * nb * np * sizeof(double), hdr_b = K * ni * nb * SAS_BANDS_HDR * sizeof(long long), pair_b = K * ni * nb * 2 * sizeof(long long);
    SHIPCHK(ctx, S.acc.alloc(acc_b));
    SHIPCHK(ctx, hipMemsetAsync(S.acc, 0, acc_b, ctx->stream));
    SHIPCHK(ctx, S.keys.alloc(key_b));
    SHIPCHK(ctx, hipMemsetAsync(S.keys, 0xff, key_b, ctx->stream));   // RH_SELECT_KEY_MASKED: every byte set
    SHIPCHK(ctx, S.hist.alloc(hist_b));
    SHIPCHK(ctx, hipMemsetAsync(S.hist, 0, hist_b, ctx->stream));
    SHIPCHK(ctx, S.words.alloc(SBW_WORDS * sizeof(long long)));
    SHIPCHK(ctx, hipMemsetAsync(S.words, 0, SBW_WORDS * sizeof(long long), ctx->stream));
    const std::vector<double> nans(K * ni * nb * np, std::nan(""));
    SHIPCHK(ctx, S.rows.alloc(row_b));
    SHIPCHK(ctx, hipMemcpyAsync(S.rows, nans.data(), row_b, hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, S.hdr.alloc(hdr_b));
    SHIPCHK(ctx, hipMemsetAsync(S.hdr, 0, hdr_b, ctx->stream));
    SHIPCHK(ctx, S.pair.alloc(pair_b));
    SHIPCHK(ctx, hipMemsetAsync(S.pair, 0xff, pair_b, ctx->stream));   // (-1, -1): every byte set
    if (mask) {
        SHIPCHK(ctx, S.mask.alloc((size_t)n));
        SHIPCHK(ctx, hipMemcpyAsync(S.mask, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    if (weights) {
        SHIPCHK(ctx, S.weight.alloc((size_t)n * sizeof(unsigned short)));
        SHIPCHK(ctx, hipMemcpyAsync(S.weight, weights, (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice, ctx->stream));
    }
    if (obs) {
        SHIPCHK(ctx, S.obs.alloc(ni * nb * K * sizeof(double)));
        SHIPCHK(ctx, hipMemcpyAsync(S.obs, obs, ni * nb * K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (!zonal) SHIPCHK(ctx, S.part.alloc(ni * select_obs_grid((long long)n) * 2 * sizeof(long long)));
    }
    if (zonal) {
        SHIPCHK(ctx, S.zone_off.alloc(zone_off.size() * sizeof(long long)));
        SHIPCHK(ctx, hipMemcpyAsync(S.zone_off, zone_off.data(), zone_off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        SHIPCHK(ctx, S.zone_cols.alloc((zone_cols.size() + 1) * sizeof(int)));   // (+ 1: never an empty allocation)
        SHIPCHK(ctx, hipMemcpyAsync(S.zone_cols, zone_cols.data(), zone_cols.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    long long *words = S.words.get();
    P.n_items = n_items;
    P.n_probs = n_probs;
    P.n = n;
    P.n_samples = n_samples;
    P.mask = S.mask.get();
    P.weight = S.weight.get();
    P.obs = S.obs.get();
    P.acc = S.acc.get();
    P.keys = S.keys.get();
    P.hist = S.hist.get();
    P.prefix = (unsigned long long *)(words + SBW_PREFIX);
    P.rank = words + SBW_RANK;
    P.m = words + SBW_M;
    P.nan = words + SBW_NAN;
    P.w = words + SBW_W;
    P.m_count = (unsigned *)(words + SBW_M_COUNT);
    P.nan_count = (unsigned *)(words + SBW_NAN_COUNT);
    P.obs_part = S.part.get();
    P.rows = S.rows.get();
    P.hdr = S.hdr.get();
    P.obs_pair = S.pair.get();
    SHIPCHK(ctx, S.cfg.alloc(sizeof(SasBandsDev)));
    SHIPCHK(ctx, hipMemcpyAsync(S.cfg, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and locals)
    if (obs) S.obs_host.assign(obs, obs + ni * nb * K);
    S.n_probs = n_probs;
    S.n_items = n_items;
    S.zones = zonal ? n_zones : 0;
    S.win.set(first_day, last_day, n_samples, accumulate);
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

int rh_sas_bands_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::bands, "rh_sas_bands_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_bands_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_bands_enqueue(ctx, day);
}

// What both band reads copy out, for the function `who` of bands that are on: the result of every window, `nb` blocks per item, the closed
// flags and the day count.  `lead` names the axes in front of a block's values in the size check's text.  Synchronises.
static int sas_bands_read(rh_sas_ctx *ctx, const char *who, size_t nb, const char *lead, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes,
                          int64_t *obs_pair, size_t pair_bytes, unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    const SasBands &S = ctx->bands;
    const size_t K = S.win.closed.size(), blocks = (size_t)S.n_items * nb, np = (size_t)S.n_probs;
    if (!rows || !hdr || !obs_pair || !closed || row_bytes != K * blocks * np * sizeof(double) || hdr_bytes != K * blocks * SAS_BANDS_HDR * sizeof(int64_t) ||
        pair_bytes != K * blocks * 2 * sizeof(int64_t) || closed_bytes != K)
        return sfail(ctx, RH_ERR_ARG, std::string(who) + ": size mismatch (" + lead + " x n_probs float64, " + lead + " x 3 and x 2 int64, n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(rows, S.rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(hdr, S.hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(obs_pair, S.pair, pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(S.win.closed.begin(), S.win.closed.end(), closed);
    if (days_recorded) *days_recorded = S.win.days;
    return rh_sas_sync(ctx);
}

int rh_sas_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair, size_t pair_bytes,
                      unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::bands, "rh_sas_bands_read")) return rc;
    if (ctx->bands.zones) return sfail(ctx, RH_ERR_STATE, "rh_sas_bands_read: the bands are configured per zone (read them with rh_sas_bands_zonal_read)");
    return sas_bands_read(ctx, "rh_sas_bands_read", 1, "n_samples x n_items", rows, row_bytes, hdr, hdr_bytes, obs_pair, pair_bytes, closed, closed_bytes,
                          days_recorded);
}

int rh_sas_bands_zonal_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair, size_t pair_bytes,
                            unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = sas_on(ctx, ctx->bands.on() && ctx->bands.zones != 0, "rh_sas_bands_zonal_read", "rh_sas_bands_configure_zonal")) return rc;
    return sas_bands_read(ctx, "rh_sas_bands_zonal_read", (size_t)ctx->bands.zones, "n_samples x n_items x n_zones", rows, row_bytes, hdr, hdr_bytes, obs_pair,
                          pair_bytes, closed, closed_bytes, days_recorded);
}

// ---- transport bands by age (include/roger_hip_sas.h; the kernels and the rule: rh_sas_age_bands.h) ----
// the next day of the count, behind what the stream holds so far: nothing unless it closes an open window; then per item the transpose
// into the ONE key plane and the selection of every age class (per zone: of the long zones and of the short ones, at most three launches),
// item after item in stream order
static int sas_age_bands_enqueue(rh_sas_ctx *ctx) {
    SasAgeBands &S = ctx->age_bands;
    const SasWindows::Tick now = S.win.tick();
    if (!now.launch) return RH_OK;   // (every item is LAST: launch == closes)
    const size_t np = (size_t)S.n_probs, nb = S.zones ? (size_t)S.zones : 1;   // nb: blocks per age class
    const SasAgeZones Z = S.dev_zones();
    size_t block = (size_t)now.k * (size_t)S.ages_total * nb;
    for (int j = 0; j < S.n_items; ++j) {
        const int W = S.width[j];
        rh_sas_age_launch_keys(ctx->stream, S.src[j], W, S.part_cols.get(), (long long)S.n_part, S.keys.get());
        rh_sas_age_launch_select(ctx->stream, W, (long long)S.n_part, S.keys.get(), S.wts_c.get(), S.zones ? &Z : nullptr, S.probs.get(), S.n_probs,
                                 S.rows + block * np, S.hdr + block * SAS_BANDS_HDR);
        block += (size_t)W * nb;
    }
    SHIPCHK(ctx, hipGetLastError());
    return RH_OK;
}

// ... of the window means: on every day of an open window, per item, k_sas_age_acc; on the closing day k_sas_age_keys_window into the
// observer's own key plane and the selection that the snapshot observer launches, item after item in stream order
static int sas_age_window_bands_enqueue(rh_sas_ctx *ctx, int64_t day) {
    SasAgeWindowBands &S = ctx->age_window_bands;
    const SasWindows::Tick now = S.win.tick();
    if (!now.launch) return RH_OK;
    const int64_t day_off = (day % ctx->cfg.forcing_days) * ctx->cfg.n_cells;
    const size_t np = (size_t)S.n_probs, nb = S.zones ? (size_t)S.zones : 1, npart = (size_t)S.n_part;
    const SasAgeZones Z = S.dev_zones();
    size_t block = (size_t)now.k * (size_t)S.ages_total * nb;
    for (int j = 0; j < S.n_items; ++j) {
        const int W = S.width[j];
        double *num = S.acc + S.acc_off[j], *den = num + npart * (size_t)W;
        rh_sas_age_launch_window(ctx->stream, S.src[j], W, S.part_cols.get(), (long long)S.n_part, S.wgt[j] ? S.wgt[j] + day_off : nullptr, now.first, now.closes,
                                 num, den, S.keys.get());
        if (now.closes)
            rh_sas_age_launch_select(ctx->stream, W, (long long)S.n_part, S.keys.get(), S.wts_c.get(), S.zones ? &Z : nullptr, S.probs.get(), S.n_probs,
                                     S.rows + block * np, S.hdr + block * SAS_BANDS_HDR);
        block += (size_t)W * nb;
    }
    SHIPCHK(ctx, hipGetLastError());
    return RH_OK;
}

// The participating set of both observers by age, on the host: the columns that take part -- (zone >= 0, with zones) & mask & weight > 0 --
// ascending, per zone in zone order by a stable counting sort (as sas_bands_configure does it); their weights at the same index; where
// each zone's run starts; the short zones' list, then the long zones'.  Refuses, for the function whose name opens `who`: a zone index out
// of range, no participating cell, and THE BOUND of a weight plane (per zone when zonal).
struct SasAgeSet {
    std::vector<int> part_cols;
    std::vector<unsigned short> wts_c;   // empty: no weight plane
    std::vector<long long> zone_off;     // per zone: [n_zones + 1] into both
    std::vector<int> zone_lists;
    int n_short = 0, n_long = 0;
};
static int sas_age_participants(rh_sas_ctx *ctx, const std::string &who, const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights,
                                SasAgeSet &P) {
    const int64_t n = ctx->cfg.n_cells;
    const bool zonal = n_zones != 0;
    const auto takes_part = [&](int64_t c) { return (!zonal || zone[c] >= 0) && (!mask || mask[c]) && (!weights || weights[c]); };
    if (zonal) {   // the zones' sizes, the bound of a weighted zone, then the stable counting sort over the participating columns
        std::vector<long long> &zone_off = P.zone_off;
        zone_off.assign((size_t)n_zones + 1, 0);
        for (int64_t c = 0; c < n; ++c) {
            if (zone[c] < -1 || zone[c] >= n_zones)
                return sfail(ctx, RH_ERR_ARG, who + "zone[" + std::to_string(c) + "] = " + std::to_string(zone[c]) + " (-1: outside every zone, else 0 ... " +
                                                  std::to_string(n_zones - 1) + ")");
            if (takes_part(c)) ++zone_off[(size_t)zone[c] + 1];
        }
        for (int z = 0; z < n_zones && weights; ++z)
            if (zone_off[(size_t)z + 1] > SAS_AGE_BANDS_MAX_WEIGHTED)
                return sfail(ctx, RH_ERR_ARG, who + "zone " + std::to_string(z) + " has " + std::to_string(zone_off[(size_t)z + 1]) +
                                                  " participating cells under a weight plane (at most " + std::to_string(SAS_AGE_BANDS_MAX_WEIGHTED) +
                                                  ": a uint32 LDS bin holds the weights of a zone's age class; without weights any size is exact)");
        for (int z = 0; z < n_zones; ++z)   // (short: 1 ... SAS_AGE_SHORT_ZONE cells; an empty zone is in neither list)
            if (zone_off[(size_t)z + 1] > 0 && zone_off[(size_t)z + 1] <= SAS_AGE_SHORT_ZONE) P.zone_lists.push_back(z);
        P.n_short = (int)P.zone_lists.size();
        for (int z = 0; z < n_zones; ++z)
            if (zone_off[(size_t)z + 1] > SAS_AGE_SHORT_ZONE) P.zone_lists.push_back(z);
        P.n_long = (int)P.zone_lists.size() - P.n_short;
        for (int z = 0; z < n_zones; ++z) zone_off[(size_t)z + 1] += zone_off[(size_t)z];
        P.part_cols.resize((size_t)zone_off[(size_t)n_zones]);
        if (weights) P.wts_c.resize(P.part_cols.size());
        std::vector<long long> at(zone_off.begin(), zone_off.end() - 1);
        for (int64_t c = 0; c < n; ++c)
            if (takes_part(c)) {
                const size_t i = (size_t)at[(size_t)zone[c]]++;
                P.part_cols[i] = (int)c;
                if (weights) P.wts_c[i] = weights[c];
            }
    } else {
        for (int64_t c = 0; c < n; ++c)
            if (takes_part(c)) {
                P.part_cols.push_back((int)c);
                if (weights) P.wts_c.push_back(weights[c]);
            }
    }
    const int64_t n_part = (int64_t)P.part_cols.size();
    if (!n_part) return sfail(ctx, RH_ERR_ARG, who + "no cell takes part (0 of " + std::to_string(n) + " cells have mask != 0 and a weight > 0)");
    if (!zonal && weights && n_part > SAS_AGE_BANDS_MAX_WEIGHTED)
        return sfail(ctx, RH_ERR_ARG, who + std::to_string(n_part) + " participating cells under a weight plane (at most " +
                                          std::to_string(SAS_AGE_BANDS_MAX_WEIGHTED) + ": a uint32 LDS bin holds an age class's weights; without weights any size is exact)");
    return RH_OK;
}

// The configure calls of the observer `obs` by age -- the snapshot's two and the window means' one -- for the function `name`; zone == nullptr,
// n_zones == 0: the plain form.  With zones the result gains the zone axis in front of the age axis, part_cols and wts_c are in zone order and
// the bound of a weight plane holds per zone (sas_age_participants).  The observers differ in the kinds they take -- the snapshot LAST
// without a weight, the window means BULK with a daily weight and MEAN -- and in the accumulators of the means; every other check and its
// wording is one.
template <class O>
static int sas_age_configure(rh_sas_ctx *ctx, O rh_sas_ctx::*obs, const char *name, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                             const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights, const int64_t *first_day,
                             const int64_t *last_day, int64_t n_samples) {
    constexpr bool MEANS = std::is_same<O, SasAgeWindowBands>::value;
    const std::string who = std::string(name) + ": ";
    const bool zonal = n_zones != 0;
    if (n_items < 0 || n_items > RH_SAS_AGE_BANDS_MAX_ITEMS)
        return sfail(ctx, RH_ERR_ARG, who + "n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SAS_AGE_BANDS_MAX_ITEMS) + ")");
    O &S = ctx->*obs;
    if (!n_items) {
        SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old result)
        SHIPCHK(ctx, S.release());
        return RH_OK;
    }
    const int64_t n = ctx->cfg.n_cells;
    O N;   // the new configuration: checked and allocated in full before the previous one is released
    if (!items || !probs || !first_day || !last_day || (zonal && !zone)) return sfail(ctx, RH_ERR_ARG, who + "null pointer");
    if (n_probs < 1 || n_probs > RH_SAS_BANDS_MAX_PROBS)
        return sfail(ctx, RH_ERR_ARG, who + "n_probs = " + std::to_string(n_probs) + " (1 ... " + std::to_string(RH_SAS_BANDS_MAX_PROBS) + ")");
    for (int q = 0; q < n_probs; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
            return sfail(ctx, RH_ERR_ARG, who + "probability " + std::to_string(q) + " is " + std::to_string(probs[q]) + " (within [0, 1])");
    int wmax = 0;
    for (int j = 0; j < n_items; ++j) {
        const int a = items[j].value, w = items[j].weight, kind = items[j].kind;
        if (a < 0 || a >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown array id " + std::to_string(a));
        const std::string name = std::string("array ") + SAS_NAMES[a];
        if (kind < RH_SAS_SCORES_BULK || kind > RH_SAS_SCORES_LAST)
            return sfail(ctx, RH_ERR_ARG, who + "kind " + std::to_string(kind) + " of " + name + " (0: BULK, 1: MEAN, 2: LAST)");
        if constexpr (MEANS) {
            if (kind == RH_SAS_SCORES_LAST)
                return sfail(ctx, RH_ERR_ARG, who + name + " is LAST (the band of a snapshot belongs to rh_sas_age_bands_configure; here BULK and MEAN)");
            if (w < -1 || w >= SA_COUNT) return sfail(ctx, RH_ERR_ARG, who + "unknown weight id " + std::to_string(w));
            if (int rc = sas_window_weight(ctx, who, name, w, kind)) return rc;
            N.wgt[j] = w >= 0 ? (const double *)ctx->arr[w].get() : nullptr;
        } else {
            if (kind != RH_SAS_SCORES_LAST)
                return sfail(ctx, RH_ERR_ARG, who + name + " is " + (kind == RH_SAS_SCORES_BULK ? "BULK" : "MEAN") +
                                                  " (only LAST is built: a window mean of an age-resolved value needs an (n, ages) accumulator per item)");
            if (w != -1) return sfail(ctx, RH_ERR_ARG, who + name + " has the weight id " + std::to_string(w) + " (LAST takes none: -1)");
        }
        for (int q = 0; q < j; ++q)
            if (items[q].value == a) return sfail(ctx, RH_ERR_ARG, who + name + " is given twice");
        if (SAS_KIND[a] == K_MASK) return sfail(ctx, RH_ERR_ARG, who + name + " is int32 (float64 arrays only)");
        if (SAS_KIND[a] == K_PARAM) return sfail(ctx, RH_ERR_ARG, who + name + " is a parameter block of the step (sas_params_* have no band)");
        if (SAS_KIND[a] == K_DAILY) return sfail(ctx, RH_ERR_ARG, who + name + " is a daily input of the step, not a result");
        if (SAS_KIND[a] == K_CELL) return sfail(ctx, RH_ERR_ARG, who + name + " has width 1 (it belongs to rh_sas_bands_configure)");
        if (!ctx->arr[a])
            return sfail(ctx, RH_ERR_STATE, who + name + " is not held by this context (age_statistics / keep_distributions / tracer)");
        N.src[j] = (const double *)ctx->arr[a].get();
        N.width[j] = (int)(ctx->elems[a] / n);
        N.ages_total += N.width[j];
        wmax = std::max(wmax, N.width[j]);
    }
    const int64_t block_b = std::max<int64_t>(n_probs * (int64_t)sizeof(double), SAS_BANDS_HDR * (int64_t)sizeof(int64_t));   // rows or hdr, the larger
    if (n_samples < 1 || n_samples > ((int64_t)1 << 31) / (N.ages_total * (zonal ? n_zones : 1) * block_b))
        return sfail(ctx, RH_ERR_ARG, who + "n_samples = " + std::to_string(n_samples) + " (at least one; rows of " +
                                          (zonal ? std::to_string(n_zones) + " zones x " : std::string()) + std::to_string(N.ages_total) + " age classes x " +
                                          std::to_string(n_probs) + " float64 and headers of 3 int64, each within 2 GiB)");
    if (int rc = sas_check_windows(ctx, who, first_day, last_day, n_samples)) return rc;
    SasAgeSet P;
    if (int rc = sas_age_participants(ctx, who, zone, n_zones, mask, weights, P)) return rc;
    N.n_part = (int64_t)P.part_cols.size();
    N.n_short = P.n_short;
    N.n_long = P.n_long;
    const size_t K = (size_t)n_samples, np = (size_t)n_probs, blocks = K * (size_t)N.ages_total * (zonal ? (size_t)n_zones : 1), npart = (size_t)N.n_part;
    const size_t row_b = blocks * np * sizeof(double), hdr_b = blocks * SAS_BANDS_HDR * sizeof(long long);
    const std::vector<double> nans(blocks * np, std::nan(""));
    SHIPCHK(ctx, N.keys.alloc((size_t)wmax * npart * sizeof(unsigned long long)));
    SHIPCHK(ctx, N.rows.alloc(row_b));
    SHIPCHK(ctx, hipMemcpyAsync(N.rows, nans.data(), row_b, hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, N.hdr.alloc(hdr_b));
    SHIPCHK(ctx, hipMemsetAsync(N.hdr, 0, hdr_b, ctx->stream));
    SHIPCHK(ctx, N.probs.alloc(np * sizeof(double)));
    SHIPCHK(ctx, hipMemcpyAsync(N.probs, probs, np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SHIPCHK(ctx, N.part_cols.alloc(npart * sizeof(int)));
    SHIPCHK(ctx, hipMemcpyAsync(N.part_cols, P.part_cols.data(), npart * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (weights) {
        SHIPCHK(ctx, N.wts_c.alloc(npart * sizeof(unsigned short)));
        SHIPCHK(ctx, hipMemcpyAsync(N.wts_c, P.wts_c.data(), npart * sizeof(unsigned short), hipMemcpyHostToDevice, ctx->stream));
    }
    if (zonal) {
        SHIPCHK(ctx, N.zone_off.alloc(P.zone_off.size() * sizeof(long long)));
        SHIPCHK(ctx, hipMemcpyAsync(N.zone_off, P.zone_off.data(), P.zone_off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        SHIPCHK(ctx, N.zone_lists.alloc(P.zone_lists.size() * sizeof(int)));   // (never empty: a cell takes part)
        SHIPCHK(ctx, hipMemcpyAsync(N.zone_lists, P.zone_lists.data(), P.zone_lists.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    if constexpr (MEANS) {   // num and den of every item, 16 B per participating column and age class, zero
        const size_t acc_b = 2 * npart * (size_t)N.ages_total * sizeof(double);
        SHIPCHK(ctx, N.acc.alloc(acc_b));
        SHIPCHK(ctx, hipMemsetAsync(N.acc, 0, acc_b, ctx->stream));
        for (int j = 1; j < n_items; ++j) N.acc_off[j] = N.acc_off[j - 1] + 2 * npart * (size_t)N.width[j - 1];
    }
    SHIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and locals; launches that write the old result)
    N.n_items = n_items;
    N.n_probs = n_probs;
    N.zones = zonal ? n_zones : 0;
    N.win.set(first_day, last_day, n_samples, MEANS);
    SHIPCHK(ctx, S.release());
    S = std::move(N);
    return RH_OK;
}

int rh_sas_age_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                               const unsigned char *mask, const uint16_t *weights, const int64_t *first_day, const int64_t *last_day,
                               int64_t n_samples) {
    if (!ctx) return RH_ERR_ARG;
    return sas_age_configure(ctx, &rh_sas_ctx::age_bands, "rh_sas_age_bands_configure", items, n_items, probs, n_probs, nullptr, 0, mask, weights, first_day,
                             last_day, n_samples);
}

// n_zones within 1 ... RH_SAS_AGE_BANDS_MAX_ZONES, for the configure call `name` that was given a zone map
static int sas_age_check_zones(rh_sas_ctx *ctx, const char *name, int n_zones) {
    if (n_zones < 1 || n_zones > RH_SAS_AGE_BANDS_MAX_ZONES)
        return sfail(ctx, RH_ERR_ARG, std::string(name) + ": n_zones = " + std::to_string(n_zones) + " (1 ... " + std::to_string(RH_SAS_AGE_BANDS_MAX_ZONES) + ")");
    return RH_OK;
}

int rh_sas_age_bands_configure_zonal(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                                     const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights, const int64_t *first_day,
                                     const int64_t *last_day, int64_t n_samples) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items)
        if (int rc = sas_age_check_zones(ctx, "rh_sas_age_bands_configure_zonal", n_zones)) return rc;
    return sas_age_configure(ctx, &rh_sas_ctx::age_bands, "rh_sas_age_bands_configure_zonal", items, n_items, probs, n_probs, zone, n_items ? n_zones : 0, mask,
                             weights, first_day, last_day, n_samples);
}

int rh_sas_age_bands_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::age_bands, "rh_sas_age_bands_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_age_bands_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_age_bands_enqueue(ctx);
}

int rh_sas_age_bands_row_elems(const rh_sas_ctx *ctx, int64_t *ages_total) {
    if (int rc = sas_on(const_cast<rh_sas_ctx *>(ctx), &rh_sas_ctx::age_bands, "rh_sas_age_bands_row_elems")) return rc;
    if (!ages_total) return RH_ERR_ARG;
    *ages_total = ctx->age_bands.ages_total;
    return RH_OK;
}

// What the reads of an observer by age `S` that is on copy out, for the function `who`: `nb` blocks per age class; `lead` names the axes in
// front of a block's values in the size check's text.  Synchronises.
static int sas_age_bands_read(rh_sas_ctx *ctx, const SasAgeBands &S, const char *who, size_t nb, const char *lead, double *rows, size_t row_bytes, int64_t *hdr,
                              size_t hdr_bytes, unsigned char *closed, size_t closed_bytes, int64_t *days_recorded) {
    const size_t K = S.win.closed.size(), blocks = K * (size_t)S.ages_total * nb;
    if (!rows || !hdr || !closed || row_bytes != blocks * (size_t)S.n_probs * sizeof(double) || hdr_bytes != blocks * SAS_BANDS_HDR * sizeof(int64_t) ||
        closed_bytes != K)
        return sfail(ctx, RH_ERR_ARG, std::string(who) + ": size mismatch (" + lead + " x n_probs float64, " + lead + " x 3 int64, n_samples bytes)");
    SHIPCHK(ctx, hipMemcpyAsync(rows, S.rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHIPCHK(ctx, hipMemcpyAsync(hdr, S.hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::copy(S.win.closed.begin(), S.win.closed.end(), closed);
    if (days_recorded) *days_recorded = S.win.days;
    return rh_sas_sync(ctx);
}

int rh_sas_age_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed, size_t closed_bytes,
                          int64_t *days_recorded) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::age_bands, "rh_sas_age_bands_read")) return rc;
    if (ctx->age_bands.zones)
        return sfail(ctx, RH_ERR_STATE, "rh_sas_age_bands_read: the bands by age are configured per zone (read them with rh_sas_age_bands_zonal_read)");
    return sas_age_bands_read(ctx, ctx->age_bands, "rh_sas_age_bands_read", 1, "n_samples x ages_total", rows, row_bytes, hdr, hdr_bytes, closed, closed_bytes,
                              days_recorded);
}

int rh_sas_age_bands_zonal_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed, size_t closed_bytes,
                                int64_t *days_recorded) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = sas_on(ctx, ctx->age_bands.on() && ctx->age_bands.zones != 0, "rh_sas_age_bands_zonal_read", "rh_sas_age_bands_configure_zonal")) return rc;
    return sas_age_bands_read(ctx, ctx->age_bands, "rh_sas_age_bands_zonal_read", (size_t)ctx->age_bands.zones, "n_samples x n_zones x ages_total", rows, row_bytes,
                              hdr, hdr_bytes, closed, closed_bytes, days_recorded);
}

// ---- window means of the bands by age (include/roger_hip_sas.h; the kernels and the rule: rh_sas_age_bands.h) ----
int rh_sas_age_window_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs, const int32_t *zone,
                                      int n_zones, const unsigned char *mask, const uint16_t *weights, const int64_t *first_day, const int64_t *last_day,
                                      int64_t n_samples) {
    const char *name = "rh_sas_age_window_bands_configure";
    if (!ctx) return RH_ERR_ARG;
    if (n_items && (zone || n_zones))   // (zone == NULL && n_zones == 0: the plain form)
        if (int rc = sas_age_check_zones(ctx, name, n_zones)) return rc;
    return sas_age_configure(ctx, &rh_sas_ctx::age_window_bands, name, items, n_items, probs, n_probs, zone, n_items ? n_zones : 0, mask, weights, first_day,
                             last_day, n_samples);
}

int rh_sas_age_window_bands_record(rh_sas_ctx *ctx, int64_t day) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::age_window_bands, "rh_sas_age_window_bands_record")) return rc;
    if (day < 0) return sfail(ctx, RH_ERR_ARG, "rh_sas_age_window_bands_record: day = " + std::to_string(day) + " (the row of the daily inputs, >= 0)");
    return sas_age_window_bands_enqueue(ctx, day);
}

int rh_sas_age_window_bands_row_elems(const rh_sas_ctx *ctx, int64_t *ages_total) {
    if (int rc = sas_on(const_cast<rh_sas_ctx *>(ctx), &rh_sas_ctx::age_window_bands, "rh_sas_age_window_bands_row_elems")) return rc;
    if (!ages_total) return RH_ERR_ARG;
    *ages_total = ctx->age_window_bands.ages_total;
    return RH_OK;
}

int rh_sas_age_window_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed, size_t closed_bytes,
                                 int64_t *days_recorded) {
    if (int rc = sas_on(ctx, &rh_sas_ctx::age_window_bands, "rh_sas_age_window_bands_read")) return rc;
    const SasAgeWindowBands &S = ctx->age_window_bands;
    return sas_age_bands_read(ctx, S, "rh_sas_age_window_bands_read", S.zones ? (size_t)S.zones : 1, S.zones ? "n_samples x n_zones x ages_total" : "n_samples x ages_total",
                              rows, row_bytes, hdr, hdr_bytes, closed, closed_bytes, days_recorded);
}
