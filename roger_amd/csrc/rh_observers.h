// rh_observers.h -- what follows every step: the output accumulators (rh_diag_*), the time series at observation columns
// (rh_points_*), the catchment totals (rh_totals_*), the zonal totals (rh_zonal_*), the scores against observed series
// (rh_scores_*), the event outputs (rh_events_*), the duration curves (rh_durations_*) and the ensemble bands (rh_bands_*).  Part of the
// one translation unit roger_hip.hip, behind rh_context.h.  ABI version 18: the last four are carried through a restart by plain copies
// (rh_scores_restore, rh_durations_restore, rh_events_state / _restore, rh_bands_state / _restore); no kernel is involved.  ABI version
// 19: rh_bands_configure_weighted / rh_bands_weight_sums, the likelihood-weighted bands (k_bands_select_w in rh_bands.h).  ABI version
// 20: rh_bands_observations / rh_bands_obs_read, where the observation falls in the ensemble (k_bands_obs* in rh_bands.h).
#pragma once
// The observers' planes changed (rh_diag_configure, rh_points_configure, rh_totals_configure, rh_zonal_configure, rh_scores_configure,
// rh_events_configure, rh_durations_configure, rh_bands_configure): what the fused kernel must leave in memory after every step, from
// the UNION of the planes of all eight -- the accumulators, the points, the totals, the zonal totals, the scores, the event outputs, the
// duration curves and the ensemble bands.
// A plane the sparse kernel leaves out -- a
// pure output, or one of the five the next lazy step derives itself, which the storage stage computes all the same -- gets its bit in
// DevState::keep: the KEEP variant stores it after all.  An X_m1 plane switches the lazy rotation off.  Synchronises.
static int observers_changed(rh_ctx *ctx) {
    unsigned long long keep[(RH_NPLANES + 63) / 64] = {};
    bool reads_sparse = false, reads_m1 = false;
    const std::vector<unsigned char> &left_out = pure_output_planes()[ctx->cfg.enable_lateral_flow ? 1 : 0];
    auto add = [&](const int *planes, int n) {
        for (int j = 0; j < n; ++j) {
            const int p = planes[j];
            if (left_out[p]) {
                reads_sparse = true;
                keep[p >> 6] |= 1ull << (p & 63);
            }
            const size_t len = std::strlen(PLANE_NAMES[p]);
            if (len > 3 && !std::strcmp(PLANE_NAMES[p] + len - 3, "_m1")) reads_m1 = true;
        }
    };
    add(ctx->diag_planes, ctx->diag_n);
    if (ctx->points_ncells) add(ctx->points_planes, ctx->points_nplanes);
    add(ctx->totals_planes, ctx->totals_nplanes);
    add(ctx->zonal_planes, ctx->zonal_nplanes);
    add(ctx->scores_planes, ctx->scores_nitems);
    add(ctx->events_planes, ctx->events_nitems);
    add(ctx->durations_planes, ctx->durations_nitems);
    add(ctx->bands_planes, ctx->bands_nitems);
    const int any = reads_sparse ? 1 : 0;
    HIPCHK(ctx, dev_put(ctx, &DevState::keep, keep));
    HIPCHK(ctx, dev_put(ctx, &DevState::keep_any, any));
    ctx->obs_reads_sparse = reads_sparse;
    ctx->obs_reads_m1 = reads_m1;
    materialise_m1(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are stack locals)
    return RH_OK;
}

// The observers behind the step that was just enqueued: the accumulators over all columns (grid: the fused launch's own, which has one
// workgroup more with RH_TAIL_PRE; 0: one workgroup per RH_BLOCK columns), then the points' row -- ONE workgroup (at most 8 192 values),
// then the totals' row -- a workgroup per RH_BLOCK columns for the partials and ONE that combines them -- then the zonal totals' row: a
// workgroup per RH_BLOCK columns and one per zone (rh_zonal.h) -- then the scores' moments over all columns, on the accumulators' grid
// (rh_scores.h) -- then the event outputs, on the same grid (rh_events.h) -- then the duration curves, on the same grid
// (rh_durations.h) -- then the ensemble bands: the keys on the same grid, and the six passes of the selection on at most
// RH_SELECT_MAX_GRID workgroups that stride over the tiles -- per zone instead ONE launch with a workgroup per (zone, item) and a
// one-thread launch for the row's header; with a weight plane the six passes of the weighted selection on bands_weighted_grid
// workgroups (rh_bands.h); and only while observations are set (rh_bands_observations) the pass that counts the keys below and equal to
// the observation's and a one-wavefront launch per item for the row's pairs -- per zone ONE launch.  after_fused: rh_control.h, k_diag.
static bool has_observers(const rh_ctx *ctx) {
    return ctx->diag_n || ctx->points_ncells || ctx->totals_nplanes || ctx->zonal_nplanes || ctx->scores_nitems || ctx->events_nitems ||
           ctx->durations_nitems || ctx->bands_nitems;
}
// What rh_*_restore may still replace: set by the observer's configure call, cleared by the first step behind it (launch_observers).
enum { RH_FRESH_SCORES = 1, RH_FRESH_EVENTS = 2, RH_FRESH_DURATIONS = 4, RH_FRESH_BANDS = 8 };
// the passes P... of the bands' selection, one launch each, in order: k_bands_select_w<P> with a weight plane, else k_bands_select<P>
template <bool WEIGHTED, int... P>
static void launch_bands_select(rh_ctx *ctx, dim3 grid, int after_fused, std::integer_sequence<int, P...>) {
    const auto launch = [&](void (*kernel)(Arena, DevState *, int)) {
        hipLaunchKernelGGL(kernel, grid, dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    };
    (launch(WEIGHTED ? k_bands_select_w<P> : k_bands_select<P>), ...);
}
static int launch_observers(rh_ctx *ctx, int after_fused, unsigned grid = 0) {
    const dim3 cells(grid ? grid : grid_for(ctx->n)), block(RH_BLOCK);
    ctx->obs_fresh = 0;   // (a step is enqueued: the observers' state is the run's from here on)
    if (ctx->diag_n) hipLaunchKernelGGL(k_diag, cells, block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    if (ctx->points_ncells) hipLaunchKernelGGL(k_points, dim3(1), block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    if (ctx->totals_nplanes) {
        hipLaunchKernelGGL(k_totals_tiles, dim3(grid_for(ctx->n)), block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
        hipLaunchKernelGGL(k_totals_finish, dim3(1), block, 0, ctx->stream, ctx->dev, after_fused);
    }
    if (ctx->zonal_nplanes) {
        hipLaunchKernelGGL(k_zonal_tiles, dim3(grid_for(ctx->n)), block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
        hipLaunchKernelGGL(k_zonal_finish, dim3(ctx->zonal_nzones), block, 0, ctx->stream, ctx->dev, after_fused);
    }
    if (ctx->scores_nitems) hipLaunchKernelGGL(k_scores, cells, block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    if (ctx->events_nitems) hipLaunchKernelGGL(k_events, cells, block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    if (ctx->durations_nitems) hipLaunchKernelGGL(k_durations, cells, block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
    if (ctx->bands_nitems) {
        hipLaunchKernelGGL(k_bands, cells, block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
        if (ctx->bands_nzones) {   // per zone: one launch for the selection, one thread for the row's header
            hipLaunchKernelGGL(k_bands_zonal, dim3(ctx->bands_nzones, ctx->bands_nitems), block, 0, ctx->stream, ctx->dev, (long long)ctx->n, after_fused);
            hipLaunchKernelGGL(k_bands_zonal_row, dim3(1), dim3(1), 0, ctx->stream, ctx->dev, after_fused);
        } else if (ctx->bands_weight_buf) {   // likelihood-weighted: the grid bounds what a workgroup's uint32 LDS bins can hold
            launch_bands_select<true>(ctx, dim3(bands_weighted_grid((long long)ctx->n)), after_fused, std::make_integer_sequence<int, RH_SELECT_PASSES>{});
        } else {
            launch_bands_select<false>(ctx, dim3(std::min<unsigned>(grid_for(ctx->n), RH_SELECT_MAX_GRID)), after_fused,
                                       std::make_integer_sequence<int, RH_SELECT_PASSES>{});
        }
        if (ctx->bands_obs_buf) {   // observations: the pairs {below, equal} behind the row, from the key planes the selection read
            if (ctx->bands_nzones) {
                hipLaunchKernelGGL(k_bands_obs_zonal, dim3(ctx->bands_nzones, ctx->bands_nitems), block, 0, ctx->stream, ctx->dev, (long long)ctx->n,
                                   after_fused);
            } else {
                const unsigned parts = select_obs_grid((long long)ctx->n);
                hipLaunchKernelGGL(k_bands_obs, dim3(parts, ctx->bands_nitems), block, 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
                hipLaunchKernelGGL(k_bands_obs_row, dim3(ctx->bands_nitems), dim3(64), 0, ctx->stream, ctx->dev, (int)parts, after_fused);
            }
        }
    }
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// ---- what the configure and the read calls below share; the rules of a ring itself are rh_host.h's ----
// `planes` into `out`: every id names a plane that this context holds, and a float64 one.  prefix: "<function>: "; tail: FLOAT64_IDS
// for the scores and the event outputs, whose texts end in it
static const char *const FLOAT64_IDS = " (plane ids must name float64 planes)";
static int check_planes(rh_ctx *ctx, const std::string &prefix, const int *planes, int n, int *out, const char *tail = nullptr) {
    for (int j = 0; j < n; ++j) {
        if (planes[j] < 0 || planes[j] >= ctx->planes_held)
            return fail(ctx, RH_ERR_ARG, prefix + "plane id " + std::to_string(planes[j]) + " is not held by this context" + (tail ? tail : ""));
        if (PLANE_IS_INT[planes[j]])
            return fail(ctx, RH_ERR_ARG, prefix + "plane " + PLANE_NAMES[planes[j]] + " is int32" + (tail ? tail : " (float64 planes only)"));
        out[j] = planes[j];
    }
    return RH_OK;
}
static int check_capacity(rh_ctx *ctx, const std::string &prefix, int64_t capacity) {
    const std::string why = ring_capacity_refusal(prefix, capacity, (int64_t)1 << 40);
    return why.empty() ? RH_OK : fail(ctx, RH_ERR_ARG, why);
}
// the rows recorded into `ring` so far (DevState::X_rows), for the function `who`; RH_ERR_STATE unless `configure` has switched it on
static int ring_rows(rh_ctx *ctx, const char *who, const ObsRing &ring, const char *configure, long long DevState::*member, long long *rows) {
    if (!ring.cap) return fail(ctx, RH_ERR_STATE, std::string(who) + ": " + configure + " has not been called");
    HIPCHK(ctx, hipMemcpyAsync(rows, &(ctx->dev.get()->*member), sizeof(*rows), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
// the rows of an accepted range, nv values each, and their headers (nh int64 each) to the host.  Synchronises.
static int ring_download(rh_ctx *ctx, const ObsRing &ring, size_t nv, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t nh = 3) {
    const int rc = ring_pieces(first_row, n_rows, ring.cap, [&](int64_t done, int64_t slot, int64_t m) -> int {
        HIPCHK(ctx, hipMemcpyAsync(values + (size_t)done * nv, ring.buf + (size_t)slot * nv, (size_t)m * nv * sizeof(double), hipMemcpyDeviceToHost,
                                   ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(hdr + nh * done, ring.hdr_buf + nh * slot, (size_t)m * nh * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        return RH_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

// the accumulators' buffers, cleared (rh_diag_configure)
static int diag_alloc(rh_ctx *ctx, int nv, int n_slots) {
    const size_t bytes = (size_t)n_slots * nv * ctx->n * sizeof(double), hdr = (size_t)n_slots * 3 * sizeof(long long);
    HIPCHK(ctx, ctx->diag_buf.alloc(bytes));
    HIPCHK(ctx, hipMemsetAsync(ctx->diag_buf, 0, bytes, ctx->stream));
    HIPCHK(ctx, ctx->diag_steps_buf.alloc(hdr));
    HIPCHK(ctx, hipMemsetAsync(ctx->diag_steps_buf, 0xff, hdr, ctx->stream));   // -1: never touched
    return RH_OK;
}
int rh_diag_configure(rh_ctx *ctx, const int *rate_planes, int n_rate, const int *collect_planes, int n_collect, int n_slots) {
    if (!ctx) return RH_ERR_ARG;
    if (n_rate < 0 || n_collect < 0 || n_rate + n_collect > 32 || n_slots < 1 || (n_rate && !rate_planes) || (n_collect && !collect_planes))
        return fail(ctx, RH_ERR_ARG, "rh_diag_configure: bad counts (n_rate + n_collect <= 32, n_slots >= 1)");
    int planes[32];
    for (int j = 0; j < n_rate + n_collect; ++j) {
        planes[j] = j < n_rate ? rate_planes[j] : collect_planes[j - n_rate];
        if (planes[j] < 0 || planes[j] >= ctx->planes_held || PLANE_IS_INT[planes[j]])
            return fail(ctx, RH_ERR_ARG, "rh_diag_configure: plane ids must name float64 planes");
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that accumulate into the old buffers)
    HIPCHK(ctx, ctx->diag_buf.release());
    HIPCHK(ctx, ctx->diag_steps_buf.release());
    ctx->diag_n = 0;
    const int nv = n_rate + n_collect;
    if (int rc = nv ? diag_alloc(ctx, nv, n_slots) : RH_OK) {   // refused: the accumulators are off, no later step launches k_diag
        const std::string why = ctx->err;
        (void)rh_diag_configure(ctx, nullptr, 0, nullptr, 0, 1);
        return fail(ctx, rc, why);
    }
    // only now the counts: an accumulated plane must be in memory after every step (the keep bits and the rotation, together with the
    // points' planes: observers_changed)
    ctx->diag_n = nv;
    ctx->diag_slots = n_slots;
    std::memcpy(ctx->diag_planes, planes, sizeof(int) * (size_t)nv);
    if (ctx->diag_interval <= 0) ctx->diag_interval = 86400;
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_steps, *ctx->diag_steps_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_interval, ctx->diag_interval));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag, *ctx->diag_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_rate, n_rate));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_collect, n_collect));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_slots, n_slots));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_planes, planes));
    return observers_changed(ctx);   // synchronises: the sources above are stack locals
}
static int diag_check(rh_ctx *ctx, int j, int slot) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->diag_n) return fail(ctx, RH_ERR_STATE, "rh_diag_configure has not been called");
    if (j < 0 || j >= ctx->diag_n || slot < 0 || slot >= ctx->diag_slots) return fail(ctx, RH_ERR_ARG, "rh_diag: variable or slot out of range");
    return RH_OK;
}
int rh_diag_download(rh_ctx *ctx, int j, int slot, double *host, size_t bytes) {
    const int rc = diag_check(ctx, j, slot);
    if (rc) return rc;
    if (!host || bytes != (size_t)ctx->n * sizeof(double)) return fail(ctx, RH_ERR_ARG, "rh_diag_download: size mismatch");
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->diag_buf + ((size_t)slot * ctx->diag_n + j) * ctx->n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_diag_upload(rh_ctx *ctx, int j, int slot, const double *host, size_t bytes) {
    const int rc = diag_check(ctx, j, slot);
    if (rc) return rc;
    if (!host || bytes != (size_t)ctx->n * sizeof(double)) return fail(ctx, RH_ERR_ARG, "rh_diag_upload: size mismatch");
    HIPCHK(ctx, hipMemcpyAsync(ctx->diag_buf + ((size_t)slot * ctx->diag_n + j) * ctx->n, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_diag_set_slot_state(rh_ctx *ctx, int slot, int64_t steps, int64_t t_start, int64_t t_end) {
    const int rc = diag_check(ctx, 0, slot);
    if (rc) return rc;
    const long long v[3] = {(long long)steps, (long long)t_start, (long long)t_end};
    HIPCHK(ctx, hipMemcpyAsync(ctx->diag_steps_buf + 3 * slot, v, sizeof(v), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_diag_steps(rh_ctx *ctx, int slot, int64_t *steps) {
    const int rc = diag_check(ctx, 0, slot);
    if (rc) return rc;
    if (!steps) return fail(ctx, RH_ERR_ARG, "rh_diag_steps: null pointer");
    long long v = 0;
    HIPCHK(ctx, hipMemcpyAsync(&v, ctx->diag_steps_buf + 3 * slot, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *steps = (int64_t)(v < 0 ? 0 : v);
    return RH_OK;
}
int rh_diag_set_interval(rh_ctx *ctx, int64_t seconds) {
    if (!ctx) return RH_ERR_ARG;
    if (seconds != 86400 && seconds != 3600 && seconds != 600)
        return fail(ctx, RH_ERR_ARG, "rh_diag_set_interval: the output interval is a day, an hour or ten minutes (the step classes)");
    ctx->diag_interval = seconds;
    if (ctx->diag_n) {
        HIPCHK(ctx, dev_put(ctx, &DevState::diag_interval, ctx->diag_interval));
        HIPCHK(ctx, hipMemsetAsync(ctx->diag_steps_buf, 0xff, (size_t)ctx->diag_slots * 3 * sizeof(long long), ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RH_OK;
}
int rh_diag_slot_times(rh_ctx *ctx, int slot, int64_t *t_start, int64_t *t_end) {
    const int rc = diag_check(ctx, 0, slot);
    if (rc) return rc;
    if (!t_start || !t_end) return fail(ctx, RH_ERR_ARG, "rh_diag_slot_times: null pointer");
    long long v[3] = {0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(v, ctx->diag_steps_buf + 3 * slot, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *t_start = (int64_t)v[1];
    *t_end = (int64_t)v[2];
    return RH_OK;
}
void *rh_diag_device_ptr(rh_ctx *ctx, int j, int slot) {
    if (diag_check(ctx, j, slot)) return nullptr;
    return ctx->diag_buf + ((size_t)slot * ctx->diag_n + j) * ctx->n;
}

// ---- time series at observation columns (include/roger_hip.h) ----
int rh_points_configure(rh_ctx *ctx, const int64_t *cells, int n_cells, const int *planes, int n_planes, int64_t capacity) {
    if (!ctx) return RH_ERR_ARG;
    if (n_cells < 0 || n_cells > RH_POINTS_MAX_CELLS)
        return fail(ctx, RH_ERR_ARG, "rh_points_configure: n_cells = " + std::to_string(n_cells) + " (0 ... " + std::to_string(RH_POINTS_MAX_CELLS) + ")");
    if (n_planes < 0 || n_planes > RH_POINTS_MAX_PLANES)
        return fail(ctx, RH_ERR_ARG, "rh_points_configure: n_planes = " + std::to_string(n_planes) + " (0 ... " + std::to_string(RH_POINTS_MAX_PLANES) + ")");
    const bool off = n_cells == 0 || n_planes == 0;
    long long cell_list[RH_POINTS_MAX_CELLS] = {};
    int plane_list[RH_POINTS_MAX_PLANES] = {};
    if (!off) {
        if (!cells || !planes) return fail(ctx, RH_ERR_ARG, "rh_points_configure: null pointer");
        if (int rc = check_capacity(ctx, "rh_points_configure: ", capacity)) return rc;
        if (int rc = check_planes(ctx, "rh_points_configure: ", planes, n_planes, plane_list)) return rc;
        std::vector<int64_t> seen(cells, cells + n_cells);
        std::sort(seen.begin(), seen.end());
        for (int c = 0; c < n_cells; ++c) {
            if (cells[c] < 0 || cells[c] >= ctx->n)
                return fail(ctx, RH_ERR_ARG, "rh_points_configure: cell " + std::to_string(cells[c]) + " is outside [0, " + std::to_string(ctx->n) + ")");
            if (c && seen[c] == seen[c - 1]) return fail(ctx, RH_ERR_ARG, "rh_points_configure: cell " + std::to_string(seen[c]) + " is given twice");
            cell_list[c] = (long long)cells[c];
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    HIPCHK(ctx, ctx->points.release());
    ctx->points_ncells = ctx->points_nplanes = 0;
    if (!off) {
        const size_t nv = (size_t)n_cells * n_planes;
        HIPCHK(ctx, ctx->points.buf.alloc((size_t)capacity * nv * sizeof(double)));
        HIPCHK(ctx, ctx->points.hdr_buf.alloc((size_t)capacity * 3 * sizeof(long long)));
        ctx->points_ncells = n_cells;
        ctx->points_nplanes = n_planes;
        ctx->points.cap = capacity;
        std::memcpy(ctx->points_planes, plane_list, sizeof(plane_list));
    }
    const long long zero = 0, cap = (long long)ctx->points.cap;
    HIPCHK(ctx, dev_put(ctx, &DevState::points, *ctx->points.buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_hdr, *ctx->points.hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_rows, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_ncells, ctx->points_ncells));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_nplanes, ctx->points_nplanes));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_cells, cell_list));
    return observers_changed(ctx);   // synchronises: the sources above are stack locals
}
int rh_points_count(rh_ctx *ctx, int64_t *rows_total) {
    if (!ctx) return RH_ERR_ARG;
    if (!rows_total) return fail(ctx, RH_ERR_ARG, "rh_points_count: null pointer");
    long long rows = 0;
    if (int rc = ring_rows(ctx, "rh_points_count", ctx->points, "rh_points_configure", &DevState::points_rows, &rows)) return rc;
    *rows_total = (int64_t)rows;
    return RH_OK;
}
int rh_points_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_points_read", ctx->points, "rh_points_configure", &DevState::points_rows, &total)) return rc;
    const size_t nv = (size_t)ctx->points_ncells * ctx->points_nplanes;
    const std::string why = ring_range_refusal("rh_points_read", first_row, n_rows, total, ctx->points.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!hdr || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_points_read: size mismatch (n_rows x n_planes x n_cells float64)");
    return ring_download(ctx, ctx->points, nv, first_row, n_rows, hdr, values);
}

// ---- catchment totals (include/roger_hip.h) ----
int rh_totals_configure(rh_ctx *ctx, const unsigned char *mask, const int *planes, int n_planes, int64_t capacity) {
    if (!ctx) return RH_ERR_ARG;
    if (n_planes < 0 || n_planes > RH_POINTS_MAX_PLANES)
        return fail(ctx, RH_ERR_ARG, "rh_totals_configure: n_planes = " + std::to_string(n_planes) + " (0 ... " + std::to_string(RH_POINTS_MAX_PLANES) + ")");
    const bool off = n_planes == 0;
    int plane_list[RH_POINTS_MAX_PLANES] = {};
    int64_t ncells = ctx->n;
    if (!off) {
        if (!planes) return fail(ctx, RH_ERR_ARG, "rh_totals_configure: null pointer");
        if (int rc = check_capacity(ctx, "rh_totals_configure: ", capacity)) return rc;
        if (int rc = check_planes(ctx, "rh_totals_configure: ", planes, n_planes, plane_list)) return rc;
        if (mask) {
            ncells = 0;
            for (int64_t i = 0; i < ctx->n; ++i) ncells += mask[i] != 0;
            if (!ncells) return fail(ctx, RH_ERR_ARG, "rh_totals_configure: the mask holds no column (0 of " + std::to_string(ctx->n) + " bytes set)");
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    HIPCHK(ctx, ctx->totals.release());
    HIPCHK(ctx, ctx->totals_part_buf.release());
    HIPCHK(ctx, ctx->totals_mask_buf.release());
    ctx->totals_nplanes = 0;
    ctx->totals_ncells = 0;
    const int ntiles = (int)grid_for(ctx->n);
    if (!off) {
        HIPCHK(ctx, ctx->totals.buf.alloc((size_t)capacity * n_planes * 3 * sizeof(double)));
        HIPCHK(ctx, ctx->totals.hdr_buf.alloc((size_t)capacity * 3 * sizeof(long long)));
        HIPCHK(ctx, ctx->totals_part_buf.alloc((size_t)n_planes * 3 * ntiles * sizeof(double)));
        if (mask) {
            HIPCHK(ctx, ctx->totals_mask_buf.alloc((size_t)ctx->n));
            HIPCHK(ctx, hipMemcpyAsync(ctx->totals_mask_buf, mask, (size_t)ctx->n, hipMemcpyHostToDevice, ctx->stream));
        }
        ctx->totals_nplanes = n_planes;
        ctx->totals.cap = capacity;
        ctx->totals_ncells = ncells;
    }
    std::memcpy(ctx->totals_planes, plane_list, sizeof(plane_list));
    const long long zero = 0, cap = (long long)ctx->totals.cap;
    const unsigned char *const mask_dev = ctx->totals_mask_buf;
    HIPCHK(ctx, dev_put(ctx, &DevState::totals, *ctx->totals.buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_hdr, *ctx->totals.hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_part, *ctx->totals_part_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_mask, mask_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_rows, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_nplanes, ctx->totals_nplanes));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_ntiles, ntiles));
    HIPCHK(ctx, dev_put(ctx, &DevState::totals_planes, plane_list));
    return observers_changed(ctx);   // synchronises: the sources above are stack locals (and the caller's mask)
}
int rh_totals_count(rh_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (!ctx) return RH_ERR_ARG;
    if (!rows_total || !ncells) return fail(ctx, RH_ERR_ARG, "rh_totals_count: null pointer");
    long long rows = 0;
    if (int rc = ring_rows(ctx, "rh_totals_count", ctx->totals, "rh_totals_configure", &DevState::totals_rows, &rows)) return rc;
    *rows_total = (int64_t)rows;
    *ncells = ctx->totals_ncells;
    return RH_OK;
}
int rh_totals_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_totals_read", ctx->totals, "rh_totals_configure", &DevState::totals_rows, &total)) return rc;
    const size_t nv = (size_t)ctx->totals_nplanes * 3;
    const std::string why = ring_range_refusal("rh_totals_read", first_row, n_rows, total, ctx->totals.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!hdr || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_totals_read: size mismatch (n_rows x n_planes x 3 float64)");
    return ring_download(ctx, ctx->totals, nv, first_row, n_rows, hdr, values);
}

// ---- zonal totals (include/roger_hip.h; the kernels and the order: rh_zonal.h) ----
// The index over a zone map: per tile of RH_BLOCK columns the ascending zones present -- the position of a (tile, zone) pair in that list
// is its slot -- and per (zone, accumulator) the slots in increasing tile order.  buf: zone[n], tile_ptr[ntiles + 1], tile_zone[S],
// acc_ptr[Z * RH_BLOCK + 1], acc_slot[S]; returns S.
static int64_t zonal_index(const int32_t *zone, int64_t n, int n_zones, std::vector<int> &buf, int64_t off[5]) {
    const int64_t ntiles = (int64_t)grid_for(n);
    std::vector<int> tile_ptr(ntiles + 1, 0), tile_zone;
    std::vector<int> present;
    for (int64_t b = 0; b < ntiles; ++b) {
        present.clear();
        for (int64_t i = b * RH_BLOCK; i < std::min<int64_t>(n, (b + 1) * RH_BLOCK); ++i)
            if (zone[i] >= 0) present.push_back(zone[i]);
        std::sort(present.begin(), present.end());
        present.erase(std::unique(present.begin(), present.end()), present.end());
        tile_zone.insert(tile_zone.end(), present.begin(), present.end());
        tile_ptr[b + 1] = (int)tile_zone.size();
    }
    const int64_t S = (int64_t)tile_zone.size();
    std::vector<int> acc_ptr((size_t)n_zones * RH_BLOCK + 1, 0), acc_slot(S);
    for (int64_t b = 0; b < ntiles; ++b)
        for (int s = tile_ptr[b]; s < tile_ptr[b + 1]; ++s) ++acc_ptr[(size_t)tile_zone[s] * RH_BLOCK + b % RH_BLOCK + 1];
    for (size_t k = 1; k < acc_ptr.size(); ++k) acc_ptr[k] += acc_ptr[k - 1];
    std::vector<int> fill(acc_ptr.begin(), acc_ptr.end() - 1);
    for (int64_t b = 0; b < ntiles; ++b)   // increasing tile order within every (zone, accumulator) list
        for (int s = tile_ptr[b]; s < tile_ptr[b + 1]; ++s) acc_slot[fill[(size_t)tile_zone[s] * RH_BLOCK + b % RH_BLOCK]++] = s;
    buf.clear();
    off[0] = 0;
    buf.insert(buf.end(), zone, zone + n);
    off[1] = (int64_t)buf.size();
    buf.insert(buf.end(), tile_ptr.begin(), tile_ptr.end());
    off[2] = (int64_t)buf.size();
    buf.insert(buf.end(), tile_zone.begin(), tile_zone.end());
    off[3] = (int64_t)buf.size();
    buf.insert(buf.end(), acc_ptr.begin(), acc_ptr.end());
    off[4] = (int64_t)buf.size();
    buf.insert(buf.end(), acc_slot.begin(), acc_slot.end());
    return S;
}
int rh_zonal_configure(rh_ctx *ctx, const int32_t *zone, int n_zones, const int *planes, int n_planes, int64_t capacity) {
    if (!ctx) return RH_ERR_ARG;
    if (n_planes < 0 || n_planes > RH_POINTS_MAX_PLANES)
        return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: n_planes = " + std::to_string(n_planes) + " (0 ... " + std::to_string(RH_POINTS_MAX_PLANES) + ")");
    const bool off = n_planes == 0;
    int plane_list[RH_POINTS_MAX_PLANES] = {};
    std::vector<int64_t> ncells;
    std::vector<int> index;
    int64_t at[5] = {}, S = 0;
    if (!off) {
        if (!planes || !zone) return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: null pointer");
        if (n_zones < 1 || n_zones > RH_ZONAL_MAX_ZONES)
            return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: n_zones = " + std::to_string(n_zones) + " (1 ... " + std::to_string(RH_ZONAL_MAX_ZONES) + ")");
        if (int rc = check_capacity(ctx, "rh_zonal_configure: ", capacity)) return rc;
        if (ctx->n >= (int64_t)1 << 31) return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: " + std::to_string(ctx->n) + " columns (the index holds int32 slots)");
        if (int rc = check_planes(ctx, "rh_zonal_configure: ", planes, n_planes, plane_list)) return rc;
        ncells.assign((size_t)n_zones, 0);
        int64_t inside = 0;
        for (int64_t i = 0; i < ctx->n; ++i) {
            if (zone[i] < -1 || zone[i] >= n_zones)
                return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: zone id " + std::to_string(zone[i]) + " of column " + std::to_string(i) +
                                             " (-1: outside, else 0 ... " + std::to_string(n_zones - 1) + ")");
            if (zone[i] >= 0) {
                ++ncells[(size_t)zone[i]];
                ++inside;
            }
        }
        if (!inside) return fail(ctx, RH_ERR_ARG, "rh_zonal_configure: the map holds no column in any zone (0 of " + std::to_string(ctx->n) + " columns)");
        S = zonal_index(zone, ctx->n, n_zones, index, at);
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    HIPCHK(ctx, ctx->zonal.release());
    HIPCHK(ctx, ctx->zonal_part_buf.release());
    HIPCHK(ctx, ctx->zonal_index_buf.release());
    ctx->zonal_nplanes = ctx->zonal_nzones = 0;
    ctx->zonal_ncells.clear();
    if (!off) {
        HIPCHK(ctx, ctx->zonal.buf.alloc((size_t)capacity * n_zones * n_planes * 3 * sizeof(double)));
        HIPCHK(ctx, ctx->zonal.hdr_buf.alloc((size_t)capacity * 3 * sizeof(long long)));
        HIPCHK(ctx, ctx->zonal_part_buf.alloc((size_t)S * n_planes * 3 * sizeof(double)));
        HIPCHK(ctx, ctx->zonal_index_buf.alloc(index.size() * sizeof(int)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->zonal_index_buf, index.data(), index.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ctx->zonal_nplanes = n_planes;
        ctx->zonal_nzones = n_zones;
        ctx->zonal.cap = capacity;
        ctx->zonal_ncells = ncells;
    }
    std::memcpy(ctx->zonal_planes, plane_list, sizeof(plane_list));
    const long long zero = 0, cap = (long long)ctx->zonal.cap;
    const int *const base = ctx->zonal_index_buf;
    const int *const part[5] = {base, base ? base + at[1] : nullptr, base ? base + at[2] : nullptr, base ? base + at[3] : nullptr,
                                base ? base + at[4] : nullptr};
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal, *ctx->zonal.buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_hdr, *ctx->zonal.hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_part, *ctx->zonal_part_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_zone, part[0]));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_tile_ptr, part[1]));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_tile_zone, part[2]));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_acc_ptr, part[3]));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_acc_slot, part[4]));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_rows, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_nplanes, ctx->zonal_nplanes));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_nzones, ctx->zonal_nzones));
    HIPCHK(ctx, dev_put(ctx, &DevState::zonal_planes, plane_list));
    return observers_changed(ctx);   // synchronises: the sources above are locals
}
int rh_zonal_count(rh_ctx *ctx, int64_t *rows_total, int64_t *ncells) {
    if (!ctx) return RH_ERR_ARG;
    if (!rows_total || !ncells) return fail(ctx, RH_ERR_ARG, "rh_zonal_count: null pointer");
    long long rows = 0;
    if (int rc = ring_rows(ctx, "rh_zonal_count", ctx->zonal, "rh_zonal_configure", &DevState::zonal_rows, &rows)) return rc;
    *rows_total = (int64_t)rows;
    std::copy(ctx->zonal_ncells.begin(), ctx->zonal_ncells.end(), ncells);
    return RH_OK;
}
int rh_zonal_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_zonal_read", ctx->zonal, "rh_zonal_configure", &DevState::zonal_rows, &total)) return rc;
    const size_t nv = (size_t)ctx->zonal_nzones * ctx->zonal_nplanes * 3;
    const std::string why = ring_range_refusal("rh_zonal_read", first_row, n_rows, total, ctx->zonal.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!hdr || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_zonal_read: size mismatch (n_rows x n_zones x n_planes x 3 float64)");
    return ring_download(ctx, ctx->zonal, nv, first_row, n_rows, hdr, values);
}

// ---- scores against observed series (include/roger_hip.h; the kernel and the rule: rh_scores.h) ----
static int scores_alloc(rh_ctx *ctx, int n_items, const double *obs, int n_series, int64_t n_intervals, const int32_t *series) {
    const size_t mb = (size_t)n_items * 5 * ctx->n * sizeof(double), ob = (size_t)n_items * n_series * n_intervals * sizeof(double);
    HIPCHK(ctx, ctx->scores_buf.alloc(mb));
    HIPCHK(ctx, hipMemsetAsync(ctx->scores_buf, 0, mb, ctx->stream));
    HIPCHK(ctx, ctx->scores_obs_buf.alloc(ob));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scores_obs_buf, obs, ob, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, ctx->scores_closed_buf.alloc((size_t)n_intervals));
    HIPCHK(ctx, hipMemsetAsync(ctx->scores_closed_buf, 0, (size_t)n_intervals, ctx->stream));
    if (series) {
        HIPCHK(ctx, ctx->scores_series_buf.alloc((size_t)ctx->n * sizeof(int)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->scores_series_buf, series, (size_t)ctx->n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    return RH_OK;
}
int rh_scores_configure(rh_ctx *ctx, const int *planes, const int *kinds, int n_items, const double *obs, int n_series, int64_t n_intervals,
                        const int32_t *series, int64_t interval_seconds, int64_t t_first) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_SCORES_MAX_ITEMS)
        return fail(ctx, RH_ERR_ARG, "rh_scores_configure: n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_SCORES_MAX_ITEMS) + ")");
    const bool off = n_items == 0;
    int plane_list[RH_SCORES_MAX_ITEMS] = {}, kind_list[RH_SCORES_MAX_ITEMS] = {};
    if (!off) {
        if (!planes || !kinds || !obs) return fail(ctx, RH_ERR_ARG, "rh_scores_configure: null pointer");
        if (n_series < 1 || n_series > RH_SCORES_MAX_SERIES)
            return fail(ctx, RH_ERR_ARG, "rh_scores_configure: n_series = " + std::to_string(n_series) + " (1 ... " + std::to_string(RH_SCORES_MAX_SERIES) + ")");
        if (n_intervals < 1 || n_intervals > (int64_t)1 << 31)
            return fail(ctx, RH_ERR_ARG, "rh_scores_configure: n_intervals = " + std::to_string(n_intervals) + " (at least one, at most 2^31)");
        if (interval_seconds != 86400 && interval_seconds != 3600 && interval_seconds != 600)
            return fail(ctx, RH_ERR_ARG, "rh_scores_configure: interval_seconds = " + std::to_string(interval_seconds) +
                                         " (the observation interval is a day, an hour or ten minutes: the step classes)");
        if (t_first < 0 || t_first % interval_seconds)
            return fail(ctx, RH_ERR_ARG, "rh_scores_configure: t_first = " + std::to_string(t_first) + " is not a multiple of the interval (" +
                                         std::to_string(interval_seconds) + " s)");
        for (int j = 0; j < n_items; ++j) {   // (item by item: an item's plane is refused before its kind, both before the next item)
            if (int rc = check_planes(ctx, "rh_scores_configure: ", planes + j, 1, plane_list + j, FLOAT64_IDS)) return rc;
            if (kinds[j] != RH_SCORES_SUM && kinds[j] != RH_SCORES_LAST)
                return fail(ctx, RH_ERR_ARG, "rh_scores_configure: kind " + std::to_string(kinds[j]) + " of item " + std::to_string(j) + " (0: SUM, 1: LAST)");
            kind_list[j] = kinds[j];
        }
        if (series)
            for (int64_t i = 0; i < ctx->n; ++i)
                if (series[i] >= n_series)
                    return fail(ctx, RH_ERR_ARG, "rh_scores_configure: series " + std::to_string(series[i]) + " of column " + std::to_string(i) +
                                                 " (< 0: not scored, else 0 ... " + std::to_string(n_series - 1) + ")");
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that add into the old moments; the clock below)
    if (!off) {
        long long now = 0;
        HIPCHK(ctx, hipMemcpyAsync(&now, &ctx->dev->S.time, sizeof(now), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (t_first < now)
            return fail(ctx, RH_ERR_ARG, "rh_scores_configure: t_first = " + std::to_string(t_first) + " lies behind the context's clock (" +
                                         std::to_string(now) + " s): pass the next interval boundary");
    }
    HIPCHK(ctx, ctx->scores_buf.release());
    HIPCHK(ctx, ctx->scores_obs_buf.release());
    HIPCHK(ctx, ctx->scores_series_buf.release());
    HIPCHK(ctx, ctx->scores_closed_buf.release());
    ctx->scores_nitems = 0;
    ctx->scores_nintervals = 0;
    ctx->obs_fresh &= ~(unsigned)RH_FRESH_SCORES;
    if (int rc = off ? RH_OK : scores_alloc(ctx, n_items, obs, n_series, n_intervals, series)) {   // refused: the scores are off
        const std::string why = ctx->err;
        (void)rh_scores_configure(ctx, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0);
        return fail(ctx, rc, why);
    }
    if (!off) {
        ctx->scores_nitems = n_items;
        ctx->scores_nintervals = n_intervals;
        ctx->scores_interval = interval_seconds;
        ctx->obs_fresh |= RH_FRESH_SCORES;
    }
    std::memcpy(ctx->scores_planes, plane_list, sizeof(plane_list));
    const long long iv = off ? 86400 : (long long)interval_seconds, tf = off ? 0 : (long long)t_first, nk = (long long)ctx->scores_nintervals;
    const int ns = off ? 0 : n_series;
    const double *const obs_dev = ctx->scores_obs_buf;
    const int *const series_dev = ctx->scores_series_buf;
    HIPCHK(ctx, dev_put(ctx, &DevState::scores, *ctx->scores_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_obs, obs_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_series, series_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_closed, *ctx->scores_closed_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_interval, iv));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_t_first, tf));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_nintervals, nk));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_nitems, ctx->scores_nitems));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_nseries, ns));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_kinds, kind_list));
    return observers_changed(ctx);   // synchronises: the sources above are locals (and the caller's observations and series map)
}
int rh_scores_read(rh_ctx *ctx, double *moments, size_t moment_bytes, unsigned char *closed, size_t closed_bytes) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->scores_nitems) return fail(ctx, RH_ERR_STATE, "rh_scores_read: rh_scores_configure has not been called");
    if (!moments || !closed || moment_bytes != (size_t)ctx->scores_nitems * 5 * ctx->n * sizeof(double) || closed_bytes != (size_t)ctx->scores_nintervals)
        return fail(ctx, RH_ERR_ARG, "rh_scores_read: size mismatch (n_items x 5 x n float64, n_intervals bytes)");
    HIPCHK(ctx, hipMemcpyAsync(moments, ctx->scores_buf, moment_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(closed, ctx->scores_closed_buf, closed_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
// What the four restore calls check first: the observer is configured and no step has run since (RH_ERR_STATE otherwise).
static int restore_check(rh_ctx *ctx, const char *who, const char *configure, int configured, unsigned fresh_bit) {
    if (!ctx) return RH_ERR_ARG;
    if (!configured) return fail(ctx, RH_ERR_STATE, std::string(who) + ": " + configure + " has not been called");
    if (!(ctx->obs_fresh & fresh_bit))
        return fail(ctx, RH_ERR_STATE, std::string(who) + ": a step has run since " + configure + " (a restore follows the configuration, before the next step)");
    return RH_OK;
}
int rh_scores_restore(rh_ctx *ctx, const double *moments, size_t moment_bytes, const unsigned char *closed, size_t closed_bytes, int64_t t_first) {
    if (int rc = restore_check(ctx, "rh_scores_restore", "rh_scores_configure", ctx ? ctx->scores_nitems : 0, RH_FRESH_SCORES)) return rc;
    if (!moments || !closed || moment_bytes != (size_t)ctx->scores_nitems * 5 * ctx->n * sizeof(double) || closed_bytes != (size_t)ctx->scores_nintervals)
        return fail(ctx, RH_ERR_ARG, "rh_scores_restore: size mismatch (n_items x 5 x n float64, n_intervals bytes)");
    if (t_first < 0 || t_first % ctx->scores_interval)
        return fail(ctx, RH_ERR_ARG, "rh_scores_restore: t_first = " + std::to_string(t_first) + " is not a multiple of the interval (" +
                                     std::to_string(ctx->scores_interval) + " s)");
    const long long tf = (long long)t_first;   // (the carried start of interval 0 may lie behind the clock: that is what a restart is)
    HIPCHK(ctx, hipMemcpyAsync(ctx->scores_buf, moments, moment_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scores_closed_buf, closed, closed_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, dev_put(ctx, &DevState::scores_t_first, tf));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's, and a stack local)
    return RH_OK;
}

// ---- event outputs (include/roger_hip.h; the kernel and the rule: rh_events.h) ----
static int events_alloc(rh_ctx *ctx, int n_items, int n_slots, int nblk) {
    const size_t vb = (size_t)n_slots * n_items * ctx->n * sizeof(double), hb = (size_t)n_slots * 6 * sizeof(long long),
                 ib = (size_t)n_slots * nblk * sizeof(long long);
    HIPCHK(ctx, ctx->events_buf.alloc(vb));
    HIPCHK(ctx, hipMemsetAsync(ctx->events_buf, 0, vb, ctx->stream));
    HIPCHK(ctx, ctx->events_hdr_buf.alloc(hb));
    HIPCHK(ctx, hipMemsetAsync(ctx->events_hdr_buf, 0xff, hb, ctx->stream));   // -1: never touched
    HIPCHK(ctx, ctx->events_ids_buf.alloc(ib));
    HIPCHK(ctx, hipMemsetAsync(ctx->events_ids_buf, 0xff, ib, ctx->stream));   // -1: no event's id
    return RH_OK;
}
int rh_events_configure(rh_ctx *ctx, const int *planes, const int *kinds, int n_items, int n_slots) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_EVENTS_MAX_ITEMS)
        return fail(ctx, RH_ERR_ARG, "rh_events_configure: n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_EVENTS_MAX_ITEMS) + ")");
    const bool off = n_items == 0;
    int plane_list[RH_EVENTS_MAX_ITEMS] = {}, kind_list[RH_EVENTS_MAX_ITEMS] = {};
    if (!off) {
        if (!planes || !kinds) return fail(ctx, RH_ERR_ARG, "rh_events_configure: null pointer");
        if (n_slots < 1 || n_slots > RH_EVENTS_MAX_SLOTS)
            return fail(ctx, RH_ERR_ARG, "rh_events_configure: n_slots = " + std::to_string(n_slots) + " (1 ... " + std::to_string(RH_EVENTS_MAX_SLOTS) + ")");
        for (int j = 0; j < n_items; ++j) {   // (item by item, as for the scores)
            if (int rc = check_planes(ctx, "rh_events_configure: ", planes + j, 1, plane_list + j, FLOAT64_IDS)) return rc;
            if (kinds[j] < RH_EVENTS_SUM || kinds[j] > RH_EVENTS_LAST)
                return fail(ctx, RH_ERR_ARG, "rh_events_configure: kind " + std::to_string(kinds[j]) + " of item " + std::to_string(j) + " (0: SUM, 1: PEAK, 2: FIRST, 3: LAST)");
            kind_list[j] = kinds[j];
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that add into the old slots; the scalars below)
    HIPCHK(ctx, ctx->events_buf.release());
    HIPCHK(ctx, ctx->events_hdr_buf.release());
    HIPCHK(ctx, ctx->events_ids_buf.release());
    ctx->events_nitems = ctx->events_nslots = 0;
    ctx->obs_fresh &= ~(unsigned)RH_FRESH_EVENTS;
    const int nblk = (int)grid_for(ctx->n) + 1;   // (the fused launch's grid with RH_TAIL_PRE)
    if (int rc = off ? RH_OK : events_alloc(ctx, n_items, n_slots, nblk)) {   // refused: the event outputs are off
        const std::string why = ctx->err;
        (void)rh_events_configure(ctx, nullptr, nullptr, 0, 0);
        return fail(ctx, rc, why);
    }
    // the event that is running now (the id of the last finished step) keeps t0 = -1; every later event has an id of at least the
    // counter's, so everything below it counts as read out
    long long running = 0, drained = 0;
    if (!off) {
        rh_scalars S;
        HIPCHK(ctx, hipMemcpyAsync(&S, &ctx->dev->S, sizeof(S), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        running = (long long)S.event_id[1];
        drained = (long long)(running > 0 ? running : S.event_id_counter) - 1;
        ctx->events_nitems = n_items;
        ctx->events_nslots = n_slots;
        ctx->obs_fresh |= RH_FRESH_EVENTS;
    }
    std::memcpy(ctx->events_planes, plane_list, sizeof(plane_list));
    const int zero = 0;
    HIPCHK(ctx, dev_put(ctx, &DevState::events, *ctx->events_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_hdr, *ctx->events_hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_ids, *ctx->events_ids_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_drained, drained));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_running, running));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_lost, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_nitems, ctx->events_nitems));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_nslots, ctx->events_nslots));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_nblk, nblk));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_kinds, kind_list));
    return observers_changed(ctx);   // synchronises: the sources above are locals
}
static int events_check(rh_ctx *ctx, const char *who) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->events_nitems) return fail(ctx, RH_ERR_STATE, std::string(who) + ": rh_events_configure has not been called");
    return RH_OK;
}
int rh_events_headers(rh_ctx *ctx, int64_t *hdr, size_t bytes) {
    if (int rc = events_check(ctx, "rh_events_headers")) return rc;
    if (!hdr || bytes != (size_t)ctx->events_nslots * 6 * sizeof(int64_t)) return fail(ctx, RH_ERR_ARG, "rh_events_headers: size mismatch (n_slots x 6 int64)");
    HIPCHK(ctx, hipMemcpyAsync(hdr, ctx->events_hdr_buf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_events_download(rh_ctx *ctx, int item, int slot, double *host, size_t bytes) {
    if (int rc = events_check(ctx, "rh_events_download")) return rc;
    if (item < 0 || item >= ctx->events_nitems || slot < 0 || slot >= ctx->events_nslots)
        return fail(ctx, RH_ERR_ARG, "rh_events_download: item " + std::to_string(item) + " or slot " + std::to_string(slot) + " out of range (" +
                                     std::to_string(ctx->events_nitems) + " items, " + std::to_string(ctx->events_nslots) + " slots)");
    if (!host || bytes != (size_t)ctx->n * sizeof(double)) return fail(ctx, RH_ERR_ARG, "rh_events_download: size mismatch (n float64)");
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->events_buf + ((size_t)slot * ctx->events_nitems + item) * ctx->n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_events_set_drained(rh_ctx *ctx, int64_t event_id) {
    if (int rc = events_check(ctx, "rh_events_set_drained")) return rc;
    const long long v = (long long)event_id;
    HIPCHK(ctx, dev_put(ctx, &DevState::events_drained, v));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (v is a stack local)
    return RH_OK;
}
int rh_events_lost(rh_ctx *ctx, int *lost) {
    if (int rc = events_check(ctx, "rh_events_lost")) return rc;
    if (!lost) return fail(ctx, RH_ERR_ARG, "rh_events_lost: null pointer");
    HIPCHK(ctx, hipMemcpyAsync(lost, &ctx->dev->events_lost, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_events_state(rh_ctx *ctx, int64_t *ids, size_t id_bytes, int64_t *running, int64_t *drained) {
    if (int rc = events_check(ctx, "rh_events_state")) return rc;
    if (!ids || !running || !drained || id_bytes != (size_t)ctx->events_nslots * sizeof(int64_t))
        return fail(ctx, RH_ERR_ARG, "rh_events_state: size mismatch (n_slots int64) or null pointer");
    // workgroup 0's copy of every slot's id: the copies of the workgroups that hold columns agree after every launch (rh_events.h)
    const size_t nblk = (size_t)grid_for(ctx->n) + 1;
    long long v[2] = {0, 0};
    HIPCHK(ctx, hipMemcpy2DAsync(ids, sizeof(int64_t), ctx->events_ids_buf, nblk * sizeof(long long), sizeof(long long), (size_t)ctx->events_nslots,
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&v[0], &ctx->dev->events_running, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&v[1], &ctx->dev->events_drained, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *running = (int64_t)v[0];
    *drained = (int64_t)v[1];
    return RH_OK;
}
int rh_events_restore(rh_ctx *ctx, const int64_t *hdr, size_t hdr_bytes, const int64_t *ids, size_t id_bytes, int64_t running, int64_t drained, int lost,
                      const int *slots, int n_maps, const double *maps, size_t map_bytes) {
    if (int rc = restore_check(ctx, "rh_events_restore", "rh_events_configure", ctx ? ctx->events_nitems : 0, RH_FRESH_EVENTS)) return rc;
    const size_t ns = (size_t)ctx->events_nslots, ni = (size_t)ctx->events_nitems, n = (size_t)ctx->n, nblk = (size_t)grid_for(ctx->n) + 1;
    if (!hdr || !ids || hdr_bytes != ns * 6 * sizeof(int64_t) || id_bytes != ns * sizeof(int64_t))
        return fail(ctx, RH_ERR_ARG, "rh_events_restore: size mismatch (n_slots x 6 int64 headers, n_slots int64 ids)");
    if (n_maps < 0 || (size_t)n_maps > ns || (n_maps && (!slots || !maps)) || map_bytes != (size_t)n_maps * ni * n * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_events_restore: size mismatch (the maps of n_maps <= n_slots slots, n_items x n float64 each)");
    for (int k = 0; k < n_maps; ++k)
        if (slots[k] < 0 || (size_t)slots[k] >= ns)
            return fail(ctx, RH_ERR_ARG, "rh_events_restore: slot " + std::to_string(slots[k]) + " out of range (" + std::to_string(ns) + " slots)");
    // every workgroup's copy of a slot's id (events_ids is (slot, workgroup)): all of them take the carried id
    std::vector<long long> copies(ns * nblk);
    for (size_t s = 0; s < ns; ++s) std::fill(copies.begin() + s * nblk, copies.begin() + (s + 1) * nblk, (long long)ids[s]);
    const long long run = (long long)running, dr = (long long)drained;
    const int was_lost = lost ? 1 : 0;
    HIPCHK(ctx, hipMemcpyAsync(ctx->events_hdr_buf, hdr, hdr_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->events_ids_buf, copies.data(), copies.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    for (int k = 0; k < n_maps; ++k)
        HIPCHK(ctx, hipMemcpyAsync(ctx->events_buf + (size_t)slots[k] * ni * n, maps + (size_t)k * ni * n, ni * n * sizeof(double), hipMemcpyHostToDevice,
                                   ctx->stream));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_running, run));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_drained, dr));
    HIPCHK(ctx, dev_put(ctx, &DevState::events_lost, was_lost));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's and locals)
    return RH_OK;
}

// ---- duration curves (include/roger_hip.h; the kernel and the rule: rh_durations.h) ----
// the buffers, cleared: counters and spells to 0, acc to +0.0, mn / mx to +inf / -inf
static int durations_alloc(rh_ctx *ctx, int n_items, int n_bins, const double *edges, int n_edges, const unsigned char *mask) {
    const size_t n = (size_t)ctx->n, cb = (size_t)n_bins * n * sizeof(unsigned), vb = (size_t)n_items * 3 * n * sizeof(double),
                 sb = (size_t)n_items * 3 * n * sizeof(unsigned);
    HIPCHK(ctx, ctx->durations_counts_buf.alloc(cb));
    HIPCHK(ctx, hipMemsetAsync(ctx->durations_counts_buf, 0, cb, ctx->stream));
    HIPCHK(ctx, ctx->durations_spells_buf.alloc(sb));
    HIPCHK(ctx, hipMemsetAsync(ctx->durations_spells_buf, 0, sb, ctx->stream));
    HIPCHK(ctx, ctx->durations_vals_buf.alloc(vb));
    HIPCHK(ctx, hipMemsetAsync(ctx->durations_vals_buf, 0, vb, ctx->stream));
    std::vector<double> init(2 * n, HUGE_VAL);   // one item's mn and mx planes
    std::fill(init.begin() + n, init.end(), -HUGE_VAL);
    for (int j = 0; j < n_items; ++j)
        HIPCHK(ctx, hipMemcpyAsync(ctx->durations_vals_buf + ((size_t)j * 3 + 1) * n, init.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, ctx->durations_edges_buf.alloc((size_t)(n_edges ? n_edges : 1) * sizeof(double)));
    if (n_edges) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->durations_edges_buf, edges, (size_t)n_edges * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (mask) {
        HIPCHK(ctx, ctx->durations_mask_buf.alloc(n));
        HIPCHK(ctx, hipMemcpyAsync(ctx->durations_mask_buf, mask, n, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (`init` is a local)
    return RH_OK;
}
int rh_durations_configure(rh_ctx *ctx, const int *planes, const int *kinds, const int *n_edges, int n_items, const double *edges,
                           const double *thresholds, const int *sides, const unsigned char *mask, int64_t interval_seconds, int64_t t_first) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_DURATIONS_MAX_ITEMS)
        return fail(ctx, RH_ERR_ARG, "rh_durations_configure: n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_DURATIONS_MAX_ITEMS) + ")");
    const bool off = n_items == 0;
    int plane_list[RH_DURATIONS_MAX_ITEMS] = {}, kind_list[RH_DURATIONS_MAX_ITEMS] = {}, m_list[RH_DURATIONS_MAX_ITEMS] = {},
        edge_off[RH_DURATIONS_MAX_ITEMS] = {}, bin_off[RH_DURATIONS_MAX_ITEMS] = {}, side_list[RH_DURATIONS_MAX_ITEMS] = {};
    double thr_list[RH_DURATIONS_MAX_ITEMS];
    std::fill(thr_list, thr_list + RH_DURATIONS_MAX_ITEMS, std::nan(""));
    int total_edges = 0, total_bins = 0, n_sum = 0;
    if (!off) {
        if (!planes || !kinds || !n_edges || !thresholds || !sides) return fail(ctx, RH_ERR_ARG, "rh_durations_configure: null pointer");
        if (interval_seconds != 86400 && interval_seconds != 3600 && interval_seconds != 600)
            return fail(ctx, RH_ERR_ARG, "rh_durations_configure: interval_seconds = " + std::to_string(interval_seconds) +
                                         " (the interval is a day, an hour or ten minutes: the step classes)");
        if (t_first < 0 || t_first % interval_seconds)
            return fail(ctx, RH_ERR_ARG, "rh_durations_configure: t_first = " + std::to_string(t_first) + " is not a multiple of the interval (" +
                                         std::to_string(interval_seconds) + " s)");
        for (int j = 0; j < n_items; ++j) {   // (item by item, as for the scores)
            const std::string item = " of item " + std::to_string(j);
            if (int rc = check_planes(ctx, "rh_durations_configure: item " + std::to_string(j) + ": ", planes + j, 1, plane_list + j, FLOAT64_IDS)) return rc;
            if (kinds[j] != RH_DURATIONS_SUM && kinds[j] != RH_DURATIONS_LAST)
                return fail(ctx, RH_ERR_ARG, "rh_durations_configure: kind " + std::to_string(kinds[j]) + item + " (0: SUM, 1: LAST)");
            if (n_edges[j] < 0 || n_edges[j] > RH_DURATIONS_MAX_EDGES)
                return fail(ctx, RH_ERR_ARG, "rh_durations_configure: " + std::to_string(n_edges[j]) + " edges" + item + " (0 ... " +
                                             std::to_string(RH_DURATIONS_MAX_EDGES) + ")");
            if (n_edges[j] && !edges) return fail(ctx, RH_ERR_ARG, "rh_durations_configure: null pointer");
            for (int q = 0; q < n_edges[j]; ++q) {
                const double e = edges[total_edges + q];
                if (!std::isfinite(e))
                    return fail(ctx, RH_ERR_ARG, "rh_durations_configure: edge " + std::to_string(q) + item + " is not finite");
                if (q && !(edges[total_edges + q - 1] < e))
                    return fail(ctx, RH_ERR_ARG, "rh_durations_configure: the edges" + item + " are not strictly ascending (edge " + std::to_string(q) + ")");
            }
            if (thresholds[j] == thresholds[j] && sides[j] != RH_DURATIONS_BELOW && sides[j] != RH_DURATIONS_AT_OR_ABOVE)
                return fail(ctx, RH_ERR_ARG, "rh_durations_configure: side " + std::to_string(sides[j]) + item + " (0: BELOW, 1: AT_OR_ABOVE)");
            kind_list[j] = kinds[j];
            m_list[j] = n_edges[j];
            edge_off[j] = total_edges;
            bin_off[j] = total_bins;
            thr_list[j] = thresholds[j];
            side_list[j] = thresholds[j] == thresholds[j] ? sides[j] : 0;
            total_edges += n_edges[j];
            total_bins += n_edges[j] + 2;
            n_sum += kinds[j] == RH_DURATIONS_SUM;
        }
        // the capacity rule of the rings, on the words per column: 4 per bin, 36 per item
        const int64_t words = ((int64_t)total_bins + 9 * (int64_t)n_items) * ctx->n;
        if (int rc = check_capacity(ctx, "rh_durations_configure: " + std::to_string(total_bins) + " bins and " + std::to_string(n_items) +
                                             " items over " + std::to_string(ctx->n) + " columns, in 4-byte words: ", words)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that count into the old buffers)
    HIPCHK(ctx, ctx->durations_counts_buf.release());
    HIPCHK(ctx, ctx->durations_spells_buf.release());
    HIPCHK(ctx, ctx->durations_vals_buf.release());
    HIPCHK(ctx, ctx->durations_edges_buf.release());
    HIPCHK(ctx, ctx->durations_mask_buf.release());
    ctx->durations_nitems = ctx->durations_nbins = 0;
    ctx->obs_fresh &= ~(unsigned)RH_FRESH_DURATIONS;
    if (int rc = off ? RH_OK : durations_alloc(ctx, n_items, total_bins, edges, total_edges, mask)) {   // refused: the observer is off
        const std::string why = ctx->err;
        (void)rh_durations_configure(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0);
        return fail(ctx, rc, why);
    }
    if (!off) {
        ctx->durations_nitems = n_items;
        ctx->durations_nbins = total_bins;
        ctx->obs_fresh |= RH_FRESH_DURATIONS;
    }
    std::memcpy(ctx->durations_planes, plane_list, sizeof(plane_list));
    const long long iv = off ? 86400 : (long long)interval_seconds, tf = off ? 0 : (long long)t_first;
    const double *const edges_dev = ctx->durations_edges_buf;
    const unsigned char *const mask_dev = ctx->durations_mask_buf;
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_counts, *ctx->durations_counts_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_spells, *ctx->durations_spells_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_vals, *ctx->durations_vals_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_edges, edges_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_mask, mask_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_interval, iv));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_t_first, tf));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_nitems, ctx->durations_nitems));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_nsum, n_sum));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_kinds, kind_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_nedges, m_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_edge_off, edge_off));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_bin_off, bin_off));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_sides, side_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::durations_thr, thr_list));
    return observers_changed(ctx);   // synchronises: the sources above are locals
}
int rh_durations_read(rh_ctx *ctx, uint32_t *counts, size_t count_bytes, double *values, size_t value_bytes, uint32_t *spells, size_t spell_bytes) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->durations_nitems) return fail(ctx, RH_ERR_STATE, "rh_durations_read: rh_durations_configure has not been called");
    const size_t n = (size_t)ctx->n, ni = (size_t)ctx->durations_nitems;
    if (!counts || !values || !spells || count_bytes != (size_t)ctx->durations_nbins * n * sizeof(uint32_t) || value_bytes != ni * 3 * n * sizeof(double) ||
        spell_bytes != ni * 3 * n * sizeof(uint32_t))
        return fail(ctx, RH_ERR_ARG, "rh_durations_read: size mismatch (n_bins x n uint32, n_items x 3 x n float64, n_items x 3 x n uint32)");
    HIPCHK(ctx, hipMemcpyAsync(counts, ctx->durations_counts_buf, count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(values, ctx->durations_vals_buf, value_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(spells, ctx->durations_spells_buf, spell_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_durations_restore(rh_ctx *ctx, const uint32_t *counts, size_t count_bytes, const double *values, size_t value_bytes, const uint32_t *spells,
                         size_t spell_bytes) {
    if (int rc = restore_check(ctx, "rh_durations_restore", "rh_durations_configure", ctx ? ctx->durations_nitems : 0, RH_FRESH_DURATIONS)) return rc;
    const size_t n = (size_t)ctx->n, ni = (size_t)ctx->durations_nitems;
    if (!counts || !values || !spells || count_bytes != (size_t)ctx->durations_nbins * n * sizeof(uint32_t) || value_bytes != ni * 3 * n * sizeof(double) ||
        spell_bytes != ni * 3 * n * sizeof(uint32_t))
        return fail(ctx, RH_ERR_ARG, "rh_durations_restore: size mismatch (n_bins x n uint32, n_items x 3 x n float64, n_items x 3 x n uint32)");
    HIPCHK(ctx, hipMemcpyAsync(ctx->durations_counts_buf, counts, count_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->durations_vals_buf, values, value_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->durations_spells_buf, spells, spell_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's)
    return RH_OK;
}

// ---- ensemble bands (include/roger_hip.h; the kernels, the rule and the selection: rh_bands.h) ----
// What a zonal configuration adds on the host: the byte mask zone >= 0 for k_bands, and zone_off[n_zones + 1] with the zones' column lists
// behind it (a stable counting sort: ascending within a zone).
struct BandsZones {
    int n_zones = 0;
    std::vector<unsigned char> mask;
    std::vector<int> index;
};
// the observations' buffers released and their members of the control block null: no later step launches k_bands_obs*.  (The caller has
// synchronised the stream; the sources are static.)
static int bands_obs_release(rh_ctx *ctx) {
    static const long long *const none = nullptr;
    static const long long zero = 0;
    HIPCHK(ctx, ctx->bands_obs_buf.release());
    HIPCHK(ctx, ctx->bands_obs_part_buf.release());
    HIPCHK(ctx, ctx->bands_obs_ring_buf.release());
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs, none));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_part, none));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_ring, none));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_n, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_first, zero));
    return RH_OK;
}
// the buffers: the ring, the accumulators at +0.0, every key "masked out" (a masked-in column stores its key on every counted step), the
// histograms at 0 (the plain selection's alone); per zone the counts and the column lists; with weights the weight plane, the 64-bit
// histograms at 0 in place of the 32-bit ones, and the ring of the rows' weight sums
static int bands_alloc(rh_ctx *ctx, int n_items, int n_probs, const unsigned char *mask, const BandsZones &zones, const uint16_t *weight,
                       int64_t capacity) {
    const size_t n = (size_t)ctx->n, ab = (size_t)n_items * n * sizeof(double),
                 hb = (size_t)n_items * RH_BANDS_MAX_PROBS * RH_SELECT_NBINS * sizeof(unsigned), nz = (size_t)zones.n_zones,
                 blocks = (size_t)n_items * (nz ? nz : 1);
    HIPCHK(ctx, ctx->bands.buf.alloc((size_t)capacity * blocks * n_probs * sizeof(double)));
    HIPCHK(ctx, ctx->bands.hdr_buf.alloc((size_t)capacity * (nz ? 2 : 2 + 2 * (size_t)n_items) * sizeof(long long)));
    HIPCHK(ctx, ctx->bands_acc_buf.alloc(ab));
    HIPCHK(ctx, hipMemsetAsync(ctx->bands_acc_buf, 0, ab, ctx->stream));
    HIPCHK(ctx, ctx->bands_keys_buf.alloc(ab));
    HIPCHK(ctx, hipMemsetAsync(ctx->bands_keys_buf, 0xff, ab, ctx->stream));   // RH_SELECT_KEY_MASKED
    if (nz) {
        HIPCHK(ctx, ctx->bands_counts_buf.alloc((size_t)capacity * blocks * 2 * sizeof(long long)));
        HIPCHK(ctx, ctx->bands_zone_buf.alloc(zones.index.size() * sizeof(int)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->bands_zone_buf, zones.index.data(), zones.index.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        mask = zones.mask.data();
    } else if (weight) {
        HIPCHK(ctx, ctx->bands_weight_buf.alloc(n * sizeof(uint16_t)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->bands_weight_buf, weight, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, ctx->bands_whist_buf.alloc(2 * hb));
        HIPCHK(ctx, hipMemsetAsync(ctx->bands_whist_buf, 0, 2 * hb, ctx->stream));
        HIPCHK(ctx, ctx->bands_wsum_buf.alloc((size_t)capacity * n_items * sizeof(long long)));
    } else {
        HIPCHK(ctx, ctx->bands_hist_buf.alloc(hb));
        HIPCHK(ctx, hipMemsetAsync(ctx->bands_hist_buf, 0, hb, ctx->stream));
    }
    if (mask) {
        HIPCHK(ctx, ctx->bands_mask_buf.alloc(n));
        HIPCHK(ctx, hipMemcpyAsync(ctx->bands_mask_buf, mask, n, hipMemcpyHostToDevice, ctx->stream));
    }
    return RH_OK;
}
// rh_bands_configure (zone == nullptr), rh_bands_configure_zonal (mask == nullptr) and rh_bands_configure_weighted (both null; weighted:
// `weight` is asked for, and its byte mask w != 0 is formed here) under the name `who`
static int bands_configure(rh_ctx *ctx, const std::string &who, const int *planes, const int *kinds, int n_items, const double *probs, int n_probs,
                           int64_t interval_seconds, int64_t t_first, const unsigned char *mask, const int32_t *zone, int n_zones, bool zonal,
                           int64_t capacity, const uint16_t *weight = nullptr, bool weighted = false) {
    if (!ctx) return RH_ERR_ARG;
    if (n_items < 0 || n_items > RH_BANDS_MAX_ITEMS)
        return fail(ctx, RH_ERR_ARG, who + ": n_items = " + std::to_string(n_items) + " (0 ... " + std::to_string(RH_BANDS_MAX_ITEMS) + ")");
    const bool off = n_items == 0;
    int plane_list[RH_BANDS_MAX_ITEMS] = {}, kind_list[RH_BANDS_MAX_ITEMS] = {}, n_sum = 0;
    double prob_list[RH_BANDS_MAX_PROBS] = {};
    BandsZones zones;
    std::vector<unsigned char> weight_mask;
    if (!off) {
        if (!planes || !kinds || !probs || (zonal && !zone) || (weighted && !weight)) return fail(ctx, RH_ERR_ARG, who + ": null pointer");
        if (n_probs < 1 || n_probs > RH_BANDS_MAX_PROBS)
            return fail(ctx, RH_ERR_ARG, who + ": n_probs = " + std::to_string(n_probs) + " (1 ... " + std::to_string(RH_BANDS_MAX_PROBS) + ")");
        for (int q = 0; q < n_probs; ++q) {
            if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
                return fail(ctx, RH_ERR_ARG, who + ": probability " + std::to_string(q) + " = " + std::to_string(probs[q]) + " (within [0, 1])");
            prob_list[q] = probs[q];
        }
        if (interval_seconds != 86400 && interval_seconds != 3600 && interval_seconds != 600)
            return fail(ctx, RH_ERR_ARG, who + ": interval_seconds = " + std::to_string(interval_seconds) +
                                         " (the interval is a day, an hour or ten minutes: the step classes)");
        if (t_first < 0 || t_first % interval_seconds)
            return fail(ctx, RH_ERR_ARG, who + ": t_first = " + std::to_string(t_first) + " is not a multiple of the interval (" +
                                         std::to_string(interval_seconds) + " s)");
        for (int j = 0; j < n_items; ++j) {   // (item by item, as for the scores)
            if (int rc = check_planes(ctx, who + ": item " + std::to_string(j) + ": ", planes + j, 1, plane_list + j, FLOAT64_IDS)) return rc;
            if (kinds[j] != RH_BANDS_SUM && kinds[j] != RH_BANDS_LAST)
                return fail(ctx, RH_ERR_ARG, who + ": kind " + std::to_string(kinds[j]) + " of item " + std::to_string(j) + " (0: SUM, 1: LAST)");
            kind_list[j] = kinds[j];
            n_sum += kinds[j] == RH_BANDS_SUM;
        }
        if (ctx->n >= (int64_t)1 << 31) return fail(ctx, RH_ERR_ARG, who + ": " + std::to_string(ctx->n) + " columns (the histograms hold uint32 counts)");
        if (int rc = check_capacity(ctx, who + ": ", capacity)) return rc;
        if (zonal) {
            if (n_zones < 1 || n_zones > RH_BANDS_MAX_ZONES)
                return fail(ctx, RH_ERR_ARG, who + ": n_zones = " + std::to_string(n_zones) + " (1 ... " + std::to_string(RH_BANDS_MAX_ZONES) + ")");
            const size_t n = (size_t)ctx->n, nz = (size_t)n_zones;
            std::vector<int> off_of(nz + 1, 0);
            for (size_t i = 0; i < n; ++i) {
                if (zone[i] >= n_zones)
                    return fail(ctx, RH_ERR_ARG, who + ": zone index " + std::to_string(zone[i]) + " of column " + std::to_string(i) + " (n_zones = " +
                                                 std::to_string(n_zones) + ")");
                if (zone[i] >= 0) ++off_of[(size_t)zone[i] + 1];
            }
            for (size_t z = 0; z < nz; ++z) off_of[z + 1] += off_of[z];
            if (!off_of[nz]) return fail(ctx, RH_ERR_ARG, who + ": no participating column (every zone index is negative)");
            zones.n_zones = n_zones;
            zones.mask.resize(n);
            zones.index.assign(nz + 1 + (size_t)off_of[nz], 0);
            std::copy(off_of.begin(), off_of.end(), zones.index.begin());
            std::vector<int> next(off_of.begin(), off_of.end() - 1);
            for (size_t i = 0; i < n; ++i) {
                zones.mask[i] = zone[i] >= 0;
                if (zone[i] >= 0) zones.index[nz + 1 + (size_t)next[(size_t)zone[i]]++] = (int)i;
            }
        }
        if (weighted) {
            const size_t n = (size_t)ctx->n;
            weight_mask.resize(n);
            for (size_t i = 0; i < n; ++i) weight_mask[i] = weight[i] != 0;
            if (std::find(weight_mask.begin(), weight_mask.end(), 1) == weight_mask.end()) return fail(ctx, RH_ERR_ARG, who + ": no participating column (every weight is 0)");
            mask = weight_mask.data();
        }
    }
    if (off || !weighted) weight = nullptr;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    HIPCHK(ctx, ctx->bands.release());
    HIPCHK(ctx, ctx->bands_acc_buf.release());
    HIPCHK(ctx, ctx->bands_keys_buf.release());
    HIPCHK(ctx, ctx->bands_hist_buf.release());
    HIPCHK(ctx, ctx->bands_mask_buf.release());
    HIPCHK(ctx, ctx->bands_counts_buf.release());
    HIPCHK(ctx, ctx->bands_zone_buf.release());
    HIPCHK(ctx, ctx->bands_weight_buf.release());
    HIPCHK(ctx, ctx->bands_whist_buf.release());
    HIPCHK(ctx, ctx->bands_wsum_buf.release());
    if (int rc = bands_obs_release(ctx)) return rc;   // (observations belong to the configuration they were set behind)
    ctx->bands_nitems = ctx->bands_nprobs = ctx->bands_nzones = 0;
    ctx->obs_fresh &= ~(unsigned)RH_FRESH_BANDS;
    if (int rc = off ? RH_OK : bands_alloc(ctx, n_items, n_probs, mask, zones, weight, capacity)) {   // refused: the observer is off
        const std::string why = ctx->err;
        (void)bands_configure(ctx, who, nullptr, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, 0, false, 0);
        return fail(ctx, rc, why);
    }
    if (!off) {
        ctx->bands_nitems = n_items;
        ctx->bands_nprobs = n_probs;
        ctx->bands_nzones = zones.n_zones;
        ctx->bands.cap = capacity;
        ctx->obs_fresh |= RH_FRESH_BANDS;
    }
    std::memcpy(ctx->bands_planes, plane_list, sizeof(plane_list));
    const long long zero = 0, cap = (long long)ctx->bands.cap, iv = off ? 86400 : (long long)interval_seconds, tf = off ? 0 : (long long)t_first;
    const unsigned none = 0, no_nan[RH_BANDS_MAX_ITEMS] = {};
    const unsigned short *const weight_dev = ctx->bands_weight_buf;
    const unsigned char *const mask_dev = ctx->bands_mask_buf;
    const int *const zone_off = ctx->bands_zone_buf, *const zone_cols = zone_off ? zone_off + zones.n_zones + 1 : nullptr;
    HIPCHK(ctx, dev_put(ctx, &DevState::bands, *ctx->bands.buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_hdr, *ctx->bands.hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_acc, *ctx->bands_acc_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_keys, *ctx->bands_keys_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_hist, *ctx->bands_hist_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_mask, mask_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_counts, *ctx->bands_counts_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_zone_off, zone_off));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_zone_cols, zone_cols));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_weight, weight_dev));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_whist, *ctx->bands_whist_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_wsum, *ctx->bands_wsum_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_m_count, no_nan));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_rows, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_interval, iv));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_t_first, tf));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_nitems, ctx->bands_nitems));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_nprobs, ctx->bands_nprobs));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_nsum, n_sum));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_done, none));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_nan_count, no_nan));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_kinds, kind_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_probs, prob_list));
    return observers_changed(ctx);   // synchronises: the sources above are locals (and the caller's mask)
}
int rh_bands_configure(rh_ctx *ctx, const int *planes, const int *kinds, int n_items, const double *probs, int n_probs, int64_t interval_seconds,
                       int64_t t_first, const unsigned char *mask, int64_t capacity) {
    return bands_configure(ctx, "rh_bands_configure", planes, kinds, n_items, probs, n_probs, interval_seconds, t_first, mask, nullptr, 0, false, capacity);
}
int rh_bands_configure_zonal(rh_ctx *ctx, const int *planes, const int *kinds, int n_items, const double *probs, int n_probs, int64_t interval_seconds,
                             int64_t t_first, const int32_t *zone, int n_zones, int64_t capacity) {
    return bands_configure(ctx, "rh_bands_configure_zonal", planes, kinds, n_items, probs, n_probs, interval_seconds, t_first, nullptr, zone, n_zones, true,
                           capacity);
}
int rh_bands_configure_weighted(rh_ctx *ctx, const int *planes, const int *kinds, int n_items, const double *probs, int n_probs, int64_t interval_seconds,
                                int64_t t_first, const uint16_t *weight, int64_t capacity) {
    return bands_configure(ctx, "rh_bands_configure_weighted", planes, kinds, n_items, probs, n_probs, interval_seconds, t_first, nullptr, nullptr, 0, false,
                           capacity, weight, true);
}
int rh_bands_count(rh_ctx *ctx, int64_t *rows_total) {
    if (!ctx) return RH_ERR_ARG;
    if (!rows_total) return fail(ctx, RH_ERR_ARG, "rh_bands_count: null pointer");
    long long rows = 0;
    if (int rc = ring_rows(ctx, "rh_bands_count", ctx->bands, "rh_bands_configure", &DevState::bands_rows, &rows)) return rc;
    *rows_total = (int64_t)rows;
    return RH_OK;
}
int rh_bands_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_bands_read", ctx->bands, "rh_bands_configure", &DevState::bands_rows, &total)) return rc;
    if (ctx->bands_nzones) return fail(ctx, RH_ERR_STATE, "rh_bands_read: the bands are configured per zone (rh_bands_zonal_read reads their rows)");
    const size_t nv = (size_t)ctx->bands_nitems * ctx->bands_nprobs;
    const std::string why = ring_range_refusal("rh_bands_read", first_row, n_rows, total, ctx->bands.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!hdr || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_bands_read: size mismatch (n_rows x n_items x n_probs float64)");
    return ring_download(ctx, ctx->bands, nv, first_row, n_rows, hdr, values, 2 + 2 * (size_t)ctx->bands_nitems);
}
int rh_bands_zonal_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, int64_t *counts, size_t count_bytes, double *values,
                        size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_bands_zonal_read", ctx->bands, "rh_bands_configure_zonal", &DevState::bands_rows, &total)) return rc;
    if (ctx->bands_weight_buf)
        return fail(ctx, RH_ERR_STATE, "rh_bands_zonal_read: the bands are configured with weights (rh_bands_read and rh_bands_weight_sums read their rows)");
    if (!ctx->bands_nzones) return fail(ctx, RH_ERR_STATE, "rh_bands_zonal_read: the bands are configured without zones (rh_bands_read reads their rows)");
    const size_t blocks = (size_t)ctx->bands_nitems * ctx->bands_nzones, nv = blocks * ctx->bands_nprobs, nc = blocks * 2;
    const std::string why = ring_range_refusal("rh_bands_zonal_read", first_row, n_rows, total, ctx->bands.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && (!hdr || !counts || !values)) || count_bytes != (size_t)n_rows * nc * sizeof(int64_t) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_bands_zonal_read: size mismatch (n_rows x n_items x n_zones x 2 int64, n_rows x n_items x n_zones x n_probs float64)");
    const int rc = ring_pieces(first_row, n_rows, ctx->bands.cap, [&](int64_t done, int64_t slot, int64_t m) -> int {
        HIPCHK(ctx, hipMemcpyAsync(counts + (size_t)done * nc, ctx->bands_counts_buf + (size_t)slot * nc, (size_t)m * nc * sizeof(long long),
                                   hipMemcpyDeviceToHost, ctx->stream));
        return RH_OK;
    });
    if (rc) return rc;
    return ring_download(ctx, ctx->bands, nv, first_row, n_rows, hdr, values, 2);
}
// W per item of the rows [first_row, first_row + n_rows) of a weighted configuration: the ring beside the headers
int rh_bands_weight_sums(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *wsum, size_t bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_bands_weight_sums", ctx->bands, "rh_bands_configure_weighted", &DevState::bands_rows, &total)) return rc;
    if (!ctx->bands_weight_buf)
        return fail(ctx, RH_ERR_STATE, "rh_bands_weight_sums: the bands are configured without weights (rh_bands_configure_weighted records the weight sums)");
    const size_t ni = (size_t)ctx->bands_nitems;
    const std::string why = ring_range_refusal("rh_bands_weight_sums", first_row, n_rows, total, ctx->bands.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && !wsum) || bytes != (size_t)n_rows * ni * sizeof(int64_t))
        return fail(ctx, RH_ERR_ARG, "rh_bands_weight_sums: size mismatch (n_rows x n_items int64)");
    const int rc = ring_pieces(first_row, n_rows, ctx->bands.cap, [&](int64_t done, int64_t slot, int64_t m) -> int {
        HIPCHK(ctx, hipMemcpyAsync(wsum + (size_t)done * ni, ctx->bands_wsum_buf + (size_t)slot * ni, (size_t)m * ni * sizeof(long long),
                                   hipMemcpyDeviceToHost, ctx->stream));
        return RH_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
// Observations behind any rh_bands_configure* call: obs (n_items, n_series, n_intervals) float64, NaN: missing; n_series 1, or n_zones
// on a zonal configuration; row interval k reads element k + first_index.  Allocates the series, the partials (plain and weighted) and
// the ring of pairs at -1 (the rows recorded before this call have no pair); n_intervals == 0 releases them.  Synchronises.
int rh_bands_observations(rh_ctx *ctx, const double *obs, int n_series, int64_t n_intervals, int64_t first_index) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->bands_nitems) return fail(ctx, RH_ERR_STATE, "rh_bands_observations: rh_bands_configure has not been called");
    if (n_intervals < 0 || n_intervals >= (int64_t)1 << 31)
        return fail(ctx, RH_ERR_ARG, "rh_bands_observations: n_intervals = " + std::to_string(n_intervals) + " (0 ... 2^31 - 1; 0 releases the observations)");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (launches that write the old ring)
    if (n_intervals == 0) {
        if (int rc = bands_obs_release(ctx)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return RH_OK;
    }
    const int want = ctx->bands_nzones ? ctx->bands_nzones : 1;
    if (n_series != want)
        return fail(ctx, RH_ERR_ARG, "rh_bands_observations: n_series = " + std::to_string(n_series) +
                                     (ctx->bands_nzones ? " (the bands are configured per zone: n_zones = " + std::to_string(want) + " series per item)"
                                                        : " (the bands are configured without zones: 1 series per item)"));
    if (!obs) return fail(ctx, RH_ERR_ARG, "rh_bands_observations: null pointer");
    if (first_index < 0)
        return fail(ctx, RH_ERR_ARG, "rh_bands_observations: first_index = " + std::to_string(first_index) + " (the index of the first counted interval, at least 0)");
    const size_t ni = (size_t)ctx->bands_nitems, ns = (size_t)n_series, ob = ni * ns * (size_t)n_intervals * sizeof(double),
                 parts = select_obs_grid((long long)ctx->n), rb = (size_t)ctx->bands.cap * ni * ns * 2 * sizeof(long long);
    int rc = RH_OK;
    auto alloc = [&]() -> int {
        HIPCHK(ctx, ctx->bands_obs_buf.alloc(ob));
        HIPCHK(ctx, hipMemcpyAsync(ctx->bands_obs_buf, obs, ob, hipMemcpyHostToDevice, ctx->stream));
        if (!ctx->bands_nzones) {
            HIPCHK(ctx, ctx->bands_obs_part_buf.alloc(ni * parts * 2 * sizeof(long long)));
            HIPCHK(ctx, hipMemsetAsync(ctx->bands_obs_part_buf, 0, ni * parts * 2 * sizeof(long long), ctx->stream));
        }
        HIPCHK(ctx, ctx->bands_obs_ring_buf.alloc(rb));
        HIPCHK(ctx, hipMemsetAsync(ctx->bands_obs_ring_buf, 0xff, rb, ctx->stream));   // -1: no observation
        return RH_OK;
    };
    if ((rc = bands_obs_release(ctx))) return rc;
    if ((rc = alloc())) {   // refused: no observations, the bands go on as they were
        const std::string why = ctx->err;
        (void)bands_obs_release(ctx);
        (void)hipStreamSynchronize(ctx->stream);
        return fail(ctx, rc, why);
    }
    const long long len = (long long)n_intervals, first = (long long)first_index;
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs, *ctx->bands_obs_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_part, *ctx->bands_obs_part_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_ring, *ctx->bands_obs_ring_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_n, len));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_obs_first, first));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's, and stack locals)
    return RH_OK;
}
// the pairs {below, equal} of the rows [first_row, first_row + n_rows): (n_rows, n_items, n_series, 2) int64, -1 where the observation is
// missing; the row range is checked as in rh_bands_read.  Synchronises.
int rh_bands_obs_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *pairs, size_t bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = ring_rows(ctx, "rh_bands_obs_read", ctx->bands, "rh_bands_configure", &DevState::bands_rows, &total)) return rc;
    if (!ctx->bands_obs_buf)
        return fail(ctx, RH_ERR_STATE, "rh_bands_obs_read: no observations are set (rh_bands_observations has not been called behind rh_bands_configure)");
    const size_t np = (size_t)ctx->bands_nitems * (ctx->bands_nzones ? ctx->bands_nzones : 1) * 2;
    const std::string why = ring_range_refusal("rh_bands_obs_read", first_row, n_rows, total, ctx->bands.cap);
    if (!why.empty()) return fail(ctx, RH_ERR_ARG, why);
    if ((n_rows && !pairs) || bytes != (size_t)n_rows * np * sizeof(int64_t))
        return fail(ctx, RH_ERR_ARG, "rh_bands_obs_read: size mismatch (n_rows x n_items x n_series x 2 int64)");
    const int rc = ring_pieces(first_row, n_rows, ctx->bands.cap, [&](int64_t done, int64_t slot, int64_t m) -> int {
        HIPCHK(ctx, hipMemcpyAsync(pairs + (size_t)done * np, ctx->bands_obs_ring_buf + (size_t)slot * np, (size_t)m * np * sizeof(long long),
                                   hipMemcpyDeviceToHost, ctx->stream));
        return RH_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
// the SUM accumulators of the interval under way, with or without zones (the ring's rows are the caller's already; the keys and the
// selection's scratch are rewritten or zero between two launches)
int rh_bands_state(rh_ctx *ctx, double *acc, size_t acc_bytes) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->bands_nitems) return fail(ctx, RH_ERR_STATE, "rh_bands_state: rh_bands_configure has not been called");
    if (!acc || acc_bytes != (size_t)ctx->bands_nitems * ctx->n * sizeof(double)) return fail(ctx, RH_ERR_ARG, "rh_bands_state: size mismatch (n_items x n float64)");
    HIPCHK(ctx, hipMemcpyAsync(acc, ctx->bands_acc_buf, acc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_bands_restore(rh_ctx *ctx, const double *acc, size_t acc_bytes, int64_t rows) {
    if (int rc = restore_check(ctx, "rh_bands_restore", "rh_bands_configure", ctx ? ctx->bands_nitems : 0, RH_FRESH_BANDS)) return rc;
    if (!acc || acc_bytes != (size_t)ctx->bands_nitems * ctx->n * sizeof(double)) return fail(ctx, RH_ERR_ARG, "rh_bands_restore: size mismatch (n_items x n float64)");
    if (rows < 0) return fail(ctx, RH_ERR_ARG, "rh_bands_restore: rows = " + std::to_string(rows) + " (the rows recorded before the restart, at least 0)");
    const long long r = (long long)rows;   // row r lands at r mod capacity: the numbering and the interval index k go on
    HIPCHK(ctx, hipMemcpyAsync(ctx->bands_acc_buf, acc, acc_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, dev_put(ctx, &DevState::bands_rows, r));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are the caller's, and a stack local)
    return RH_OK;
}
