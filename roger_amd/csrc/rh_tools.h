// rh_tools.h -- timing, selftests and the other entry points of tools and tests.  Part of the one translation unit roger_hip.hip.
#pragma once
int rh_predicates_expand(rh_ctx *ctx, int word, int32_t *dev_dst64) {
    if (!ctx || word < 0 || word > 3 || !dev_dst64) return RH_ERR_ARG;
    hipLaunchKernelGGL(k_words_expand, dim3(1), dim3(64), 0, ctx->stream, ctx->dev, word, dev_dst64);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
int rh_predicates_compress(rh_ctx *ctx, int word, const int32_t *dev_src64) {
    if (!ctx || word < 0 || word > 3 || !dev_src64) return RH_ERR_ARG;
    hipLaunchKernelGGL(k_words_compress, dim3(1), dim3(64), 0, ctx->stream, ctx->dev, word, dev_src64);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

int rh_calibrate_copy(rh_ctx *ctx, int src_plane0, int dst_plane0, int nplanes) {
    if (!ctx || nplanes <= 0 || src_plane0 < 0 || dst_plane0 < 0 || src_plane0 + nplanes > ctx->planes_held ||
        dst_plane0 + nplanes > ctx->planes_held)
        return RH_ERR_ARG;
    for (int p = 0; p < nplanes; ++p)
        if (PLANE_IS_INT[src_plane0 + p] || PLANE_IS_INT[dst_plane0 + p]) return fail(ctx, RH_ERR_ARG, "calibration planes must be float64");
    planes_touched(ctx);
    hipLaunchKernelGGL(k_calib_copy, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, src_plane0, dst_plane0, nplanes);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// Experiment (tools/swap_levels.py): two contexts of the same shape exchange their arenas -- does the fused kernel's speed level follow the
// arena or the rest of the context?  The caller has brought both to the same state (same steps from the same start).
int rh_debug_swap_arenas(rh_ctx *a, rh_ctx *b) {
    if (!a || !b || a->n != b->n || a->arena.stride != b->arena.stride || a->planes_held != b->planes_held) return RH_ERR_ARG;
    HIPCHK(a, hipStreamSynchronize(a->stream));
    HIPCHK(b, hipStreamSynchronize(b->stream));
    std::swap(a->arena_mem, b->arena_mem);
    std::swap(a->arena.base, b->arena.base);
    a->held.pmask_valid = b->held.pmask_valid = false;   // (the wave words describe the planes of the arena a context steps on)
    return RH_OK;
}

int rh_selftest_pow(const double *x, const double *y, double *out, int64_t n) {
    if (!x || !y || !out || n <= 0) return RH_ERR_ARG;
    double *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)n * 3 * sizeof(double)) != hipSuccess) return RH_ERR_HIP;
    int rc = RH_OK;
    if (hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = RH_ERR_HIP;
    if (rc == RH_OK) {
        hipLaunchKernelGGL(k_selftest_rh_pow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, d + n, d + 2 * n, n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = RH_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
}

int rh_selftest_window_sum(const double *v144, const int64_t *itd, int64_t n, double *out2n) {
    if (!v144 || !itd || !out2n || n <= 0) return RH_ERR_ARG;
    char *d = nullptr;
    const size_t bv = RH_SLOTS_PER_DAY * sizeof(double), bi = (size_t)n * sizeof(int64_t), bo = (size_t)n * 2 * sizeof(double);
    if (hipMalloc((void **)&d, bv + bi + bo) != hipSuccess) return RH_ERR_HIP;
    int rc = RH_OK;
    if (hipMemcpy(d, v144, bv, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + bv, itd, bi, hipMemcpyHostToDevice) != hipSuccess) rc = RH_ERR_HIP;
    if (rc == RH_OK) {
        hipLaunchKernelGGL(k_selftest_window, dim3((unsigned)n), dim3(64), 0, 0, (const double *)d, (const int64_t *)(d + bv), (double *)(d + bv + bi));
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out2n, d + bv + bi, bo, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RH_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
}

int rh_placement_report(const rh_ctx *ctx, double *ms, int cap) {
    if (!ctx) return 0;
    const int n = (int)ctx->probe_ms.size();
    for (int k = 0; k < n && k < cap && ms; ++k) ms[k] = ctx->probe_ms[k];
    return n;
}

// planes NO variant of the fused step reads (the sparse kernels additionally leave out the state the next lazy step derives itself:
// RH_LAZY_DERIVED_FIELDS, which the eager kernel still loads)
int rh_plane_is_pure_output(int model, int plane) {
    static const std::vector<unsigned char> tab[2] = {
        [] { std::vector<unsigned char> t(RH_NPLANES, 0);
#define RH_MARK(name) t[RH_P_##name] = 1;
             RH_NEVER_READ_FIELDS_SVAT(RH_MARK) return t; }(),
        [] { std::vector<unsigned char> t(RH_NPLANES, 0);
             RH_NEVER_READ_FIELDS_ONED(RH_MARK)
#undef RH_MARK
             return t; }()};
    if (plane < 0 || plane >= RH_NPLANES || model < 0 || model > 2) return -1;
    return model == 2 ? pure_output_planes()[2][plane] : tab[model][plane];
}
int64_t rh_sparse_steps(const rh_ctx *ctx) { return ctx ? ctx->call_sparse_steps : 0; }
int rh_param_stats(rh_ctx *ctx, double *derived_fraction, double *uniform_bytes_per_cell) {
    if (!ctx || !derived_fraction || !uniform_bytes_per_cell) return ctx ? fail(ctx, RH_ERR_ARG, "rh_param_stats: null pointer") : RH_ERR_ARG;
    if (int rc = form_param_mask(ctx, dim3(grid_for(ctx->n)))) return rc;
    const size_t words = ((size_t)ctx->n + 63) / 64;
    std::vector<unsigned long long> w(words);
    HIPCHK(ctx, hipMemcpyAsync(w.data(), ctx->pmask_buf, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the parameter planes the step loads unless the month changes, by element size; the derived ones apart
    unsigned long long f64_bits = 0, i32_bits = 0, derived_bits = 0;
#define RH_PB(name, bit) const unsigned long long pbit_##name = 1ull << bit;
    RH_PARAM_BITS(RH_PB)
#undef RH_PB
#define RH_PL(name) (PLANE_IS_INT[RH_P_##name] ? i32_bits : f64_bits) |= pbit_##name;
    if (ctx->cfg.enable_lateral_flow) { RH_PARAM_LOADED_ONED(RH_PL) } else { RH_PARAM_LOADED_SVAT(RH_PL) }
#undef RH_PL
#define RH_PD(name) derived_bits |= pbit_##name;
    RH_DERIVED_FIELDS(RH_PD)
#undef RH_PD
    double derived = 0, bytes = 0;
    for (size_t k = 0; k < words; ++k) {
        const bool der = (w[k] >> 63) & 1ull;
        derived += der ? 1 : 0;
        const unsigned long long u = w[k] & (der ? ~derived_bits : ~0ull);   // (a derived plane is not loaded at all)
        bytes += 8.0 * __builtin_popcountll(u & f64_bits) + 4.0 * __builtin_popcountll(u & i32_bits);
    }
    *derived_fraction = derived / (double)words;
    *uniform_bytes_per_cell = bytes / (double)words;
    return RH_OK;
}
int rh_step_mode(const rh_ctx *ctx) {
    if (!ctx) return 0;
    return (ctx->held.m1_stale ? RH_STEP_MODE_LAZY : 0) | (ctx->held.pending_valid ? RH_STEP_MODE_TAIL : 0) | (ctx->held.last_sparse ? RH_STEP_MODE_SPARSE : 0);
}

void *rh_predicate_words(rh_ctx *ctx) { return ctx ? (void *)ctx->dev->words : nullptr; }

int rh_enable_timing(rh_ctx *ctx, int on) {
    if (!ctx) return RH_ERR_ARG;
    ctx->timing = on != 0;
    ctx->events.restart();
    control_inputs_changed(ctx);   // the step log restarts: the next step's entry must be written after this call
    if (on) HIPCHK(ctx, ctx->dt_log_buf.alloc_once(sizeof(int) * RH_DT_LOG_CAP));
    int *log = on ? ctx->dt_log_buf.get() : nullptr;
    const int cap = RH_DT_LOG_CAP, zero = 0;
    HIPCHK(ctx, dev_put(ctx, &DevState::dt_log, log));
    HIPCHK(ctx, dev_put(ctx, &DevState::dt_log_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::dt_log_n, zero));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_timing_detail(rh_ctx *ctx, double *kernel_ms, int32_t *dt_secs, int64_t cap, int64_t *launches) {
    if (!ctx || !kernel_ms || !dt_secs || !launches || cap < 0) return RH_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int logged = 0;
    if (ctx->dt_log_buf) HIPCHK(ctx, hipMemcpy(&logged, &ctx->dev->dt_log_n, sizeof(int), hipMemcpyDeviceToHost));
    const int64_t n = (int64_t)ctx->events.launches();
    // (the tail of the last timed kernel has logged the step after it already: one entry more than launches)
    if ((logged != n && logged != n + 1) || n > RH_DT_LOG_CAP)
        return fail(ctx, RH_ERR_STATE, "rh_timing_detail: the step log does not match the timed launches (timing enabled mid-step, "
                                       "or more than 65536 steps)");
    *launches = n;
    const int64_t m = n < cap ? n : cap;
    for (int64_t k = 0; k < m; ++k) {
        float ms = 0;
        HIPCHK(ctx, ctx->events.elapsed_ms((size_t)k, &ms));
        kernel_ms[k] = ms;
    }
    if (m) HIPCHK(ctx, hipMemcpy(dt_secs, ctx->dt_log_buf, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    return RH_OK;
}
int rh_timing_summary(rh_ctx *ctx, double *total_ms, int64_t *launches) {
    if (!ctx || !total_ms || !launches) return RH_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, ctx->events.total_ms(total_ms));
    *launches = (int64_t)ctx->events.launches();
    return RH_OK;
}
