// rh_forcing.h -- the four ways of setting forcing: one day, the resident series, station series, per-cell weights.
// Part of the one translation unit roger_hip.hip, behind rh_context.h.
#pragma once
int rh_set_forcing_day(rh_ctx *ctx, const double *prec_day, const double *ta_day, const double *pet_day, int per_cell) {
    if (!ctx || !prec_day || !ta_day || !pet_day) return RH_ERR_ARG;
    const double *src[3] = {prec_day, ta_day, pet_day};
    const int pc = per_cell ? 1 : 0;
    const double *cell[3];
    if (!pc) {
        for (int k = 0; k < 3; ++k)
            HIPCHK(ctx, hipMemcpyAsync(ctx->dev->forc[k], src[k], sizeof(double) * RH_SLOTS_PER_DAY, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, dev_zero(ctx, &DevState::day_cache_ok));   // (ctrl_wave's cache of the day)
    } else {
        const size_t bytes = sizeof(double) * RH_SLOTS_PER_DAY * (size_t)ctx->n;
        HIPCHK(ctx, ctx->transpose_buf.alloc_once(bytes));
        for (int k = 0; k < 3; ++k) {   // (n, 144) from the host -> (144, n) on the device
            HIPCHK(ctx, ctx->forc_cell_buf[k].alloc_once(bytes));
            cell[k] = ctx->forc_cell_buf[k];
            HIPCHK(ctx, hipMemcpyAsync(ctx->transpose_buf, src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_transpose_forcing, dim3((unsigned)((ctx->n + 63) / 64), (RH_SLOTS_PER_DAY + 63) / 64), dim3(RH_BLOCK), 0, ctx->stream,
                               (const double *)ctx->transpose_buf, ctx->forc_cell_buf[k].get(), ctx->n);
            CHECK_LAUNCH(ctx);
        }
        HIPCHK(ctx, dev_put(ctx, &DevState::forc_cell, cell));
        if (int rc = need_agg_cell_buf(ctx)) return rc;
    }
    ctx->per_cell = pc != 0;
    control_inputs_changed(ctx);
    HIPCHK(ctx, dev_put(ctx, &DevState::per_cell, pc));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->forcing_set = true;
    return RH_OK;
}

// The resident series -- (stations, nitt_forc) per variable, then the three calendar vectors -- and their addresses in the control
// block; n_stations = 0: one series for all columns.  Synchronises (the address tables are stack locals).
static int upload_series(rh_ctx *ctx, const double *prec, const double *ta, const double *pet, const int64_t *year, const int64_t *month,
                         const int64_t *doy, int64_t nitt_forc, int n_stations) {
    const size_t nb1 = sizeof(double) * (size_t)nitt_forc, nbS = nb1 * (size_t)(n_stations ? n_stations : 1);
    HIPCHK(ctx, ctx->series_buf.alloc(3 * nbS + 3 * nb1));
    char *base = ctx->series_buf;
    const void *fsrc[3] = {prec, ta, pet}, *csrc[3] = {year, month, doy};
    for (int k = 0; k < 3; ++k) HIPCHK(ctx, hipMemcpyAsync(base + k * nbS, fsrc[k], nbS, hipMemcpyHostToDevice, ctx->stream));
    for (int k = 0; k < 3; ++k) HIPCHK(ctx, hipMemcpyAsync(base + 3 * nbS + k * nb1, csrc[k], nb1, hipMemcpyHostToDevice, ctx->stream));
    const double *sp[3] = {(double *)base, (double *)(base + nbS), (double *)(base + 2 * nbS)};
    const int64_t *cp[3] = {(int64_t *)(base + 3 * nbS), (int64_t *)(base + 3 * nbS + nb1), (int64_t *)(base + 3 * nbS + 2 * nb1)};
    HIPCHK(ctx, dev_put(ctx, &DevState::series, sp));
    HIPCHK(ctx, dev_put(ctx, &DevState::calendar, cp));
    HIPCHK(ctx, dev_put(ctx, &DevState::nitt_forc, nitt_forc));
    HIPCHK(ctx, dev_put(ctx, &DevState::n_stations, n_stations));
    HIPCHK(ctx, dev_zero(ctx, &DevState::err_flags));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

int rh_set_forcing_series(rh_ctx *ctx, const double *prec, const double *ta, const double *pet, const int64_t *year,
                          const int64_t *month, const int64_t *doy, int64_t nitt_forc) {
    if (!ctx || !prec || !ta || !pet || !year || !month || !doy || nitt_forc <= 0) return RH_ERR_ARG;
    if (int rc = upload_series(ctx, prec, ta, pet, year, month, doy, nitt_forc, 0)) return rc;
    ctx->forcing_set = true;
    control_inputs_changed(ctx);
    ctx->per_cell = false;
    return RH_OK;
}

int rh_set_forcing_stations(rh_ctx *ctx, const double *prec, const double *ta, const double *pet, const int64_t *year, const int64_t *month,
                            const int64_t *doy, int64_t nitt_forc, int n_stations, const int32_t *station_index) {
    if (!ctx || !prec || !ta || !pet || !year || !month || !doy || !station_index || nitt_forc <= 0 || n_stations < 1)
        return ctx ? fail(ctx, RH_ERR_ARG, "rh_set_forcing_stations: bad arguments") : RH_ERR_ARG;
    if (n_stations > 4096) return fail(ctx, RH_ERR_ARG, "rh_set_forcing_stations: at most 4096 stations");
    if (int rc = upload_series(ctx, prec, ta, pet, year, month, doy, nitt_forc, n_stations)) return rc;
    // the station of every column, the staging table of a day
    HIPCHK(ctx, ctx->station_buf.alloc_once(sizeof(int) * (size_t)ctx->n));
    HIPCHK(ctx, hipMemcpyAsync(ctx->station_buf, station_index, sizeof(int) * (size_t)ctx->n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, ctx->forc_multi_buf.alloc(sizeof(double) * 3 * (size_t)n_stations * RH_SLOTS_PER_DAY));
    HIPCHK(ctx, dev_put(ctx, &DevState::station_idx, *ctx->station_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::forc_multi, *ctx->forc_multi_buf.addr()));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->forcing_set = true;
    control_inputs_changed(ctx);
    // the station series reach the columns through the per-cell (weighted) path: neutral weights unless the caller sets some
    if (!ctx->weight_buf[0]) {
        std::vector<double> one((size_t)ctx->n, 1.0), zero((size_t)ctx->n, 0.0);
        const int rc = rh_set_forcing_weights(ctx, one.data(), zero.data(), one.data());
        if (rc) return rc;
    }
    ctx->per_cell = true;
    cell_forcing_changed(ctx);
    return RH_OK;
}

int rh_set_forcing_weights(rh_ctx *ctx, const double *prec_weight, const double *ta_offset, const double *pet_weight) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->series_buf) return fail(ctx, RH_ERR_STATE, "rh_set_forcing_series must be called first");
    const double *src[3] = {prec_weight, ta_offset, pet_weight};
    const bool clear = !prec_weight && !ta_offset && !pet_weight;
    if (!clear && (!prec_weight || !ta_offset || !pet_weight)) return fail(ctx, RH_ERR_ARG, "rh_set_forcing_weights: give all three arrays or none");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t nb = sizeof(double) * (size_t)ctx->n;
    const double *dptr[3] = {nullptr, nullptr, nullptr};
    if (clear) {
        for (auto &b : ctx->weight_buf) HIPCHK(ctx, b.release());
    } else {
        for (int k = 0; k < 3; ++k) {
            HIPCHK(ctx, ctx->weight_buf[k].alloc_once(nb));
            HIPCHK(ctx, hipMemcpyAsync(ctx->weight_buf[k], src[k], nb, hipMemcpyHostToDevice, ctx->stream));
            dptr[k] = ctx->weight_buf[k];
        }
        if (int rc = need_agg_cell_buf(ctx)) return rc;
    }
    HIPCHK(ctx, dev_put(ctx, &DevState::weights, dptr));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    control_inputs_changed(ctx);
    ctx->per_cell = !clear;   // from the next midnight on; rh_set_forcing_weights is a setup-time call
    cell_forcing_changed(ctx);
    return RH_OK;
}
