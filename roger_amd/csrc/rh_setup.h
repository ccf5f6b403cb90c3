// rh_setup.h -- a context created and destroyed, the plane registry, planes / scalars / look-up tables between host and device.
// Part of the one translation unit roger_hip.hip, behind rh_context.h and rh_rccl.h.
#pragma once
int rh_abi_version(void) { return RH_ABI_VERSION; }

void rh_default_config(rh_config *cfg) {
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->nx = cfg->ny = 1;
    // roger/settings.py:52-122
    cfg->pi = 3.14159265358979323846264338327950588;
    cfg->r_mp = 2.5;
    cfg->l_sc = 10000;
    cfg->sf = 3;
    cfg->ta_fm = 0;
    cfg->rmax = 30;
    cfg->transp_water_stress = 0.75;
    cfg->atol = 1e-2;
    cfg->rtol = 1e-2;
    cfg->clay_min = 0.01;
    cfg->clay_max = 0.71;
    cfg->theta_rew_min = 0.02;
    cfg->theta_rew_max = 0.24;
    cfg->rew_min = 2;
    cfg->rew_max = 12;
    cfg->z_evap_max = 150;
    cfg->zroot_to_zsoil_max = 0.7;
    cfg->a_bc = 2;
    cfg->b_bc = 2;
    cfg->end_event = 21600;
    cfg->hpi = 5;
    cfg->dx = 1;
    cfg->enable_lateral_flow = 0;
    cfg->enable_routing_1D = 0;
    cfg->dy = 1.0;
    cfg->placement_probes = 8;   // up to eight candidate arenas, never more than a quarter of the free memory held at once (1 or RH_PLACEMENT_PROBES=1: none)
}

const char *rh_last_error(const rh_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }
int rh_num_planes(void) { return RH_NPLANES; }
int rh_planes_held(const rh_ctx *ctx) { return ctx ? ctx->planes_held : 0; }
const char *rh_plane_name(int p) { return (p >= 0 && p < RH_NPLANES) ? PLANE_NAMES[p] : nullptr; }
int rh_plane_is_int(int p) { return (p >= 0 && p < RH_NPLANES) ? PLANE_IS_INT[p] : -1; }
int rh_plane_index(const char *name) {
    if (!name) return -1;
    for (int p = 0; p < RH_NPLANES; ++p)
        if (!std::strcmp(PLANE_NAMES[p], name)) return p;
    return -1;
}
int64_t rh_num_cells(const rh_ctx *ctx) { return ctx ? ctx->n : 0; }

int rh_create(const rh_config *cfg, rh_ctx **out) {
    if (!cfg || !out) return fail(nullptr, RH_ERR_ARG, "rh_create: null argument");
    if (cfg->nx <= 0 || cfg->ny <= 0) return fail(nullptr, RH_ERR_ARG, "rh_create: nx and ny must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RH_ERR_NODEVICE, "rh_create: no HIP device visible (this backend has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, RH_ERR_ARG, "rh_create: device ordinal out of range");
    HIPCHK(nullptr, hipSetDevice(cfg->device));
    rh_ctx *ctx = new (std::nothrow) rh_ctx();
    if (!ctx) return fail(nullptr, RH_ERR_ARG, "rh_create: out of host memory");
    ctx->cfg = *cfg;
    ctx->n = cfg->nx * cfg->ny;
    ctx->sw = read_switches(*cfg);
    const size_t n_tiles = ((size_t)ctx->n + RH_TILE_CELLS - 1) / RH_TILE_CELLS;
    ctx->planes_held = cfg->enable_routing_1D ? (int)RH_NPLANES : (int)RH_P_flow_dir_topo;
    const size_t stride = (size_t)(ctx->planes_held + RH_STRIDE_PAD) * RH_SLOT_BYTES, arena_bytes = n_tiles * stride;
    ctx->arena.stride = stride;
    ctx->arena.n = ctx->n;
    if (cfg->enable_routing_1D && !cfg->enable_lateral_flow) {
        delete ctx;
        return fail(nullptr, RH_ERR_ARG, "rh_create: enable_routing_1D needs enable_lateral_flow (the routed subsurface runoff is the lateral flow)");
    }
    auto bail = [&](hipError_t e, const char *what) {
        std::string msg = std::string(what) + ": " + hipGetErrorString(e);
        rh_destroy(ctx);
        return fail(nullptr, RH_ERR_HIP, msg);
    };
    hipError_t e;
    if ((e = ctx->stream.create()) != hipSuccess) return bail(e, "hipStreamCreate");
    {
        // Placement probing (rh_config.placement_probes): candidates are allocated one after the other and held until
        // the choice is made, so that each lands somewhere else; a copy of 96 planes with the fused kernel's access
        // shape (k_calib_copy) is timed on each (its time tracks the fused kernel's level, tools/placement_diag3.py).
        int probes = ctx->sw.placement_probes;
        if (probes < 1 || ctx->n < 65536) probes = 1;   // small grids are latency-bound
        std::vector<DevBuf<char>> cand;   // (the ones that are not chosen are released at the end of this block)
        std::vector<double> cand_ms;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if (probes > 1 && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) probes = 1;
        for (int k = 0; k < probes; ++k) {
            if (k > 0) {   // all candidates are held until the choice is made: never more than a quarter of the free memory in total
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) != hipSuccess ||
                    (free_b + k * arena_bytes) / 4 < (k + 1) * arena_bytes) break;
            }
            DevBuf<char> p;
            if ((e = p.alloc(arena_bytes)) != hipSuccess) {
                if (k == 0) return bail(e, "hipMalloc(arena)");
                (void)hipGetLastError();
                break;
            }
            cand.push_back(std::move(p));
            if ((e = hipMemsetAsync(cand.back(), 0, arena_bytes, ctx->stream)) != hipSuccess) {
                cand.clear();
                return bail(e, "hipMemset");
            }
            double ms = 0;
            if (probes > 1) {
                Arena probe = ctx->arena;
                probe.base = cand.back();
                float best = 1e30f;
                for (int rep = 0; rep < 4; ++rep) {   // the first repetition warms up
                    (void)hipEventRecord(ev0, ctx->stream);
                    hipLaunchKernelGGL(k_calib_copy, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, probe, 0, 100, 96);
                    (void)hipEventRecord(ev1, ctx->stream);
                    (void)hipEventSynchronize(ev1);
                    float t = 0;
                    if (rep > 0 && hipEventElapsedTime(&t, ev0, ev1) == hipSuccess && t < best) best = t;
                }
                ms = best;
            }
            cand_ms.push_back(ms);
        }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        size_t pick = 0;
        for (size_t k = 1; k < cand.size(); ++k)
            if (cand_ms[k] < cand_ms[pick]) pick = k;
        ctx->arena_mem = std::move(cand[pick]);
        ctx->arena.base = ctx->arena_mem;
        if (probes > 1) {
            ctx->probe_ms.push_back(cand_ms[pick]);
            for (size_t k = 0; k < cand.size(); ++k)
                if (k != pick) ctx->probe_ms.push_back(cand_ms[k]);
        }
    }
    if ((e = ctx->stage_buf.alloc((size_t)ctx->n * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(staging plane)");
    if ((e = ctx->dev.alloc(sizeof(DevState))) != hipSuccess) return bail(e, "hipMalloc(DevState)");
    if ((e = ctx->hexp.alloc()) != hipSuccess) return bail(e, "hipHostMalloc(scalar export block)");
    if ((e = hipMemsetAsync(ctx->dev, 0, sizeof(DevState), ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
    {   // the parameter words of the fused step's wavefronts (all zero: plain loads; AFTER the control block was cleared) and their address in the control block
        const size_t words = ((size_t)ctx->n + 63) / 64;
        if ((e = ctx->pmask_buf.alloc(words * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc(parameter words)");
        if ((e = hipMemsetAsync(ctx->pmask_buf, 0, words * sizeof(unsigned long long), ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
        if ((e = dev_put(ctx, &DevState::pmask, *ctx->pmask_buf.addr())) != hipSuccess) return bail(e, "hipMemcpy(pmask)");
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    }
    {
        static const long long no_limit = -1;
        if ((e = dev_put(ctx, &DevState::t_end, no_limit)) != hipSuccess) return bail(e, "hipMemcpy(t_end)");
    }
    Consts K;
    K.pi = cfg->pi; K.r_mp = cfg->r_mp; K.l_sc = cfg->l_sc; K.sf = cfg->sf; K.ta_fm = cfg->ta_fm; K.rmax = cfg->rmax;
    K.transp_water_stress = cfg->transp_water_stress; K.atol = cfg->atol; K.rtol = cfg->rtol;
    K.clay_min = cfg->clay_min; K.clay_max = cfg->clay_max; K.theta_rew_min = cfg->theta_rew_min;
    K.theta_rew_max = cfg->theta_rew_max; K.rew_min = cfg->rew_min; K.rew_max = cfg->rew_max;
    K.z_evap_max = cfg->z_evap_max; K.zroot_to_zsoil_max = cfg->zroot_to_zsoil_max; K.a_bc = cfg->a_bc; K.b_bc = cfg->b_bc;
    K.end_event = cfg->end_event; K.hpi = cfg->hpi;
    K.dx = cfg->dx; K.lateral = cfg->enable_lateral_flow ? 1 : 0;
    K.dy = cfg->dy; K.routing = cfg->enable_routing_1D ? 1 : 0;
    if ((e = dev_put(ctx, &DevState::K, K)) != hipSuccess) return bail(e, "hipMemcpy(Consts)");
    // scalars: roger/variables.py initial values (dt=1, dt_secs=3600, event_id_counter=1, year=1900, month=doy=1)
    rh_scalars S;
    std::memset(&S, 0, sizeof(S));
    S.dt = 1;
    S.dt_secs = 3600;
    S.event_id_counter = 1;
    S.year[0] = S.year[1] = 1900;
    S.month[0] = S.month[1] = 1;
    S.doy[0] = S.doy[1] = 1;
    S.sanity_ok = 1;
    if ((e = dev_put(ctx, &DevState::S, S)) != hipSuccess) return bail(e, "hipMemcpy(scalars)");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");  // K, S are stack locals
    ctx->n_groups = (int)((grid_for(ctx->n) + 63) / 64);
    if (ctx->n_groups > RH_DONE_GROUPS) ctx->n_groups = RH_DONE_GROUPS;
    if (ctx->n_groups < 1) ctx->n_groups = 1;
    ctx->pred_blocks = (int)(grid_for(ctx->n) < RH_PRED_BLOCKS ? grid_for(ctx->n) : RH_PRED_BLOCKS);
    if ((e = dev_put(ctx, &DevState::pred_blocks, ctx->pred_blocks)) != hipSuccess) return bail(e, "hipMemcpy(pred_blocks)");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    hipLaunchKernelGGL(k_init_registry, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena);
    hipLaunchKernelGGL(k_sync_ctx, dim3(1), dim3(1), 0, ctx->stream, ctx->dev);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e, "kernel launch (is this a gfx950 device?)");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    *out = ctx;
    return RH_OK;
}

void rh_destroy(rh_ctx *ctx) {
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
#ifdef RH_STEP_PHASES
    {
        unsigned long long tp[8];
        if (hipMemcpyFromSymbol(tp, HIP_SYMBOL(g_tail_phases), sizeof(tp)) == hipSuccess && tp[7])
            std::fprintf(stderr, "tail phases: %llu tails, cycles per tail: loads %.0f, hooks+staging %.0f, bits+sums %.0f, decisions %.0f, scalars %.0f, log %.0f; whole tail %.0f\n",
                         tp[7], (double)tp[0] / tp[7], (double)tp[1] / tp[7], (double)tp[2] / tp[7], (double)tp[3] / tp[7], (double)tp[4] / tp[7],
                         (double)tp[5] / tp[7], (double)tp[6] / tp[7]);
        static unsigned long long all[256 * 64];
        unsigned long long h[60] = {0};
        if (hipMemcpyFromSymbol(all, HIP_SYMBOL(g_step_phases), sizeof(all)) == hipSuccess) {
            for (int b = 0; b < 256; ++b)
                for (int k = 0; k < 60; ++k) h[k] += all[b * 64 + k];
            static const char *cls[3] = {"10min", "hourly", "daily"};
            for (int c = 0; c < 3; ++c) {
                if (!h[c * 20 + 19]) continue;
                double tot = 0;
                for (int k = 0; k < 19; ++k) tot += (double)h[c * 20 + k];
                std::fprintf(stderr, "step phases %s: %llu waves, cycles per wave %.0f:", cls[c], h[c * 20 + 19], tot / (double)h[c * 20 + 19]);
                for (int k = 1; k <= 14; ++k) std::fprintf(stderr, " %d:%.1f%%", k, 100.0 * (double)h[c * 20 + k] / tot);
                std::fprintf(stderr, "\n");
            }
        }
    }
#endif
    release_comm(ctx);
    delete ctx;
}

int rh_set_stream(rh_ctx *ctx, void *hip_stream) {
    if (!ctx) return RH_ERR_ARG;
    HIPCHK(ctx, ctx->stream.adopt((hipStream_t)hip_stream));
    return RH_OK;
}

static int device_error(rh_ctx *ctx, unsigned err) {
    if (err & RH_DEVERR_FORCING)
        return fail(ctx, RH_ERR_STATE, "a step began a day beyond the end of the resident forcing series (rh_set_forcing_series): it ran on the "
                                       "previous day's forcing; hand over a longer series (the reference fails on the short slice, "
                                       "benchmarks/SVAT_benchmark.py:151-171)");
    return RH_OK;
}
int rh_sync(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    unsigned err = 0;
    HIPCHK(ctx, hipMemcpyAsync(&err, &ctx->dev->err_flags, sizeof(err), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return device_error(ctx, err);
}

static int plane_bytes(rh_ctx *ctx, int plane, size_t bytes, size_t *elem) {
    if (!ctx) return RH_ERR_ARG;
    if (plane < 0 || plane >= RH_NPLANES) return fail(ctx, RH_ERR_ARG, "unknown plane id");
    if (plane >= ctx->planes_held)
        return fail(ctx, RH_ERR_STATE, std::string("plane ") + PLANE_NAMES[plane] + " belongs to the routing: the context was created without enable_routing_1D");
    *elem = PLANE_IS_INT[plane] ? sizeof(int32_t) : sizeof(double);
    if (bytes != *elem * (size_t)ctx->n)
        return fail(ctx, RH_ERR_ARG, std::string("size mismatch for plane ") + PLANE_NAMES[plane]);
    return RH_OK;
}

int rh_upload(rh_ctx *ctx, int plane, const void *host, size_t bytes) {
    size_t elem;
    int rc = plane_bytes(ctx, plane, bytes, &elem);
    if (rc) return rc;
    if (!host) return fail(ctx, RH_ERR_ARG, "rh_upload: null host pointer");
    planes_touched(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->stage_buf, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (elem == sizeof(double))
        hipLaunchKernelGGL(k_plane_scatter<double>, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, plane, (const double *)ctx->stage_buf.get());
    else
        hipLaunchKernelGGL(k_plane_scatter<int>, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, plane, (const int *)ctx->stage_buf.get());
    CHECK_LAUNCH(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the host buffer may be a temporary
    return RH_OK;
}

int rh_download(rh_ctx *ctx, int plane, void *host, size_t bytes) {
    size_t elem;
    int rc = plane_bytes(ctx, plane, bytes, &elem);
    if (rc) return rc;
    if (!host) return fail(ctx, RH_ERR_ARG, "rh_download: null host pointer");
    if (plane_is_stale(ctx, plane))   // only after an rh_run_steps call that failed half-way
        return fail(ctx, RH_ERR_STATE, "rh_download: the last rh_run_steps call ended before its final step; this flux / diagnostic plane holds an "
                                       "earlier step's values (run one more step)");
    materialise_m1(ctx);
    if (elem == sizeof(double))
        hipLaunchKernelGGL(k_plane_gather<double>, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, plane, (double *)ctx->stage_buf.get());
    else
        hipLaunchKernelGGL(k_plane_gather<int>, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, plane, (int *)ctx->stage_buf.get());
    CHECK_LAUNCH(ctx);
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->stage_buf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

void *rh_plane_device_ptr(rh_ctx *ctx, int plane) {
    if (!ctx || plane < 0 || plane >= ctx->planes_held) return nullptr;
    if (plane_is_stale(ctx, plane)) {
        // (as rh_download: only after a stepping call that ended before its final, full-store step -- ADVICE r3)
        fail(ctx, RH_ERR_STATE, "rh_plane_device_ptr: the last rh_run_steps call ended before its final step; this plane holds an earlier step's values");
        return nullptr;
    }
    planes_touched(ctx);  // the caller may write through the pointer
    return ctx->arena.base + (size_t)plane * RH_SLOT_BYTES;   // cell i: + (i / 64) * tile_bytes + (i % 64) * element size
}

int rh_set_scalars(rh_ctx *ctx, const rh_scalars *s) {
    if (!ctx || !s) return RH_ERR_ARG;
    control_inputs_changed(ctx);
    HIPCHK(ctx, dev_zero(ctx, &DevState::err_flags));
    HIPCHK(ctx, dev_put(ctx, &DevState::S, *s));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    LAUNCH_ONE(ctx, k_sync_ctx, ctx->dev);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// Enqueue the export of the scalars behind whatever is on the stream and wait for it: the host spins on the block's sequence number
// (the write arrives a few microseconds after the kernel in front has finished; hipStreamSynchronize wakes up later) and looks at the
// stream from time to time, so that a launch that failed ends the wait with its error instead of hanging.
static int export_scalars(rh_ctx *ctx, rh_scalars *s) {
    const unsigned long long seq = ++ctx->hexp_seq;
    hipLaunchKernelGGL(k_export, dim3(1), dim3(1), 0, ctx->stream, (const DevState *)ctx->dev, ctx->hexp.get(), seq);
    CHECK_LAUNCH(ctx);
    const unsigned long long *p = &ctx->hexp->seq;
    for (unsigned long spins = 1;; ++spins) {
        if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) break;
        if ((spins & 0xfffful) == 0) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) break;
                return fail(ctx, RH_ERR_HIP, "the scalar export kernel finished without its block arriving in host memory");
            }
            if (q != hipErrorNotReady) HIPCHK(ctx, q);
        }
    }
    const HostExport &H = *ctx->hexp.get();
    *s = H.S;
    // word 2 collects the sanity violations of the last step; the fused kernel's tail moves it to sanity_last
    s->sanity_ok = (H.bad | H.bad_last) ? 0 : 1;
    return device_error(ctx, H.err);
}

int rh_get_scalars(rh_ctx *ctx, rh_scalars *s) {
    if (!ctx || !s) return RH_ERR_ARG;
    return export_scalars(ctx, s);
}

int rh_set_luts(rh_ctx *ctx, const double *ilu, const double *gc, const double *gcm, const double *rdlu) {
    if (!ctx || !ilu || !gc || !gcm || !rdlu) return RH_ERR_ARG;
    HIPCHK(ctx, hipMemcpyAsync(ctx->dev->L.ilu, ilu, sizeof(double) * 25 * 13, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dev->L.gc, gc, sizeof(double) * 25 * 13, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dev->L.gcm, gcm, sizeof(double) * 25 * 2, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dev->L.rdlu, rdlu, sizeof(double) * 25 * 7, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

int rh_set_lut_mlms(rh_ctx *ctx, const double *mlms, int64_t nrows) {
    if (!ctx || !mlms || nrows <= 0) return RH_ERR_ARG;
    const size_t nb = sizeof(double) * 9 * (size_t)nrows;
    HIPCHK(ctx, ctx->mlms_buf.alloc(nb));
    HIPCHK(ctx, hipMemcpyAsync(ctx->mlms_buf, mlms, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, dev_put(ctx, &DevState::mlms, *ctx->mlms_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::mlms_rows, nrows));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

int rh_params_lateral(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->mlms_buf) return fail(ctx, RH_ERR_STATE, "rh_set_lut_mlms must be called first");
    HIPCHK(ctx, dev_zero(ctx, &DevState::max_slope_per));
    LAUNCH_CELLS(ctx, k_max_slope);
    LAUNCH_CELLS(ctx, k_params_lateral);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
