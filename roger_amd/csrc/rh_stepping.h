// rh_stepping.h -- every way of stepping: routine by routine, the fused launch behind its fronts, the phase entries, the routed step,
// rh_run_steps / rh_run_steps_dist.  Part of the one translation unit roger_hip.hip, behind rh_observers.h and rh_routing_host.h.
#pragma once
// the next pair of timing events, if timing is on (rh_enable_timing; null otherwise): they ride on a kernel's own dispatch
// (hipExtLaunchKernelGGL).  The pool is reused by the next rh_enable_timing(1), never beyond the cap
static int timing_pair(rh_ctx *ctx, hipEvent_t *ev0, hipEvent_t *ev1) {
    if (!ctx->timing) return RH_OK;
    if (ctx->events.used + 2 > 2 * (size_t)RH_DT_LOG_CAP)
        return fail(ctx, RH_ERR_STATE, "timing: more than 65536 timed steps since rh_enable_timing(1); read the timings and enable again");
    HIPCHK(ctx, ctx->events.next_pair(ev0, ev1));
    return RH_OK;
}

#define SIMPLE_ENTRY(fname, kern)           \
    int fname(rh_ctx *ctx) {                \
        if (!ctx) return RH_ERR_ARG;        \
        LAUNCH_CELLS(ctx, kern);            \
        CHECK_LAUNCH(ctx);                  \
        return RH_OK;                       \
    }

SIMPLE_ENTRY(rh_topo, k_topo)
SIMPLE_ENTRY(rh_params_surface, k_params_surface)
SIMPLE_ENTRY(rh_params_soil, k_params_soil)
SIMPLE_ENTRY(rh_initial_conditions, k_initial_conditions)
SIMPLE_ENTRY(rh_interception, k_interception)
SIMPLE_ENTRY(rh_evapotranspiration, k_evapotranspiration)
SIMPLE_ENTRY(rh_snow, k_snow)
SIMPLE_ENTRY(rh_capillary_rise, k_capillary_rise)
SIMPLE_ENTRY(rh_storage, k_storage)

int rh_subsurface_runoff(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->cfg.enable_lateral_flow) LAUNCH_CELLS(ctx, k_subsurface_runoff_lateral);
    else LAUNCH_CELLS(ctx, k_subsurface_runoff);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

int rh_infiltration(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    LAUNCH_CELLS(ctx, k_inf_pred);
    LAUNCH_ONE(ctx, k_inf_conds, ctx->dev);
    if (ctx->cfg.enable_routing_1D) LAUNCH_CELLS(ctx, k_infiltration_routed);
    else LAUNCH_CELLS(ctx, k_infiltration);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// the sanity word of the step (words[2]) and what the last fused kernel's tail kept of it
static int reset_sanity(rh_ctx *ctx) {
    HIPCHK(ctx, hipMemsetAsync(&ctx->dev->words[2], 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, dev_zero(ctx, &DevState::sanity_last));
    return RH_OK;
}
int rh_num_error(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = reset_sanity(ctx)) return rc;
    if (ctx->cfg.enable_routing_1D) LAUNCH_CELLS(ctx, k_num_error_routed);
    else if (ctx->cfg.enable_lateral_flow) LAUNCH_CELLS(ctx, k_num_error_lateral);
    else LAUNCH_CELLS(ctx, k_num_error);
    LAUNCH_ONE(ctx, k_sanity_to_scalars, ctx->dev);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

int rh_after_timestep(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->cfg.enable_lateral_flow) LAUNCH_CELLS(ctx, k_after_timestep_oned);
    else LAUNCH_CELLS(ctx, k_after_timestep);
    LAUNCH_ONE(ctx, k_rotate_scalars, ctx->dev);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// 64 int32 all-reduced (max) over the context's communicator, from exch_buf[0..63] into exch_buf[64..127].  fill(send) enqueues whatever
// writes the send half (RH_OK, or an error code that ends the call); who: the caller's name in front of a missing RCCL's message.
template <class Fill>
static int allreduce_exch(rh_ctx *ctx, const char *who, Fill fill) {
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, std::string(who) + ": " + api->why);
    if (int rc = need_exch_buf(ctx)) return rc;
    int *send = ctx->exch_buf, *recv = ctx->exch_buf + 64;
    if (int rc = fill(send)) return rc;
    NCCLCHK(ctx, api->AllReduce(send, recv, 64, ncclInt32, ncclMax, ctx->comm, ctx->stream));
    return RH_OK;
}
// One whole step with the routing, routine by routine in the order of RogerSetup.step (roger/roger.py:396-457): the columns are
// coupled twice (after the infiltration and after the lateral flow), so the step is eleven per-column passes with two gathers in
// between instead of the fused kernel.  monthly: 1 / 0 = the caller's set_parameters decision, -1 = the device's (after the
// device-side set_forcing hook, rh_run_steps).  Several ranks: the two predicate words of the adaptive time stepping are all-reduced
// over the context's communicator (64 int32 each, as rh_run_steps_dist's summary word), the border cells go to the neighbours.
static int allreduce_word(rh_ctx *ctx, int word) {
    if (int rc = allreduce_exch(ctx, "rh_step_routed", [&](int *send) { return rh_predicates_expand(ctx, word, send); })) return rc;
    ctx->held.exch_valid = false;   // (the buffer holds a predicate word now)
    return rh_predicates_compress(ctx, word, ctx->exch_buf + 64);
}
// interception ... numerics, itt / time (what rh_step_core is for the uncoupled columns)
static int routed_core(rh_ctx *ctx, bool with_after) {
    int rc;
    if ((rc = reset_sanity(ctx))) return rc;
    {   // interception ... infiltration, the surface outflow: the longest of the three passes, the one rh_enable_timing times
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if ((rc = timing_pair(ctx, &ev0, &ev1))) return rc;
        planes_touched(ctx);
        hipExtLaunchKernelGGL(k_routed_a, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ev0, ev1, 0, ctx->arena, ctx->dev.get());
        if (ctx->timing) ctx->events.taken();
    }
    if (ctx->comm && ctx->comm_nranks > 1 && (rc = route_exchange(ctx, 0))) return rc;
    if ((rc = rh_route_gather_only(ctx, 0))) return rc;
    LAUNCH_CELLS(ctx, k_routed_b);                    // the surface inflow, the lateral subsurface runoff, its outflow
    if (ctx->comm && ctx->comm_nranks > 1 && (rc = route_exchange(ctx, 1))) return rc;
    if ((rc = rh_route_gather_only(ctx, 1))) return rc;
    // the subsurface inflow, capillary rise, storages, numerics [, after_timestep: the observers (accumulators, points) then read the taum1 planes
    // only for variables the rotation has just made equal to tau -- they accumulate tau values, kept by a separate pass otherwise]
    const bool fuse_after = with_after && !has_observers(ctx);
    if (fuse_after) LAUNCH_CELLS(ctx, k_routed_c_after);
    else LAUNCH_CELLS(ctx, k_routed_c);
    LAUNCH_ONE(ctx, k_sanity_to_scalars, ctx->dev);
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, ctx->stream, ctx->dev);
    if ((rc = launch_observers(ctx, 0))) return rc;
    if (with_after) {
        if (fuse_after) LAUNCH_ONE(ctx, k_rotate_scalars, ctx->dev);
        else if ((rc = rh_after_timestep(ctx))) return rc;
    }
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// interception ... numerics in one kernel, then itt/time (roger/roger.py:410-457); for drivers that
// keep the user hooks `set_parameters` and `after_timestep` on the host
int rh_step_core(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->cfg.enable_routing_1D) return routed_core(ctx, false);   // the columns are coupled: routine by routine with the two gathers
    if (ctx->cfg.enable_lateral_flow) LAUNCH_CELLS(ctx, k_core_staged_lateral);
    else LAUNCH_CELLS(ctx, k_core_staged);
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, ctx->stream, ctx->dev);
    // the observers follow every step, also in the hook-preserving flow (itt / time were just advanced)
    return launch_observers(ctx, 0);
}

// The k_step instantiation of a fused launch.  mode: set_parameters' monthly decision, 0 / 1 from the host, 2 on the device.  The tables name
// the library's 20 instantiations and no other (sparse stores: mode 2, lazy launches only) in the library's order: a feature before its absence.
using StepKernel = void (*)(Arena, DevState *, int, int, int *);
static StepKernel step_kernel(int mode, bool lateral, bool lazy, bool sparse, bool keep) {
#define RH_K4(M) {{k_step<M, true, true>, k_step<M, true, false>}, {k_step<M, false, true>, k_step<M, false, false>}}
    static const StepKernel sparse2[2][2] = {{k_step<2, true, true, true, true>, k_step<2, false, true, true, true>},   // [!keep][!lateral]
                                             {k_step<2, true, true, true>, k_step<2, false, true, true>}};
    static const StepKernel plain[3][2][2] = {RH_K4(2), RH_K4(1), RH_K4(0)};   // [2 - mode][!lateral][!lazy]
#undef RH_K4
    return sparse ? sparse2[!keep][!lateral] : plain[2 - mode][!lateral][!lazy];
}
static int launch_fused_kernel(rh_ctx *ctx, int monthly, int flags = 0, int *dst64 = nullptr) {
    // Timing: the event pair rides on the kernel's own dispatch (hipExtLaunchKernelGGL: start / stop are taken from the
    // dispatch's completion signal) instead of two hipEventRecord packets around it, which cost 5 us per step at 10^6
    // columns.
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (int rc = timing_pair(ctx, &ev0, &ev1)) return rc;
    // a launch whose tail forms the next step's control part gets one workgroup more: pre_tail
    if (flags & RH_TAIL_CTRL) flags |= RH_TAIL_PRE;
    const dim3 grid(grid_for(ctx->n) + ((flags & RH_TAIL_PRE) ? 1u : 0u)), block(RH_BLOCK);
    const bool lat = ctx->cfg.enable_lateral_flow != 0;
    // lazy rotation: the planes were last touched by a complete fused step (X_m1 == X) and nobody who reads X_m1 planes
    // follows inside this call (an observer kernel may, if it was given an X_m1 plane)
    const bool lazy = ctx->sw.lazy_ok && ctx->held.rot_consistent && !ctx->obs_reads_m1;
    // sparse stores: another step of the same rh_run_steps call follows and nothing in between reads what this one only produces
    const bool sparse = lazy && ctx->held.sparse_next && monthly < 0;   // (planes an observer reads are kept: DevState::keep, the KEEP variant)
    const bool keep = sparse && ctx->obs_reads_sparse;
    ctx->held.sparse_next = false;
    if (lazy)   // the lazy kernels read the parameter planes through the wave words
        if (int rc = form_param_mask(ctx, grid)) return rc;
    hipExtLaunchKernelGGL(step_kernel(monthly < 0 ? 2 : (monthly ? 1 : 0), lat, lazy, sparse, keep), grid, block, 0, ctx->stream, ev0, ev1, 0,
                          ctx->arena, ctx->dev.get(), flags, ctx->n_groups, dst64);   // (monthly < 0: decided on the device)
    CHECK_LAUNCH(ctx);
    if (ctx->timing) ctx->events.taken();
    fused_step_enqueued(ctx, flags, lazy, sparse, dst64 != nullptr);
    return launch_observers(ctx, 1, grid.x);
}

// the start-of-step predicates of the predicate-kernel front, with the day's forcing bits if they must be formed again
static void launch_pred1(rh_ctx *ctx) {
    hipLaunchKernelGGL(k_pred1, dim3(ctx->pred_blocks), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, ctx->held.pred_daily_stale ? 1 : 0);
    ctx->held.pred_daily_stale = false;
}
int rh_step_phase1(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = need_forcing(ctx)) return rc;
    planes_touched(ctx);
    front_takes_over(ctx, 1);
    launch_pred1(ctx);
    LAUNCH_WG(ctx, k_reduce, ctx->dev, 0);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
// per-cell forcing: the columns' aggregates of the step (k_cell_agg); does not touch the planes
static void launch_cell_agg(rh_ctx *ctx) {
    const dim3 grid(grid_for(ctx->n)), block(RH_BLOCK);
    const int force = ctx->held.agg_daily_stale ? 1 : 0;
    if (ctx->n >= ctx->sw.cell_agg_split_min) {
        hipLaunchKernelGGL(k_cell_agg<2>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force);
        hipLaunchKernelGGL(k_cell_agg<1>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force);
    } else
        hipLaunchKernelGGL(k_cell_agg<0>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force);
    ctx->held.agg_daily_stale = false;
}
int rh_step_phase2(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    LAUNCH_WG(ctx, k_agg, ctx->dev, 0, 0);
    if (ctx->per_cell) launch_cell_agg(ctx);   // (does not touch the planes: no LAUNCH_CELLS)
    LAUNCH_PRED(ctx, k_select);   // (k_select rewrites prec / ta: the summary word is not that of the planes any more)
    LAUNCH_WG(ctx, k_reduce, ctx->dev, 1);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
int rh_step_phase3(rh_ctx *ctx, int monthly) {
    if (!ctx) return RH_ERR_ARG;
    LAUNCH_WG(ctx, k_scalars, ctx->dev, 0, 1);
    return launch_fused_kernel(ctx, monthly);
}
// the summary bits of the columns as they are in the arena, into sumw
static int rebuild_summary_bits(rh_ctx *ctx) {
    HIPCHK(ctx, dev_zero(ctx, &DevState::sumw));
    LAUNCH_CELLS(ctx, k_summary);
    return RH_OK;
}
// Where the next control kernel finds the summary word of the columns as they are: RH_SRC_WORD3 if the last fused kernel left it in
// words[3], otherwise RH_SRC_SUMW, rebuilt from the arena here (or a negative error code).  stays_valid: only control kernels follow
// before the next look at it (the exchange paths); a fused launch that follows re-forms it anyway.
static int summary_from_arena(rh_ctx *ctx, bool stays_valid) {
    if (ctx->held.summary_valid) return RH_SRC_WORD3;
    if (int rc = rebuild_summary_bits(ctx)) return rc;
    ctx->held.summary_valid = stays_valid;
    return RH_SRC_SUMW;
}
// per-cell forcing, ONE per-column launch in front of the fused kernel (k_cell_front; a second one, returning at once unless a new day
// began, for the daily sums of large grids): the set_forcing hook rides along with it (fresh_day / front_ctrl)
static int launch_cell_front(rh_ctx *ctx, int hooks) {
    const dim3 grid(grid_for(ctx->n)), block(RH_BLOCK);
    const int force = ctx->held.front_daily_stale ? 1 : 0, m1 = ctx->held.m1_stale ? 1 : 0;
    if (ctx->n >= ctx->sw.cell_agg_split_min) {
        hipLaunchKernelGGL(k_cell_front<2>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
        hipLaunchKernelGGL(k_cell_front<0>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
    } else {
        hipLaunchKernelGGL(k_cell_front<1>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
    }
    CHECK_LAUNCH(ctx);
    ctx->held.front_daily_stale = false;
    return RH_OK;
}

static void launch_hooks(rh_ctx *ctx) {
    // the hook rewrites D->S (itt_forc, itt_day, the calendar), D->forc and D->monthly: a control part the previous fused kernel's
    // tail formed for the next step (S_next / X_next) was formed BEFORE this hook ran and must not be used
    control_inputs_changed(ctx, true);
    hipLaunchKernelGGL(k_set_forcing, dim3(1), dim3(RH_BLOCK), 0, ctx->stream, ctx->dev);
}
int rh_hooks_phase(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->series_buf) return fail(ctx, RH_ERR_STATE, "rh_set_forcing_series must be called first");
    launch_hooks(ctx);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// single GPU: the same step with the reductions folded into the single-workgroup kernels
static int step_fused_launches(rh_ctx *ctx, int monthly, int hooks) {
    if (ctx->cfg.enable_routing_1D)
        return fail(ctx, RH_ERR_STATE, "enable_routing_1D couples the columns twice per step: the fused step is not available, run the step "
                                       "routine by routine (rh_adaptive_dt ... rh_infiltration, rh_surface_routing, rh_subsurface_runoff, "
                                       "rh_subsurface_routing, ... rh_after_timestep)");
    if (int rc = need_forcing(ctx)) return rc;
    if (!ctx->per_cell) {
        // summary path: the previous fused kernel left what the predicates need; one control kernel, one fused kernel
        // ... unless the previous fused kernel's tail has formed this step's control part already (S_next / X_next)
        const bool use_next = ctx->held.pending_valid && ctx->held.pending_hooks == (hooks != 0);
        if (!use_next) {
            const int src = summary_from_arena(ctx, false);
            if (src < 0) return src;
            LAUNCH_ONE(ctx, k_ctrl, ctx->dev, hooks, src, (const int *)nullptr);
            CHECK_LAUNCH(ctx);
        }
        const int flags = (use_next ? RH_TAIL_USE_NEXT : 0) | (ctx->sw.tail_ok ? RH_TAIL_CTRL | (hooks ? RH_TAIL_HOOKS : 0) : 0);
        return launch_fused_kernel(ctx, monthly, flags);
    }
    const bool front = ctx->sw.cell_front_ok && ctx->n <= ctx->sw.cell_front_max;
    if (hooks && !front) {  // per-cell forcing from the resident series: the hooks must have formed it before k_pred1 reads it
        launch_hooks(ctx);
        hooks = 0;
    }
    int rc;
    if (front) {
        summary_path_left(ctx);
        front_takes_over(ctx, 2);
        if ((rc = launch_cell_front(ctx, hooks))) return rc;
        rc = launch_fused_kernel(ctx, monthly, RH_TAIL_SKIP);   // (the next front reads the planes, not the summary word)
    } else {
        front_takes_over(ctx, 1);
        // None of the kernels in front of the fused one writes a plane: the selected prec / ta are applied inside the fused kernel
        // (apply_sel = 2, from the per-cell aggregates), the predicate kernels read tau planes only -- with the rotation pending,
        // prec_m1 / swe_m1 are the tau planes themselves.  So the fused kernel keeps its lazy rotation in the per-cell path too.
        summary_path_left(ctx);
        launch_pred1(ctx);
        LAUNCH_WG(ctx, k_agg, ctx->dev, hooks, 1);
        if (ctx->per_cell) launch_cell_agg(ctx);
        const bool defer = ctx->per_cell && ctx->sw.defer_select_ok;   // (shared forcing on this path, e.g. before the series is resident: k_select stores)
        if (!defer) planes_touched(ctx);
        hipLaunchKernelGGL(k_select, dim3(ctx->pred_blocks), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev,
                           (ctx->held.m1_stale ? RH_SELECT_M1_PENDING : 0) | (defer ? RH_SELECT_DEFER : 0));
        LAUNCH_WG(ctx, k_scalars, ctx->dev, 1, 1, defer ? 2 : 0);
        rc = launch_fused_kernel(ctx, monthly);
    }
    return rc;
}
static int step_summary(rh_ctx *ctx, int32_t *dev_dst64) {
    if (!ctx) return RH_ERR_ARG;
    if (int rc = need_forcing(ctx)) return rc;
    if (ctx->per_cell) return fail(ctx, RH_ERR_STATE, "rh_step_summary: the summary path needs forcing shared by all columns; use rh_step_phase1/2/3");
    const int src = summary_from_arena(ctx, true);
    if (src < 0) return src;
    control_inputs_changed(ctx);   // the ranks decide together: the control kernel follows the exchange
    LAUNCH_WG(ctx, k_summary_reduce, ctx->dev, ctx->series_buf ? 1 : 0, (int *)dev_dst64, src);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
static int step_finish(rh_ctx *ctx, int monthly, const int32_t *dev_src64) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->per_cell) return fail(ctx, RH_ERR_STATE, "rh_step_finish: the summary path needs forcing shared by all columns");
    LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 0, RH_SRC_WORD3, (const int *)dev_src64);
    return launch_fused_kernel(ctx, monthly);
}
int rh_step_summary(rh_ctx *ctx) { return step_summary(ctx, nullptr); }
int rh_step_finish(rh_ctx *ctx, int monthly) { return step_finish(ctx, monthly, nullptr); }
int rh_step_summary_expand(rh_ctx *ctx, int32_t *dev_dst64) {
    if (!dev_dst64) return RH_ERR_ARG;
    return step_summary(ctx, dev_dst64);
}
int rh_step_finish_compress(rh_ctx *ctx, int monthly, const int32_t *dev_src64) {
    if (!dev_src64) return RH_ERR_ARG;
    return step_finish(ctx, monthly, dev_src64);
}
int rh_svat_step(rh_ctx *ctx, int monthly) {
    if (!ctx) return RH_ERR_ARG;
    return step_fused_launches(ctx, monthly, 0);
}
int rh_svat_step_scalars(rh_ctx *ctx, int monthly, rh_scalars *s) {
    if (!ctx || !s) return RH_ERR_ARG;
    if (int rc = step_fused_launches(ctx, monthly, 0)) return rc;
    return export_scalars(ctx, s);
}

// stand-alone adaptive time stepping: phases 1-2, the scalar kernel and the pet/ta selection
int rh_adaptive_dt(rh_ctx *ctx) {
    if (int rc = rh_step_phase1(ctx)) return rc;
    if (int rc = rh_step_phase2(ctx)) return rc;
    return rh_adaptive_dt_finish(ctx);
}

// the last part of rh_adaptive_dt on its own: with several ranks the two predicate words are exchanged between rh_step_phase1 /
// rh_step_phase2 and this call (adaptive_time_stepping_dist_safe.py:6-26 gathers 18 fields to rank 0 for the same decision)
int rh_adaptive_dt_finish(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    LAUNCH_WG(ctx, k_scalars, ctx->dev, 0, 0);
    LAUNCH_CELLS(ctx, k_select_pet);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// the three passes of the device-driven routed step with the two halo exchanges between them; SPARSE: sparse stores (never with observers)
template <bool SPARSE>
static int routed_passes(rh_ctx *ctx, bool ranks) {
    int rc;
    const dim3 grid(grid_for(ctx->n)), block(RH_BLOCK);
    const int nx = (int)ctx->cfg.nx, ny = (int)ctx->cfg.ny;
    {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if ((rc = timing_pair(ctx, &ev0, &ev1))) return rc;
        hipExtLaunchKernelGGL(k_routed_a2<SPARSE>, grid, block, 0, ctx->stream, ev0, ev1, 0, ctx->arena, ctx->dev.get());
        if (ctx->timing) ctx->events.taken();
    }
    if ((rc = route_check(ctx, 0, "routed step"))) return rc;
    if (ranks && (rc = route_exchange(ctx, 0))) return rc;
    hipLaunchKernelGGL(k_routed_bg<SPARSE>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, nx, ny, route_halo_of(ctx));
    if (ranks && (rc = route_exchange(ctx, 1))) return rc;
    // (the control kernel has advanced itt / time and rotated the scalars, scalars_update; the sanity word stays in words[2], where
    // rh_get_scalars reads it)
    if (has_observers(ctx)) {   // the observers read the planes between the numerics and the rotation
        hipLaunchKernelGGL((k_routed_cg<false, false>), grid, block, 0, ctx->stream, ctx->arena, ctx->dev, nx, ny, route_halo_of(ctx));
        if ((rc = launch_observers(ctx, 0))) return rc;
        LAUNCH_CELLS(ctx, k_after_timestep_oned);
    } else
        hipLaunchKernelGGL((k_routed_cg<true, SPARSE>), grid, block, 0, ctx->stream, ctx->arena, ctx->dev, nx, ny, route_halo_of(ctx));
    return RH_OK;
}
// One routed step of rh_run_steps / rh_run_steps_dist (forcing shared by all columns): control kernel on the summary word (all-reduced
// between the ranks), three passes around the two gathers -- 6 launches instead of 17.
static int routed_step_device(rh_ctx *ctx, bool sparse_wanted = false) {
    int rc;
    // sparse stores: another step of the same rh_run_steps call follows and no observer reads the planes in between
    const bool sparse = sparse_wanted && ctx->sw.sparse_ok && !has_observers(ctx);
    const bool ranks = ctx->comm && ctx->comm_nranks > 1;
    // first step, or somebody else touched the planes: the summary bits from the arena
    if (!ctx->held.routed_summary && (rc = rebuild_summary_bits(ctx))) return rc;
    if (ctx->comm) {   // (a one-rank communicator takes the same path: tests)
        rc = allreduce_exch(ctx, "routed step", [&](int *send) {
            LAUNCH_WG(ctx, k_summary_reduce, ctx->dev, 0, send, RH_SRC_SUMW);
            return (int)RH_OK;
        });
        if (rc) return rc;
        LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 1, RH_SRC_WORD3, (const int *)(ctx->exch_buf + 64));
    } else
        LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 1, RH_SRC_SUMW, (const int *)nullptr);
    planes_touched(ctx);
    if ((rc = sparse ? routed_passes<true>(ctx, ranks) : routed_passes<false>(ctx, ranks))) return rc;
    CHECK_LAUNCH(ctx);
    routed_step_enqueued(ctx, sparse);
    return RH_OK;
}
int rh_step_routed(rh_ctx *ctx, int monthly) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->cfg.enable_routing_1D) return fail(ctx, RH_ERR_STATE, "rh_step_routed: the context was created without enable_routing_1D");
    int rc;
    if (ctx->comm && ctx->comm_nranks > 1) {
        if ((rc = rh_step_phase1(ctx)) || (rc = allreduce_word(ctx, 0)) || (rc = rh_step_phase2(ctx)) || (rc = allreduce_word(ctx, 1)) ||
            (rc = rh_adaptive_dt_finish(ctx)))
            return rc;
    } else if ((rc = rh_adaptive_dt(ctx)))
        return rc;
    if (monthly < 0) LAUNCH_CELLS(ctx, k_params_surface_if_monthly);
    else if (monthly) LAUNCH_CELLS(ctx, k_params_surface);
    return routed_core(ctx, true);
}

int rh_set_time_limit(rh_ctx *ctx, int64_t t_end) {
    if (!ctx) return RH_ERR_ARG;
    const long long v = t_end < 0 ? -1 : (long long)t_end;
    HIPCHK(ctx, dev_put(ctx, &DevState::t_end, v));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (v is a stack local)
    ctx->t_end = v;
    control_inputs_changed(ctx);   // a control part formed under the old limit (possibly "halt") is not the next step's
    return RH_OK;
}
// with a time limit: 1 if the limit is reached already (nothing to enqueue), 0 if the first launch of the call will run a step --
// the host-side flags that a fused launch leaves behind (rotation, summary, pending control part) are those of a launch that RAN,
// which holds for every later launch of the call too once the first one did (a halted launch changes nothing on the device)
static int limit_reached(rh_ctx *ctx, bool *reached) {
    *reached = false;
    if (ctx->t_end < 0) return RH_OK;
    if (ctx->cfg.enable_routing_1D || ctx->per_cell)
        return fail(ctx, RH_ERR_STATE, "rh_set_time_limit: the limit is observed by the summary path's control part (forcing shared by all columns, "
                                       "no routing); clear it (rh_set_time_limit(ctx, -1)) and bound the steps from the host");
    int64_t now = 0;
    HIPCHK(ctx, hipMemcpyAsync(&now, &ctx->dev->S.time, sizeof(now), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *reached = now >= ctx->t_end;
    return RH_OK;
}

// sparse_next is the request of ONE enqueued step; whatever way a stepping call ends (a failing launch, the timing cap, forcing that was
// never set), it must not survive the call: the next single-step entry point would run the sparse kernel as a call's last step
struct SparseRequestScope {
    rh_ctx *ctx;
    explicit SparseRequestScope(rh_ctx *c) : ctx(c) { ctx->held.sparse_next = false; }
    ~SparseRequestScope() { ctx->held.sparse_next = false; }
};

// step k of the nsteps of a single-GPU call, or of any call with the routing (the routed step exchanges its predicate words and
// border cells itself)
static int call_step(rh_ctx *ctx, int64_t k, int64_t nsteps) {
    if (!ctx->cfg.enable_routing_1D) {
        ctx->held.sparse_next = ctx->sw.sparse_ok && k + 1 < nsteps;   // the call's last step stores every plane
        return step_fused_launches(ctx, -1, 1);
    }
    if (!ctx->per_cell && ctx->sw.routed_device_ok) return routed_step_device(ctx, k + 1 < nsteps);
    launch_hooks(ctx);   // the hooks, then the step routine by routine (rh_step_routed)
    return rh_step_routed(ctx, -1);
}
// the steps of rh_run_steps_dist without the routing: one exchange of the summary word per step
static int dist_steps(rh_ctx *ctx, int64_t nsteps) {
    if (ctx->per_cell) return fail(ctx, RH_ERR_STATE, "rh_run_steps_dist: the one-exchange step needs forcing shared by all columns (rh_step_phase1/2/3 otherwise)");
    for (int64_t k = 0; k < nsteps; ++k) {
        int rc = allreduce_exch(ctx, "rh_run_steps_dist", [&](int *send) {
            if (ctx->held.exch_valid) return (int)RH_OK;   // (the previous fused kernel's tail wrote the send half)
            // first step, or the host touched the planes: the summary word from words[3] or from the arena
            const int src = summary_from_arena(ctx, true);
            if (src < 0) return src;
            LAUNCH_WG(ctx, k_summary_reduce, ctx->dev, 0, send, src);
            CHECK_LAUNCH(ctx);
            return (int)RH_OK;
        });
        if (rc) return rc;
        int *send = ctx->exch_buf, *recv = send + 64;
        // the fused launch in front of the exchange formed the columns-independent half of this control part (pre_tail): the kernel behind
        // the exchange keeps the decisions
        LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 1, RH_SRC_WORD3, (const int *)recv, ctx->held.pre_valid ? 1 : 0);
        CHECK_LAUNCH(ctx);
        ctx->held.sparse_next = ctx->sw.sparse_ok && k + 1 < nsteps;
        rc = launch_fused_kernel(ctx, -1, RH_TAIL_PRE | RH_TAIL_HOOKS, send);   // the tail spreads the next step's summary word into `send`
        if (rc) return rc;
    }
    return RH_OK;
}
// rh_run_steps (dist = false) and rh_run_steps_dist
static int run_steps(rh_ctx *ctx, int64_t nsteps, bool dist) {
    SparseRequestScope sparse_scope(ctx);
    ctx->call_sparse_steps = 0;
    bool over = false;
    if (int rc = limit_reached(ctx, &over)) return rc;
    if (over) return RH_OK;
    if (dist && !ctx->cfg.enable_routing_1D) return dist_steps(ctx, nsteps);
    for (int64_t k = 0; k < nsteps; ++k)
        if (int rc = call_step(ctx, k, nsteps)) return rc;
    return RH_OK;
}

int rh_run_steps(rh_ctx *ctx, int64_t nsteps) {
    if (!ctx || nsteps < 0) return RH_ERR_ARG;
    if (!ctx->series_buf) return fail(ctx, RH_ERR_STATE, "rh_set_forcing_series must be called first");
    return run_steps(ctx, nsteps, false);
}

int rh_run_steps_dist(rh_ctx *ctx, int64_t nsteps) {
    if (!ctx || nsteps < 0) return RH_ERR_ARG;
    if (!ctx->series_buf) return fail(ctx, RH_ERR_STATE, "rh_set_forcing_series must be called first");
    if (!ctx->comm) return fail(ctx, RH_ERR_STATE, "rh_run_steps_dist: no communicator (rh_comm_init / rh_set_comm)");
    return run_steps(ctx, nsteps, true);
}
