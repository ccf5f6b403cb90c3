// rh_step.h -- the per-column kernels: parameter words (k_param_mask), the stage pipeline, the fused step k_step, the
// per-routine and staged-pass kernels.  Part of the one translation unit roger_hip.hip.
#ifndef RH_STEP_H
#define RH_STEP_H

// ---------------------------------------------------------------------------------------------
// per-column kernels
// ---------------------------------------------------------------------------------------------
#define LD(name) rh_ld(a, RH_P_##name, i, c.name);
#define ST(name) rh_st(a, RH_P_##name, i, c.name);

// ---- parameter planes: uniform over a wave -> one element; derivable -> not loaded at all (DevState::pmask) ----
constexpr int rh_param_bit(int plane) {
    switch (plane) {
#define RH_PB(name, bit) case RH_P_##name: return bit;
        RH_PARAM_BITS(RH_PB)
#undef RH_PB
        default: return -1;
    }
}
constexpr bool rh_param_derived(int plane) {
    switch (plane) {
#define RH_PD(name) case RH_P_##name:
        RH_DERIVED_FIELDS(RH_PD)
#undef RH_PD
        return true;
        default: return false;
    }
}
#if defined(RH_CENSUS)   // tools/isa_census.py: the wave's word as a compile-time constant (RH_CENSUS_PMASK), so that the count is of ONE path
#ifndef RH_CENSUS_PMASK
#define RH_CENSUS_PMASK 0ull
#endif
#endif
// Load of plane PLANE for the LAZY kernels: a parameter plane whose bit is set in the wave's word is read at the wave's FIRST column by
// every lane (one 64-byte sector from HBM instead of 512 bytes: the values are equal, k_param_mask compared them bit for bit); a
// derived parameter is not loaded when bit 63 is set (the stage's rd_* function assigns it).
// MK1: the wave's columns all lie in the catchment (bit 62: maskCatch == 1 on every one): the mask is the constant 1, not loaded, and
// the ~ 350 multiplications by it per column and step (the reference masks every assignment) fold away -- x * 1.0 is x, bit for bit.
template <int PLANE, bool MK1, typename T>
RH_DEV void rh_ld_p(const Arena &a, int64_t i, T &dst, unsigned long long um) {
    constexpr int bit = rh_param_bit(PLANE);
    if constexpr (MK1 && PLANE == RH_P_maskCatch) {
        dst = 1;
    } else if constexpr (bit < 0) {
        rh_ld(a, PLANE, i, dst);
    } else {
        if constexpr (rh_param_derived(PLANE)) {
            if (um >> 63) return;
        }
        const bool uni = (um >> bit) & 1ull;
        const int tile = __builtin_amdgcn_readfirstlane((int)(i >> RH_TILE_SHIFT));
        const int piece = __builtin_amdgcn_readfirstlane((int)(i & (RH_TILE_CELLS - 1)) & ~63);
        const T *p = reinterpret_cast<const T *>(a.base + (size_t)tile * a.stride + (size_t)PLANE * RH_SLOT_BYTES) + piece + (uni ? 0 : (int)(i & 63));
        dst = __builtin_nontemporal_load(p);
    }
}
#define LDP(name) rh_ld_p<RH_P_##name, MK1>(a, i, c.name, um);
RH_DEV unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }
RH_DEV unsigned long long bits_of(int v) { return (unsigned long long)(unsigned)v; }
// The wave's word of DevState::pmask.  flags bit 0: uniformity bits, bit 1: the derive bit.  One thread per column; a wave whose upper
// lanes lie beyond the grid compares its active lanes only (the uniform load reads the wave's first column, which exists).
__global__ __launch_bounds__(RH_BLOCK) void k_param_mask(Arena a, DevState *D, unsigned long long *out, int flags) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    const bool active = i < a.n;
    const int64_t ii = active ? i : a.n - 1;   // (a lane beyond the grid looks at the last column: it does not vote)
    if ((int64_t)blockIdx.x * RH_BLOCK + (threadIdx.x & ~63) >= a.n) return;   // the whole wave lies beyond the grid
    Col c;
    unsigned long long um = 0;
#define RH_PU(name, bit)                                                                                       \
    {                                                                                                          \
        rh_ld(a, RH_P_##name, ii, c.name);                                                                     \
        const unsigned long long mine = bits_of(c.name);                                                       \
        const unsigned long long first = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mine >> 32)) << 32) | \
                                         (unsigned)__builtin_amdgcn_readfirstlane((int)mine);                  \
        if (__ballot(active && mine != first) == 0) um |= 1ull << bit;                                         \
    }
    RH_PARAM_BITS(RH_PU)
#undef RH_PU
    // a plane the monthly surface parameters assign stays uniform over the wave only if what they are computed from is
    unsigned long long in_bits = 0, mon_bits = 0;
#define RH_PB(name, bit) const unsigned long long pbit_##name = 1ull << bit;
    RH_PARAM_BITS(RH_PB)
#undef RH_PB
#define RH_PI(name) in_bits |= pbit_##name;
    RH_PARAM_MONTHLY_INPUTS(RH_PI)
#undef RH_PI
#define RH_PM(name) mon_bits |= pbit_##name;
    RH_PARAM_MONTHLY(RH_PM)
#undef RH_PM
    if ((um & in_bits) != in_bits) um &= ~mon_bits;
    const bool all_in = __ballot(active && c.maskCatch != 1) == 0;   // every column of the wave lies in the catchment
    if (!(flags & 1)) um = 0;
    if (all_in && (flags & 4)) um |= 1ull << 62;
    if (flags & 2) {
        // the derived parameters: what the stages would compute from the primaries (already in c) against what the planes hold
        Col d = c;
        rd_all(d, D->K);
        bool same = true;
#define RH_PD(name) same = same && bits_of(d.name) == bits_of(c.name);
        RH_DERIVED_FIELDS(RH_PD)
#undef RH_PD
        if (__ballot(active && !same) == 0) um |= 1ull << 63;
    }
    if ((threadIdx.x & 63) == 0) out[i >> 6] = um;
}
#define ROT(name) rh_st(a, RH_P_##name##_m1, i, c.name);  // tau -> taum1 copy of after_timestep, done early

// THE hot kernel.  Loads every plane the step reads once, runs the whole step in registers,
// stores every plane the step assigns once.
// The fused step runs as a pipeline of stages (sets generated per sequence by tools/gen_sets.py):
// every routine stores the planes it is the last to assign right away, and the planes the NEXT
// routine is the first to mention are requested before the current routine computes, so their
// latency hides behind its arithmetic.
// LAZY (template parameter of step_column): the previous operation was a complete step, so X_m1 == X for every rotation
// pair of after_timestep.  Then the X_m1 planes are neither loaded (the register is filled from X's, AL) nor stored;
// they are materialised from the X planes when somebody else needs them (materialise_m1).  Per column and step this
// saves the 30 rotation stores and the 11 X_m1 loads of the step: 328 of 1 986 bytes.
// SPARSE (with LAZY; every step of an rh_run_steps call that another step of the same call follows): the planes the step only
// PRODUCES -- fluxes and diagnostics that no step reads back, RH_SPARSE_FIELDS_* from the flow analysis of tools/liveness.py -- are
// not stored.  Nothing but the next step looks at the planes between two steps of one call, that step overwrites them as the
// reference's arrays are overwritten, and the call's last step stores everything: what the caller can observe is unchanged.
#define AL(xm1, x) c.xm1 = c.x;
#define RH_LOADS(seq, rt)                                          \
    if constexpr (LAZY) {                                          \
        RH_SEQ_##seq##_LLOAD_##rt(LDP) RH_SEQ_##seq##_ALIAS_##rt(AL) \
    } else {                                                       \
        RH_SEQ_##seq##_LOAD_##rt(LD)                               \
    }
// the stage's derived parameters (rh_physics.h rd_<stage>), where the wave's planes were found to hold exactly these values
// ... and the state every lazy step derives itself (rl_<stage>: k / h of root zone and subsoil from the previous step's water contents)
#define RH_DERIVE(rt)                        \
    if constexpr (LAZY) {                    \
        if (um >> 63) rd_##rt(c, K);         \
        rl_##rt(c, K);                       \
    }
#ifdef RH_CENSUS   // (tools/isa_census.py counts what the sparse kernel stores when no accumulator asks for more)
#define STK(name)
#else
#define STK(name) \
    if ((keepw[RH_P_##name >> 6] >> (RH_P_##name & 63)) & 1ull) rh_st(a, RH_P_##name, i, c.name);
#endif
#define RH_STORES(seq, rt)                                               \
    if constexpr (LAZY && SPARSE) {                                      \
        RH_SEQ_##seq##_SSTORE_##rt(ST)                                   \
        if constexpr (KEEP) { RH_SEQ_##seq##_KSTORE_##rt(STK) }          \
    } else if constexpr (LAZY) {                                         \
        RH_SEQ_##seq##_LSTORE_##rt(ST)                                   \
    } else {                                                             \
        RH_SEQ_##seq##_STORE_##rt(ST) RH_SEQ_##seq##_ROT_##rt(ROT)       \
    }
// the loads of the NEXT stage are requested before the current stage computes, with a scheduling barrier behind them, so that a
// stage's arithmetic runs under the next stage's loads (round 3: 197 VGPRs as before, nothing spilled, 2 - 3 % per step against
// requesting a stage's planes right in front of it -- 10^6 columns 0.2294 -> 0.2228 ms, 10^7 2.047 -> 2.000 ms, oneD 0.2413 -> 0.2354
// ms; library variants alternating inside one call, tools/ab_variants.sh)
#define RH_PIN __builtin_amdgcn_sched_barrier(0);
#ifdef RH_STEP_PHASES   // measurement builds (tools/step_phases.sh): wave cycles per stage of the step, by class of step length
__device__ unsigned long long g_step_phases[256 * 64];   // 256 copies (one address would serialise the chip's atomics)
#define RH_PH(k)                                                                          \
    if ((threadIdx.x & 63) == 0) {                                                        \
        const unsigned long long t_ = clock64();                                          \
        atomicAdd(&g_step_phases[(blockIdx.x & 255) * 64 + ph_cls * 20 + (k)], t_ - ph_t);                          \
        ph_t = t_;                                                                        \
    }
#else
#define RH_PH(k)
#endif
// q_pt / q_sw: the column's summary values for the next step's predicates, sampled where they are final
// (tools/gen_sets.py asserts that no later stage assigns them)
#define RH_STEP_BODY(seq, mon_rt, MON_LOADS, MON_RUN, sub_rt, sub_call, ne_rt, ne_call, at_rt, at_call) \
    RH_LOADS(seq, rt_select_prec) RH_LOADS(seq, rt_select_pet) MON_LOADS RH_LOADS(seq, rt_interception) RH_PIN  \
    rt_select_prec(c, X, prec_s, ta_s); RH_STORES(seq, rt_select_prec)                                                \
    rt_select_pet(c, X, pet_v, ta_v); RH_STORES(seq, rt_select_pet) RH_PH(1)                                      \
    q = summary_bits_pt(c.prec, c.ta, K);                                                                \
    MON_RUN                                                                                              \
    RH_LOADS(seq, rt_evapotranspiration) RH_PIN                                                                 \
    rt_interception(c, K); RH_STORES(seq, rt_interception) RH_PH(2)                                               \
    RH_LOADS(seq, rt_snow) RH_PIN                                                                               \
    RH_DERIVE(rt_evapotranspiration) rt_evapotranspiration(c, K); RH_STORES(seq, rt_evapotranspiration) RH_PH(3)  \
    RH_LOADS(seq, rt_inf_events) RH_PIN                                                                         \
    rt_snow(c, K, X); RH_STORES(seq, rt_snow) RH_PH(4)                                                            \
    q = summary_bits_sw(q, c.swe, c.swe_top); if (post) post_summary(D, q, dep);                         \
    RH_LOADS(seq, rt_inf_matrix) RH_PIN                                                                         \
    rt_inf_events(c, K, X); RH_STORES(seq, rt_inf_events) RH_PH(5)                                                \
    RH_LOADS(seq, rt_inf_macropores) RH_PIN                                                                     \
    RH_DERIVE(rt_inf_matrix) rt_inf_matrix(c, K, X); RH_STORES(seq, rt_inf_matrix) RH_PH(6)                       \
    RH_LOADS(seq, rt_inf_cracks) RH_PIN                                                                         \
    RH_DERIVE(rt_inf_macropores) rt_inf_macropores(c, K, X, DryPath<LAZY>()); RH_STORES(seq, rt_inf_macropores) RH_PH(7) \
    RH_LOADS(seq, rt_inf_finish) RH_PIN                                                                         \
    rt_inf_cracks(c, K, X, DryPath<LAZY>()); RH_STORES(seq, rt_inf_cracks) RH_PH(8)                               \
    RH_LOADS(seq, sub_rt) RH_PIN                                                                                \
    rt_inf_finish(c, K, X); RH_STORES(seq, rt_inf_finish) RH_PH(9)                                                \
    RH_LOADS(seq, rt_capillary_rise) RH_PIN                                                                     \
    RH_DERIVE(sub_rt) sub_call; RH_STORES(seq, sub_rt) RH_PH(10)                                                   \
    RH_LOADS(seq, rt_storage) RH_PIN                                                                            \
    rt_capillary_rise(c, X); RH_STORES(seq, rt_capillary_rise) RH_PH(11)                                           \
    RH_LOADS(seq, ne_rt) RH_PIN                                                                                 \
    RH_DERIVE(rt_storage) rt_storage(c, X); RH_STORES(seq, rt_storage) RH_PH(12)                                   \
    RH_LOADS(seq, at_rt) RH_PIN                                                                                 \
    bad = ne_call; RH_STORES(seq, ne_rt) RH_PH(13)                                                                 \
    at_call; RH_STORES(seq, at_rt) RH_PH(14)

// A wavefront's summary bits into the device-wide words, as soon as they are final (right after the snow stage: the latency of
// the returning atomic hides behind the infiltration stages).  `dep` carries the returned value to the completion count at the end
// of the kernel, so that the wave is counted as done only after its bits have arrived.
RH_DEV void post_summary(DevState *D, unsigned long long q, unsigned &dep) {
    // (by ballots, not lane exchanges: the last wavefront of the grid may run with its upper lanes switched off)
    unsigned long long qq = 0;
#pragma unroll
    for (int b = 0; b <= QB_P_NE0; ++b) qq |= __ballot((q >> b) & 1ull) ? (1ull << b) : 0ull;
    if ((threadIdx.x & 63) == 0 && qq) {
        const unsigned long long old = __hip_atomic_fetch_or(&D->sumw[(blockIdx.x & 63) * RH_WSTRIDE], qq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dep |= (unsigned)(old >> 63);   // (bit 63 is never set: dep stays as it is, but depends on the atomic's return)
    }
}

// the step of one column: loads, the staged pipeline, stores; q = summary bits of the column for the next step's predicates
// KEEP (with SPARSE): an accumulator was given planes the sparse kernel does not store -- those are stored after all (DevState::keep)
template <bool MONTHLY, bool LATERAL, bool LAZY, bool SPARSE, bool KEEP = false, bool MK1 = false>
RH_DEV void step_column(const Arena &a, DevState *D, const StepCtx *Xp, int64_t i, unsigned long long &q, bool &bad, unsigned &dep, unsigned long long um,
                        bool post) {
    {
    const Consts K = D->K;
    const StepCtx X = *Xp;
    Col c;
    double pet_v = X.pet_sel_w, ta_v = X.ta_sel_w;
    double prec_s = X.prec_sel, ta_s = X.ta_sel;   // the column's own when the per-cell selection was deferred to this kernel
    // KEEP: the words that say which pure-output planes an accumulator reads, read ONCE -- tested at the store sites out of D they were
    // loaded again behind every store (the stores may alias them, for all the compiler knows): 72 dependent trips per wavefront,
    // + 65 us per step at 10^6 columns (k_step<..., KEEP> 244 against 179 us; tools/experiments/diag_prof.sh)
    unsigned long long keepw[(RH_NPLANES + 63) / 64];
#pragma unroll
    for (int k = 0; k < (RH_NPLANES + 63) / 64; ++k) keepw[k] = KEEP ? D->keep[k] : 0ull;
#ifdef RH_STEP_PHASES
    const int ph_cls = X.dt < 0.5 ? 0 : (X.dt < 12 ? 1 : 2);
    unsigned long long ph_t = clock64();
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_step_phases[(blockIdx.x & 255) * 64 + ph_cls * 20 + 19], 1ull);
#endif
#ifndef RH_CENSUS   // (tools/isa_census.py counts the step with shared forcing: these four loads belong to the per-cell path only)
    if (D->per_cell && X.sel_w >= 0) {
        pet_v = cell_agg(D, a.n, i, 3 * X.sel_w + 2);
        ta_v = cell_agg(D, a.n, i, 3 * X.sel_w + 1);
    }
    if (X.apply_sel == 2 && D->per_cell && X.sel_p >= 0) {
        prec_s = cell_agg(D, a.n, i, 3 * X.sel_p);
        ta_s = cell_agg(D, a.n, i, 3 * X.sel_p + 1);
    }
#endif
    if (MONTHLY && LATERAL) {
        RH_STEP_BODY(step_lateral_monthly, rt_params_surface, RH_LOADS(step_lateral_monthly, rt_params_surface),
                     rt_params_surface(c, D->L, X); RH_STORES(step_lateral_monthly, rt_params_surface),
                     rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X), rt_num_error_lateral,
                     rt_num_error_lateral(c, K), rt_after_timestep_oned, rt_after_timestep_oned(c))
    } else if (LATERAL) {
        RH_STEP_BODY(step_lateral, , , , rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X),
                     rt_num_error_lateral, rt_num_error_lateral(c, K), rt_after_timestep_oned, rt_after_timestep_oned(c))
    } else if (MONTHLY) {
        RH_STEP_BODY(step_monthly, rt_params_surface, RH_LOADS(step_monthly, rt_params_surface),
                     rt_params_surface(c, D->L, X); RH_STORES(step_monthly, rt_params_surface), rt_subsurface_runoff,
                     rt_subsurface_runoff(c, X), rt_num_error, rt_num_error(c, K), rt_after_timestep, rt_after_timestep(c))
    } else {
        RH_STEP_BODY(step, , , , rt_subsurface_runoff, rt_subsurface_runoff(c, X), rt_num_error, rt_num_error(c, K),
                     rt_after_timestep, rt_after_timestep(c))
    }
    }
}

// MODE: 0 = the plain step, 1 = with the monthly surface parameters (calc_parameters_surface_kernel first), 2 = decided
// by the device-side month-change flag (rh_run_steps, rh_step_finish: one launch whatever the month does)
// flags: RH_TAIL_*; n_groups: completion groups (grid_completion); dst64: the summary word for the exchange between
// ranks, written by the tail (or null)
template <int MODE, bool LATERAL, bool LAZY, bool SPARSE = false, bool KEEP = false>
__global__ __launch_bounds__(RH_BLOCK, RH_STEP_WAVES) void k_step(Arena a, DevState *D, int flags, int n_groups, int *dst64) {
    // Workgroups are dealt round-robin over the 8 XCDs (each with its own L2 and address-translation cache).  Mapping
    // workgroup b to the column block  (b mod 8) * blocks_per_xcd + b / 8  lets every XCD walk ONE contiguous eighth of
    // the arena instead of every XCD touching every page.  Never slower; on one box 6 - 11 % faster at 10^7 columns (21 GB
    // arena: 3.87 -> 3.44 .. 3.64 ms per step; oneD 4.38 -> 4.12 ms), on another box and up to 4 x 10^6 columns the same
    // (DESIGN.md section 5 on the speed levels of this kernel).
    // RH_TAIL_PRE: the last workgroup of the grid has no columns -- its first wavefront is pre_tail
    const unsigned nb = gridDim.x - ((flags & RH_TAIL_PRE) ? 1u : 0u);
    const bool extra = blockIdx.x >= nb;
    const unsigned x = blockIdx.x & 7u, base_cnt = nb >> 3, rem = nb & 7u;
    const unsigned blk = x * base_cnt + (x < rem ? x : rem) + (blockIdx.x >> 3);
    const int64_t i = extra ? a.n : (int64_t)blk * RH_BLOCK + threadIdx.x;
    __shared__ unsigned wg_done;      // wavefronts of this workgroup that are through
    __shared__ CtrlLds tail_lds;      // scratch of the tail and of pre_tail (one wavefront each of the whole grid)
    const StepCtx *Xp = (flags & RH_TAIL_USE_NEXT) ? &D->X_next : &D->X;
    // rh_set_time_limit: the control part found the run over before this step (uniform over the grid).  Nothing runs, the tail
    // included: S_next / X_next keep saying so to every launch that follows.
#ifndef RH_CENSUS   // (tools/isa_census.py counts the per-column memory instructions of ONE pipeline: no halt prologue, no tail)
    const bool halted = Xp->halt != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        D->skipped = halted ? 1 : 0;
        if (halted) log_dt(D, 0);     // (timing: a launch that did nothing is logged with dt = 0)
    }
    if (halted) return;
#endif
    if (threadIdx.x == 0) wg_done = 0;
    __syncthreads();                  // (at the start, where all waves are in step; the kernel has no closing barrier)
    unsigned long long q = 0;
    bool bad = false;
    unsigned dep = 1;
    const bool post = !(flags & RH_TAIL_SKIP);
    if (i < a.n) {
        const bool monthly = MODE == 1 || (MODE == 2 && D->monthly != 0);
        // the wave's word of the parameter planes (uniform / derivable / all in the catchment; zero: plain loads) -- wave-uniform, in
        // scalar registers
        unsigned long long um = 0;
        if constexpr (LAZY) {
#ifdef RH_CENSUS
            um = RH_CENSUS_PMASK;
#else
            const unsigned long long *pm = D->pmask;
            const unsigned long long w = pm ? pm[__builtin_amdgcn_readfirstlane((int)(i >> 6))] : 0ull;
            um = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)w);
#endif
        }
        const bool mk1 = LAZY && ((um >> 62) & 1ull);   // (the monthly pipeline, once a month, keeps the generic code)
        // the SPARSE kernel holds the full-store pipeline too: the step that reaches the time limit is the run's last one
        // (X.last, decided by the control part on the device) and stores every plane -- a wave-uniform branch
#ifdef RH_CENSUS
        if (SPARSE) {
#else
        if (SPARSE && !Xp->last) {
#endif
            if (monthly) step_column<true, LATERAL, LAZY, SPARSE, KEEP>(a, D, Xp, i, q, bad, dep, um, post);
            else if (mk1) step_column<false, LATERAL, LAZY, SPARSE, KEEP, LAZY>(a, D, Xp, i, q, bad, dep, um, post);
            else step_column<false, LATERAL, LAZY, SPARSE, KEEP>(a, D, Xp, i, q, bad, dep, um, post);
        } else {
            // (the full-store pipeline keeps the generic code: with a third copy the full-store kernels spill registers)
            if (monthly) step_column<true, LATERAL, LAZY, false>(a, D, Xp, i, q, bad, dep, um, post);
            else step_column<false, LATERAL, LAZY, false>(a, D, Xp, i, q, bad, dep, um, post);
        }
    } else if (post) {
        post_summary(D, 0ull, dep);
    }
    // (behind the column pipeline in the kernel's text: in front of it, the allocator spilled 36 - 63 of the pipeline's registers)
#ifndef RH_CENSUS
    if (__builtin_expect(extra && threadIdx.x < 64, 0)) pre_tail(D, tail_lds, flags, dep);
#endif
    const bool any_bad = __any(bad);
    if (!post) {   // RH_TAIL_SKIP: the sanity word is all anybody reads of this launch
        if (any_bad && (threadIdx.x & 63) == 0) __hip_atomic_fetch_or(&D->words[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // Completion, without a barrier and without fences (a release fence at device scope writes the XCD's L2 back): everything the
    // tail reads from other waves went through device-scope atomics that have RETURNED before the wave counts itself done.
    bool last = false;
    if ((threadIdx.x & 63) == 0) {
        if (any_bad) dep |= (unsigned)(__hip_atomic_fetch_or(&D->words[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 63);
        const unsigned o = atomicAdd(&wg_done, dep);   // LDS; dep == 1
        if (o == (RH_BLOCK / 64) - 1) last = grid_completion(D, n_groups);   // the last wave of the workgroup reports the workgroup
    }
#ifndef RH_CENSUS   // tools/isa_census.py counts the per-column memory instructions of the kernel without its tail
    if (__shfl((int)last, 0)) step_tail(D, tail_lds, flags, dst64);
#endif
}

#ifdef RH_CENSUS   // tools/isa_census.py: the sparse variant of the non-monthly pipeline on its own (the product launches MODE 2 only)
template __global__ void k_step<0, false, true, true>(Arena, DevState *, int, int, int *);
template __global__ void k_step<0, true, true, true>(Arena, DevState *, int, int, int *);
#endif

#define RH_CELL_KERNEL(kname, rt, call)                                       \
    __global__ __launch_bounds__(RH_BLOCK) void kname(Arena a, DevState *D) { \
        const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;       \
        if (i >= a.n) return;                                                 \
        const Consts K = D->K;                                                \
        const StepCtx X = D->X;                                               \
        (void)K;                                                              \
        (void)X;                                                              \
        Col c;                                                                \
        RH_SET_LOAD_##rt(LD) call;                                            \
        RH_SET_STORE_##rt(ST)                                                 \
    }

RH_CELL_KERNEL(k_interception, rt_interception, rt_interception(c, K))
RH_CELL_KERNEL(k_evapotranspiration, rt_evapotranspiration, rt_evapotranspiration(c, K))
RH_CELL_KERNEL(k_snow, rt_snow, rt_snow(c, K, X))
RH_CELL_KERNEL(k_infiltration, rt_infiltration, rt_infiltration(c, K, X))
RH_CELL_KERNEL(k_subsurface_runoff, rt_subsurface_runoff, rt_subsurface_runoff(c, X))
RH_CELL_KERNEL(k_capillary_rise, rt_capillary_rise, rt_capillary_rise(c, X))
RH_CELL_KERNEL(k_storage, rt_storage, rt_storage(c, X))
RH_CELL_KERNEL(k_num_error, rt_num_error, if (rt_num_error(c, K)) atomicOr(&D->words[2], 1ull))
RH_CELL_KERNEL(k_after_timestep, rt_after_timestep, rt_after_timestep(c))
// oneD model variants
RH_CELL_KERNEL(k_subsurface_runoff_lateral, rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X))
RH_CELL_KERNEL(k_num_error_lateral, rt_num_error_lateral, if (rt_num_error_lateral(c, K)) atomicOr(&D->words[2], 1ull))
RH_CELL_KERNEL(k_after_timestep_oned, rt_after_timestep_oned, rt_after_timestep_oned(c))
RH_CELL_KERNEL(k_params_lateral, rt_params_lateral, rt_params_lateral(c, D->mlms, D->mlms_rows, D->max_slope_per))
// Passes staged like the fused step (tools/gen_sets.py PLAIN_SEQUENCES): every plane is loaded right before the first stage that mentions it
// and stored right after the last one that assigns it (short live ranges instead of all loads up front)
#define RH_PSTAGE(seq, rt, call) RH_SEQ_##seq##_LOAD_##rt(LD) call; RH_SEQ_##seq##_STORE_##rt(ST)
// ... in a kernel with a template parameter SPARSE (the device-driven routed step inside rh_run_steps: every step of a call but the last
// leaves out the stores of the planes the routed step only produces and no later pass of the step loads, RH_SEQ_*_SSTORE_*, tools/gen_sets.py)
#define RH_PSTAGE_S(seq, rt, call)                            \
    RH_SEQ_##seq##_LOAD_##rt(LD) call;                        \
    if constexpr (SPARSE) { RH_SEQ_##seq##_SSTORE_##rt(ST) }  \
    else { RH_SEQ_##seq##_STORE_##rt(ST) }
#define RH_PASS_KERNEL(kname, body)                                                                        \
    __global__ __launch_bounds__(RH_BLOCK, RH_STEP_WAVES) void kname(Arena a, DevState *D) {               \
        const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;                                    \
        if (i >= a.n) return;                                                                              \
        const Consts K = D->K;                                                                             \
        const StepCtx X = D->X;                                                                            \
        Col c;                                                                                             \
        bool bad = false;                                                                                  \
        body                                                                                               \
        if (bad) atomicOr(&D->words[2], 1ull);                                                             \
    }
// The step core of the hook-preserving flow (rh_step_core: RogerSetup.step() with the user hooks on the host) as ONE staged pass -- the
// fused kernel's pipeline without its selection, rotation and control parts.  (Kernels that load every plane up front need 256 VGPRs
// + 92 / 118 AGPRs and run at one wave per SIMD, VERDICT r2 weak #5.)
#define RH_CORE_HEAD(seq)                                                                          \
    RH_PSTAGE(seq, rt_interception, rt_interception(c, K))                                         \
    RH_PSTAGE(seq, rt_evapotranspiration, rt_evapotranspiration(c, K))                             \
    RH_PSTAGE(seq, rt_snow, rt_snow(c, K, X))                                                      \
    RH_PSTAGE(seq, rt_inf_events, rt_inf_events(c, K, X))                                          \
    RH_PSTAGE(seq, rt_inf_matrix, rt_inf_matrix(c, K, X))                                          \
    RH_PSTAGE(seq, rt_inf_macropores, rt_inf_macropores(c, K, X))                                  \
    RH_PSTAGE(seq, rt_inf_cracks, rt_inf_cracks(c, K, X))                                          \
    RH_PSTAGE(seq, rt_inf_finish, rt_inf_finish(c, K, X))
RH_PASS_KERNEL(k_core_staged,
               RH_CORE_HEAD(core)
               RH_PSTAGE(core, rt_subsurface_runoff, rt_subsurface_runoff(c, X))
               RH_PSTAGE(core, rt_capillary_rise, rt_capillary_rise(c, X))
               RH_PSTAGE(core, rt_storage, rt_storage(c, X))
               RH_PSTAGE(core, rt_num_error, bad = rt_num_error(c, K)))
RH_PASS_KERNEL(k_core_staged_lateral,
               RH_CORE_HEAD(core_lateral)
               RH_PSTAGE(core_lateral, rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X))
               RH_PSTAGE(core_lateral, rt_capillary_rise, rt_capillary_rise(c, X))
               RH_PSTAGE(core_lateral, rt_storage, rt_storage(c, X))
               RH_PSTAGE(core_lateral, rt_num_error_lateral, bad = rt_num_error_lateral(c, K)))

#endif  // RH_STEP_H
