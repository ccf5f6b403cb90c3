// roger_hip.hip -- kernels and C ABI of the MI355X-native SVAT backend (see include/roger_hip.h).
//
// Kernel inventory (one thread = one soil column, 256-thread workgroups = 4 wavefronts):
//   k_pred1        start-of-step predicates over swe/swe_top, grid-stride, one word per workgroup
//   k_agg          1 workgroup: [user hooks] + OR of the workgroup words + forcing predicates,
//                  step-class flags, aggregates of the shared forcing series (numpy summation order)
//   k_select       prec/ta selection per column, event + infiltration predicates, one word per workgroup
//   k_scalars      1 workgroup: OR of the words, time-step bookkeeping (dt, event ids, itt, time),
//                  StepCtx for the step
//   k_step<M>      THE hot kernel: whole SVAT step per column, state read once / written once
//   k_reduce       only for multi-GPU runs: materialises a predicate word for the all-reduce
// plus one kernel per routine for the per-routine entry points and the setup-time kernels.
// All per-column kernels are HBM-bound streaming kernels (no data reuse, no LDS tiling, no
// MFMA); k_step moves ~2 KB per column (2.8 KB by the reference's variable read/write sets).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the entry points are resolved with dlsym on first use (rccl_api)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rh_host.h"
#include "rh_physics.h"
#include "rh_sets.inc"
#include "roger_hip.h"

#include "rh_dev_state.h"
#include "rh_control.h"
#include "rh_step.h"
#include "rh_routing.h"

// max over the columns of slope_per (the trip count of the reference's look-up loop, soil.py:621)
__global__ __launch_bounds__(RH_BLOCK) void k_max_slope(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    int v = 0;
    if (i < a.n) rh_ld(a, RH_P_slope_per, i, v);
    for (int off = 32; off; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(&D->max_slope_per, v);
}
RH_CELL_KERNEL(k_topo, rt_topo, rt_topo(c))
RH_CELL_KERNEL(k_params_surface, rt_params_surface, rt_params_surface(c, D->L, X))
RH_CELL_KERNEL(k_params_soil, rt_params_soil, rt_params_soil(c, K, D->L))
RH_CELL_KERNEL(k_initial_conditions, rt_initial_conditions, rt_initial_conditions(c))

__global__ __launch_bounds__(RH_BLOCK) void k_select_pet(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const StepCtx X = D->X;
    Col c;
    RH_SET_LOAD_rt_select_pet(LD)
    if (D->per_cell && X.sel_w >= 0)
        rt_select_pet(c, X, cell_agg(D, a.n, i, 3 * X.sel_w + 2), cell_agg(D, a.n, i, 3 * X.sel_w + 1));
    else
        rt_select_pet(c, X, X.pet_sel_w, X.ta_sel_w);
    RH_SET_STORE_rt_select_pet(ST)
}

// predicates of calculate_infiltration for the stand-alone entry point
__global__ __launch_bounds__(RH_BLOCK) void k_inf_pred(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    unsigned long long b = 0;
    if (i < a.n) {
        double prec, prec_m1;
        rh_ld(a, RH_P_prec, i, prec);
        rh_ld(a, RH_P_prec_m1, i, prec_m1);
        b |= (prec == 0) ? BIT(PC_P_EQ0) : 0;
        b |= (prec_m1 != 0) ? BIT(PC_PM1_NE0) : 0;
        b |= (prec != 0) ? BIT(PC_P_NE0) : 0;
        b |= (prec_m1 == 0) ? BIT(PC_PM1_EQ0) : 0;
    }
    wave_or_to(&D->words[3], b);
}
__global__ void k_inf_conds(DevState *D) {
    infiltration_conds(D->S, D->X, D->words[3]);
    D->words[3] = 0;
}

// Counter calibration (profiles/): copies `nplanes` float64 planes with the access shape of k_step
// (one 8-byte element per lane and plane), so FETCH_SIZE / WRITE_SIZE can be scaled on a known
// byte count as MI355X_MICROARCH.md prescribes for access widths other than 16 B per lane.
__global__ __launch_bounds__(RH_BLOCK) void k_calib_copy(Arena a, int src0, int dst0, int nplanes) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    double v[32];
    for (int p0 = 0; p0 < nplanes; p0 += 32) {
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (p0 + k < nplanes) rh_ld(a, src0 + p0 + k, i, v[k]);
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (p0 + k < nplanes) rh_st(a, dst0 + p0 + k, i, v[k]);
    }
}

// one plane between the arena and a contiguous buffer of n elements (rh_upload / rh_download / rh_plane_device_ptr)
template <typename T>
__global__ __launch_bounds__(RH_BLOCK) void k_plane_gather(Arena a, int plane, T *dst) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i < a.n) dst[i] = *rh_cell<const T>(a, plane, i);
}
template <typename T>
__global__ __launch_bounds__(RH_BLOCK) void k_plane_scatter(Arena a, int plane, const T *src) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i < a.n) *rh_cell<T>(a, plane, i) = src[i];
}

// (n, 144) -> (144, n): a per-cell forcing array as the host hands it over (the reference's vs.prec_day[x, y, :]) into the layout the
// kernels read with unit stride over the columns.  One 64 x 64 tile per workgroup through LDS, both sides coalesced.
__global__ __launch_bounds__(RH_BLOCK) void k_transpose_forcing(const double *src, double *dst, int64_t n) {
    __shared__ double tile[64][65];
    const int64_t c0 = (int64_t)blockIdx.x * 64;   // first column of the tile
    const int s0 = blockIdx.y * 64;                // first slot
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += RH_BLOCK / 64) {   // rows = columns of the grid, contiguous slots
        const int64_t c = c0 + r;
        const int sl = s0 + tx;
        tile[r][tx] = (c < n && sl < RH_SLOTS_PER_DAY) ? src[c * RH_SLOTS_PER_DAY + sl] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += RH_BLOCK / 64) {   // rows = slots, contiguous columns
        const int sl = s0 + r;
        const int64_t c = c0 + tx;
        if (c < n && sl < RH_SLOTS_PER_DAY) dst[(size_t)sl * n + c] = tile[tx][r];
    }
}

// X_m1 = X for every rotation pair of after_timestep: what the lazy steps left undone (materialise_m1)
__global__ __launch_bounds__(RH_BLOCK) void k_rotate_all(Arena a) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    Col c;
    RH_ROTATION_FIELDS(LD)
    RH_ROTATION_FIELDS(ROT)
}

// initial values of the variable registry that are not zero (roger/variables.py `initial=`)
__global__ __launch_bounds__(RH_BLOCK) void k_init_registry(Arena a) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    rh_st(a, RH_P_maskCatch, i, 1);
    rh_st(a, RH_P_ta, i, 15.0);
    rh_st(a, RH_P_ta_m1, i, 15.0);
    rh_st(a, RH_P_z_gw, i, 1000.0);
    rh_st(a, RH_P_z_gw_m1, i, 1000.0);
    rh_st(a, RH_P_c_int, i, 1.0);
    rh_st(a, RH_P_c_root, i, 1.0);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What the device currently holds that the next step may reuse.  A wrong flag is a silent wrong result, so they are written by the
// named events next to planes_touched (host side, below) and by nobody else, two local exceptions apart: pmask_valid, which
// rh_debug_swap_arenas also clears, and sparse_next, the request of the stepping loops (SparseRequestScope).
struct DeviceHolds {
    // --- the planes.  Cleared by planes_touched (somebody other than the fused kernel is about to change planes)
    bool pmask_valid = false;      // DevState::pmask describes the planes as they are now.  Set by form_param_mask
    // lazy tau -> taum1 rotation (k_step<.,.,LAZY>): rot_consistent = the last thing that touched the planes was a complete fused step,
    // i.e. X_m1 == X logically for every rotation pair (set by fused_step_enqueued); m1_stale = the X_m1 PLANES do not hold that yet
    // (set by fused_step_enqueued after a lazy step, cleared by materialise_m1)
    bool rot_consistent = false, m1_stale = false;
    // --- the summary path.  Cleared by planes_touched; the per-cell fronts, which do not read the summary word, clear the ones of
    // this group they outdate (summary_path_left)
    bool summary_valid = false;    // the summary word (words[3]) describes the columns as they are in the arena now.  Set by
                                   // fused_step_enqueued (unless RH_TAIL_SKIP) and by summary_from_arena for the exchange paths
    bool routed_summary = false;   // routing: sumw holds the summary bits of the arena's state (posted by k_routed_a2).  Set by
                                   // routed_step_enqueued
    bool exch_valid = false;       // exch_buf[0..63] holds the summary word of the columns as they are now (written by the last fused
                                   // kernel's tail: fused_step_enqueued).  Also cleared when the buffer is reused (allreduce_word) and when
                                   // the device's control inputs change behind it (control_inputs_changed(on_device): a hook launch)
    // --- the control part of the next step.  Set by fused_step_enqueued from the launch's tail flags; cleared by planes_touched and by
    // control_inputs_changed (scalars, forcing, weights, the time limit, the step log, a hook launch: whatever the control part reads)
    bool pending_valid = false;    // S_next / X_next hold the control part of the next step (formed by the last fused kernel's tail)
    bool pre_valid = false;        // ... or, multi-GPU step: pre_words hold its columns-independent half (pre_tail of the last fused
                                   // launch), for k_ctrl behind the exchange
    int pending_hooks = 0;         // ... formed with / without the device-side hooks
    // --- sparse stores (k_step<.,.,LAZY,SPARSE>, k_routed_*<true>)
    bool sparse_next = false;      // the step being enqueued is followed by another step of the same rh_run_steps call.  Set by the
                                   // stepping loops, consumed by launch_fused_kernel, never survives a call (SparseRequestScope)
    bool outputs_stale = false;    // the last step did not store the pure-output planes (only ever true INSIDE a call, or after a call
                                   // that failed half-way).  Set by fused_step_enqueued / routed_step_enqueued, as is
    bool last_sparse = false;      // ... what rh_step_mode reports of the last step
    // --- per-cell forcing: the parts of the DAY that the front kernels cache on the device.  Set by cell_forcing_changed (new weights or
    // stations; first use) and by front_takes_over (the other front formed them last); each is cleared by the launch that re-forms
    // its part (launch_pred1, launch_cell_agg, launch_cell_front)
    bool agg_daily_stale = true;   // per-cell daily forcing sums must be re-formed
    bool pred_daily_stale = true;  // the same for the day's forcing bits kept by k_pred1
    bool front_daily_stale = true; // ... and for the one-launch front (k_cell_front: daily sums + DevState::day_word)
    int last_front = 0;            // which of the two formed the day's cached parts last (1: k_pred1 ... k_select, 2: k_cell_front)
};

struct rh_ctx {
    Stream stream;                   // first member: destroyed last, after everything that was enqueued on it has been released
    rh_config cfg = {};
    int64_t n = 0;
    Arena arena = {};                // what the kernels are given; arena.base is arena_mem
    DevBuf<char> arena_mem;
    DevBuf<DevState> dev;
    PinnedBlock<HostExport> hexp;    // pinned + mapped
    unsigned long long hexp_seq = 0;
    DevBuf<unsigned long long> pmask_buf;   // DevState::pmask
    int pmask_flags = 7;             // bit 0: uniform loads, bit 1: derived parameters, bit 2: the catchment mask as a constant (RH_NO_PARAM_UNIFORM / RH_NO_PARAM_DERIVE / RH_NO_MASK_CONSTANT clear them)
    DevBuf<double> forc_cell_buf[3];
    DevBuf<double> weight_buf[3];
    DevBuf<int> station_buf;
    DevBuf<double> forc_multi_buf;
    DevBuf<double> transpose_buf;    // staging of one (n, 144) per-cell forcing array before its transposition
    DevBuf<double> agg_cell_buf;
    DevBuf<char> series_buf;
    DevBuf<double> mlms_buf;
    DevBuf<void> stage_buf;          // one contiguous plane (n * 8 bytes): uploads and downloads pass through it
    bool per_cell = false;
    bool forcing_set = false;
    DeviceHolds held;
    bool routed_device_ok = true;    // RH_ROUTED_BY_ROUTINE: rh_run_steps takes rh_step_routed per step (A/B, tests)
    bool defer_select_ok = true;     // RH_NO_DEFERRED_SELECT: k_select stores the per-cell prec / ta itself (A/B, tests)
    int64_t cell_agg_split_min = 65536;   // columns from which the per-cell aggregates run as two kernels (RH_CELL_AGG_SPLIT_MIN: tests)
    bool tail_ok = true;             // RH_NO_TAIL_CTRL unset
    int n_groups = 1;                // fused kernel: completion groups (about 64 workgroups each, at most RH_DONE_GROUPS)
    bool lazy_ok = true;             // RH_NO_LAZY_ROTATION unset
    bool obs_reads_m1 = false;       // an observer (accumulators, points) was given an X_m1 plane: the fused kernel does not skip those stores
    bool sparse_ok = true;           // RH_NO_SPARSE_STORES unset
    bool obs_reads_sparse = false;   // an observer was given a plane the sparse kernel leaves out (its KEEP variant stores those); both
                                     // formed by observers_changed from the union of the observers' planes, and by nobody else
    int64_t t_end = -1;              // rh_set_time_limit (host copy of DevState::t_end)
    int64_t call_sparse_steps = 0;   // steps of the most recent rh_run_steps / rh_run_steps_dist call that ran with sparse stores
    bool cell_front_ok = true;       // RH_PER_CELL_OLD_FRONT unset: per-cell forcing takes k_cell_front instead of the five predicate-generation launches
    int64_t cell_front_max = 2097152; // ... on grids up to this many columns (RH_CELL_FRONT_MAX).  Measured, round 4 (profiles/r04_per_cell_front.txt), ms
                                     // per step with the predicate kernels / with the front: 80 x 53 columns 0.055 / 0.039 (launch-bound: one
                                     // launch in front of the fused kernel instead of six -- the set_forcing hook rides along), 10^6 columns
                                     // 0.261 / 0.252, 10^7 columns 2.15 / 2.23 (one thread doing a column's aggregates, plane reads and bits in
                                     // sequence is latency-bound; two of the five predicate kernels are grid-stride).  Before the slots of the
                                     // device-wide words and the completion counters had a cache line each, the front took 0.320 ms at 10^6.
    DevBuf<double> diag_buf;
    DevBuf<long long> diag_steps_buf;
    long long diag_interval = 86400;
    int diag_n = 0, diag_slots = 0;
    int diag_planes[32] = {};        // host copy of DevState::diag_planes (diag_n of them)
    // time series at observation columns (rh_points_configure): the ring of points_cap rows and its headers
    DevBuf<double> points_buf;
    DevBuf<long long> points_hdr_buf;
    int points_ncells = 0, points_nplanes = 0;   // both 0: not configured, no k_points launch
    int64_t points_cap = 0;
    int points_planes[RH_POINTS_MAX_PLANES] = {};
    int pred_blocks = 0;
    bool timing = false;
    EventPool events;                // pairs (start, stop) around the fused kernel, one per timed step
    DevBuf<int> dt_log_buf;
    std::vector<double> probe_ms;    // placement probing: streaming-kernel time per candidate arena, the chosen one first
    // multi-GPU: RCCL communicator and the exchange buffers of the summary word (64 int32 sent, 64 received)
    ncclComm_t comm = nullptr;
    bool own_comm = false;
    DevBuf<int> exch_buf;
    int comm_nranks = 1, comm_rank = 0;
    int grid_px = 1, grid_py = 1;    // process grid of the communicator, ranks x-fastest (rh_comm_set_grid; default (nranks, 1))
    int planes_held = 0;  // planes the arena has slots for: all of them for a routing context, otherwise all but the routing's (the last
                          // ones of rh_fields.def) -- the tile stride of the non-routing contexts stays what it was before the routing was
                          // added (at 10^6 columns the fused step ran 13 % slower with nine more slots per tile: 2.21 instead of 2.14 GB,
                          // A/B on one box)
    // routing (settings.enable_routing_1D): the rank's own border and the one-cell halo frame of its neighbours, both in the frame
    // layout of F = 2 ny + 2 nx + 4 values (route_frame_parts: west / east columns, south / north rows, four corners)
    DevBuf<double> route_q;          // q_out: [0, F) own border, [F, 2 F) halo frame
    DevBuf<int> route_i;             // [0, F) own flow direction, [F, 2 F) own mask, [2 F, 3 F) halo flow direction, [3 F, 4 F) halo mask
    bool route_halo[2] = {false, false};   // a halo column is present on that side (rh_route_set_halo or the RCCL exchange)
    bool route_frame = false;        // the halo frame holds a neighbour's data; the gathers read it (a part without a neighbour holds zeros)
    bool route_static_done = false;  // the neighbours' flow direction and mask have been exchanged over RCCL
    std::string err;
};
#define RH_DT_LOG_CAP 65536

static std::string g_create_err;

static const char *const PLANE_NAMES[] = {
#define RH_N1(name) #name,
#define RH_N2(name) #name, #name "_m1",
#define RH_FIELD(name, type, levels) RH_N##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_N1
#undef RH_N2
};
static const unsigned char PLANE_IS_INT[] = {
#define RH_T_F64 0
#define RH_T_I32 1
#define RH_I1(type) RH_T_##type,
#define RH_I2(type) RH_T_##type, RH_T_##type,
#define RH_FIELD(name, type, levels) RH_I##levels(type)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_I1
#undef RH_I2
};

// planes the fused step only produces (tools/liveness.py -> RH_SPARSE_FIELDS_* in rh_sets.inc), per model: [0] SVAT, [1] oneD
static const std::vector<unsigned char> *pure_output_planes() {   // [0] SVAT, [1] oneD (fused steps), [2] the routed step
    static const std::vector<unsigned char> tab[3] = {
        [] { std::vector<unsigned char> t(RH_NPLANES, 0);
#define RH_MARK(name) t[RH_P_##name] = 1;
             RH_SPARSE_FIELDS_SVAT(RH_MARK) return t; }(),
        [] { std::vector<unsigned char> t(RH_NPLANES, 0);
             RH_SPARSE_FIELDS_ONED(RH_MARK) return t; }(),
        [] { std::vector<unsigned char> t(RH_NPLANES, 0);
             RH_SPARSE_FIELDS_ROUTED(RH_MARK)
#undef RH_MARK
             return t; }()};
    return tab;
}

static int fail(rh_ctx *ctx, int code, const std::string &msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_err = msg;
    return code;
}
#define HIPCHK(ctx, call)                                                                                      \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) return fail(ctx, RH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline unsigned grid_for(int64_t n) { return (unsigned)((n + RH_BLOCK - 1) / RH_BLOCK); }

// A host value into a member of the device's control block, on the context's stream.  The copy is asynchronous: `v` must live until
// the caller has synchronised the stream -- a stack local, before it goes out of scope.
template <class M, class V>
static hipError_t dev_put(rh_ctx *ctx, M DevState::*member, const V &v) {
    static_assert(sizeof(M) == sizeof(V), "the host value must have the member's size");
    return hipMemcpyAsync(&(ctx->dev.get()->*member), &v, sizeof(M), hipMemcpyHostToDevice, ctx->stream);
}
template <class M>
static hipError_t dev_zero(rh_ctx *ctx, M DevState::*member) {
    return hipMemsetAsync(&(ctx->dev.get()->*member), 0, sizeof(M), ctx->stream);
}

// ---- the events that change what the device holds (DeviceHolds) ---------------------------------------------------------------
// The X_m1 planes from the X planes, if lazy steps left them behind (anything but the fused kernel that looks at the
// planes calls this first).
static void materialise_m1(rh_ctx *ctx) {
    if (!ctx->held.m1_stale) return;
    hipLaunchKernelGGL(k_rotate_all, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena);
    ctx->held.m1_stale = false;
}
// an input of the control part changed: what the last fused kernel's tail formed for the next step is not that step's.  on_device: the
// change is made by a launch (the hooks), behind the summary word that the tail spread into the exchange buffer
static void control_inputs_changed(rh_ctx *ctx, bool on_device = false) {
    ctx->held.pending_valid = ctx->held.pre_valid = false;
    if (on_device) ctx->held.exch_valid = false;
}
// somebody other than the fused kernel is about to change planes: X_m1 == X cannot be taken for granted afterwards, and any per-column
// kernel other than the fused step may change what the summary words describe
static void planes_touched(rh_ctx *ctx) {
    materialise_m1(ctx);
    ctx->held.pmask_valid = false;   // (a parameter plane may be about to change: the wave words are formed again before the next lazy step)
    ctx->held.rot_consistent = false;
    ctx->held.summary_valid = false;
    ctx->held.routed_summary = false;
    control_inputs_changed(ctx, true);
}
// per-cell forcing: the step's control part comes from a front that looks at the planes, not from the summary word -- nothing in front of
// the fused kernel writes a plane (its lazy rotation stays), but what the summary path keeps does not describe the next step
static void summary_path_left(rh_ctx *ctx) {
    ctx->held.summary_valid = false;
    control_inputs_changed(ctx, true);
}
// the per-cell forcing inputs changed (weights, stations): every cached part of the day is formed again
static void cell_forcing_changed(rh_ctx *ctx) {
    ctx->held.agg_daily_stale = true;
    ctx->held.pred_daily_stale = true;
    ctx->held.front_daily_stale = true;
}
// a front of kind 1 (k_pred1 ... k_select) or 2 (k_cell_front) forms this step's predicates: it re-forms the day's cached parts if the other
// kind formed them last
static void front_takes_over(rh_ctx *ctx, int kind) {
    if (ctx->held.last_front != kind) {
        if (kind == 1) ctx->held.agg_daily_stale = ctx->held.pred_daily_stale = true;
        else ctx->held.front_daily_stale = true;
    }
    ctx->held.last_front = kind;
}
// a step was enqueued with / without sparse stores
static void sparse_step_enqueued(rh_ctx *ctx, bool sparse) {
    ctx->held.outputs_stale = ctx->held.last_sparse = sparse;
    ctx->call_sparse_steps += sparse ? 1 : 0;
}
// a fused launch with these tail flags was enqueued (exch: its tail spreads the next step's summary word into the exchange buffer)
static void fused_step_enqueued(rh_ctx *ctx, int flags, bool lazy, bool sparse, bool exch) {
    ctx->held.rot_consistent = true;   // a complete step: after_timestep's X_m1 = X holds, physically (eager) or logically (lazy)
    ctx->held.m1_stale = lazy;
    sparse_step_enqueued(ctx, sparse);
    ctx->held.summary_valid = !(flags & RH_TAIL_SKIP);  // the fused kernel's tail leaves the summary word of the state it wrote (words[3])
    ctx->held.pending_valid = (flags & RH_TAIL_CTRL) != 0;
    ctx->held.pre_valid = (flags & RH_TAIL_PRE) && !(flags & RH_TAIL_CTRL);
    ctx->held.pending_hooks = (flags & RH_TAIL_HOOKS) != 0;
    ctx->held.exch_valid = exch;
}
// a routed device step was enqueued: k_routed_a2 left the summary bits of the state the step ends in
static void routed_step_enqueued(rh_ctx *ctx, bool sparse) {
    ctx->held.routed_summary = true;
    sparse_step_enqueued(ctx, sparse);
}

#define LAUNCH_CELLS(ctx, kern)                                                                                          \
    do {                                                                                                                 \
        planes_touched(ctx);                                                                                             \
        hipLaunchKernelGGL(kern, dim3(grid_for((ctx)->n)), dim3(RH_BLOCK), 0, (ctx)->stream, (ctx)->arena, (ctx)->dev); \
    } while (0)
#define LAUNCH_PRED(ctx, kern)                                                                                           \
    do {                                                                                                                 \
        planes_touched(ctx);                                                                                             \
        hipLaunchKernelGGL(kern, dim3((ctx)->pred_blocks), dim3(RH_BLOCK), 0, (ctx)->stream, (ctx)->arena, (ctx)->dev, 0); \
    } while (0)
#define LAUNCH_ONE(ctx, kern, ...) hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, (ctx)->stream, __VA_ARGS__)
#define LAUNCH_WG(ctx, kern, ...) hipLaunchKernelGGL(kern, dim3(1), dim3(RH_BLOCK), 0, (ctx)->stream, __VA_ARGS__)
#define CHECK_LAUNCH(ctx) HIPCHK(ctx, hipGetLastError())

// a plane that the last step of a call that ended half-way did not store (sparse stores): rh_download and rh_plane_device_ptr refuse it
static bool plane_is_stale(const rh_ctx *ctx, int plane) {
    return ctx->held.outputs_stale && pure_output_planes()[ctx->cfg.enable_routing_1D ? 2 : (ctx->cfg.enable_lateral_flow ? 1 : 0)][plane];
}
// the parameter words of the lazy kernels' wavefronts, formed from the planes as they are (grid: the launch shape of the caller)
static int form_param_mask(rh_ctx *ctx, dim3 grid) {
    if (ctx->held.pmask_valid) return RH_OK;
    hipLaunchKernelGGL(k_param_mask, grid, dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, ctx->pmask_buf, ctx->pmask_flags);
    CHECK_LAUNCH(ctx);
    ctx->held.pmask_valid = true;
    return RH_OK;
}
// every way into a step asks this first
static int need_forcing(rh_ctx *ctx) {
    if (ctx->forcing_set) return RH_OK;
    return fail(ctx, RH_ERR_STATE, "rh_set_forcing_day / rh_set_forcing_series must be called before the first step");
}
// buffers allocated when the first caller needs them
static int need_exch_buf(rh_ctx *ctx) {
    HIPCHK(ctx, ctx->exch_buf.alloc_once(128 * sizeof(int)));
    return RH_OK;
}
static int need_agg_cell_buf(rh_ctx *ctx) {
    if (ctx->agg_cell_buf) return RH_OK;
    HIPCHK(ctx, ctx->agg_cell_buf.alloc(sizeof(double) * 9 * (size_t)ctx->n));
    HIPCHK(ctx, dev_put(ctx, &DevState::agg_cell, *ctx->agg_cell_buf.addr()));
    return RH_OK;
}

// the points' row of the step that was just enqueued: ONE workgroup (at most 8 192 values)
static void launch_points(rh_ctx *ctx, int after_fused) {
    hipLaunchKernelGGL(k_points, dim3(1), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, after_fused);
}
// The observers' planes changed (rh_diag_configure, rh_points_configure): what the fused kernel must leave in memory after every step,
// from the UNION of the accumulators' and the points' planes.  A plane the sparse kernel leaves out -- a pure output, or one of the
// five the next lazy step derives itself, which the storage stage computes all the same -- gets its bit in DevState::keep: the KEEP
// variant stores it after all.  An X_m1 plane switches the lazy rotation off.  Synchronises.
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
    const int any = reads_sparse ? 1 : 0;
    HIPCHK(ctx, dev_put(ctx, &DevState::keep, keep));
    HIPCHK(ctx, dev_put(ctx, &DevState::keep_any, any));
    ctx->obs_reads_sparse = reads_sparse;
    ctx->obs_reads_m1 = reads_m1;
    materialise_m1(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the sources are stack locals)
    return RH_OK;
}

#include "rh_rccl.h"

extern "C" {

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
    ctx->lazy_ok = std::getenv("RH_NO_LAZY_ROTATION") == nullptr;
    ctx->sparse_ok = std::getenv("RH_NO_SPARSE_STORES") == nullptr;
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
        int probes = cfg->placement_probes;
        if (const char *env = std::getenv("RH_PLACEMENT_PROBES")) probes = std::atoi(env);
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
        ctx->pmask_flags = (std::getenv("RH_NO_PARAM_UNIFORM") ? 0 : 1) | (std::getenv("RH_NO_PARAM_DERIVE") ? 0 : 2) | (std::getenv("RH_NO_MASK_CONSTANT") ? 0 : 4);
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
    ctx->tail_ok = std::getenv("RH_NO_TAIL_CTRL") == nullptr;
    ctx->routed_device_ok = std::getenv("RH_ROUTED_BY_ROUTINE") == nullptr;
    ctx->defer_select_ok = std::getenv("RH_NO_DEFERRED_SELECT") == nullptr;
    ctx->cell_front_ok = std::getenv("RH_PER_CELL_OLD_FRONT") == nullptr && ctx->defer_select_ok;
    if (const char *v = std::getenv("RH_CELL_FRONT_MAX")) ctx->cell_front_max = std::atoll(v);
    if (const char *v = std::getenv("RH_CELL_AGG_SPLIT_MIN")) ctx->cell_agg_split_min = std::atoll(v);
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
    if (ctx->cfg.enable_lateral_flow)
        LAUNCH_CELLS(ctx, k_subsurface_runoff_lateral);
    else
        LAUNCH_CELLS(ctx, k_subsurface_runoff);
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

int rh_num_error(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    HIPCHK(ctx, hipMemsetAsync(&ctx->dev->words[2], 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, dev_zero(ctx, &DevState::sanity_last));
    if (ctx->cfg.enable_routing_1D)
        LAUNCH_CELLS(ctx, k_num_error_routed);
    else if (ctx->cfg.enable_lateral_flow)
        LAUNCH_CELLS(ctx, k_num_error_lateral);
    else
        LAUNCH_CELLS(ctx, k_num_error);
    LAUNCH_ONE(ctx, k_sanity_to_scalars, ctx->dev);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

// interception ... numerics in one kernel, then itt/time (roger/roger.py:410-457); for drivers that
// keep the user hooks `set_parameters` and `after_timestep` on the host
static int routed_core(rh_ctx *ctx, bool with_after);
int rh_step_core(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->cfg.enable_routing_1D) return routed_core(ctx, false);   // the columns are coupled: routine by routine with the two gathers
    if (ctx->cfg.enable_lateral_flow)
        LAUNCH_CELLS(ctx, k_core_staged_lateral);
    else
        LAUNCH_CELLS(ctx, k_core_staged);
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, ctx->stream, ctx->dev);
    // the output accumulators follow every step, also in the hook-preserving flow (itt / time were just advanced)
    if (ctx->diag_n) hipLaunchKernelGGL(k_diag, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, 0);
    if (ctx->points_ncells) launch_points(ctx, 0);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

int rh_after_timestep(rh_ctx *ctx) {
    if (!ctx) return RH_ERR_ARG;
    if (ctx->cfg.enable_lateral_flow)
        LAUNCH_CELLS(ctx, k_after_timestep_oned);
    else
        LAUNCH_CELLS(ctx, k_after_timestep);
    LAUNCH_ONE(ctx, k_rotate_scalars, ctx->dev);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}

#include "rh_routing_host.h"

// the next pair of timing events, if timing is on (rh_enable_timing; null otherwise): they ride on a kernel's own dispatch
// (hipExtLaunchKernelGGL).  The pool is reused by the next rh_enable_timing(1), never beyond the cap
static int timing_pair(rh_ctx *ctx, hipEvent_t *ev0, hipEvent_t *ev1) {
    if (!ctx->timing) return RH_OK;
    if (ctx->events.used + 2 > 2 * (size_t)RH_DT_LOG_CAP)
        return fail(ctx, RH_ERR_STATE, "timing: more than 65536 timed steps since rh_enable_timing(1); read the timings and enable again");
    HIPCHK(ctx, ctx->events.next_pair(ev0, ev1));
    return RH_OK;
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
#define RH_LAUNCH_K(K) hipExtLaunchKernelGGL(K, grid, block, 0, ctx->stream, ev0, ev1, 0, ctx->arena, ctx->dev.get(), flags, ctx->n_groups, dst64)
    // lazy rotation: the planes were last touched by a complete fused step (X_m1 == X) and nobody who reads X_m1 planes
    // follows inside this call (an observer kernel may, if it was given an X_m1 plane)
    const bool lazy = ctx->lazy_ok && ctx->held.rot_consistent && !ctx->obs_reads_m1;
    // sparse stores: another step of the same rh_run_steps call follows and nothing in between reads what this one only produces
    const bool sparse = lazy && ctx->held.sparse_next && monthly < 0;   // (planes an observer reads are kept: DevState::keep, the KEEP variant)
    const bool keep = sparse && ctx->obs_reads_sparse;
    ctx->held.sparse_next = false;
    if (lazy)   // the lazy kernels read the parameter planes through the wave words
        if (int rc = form_param_mask(ctx, grid)) return rc;
#define RH_LAUNCH_STEP(MODE)                                          \
    do {                                                              \
        if (MODE == 2 && lat && keep)                                 \
            RH_LAUNCH_K((k_step<2, true, true, true, true>));         \
        else if (MODE == 2 && keep)                                   \
            RH_LAUNCH_K((k_step<2, false, true, true, true>));        \
        else if (MODE == 2 && lat && sparse)                          \
            RH_LAUNCH_K((k_step<2, true, true, true>));               \
        else if (MODE == 2 && sparse)                                 \
            RH_LAUNCH_K((k_step<2, false, true, true>));              \
        else if (lat && lazy)                                         \
            RH_LAUNCH_K((k_step<MODE, true, true>));                  \
        else if (lat)                                                 \
            RH_LAUNCH_K((k_step<MODE, true, false>));                 \
        else if (lazy)                                                \
            RH_LAUNCH_K((k_step<MODE, false, true>));                 \
        else                                                          \
            RH_LAUNCH_K((k_step<MODE, false, false>));                \
    } while (0)
    if (monthly < 0) RH_LAUNCH_STEP(2);  // decided on the device
    else if (monthly) RH_LAUNCH_STEP(1);
    else RH_LAUNCH_STEP(0);
#undef RH_LAUNCH_STEP
#undef RH_LAUNCH_K
    CHECK_LAUNCH(ctx);
    if (ctx->timing) ctx->events.taken();
    fused_step_enqueued(ctx, flags, lazy, sparse, dst64 != nullptr);
    if (ctx->diag_n) {
        hipLaunchKernelGGL(k_diag, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, 1);
        CHECK_LAUNCH(ctx);
    }
    if (ctx->points_ncells) {
        launch_points(ctx, 1);
        CHECK_LAUNCH(ctx);
    }
    return RH_OK;
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
    if (ctx->n >= ctx->cell_agg_split_min) {
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
    int rc = launch_fused_kernel(ctx, monthly);
    if (rc) return rc;
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
// Where the next control kernel finds the summary word of the columns as they are: RH_SRC_WORD3 if the last fused kernel left it in
// words[3], otherwise RH_SRC_SUMW, rebuilt from the arena here (or a negative error code).  stays_valid: only control kernels follow
// before the next look at it (the exchange paths); a fused launch that follows re-forms it anyway.
static int summary_from_arena(rh_ctx *ctx, bool stays_valid) {
    if (ctx->held.summary_valid) return RH_SRC_WORD3;
    HIPCHK(ctx, dev_zero(ctx, &DevState::sumw));
    LAUNCH_CELLS(ctx, k_summary);
    ctx->held.summary_valid = stays_valid;
    return RH_SRC_SUMW;
}
// per-cell forcing, ONE per-column launch in front of the fused kernel (k_cell_front; a second one, returning at once unless a new day
// began, for the daily sums of large grids): the set_forcing hook rides along with it (fresh_day / front_ctrl)
static int launch_cell_front(rh_ctx *ctx, int hooks) {
    const dim3 grid(grid_for(ctx->n)), block(RH_BLOCK);
    const int force = ctx->held.front_daily_stale ? 1 : 0, m1 = ctx->held.m1_stale ? 1 : 0;
    if (ctx->n >= ctx->cell_agg_split_min) {
        hipLaunchKernelGGL(k_cell_front<2>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
        hipLaunchKernelGGL(k_cell_front<0>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
    } else {
        hipLaunchKernelGGL(k_cell_front<1>, grid, block, 0, ctx->stream, ctx->arena, ctx->dev, force, m1, ctx->n_groups, hooks);
    }
    CHECK_LAUNCH(ctx);
    ctx->held.front_daily_stale = false;
    return RH_OK;
}
static void launch_hooks(rh_ctx *ctx);
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
        const int flags = (use_next ? RH_TAIL_USE_NEXT : 0) | (ctx->tail_ok ? RH_TAIL_CTRL | (hooks ? RH_TAIL_HOOKS : 0) : 0);
        return launch_fused_kernel(ctx, monthly, flags);
    }
    const bool front = ctx->cell_front_ok && ctx->n <= ctx->cell_front_max;
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
        const bool defer = ctx->per_cell && ctx->defer_select_ok;   // (shared forcing on this path, e.g. before the series is resident: k_select stores)
        if (!defer) planes_touched(ctx);
        hipLaunchKernelGGL(k_select, dim3(ctx->pred_blocks), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev,
                           (ctx->held.m1_stale ? RH_SELECT_M1_PENDING : 0) | (defer ? RH_SELECT_DEFER : 0));
        LAUNCH_WG(ctx, k_scalars, ctx->dev, 1, 1, defer ? 2 : 0);
        rc = launch_fused_kernel(ctx, monthly);
    }
    if (rc) return rc;
    CHECK_LAUNCH(ctx);
    return RH_OK;
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
    int rc = launch_fused_kernel(ctx, monthly);
    if (rc) return rc;
    CHECK_LAUNCH(ctx);
    return RH_OK;
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
    int rc = rh_step_phase1(ctx);
    if (rc) return rc;
    rc = rh_step_phase2(ctx);
    if (rc) return rc;
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

// One whole step with the routing, routine by routine in the order of RogerSetup.step (roger/roger.py:396-457): the columns are
// coupled twice (after the infiltration and after the lateral flow), so the step is eleven per-column passes with two gathers in
// between instead of the fused kernel.  monthly: 1 / 0 = the caller's set_parameters decision, -1 = the device's (after the
// device-side set_forcing hook, rh_run_steps).  Several ranks: the two predicate words of the adaptive time stepping are all-reduced
// over the context's communicator (64 int32 each, as rh_run_steps_dist's summary word), the border cells go to the neighbours.
static int allreduce_word(rh_ctx *ctx, int word) {
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, "rh_step_routed: " + api->why);
    int rc = need_exch_buf(ctx);
    if (rc) return rc;
    rc = rh_predicates_expand(ctx, word, ctx->exch_buf);
    if (rc) return rc;
    NCCLCHK(ctx, api->AllReduce(ctx->exch_buf, ctx->exch_buf + 64, 64, ncclInt32, ncclMax, ctx->comm, ctx->stream));
    ctx->held.exch_valid = false;   // (the buffer holds a predicate word now)
    return rh_predicates_compress(ctx, word, ctx->exch_buf + 64);
}
// interception ... numerics, itt / time (what rh_step_core is for the uncoupled columns)
static int routed_core(rh_ctx *ctx, bool with_after) {
    int rc;
    HIPCHK(ctx, hipMemsetAsync(&ctx->dev->words[2], 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, dev_zero(ctx, &DevState::sanity_last));
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
    const bool fuse_after = with_after && !ctx->diag_n && !ctx->points_ncells;
    if (fuse_after) LAUNCH_CELLS(ctx, k_routed_c_after);
    else LAUNCH_CELLS(ctx, k_routed_c);
    LAUNCH_ONE(ctx, k_sanity_to_scalars, ctx->dev);
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, ctx->stream, ctx->dev);
    if (ctx->diag_n) hipLaunchKernelGGL(k_diag, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, 0);
    if (ctx->points_ncells) launch_points(ctx, 0);
    if (with_after) {
        if (fuse_after) LAUNCH_ONE(ctx, k_rotate_scalars, ctx->dev);
        else if ((rc = rh_after_timestep(ctx))) return rc;
    }
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
extern "C++" {   // (a template: not inside the extern "C" block)
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
    if (ctx->diag_n || ctx->points_ncells) {   // the observers read the planes between the numerics and the rotation
        hipLaunchKernelGGL((k_routed_cg<false, false>), grid, block, 0, ctx->stream, ctx->arena, ctx->dev, nx, ny, route_halo_of(ctx));
        if (ctx->diag_n) hipLaunchKernelGGL(k_diag, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, 0);
        if (ctx->points_ncells) launch_points(ctx, 0);
        LAUNCH_CELLS(ctx, k_after_timestep_oned);
    } else
        hipLaunchKernelGGL((k_routed_cg<true, SPARSE>), grid, block, 0, ctx->stream, ctx->arena, ctx->dev, nx, ny, route_halo_of(ctx));
    return RH_OK;
}
}
// One routed step of rh_run_steps / rh_run_steps_dist (forcing shared by all columns): control kernel on the summary word (all-reduced
// between the ranks), three passes around the two gathers -- 6 launches instead of 17.
static int routed_step_device(rh_ctx *ctx, bool sparse_wanted = false) {
    int rc;
    // sparse stores: another step of the same rh_run_steps call follows and no observer reads the planes in between
    const bool sparse = sparse_wanted && ctx->sparse_ok && !ctx->diag_n && !ctx->points_ncells;
    RcclApi *api = nullptr;
    const bool ranks = ctx->comm && ctx->comm_nranks > 1;
    if (ctx->comm) {
        api = rccl_api();
        if (!api->ok) return fail(ctx, RH_ERR_STATE, "routed step: " + api->why);
    }
    if (!ctx->held.routed_summary) {   // first step, or somebody else touched the planes: the summary bits from the arena
        HIPCHK(ctx, dev_zero(ctx, &DevState::sumw));
        LAUNCH_CELLS(ctx, k_summary);
    }
    if (ctx->comm) {   // (a one-rank communicator takes the same path: tests)
        if ((rc = need_exch_buf(ctx))) return rc;
        int *send = ctx->exch_buf, *recv = ctx->exch_buf + 64;
        LAUNCH_WG(ctx, k_summary_reduce, ctx->dev, 0, send, RH_SRC_SUMW);
        NCCLCHK(ctx, api->AllReduce(send, recv, 64, ncclInt32, ncclMax, ctx->comm, ctx->stream));
        LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 1, RH_SRC_WORD3, (const int *)recv);
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
        ctx->held.sparse_next = ctx->sparse_ok && k + 1 < nsteps;   // the call's last step stores every plane
        return step_fused_launches(ctx, -1, 1);
    }
    if (!ctx->per_cell && ctx->routed_device_ok) return routed_step_device(ctx, k + 1 < nsteps);
    launch_hooks(ctx);   // the hooks, then the step routine by routine (rh_step_routed)
    return rh_step_routed(ctx, -1);
}
// the steps of rh_run_steps_dist without the routing: one exchange of the summary word per step
static int dist_steps(rh_ctx *ctx, int64_t nsteps) {
    if (ctx->per_cell) return fail(ctx, RH_ERR_STATE, "rh_run_steps_dist: the one-exchange step needs forcing shared by all columns (rh_step_phase1/2/3 otherwise)");
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, "rh_run_steps_dist: " + api->why);
    if (int rc = need_exch_buf(ctx)) return rc;
    int *send = ctx->exch_buf, *recv = ctx->exch_buf + 64;
    for (int64_t k = 0; k < nsteps; ++k) {
        if (!ctx->held.exch_valid) {   // first step, or the host touched the planes: the summary word from words[3] or from the arena
            const int src = summary_from_arena(ctx, true);
            if (src < 0) return src;
            LAUNCH_WG(ctx, k_summary_reduce, ctx->dev, 0, send, src);
            CHECK_LAUNCH(ctx);
        }
        NCCLCHK(ctx, api->AllReduce(send, recv, 64, ncclInt32, ncclMax, ctx->comm, ctx->stream));
        // the fused launch in front of the exchange formed the columns-independent half of this control part (pre_tail): the kernel behind
        // the exchange keeps the decisions
        LAUNCH_ONE(ctx, k_ctrl, ctx->dev, 1, RH_SRC_WORD3, (const int *)recv, ctx->held.pre_valid ? 1 : 0);
        CHECK_LAUNCH(ctx);
        ctx->held.sparse_next = ctx->sparse_ok && k + 1 < nsteps;
        int rc = launch_fused_kernel(ctx, -1, RH_TAIL_PRE | RH_TAIL_HOOKS, send);   // the tail spreads the next step's summary word into `send`
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
    // an accumulated plane must be in memory after every step: the keep bits and the rotation, together with the points' planes
    const int nv = n_rate + n_collect;
    ctx->diag_n = nv;
    std::memcpy(ctx->diag_planes, planes, sizeof(int) * (size_t)nv);
    if (int rc = observers_changed(ctx)) return rc;
    HIPCHK(ctx, ctx->diag_buf.release());
    HIPCHK(ctx, ctx->diag_steps_buf.release());
    ctx->diag_slots = n_slots;
    if (nv) {
        const size_t bytes = (size_t)n_slots * nv * ctx->n * sizeof(double);
        HIPCHK(ctx, ctx->diag_buf.alloc(bytes));
        HIPCHK(ctx, hipMemsetAsync(ctx->diag_buf, 0, bytes, ctx->stream));
        HIPCHK(ctx, ctx->diag_steps_buf.alloc((size_t)n_slots * 3 * sizeof(long long)));
        HIPCHK(ctx, hipMemsetAsync(ctx->diag_steps_buf, 0xff, (size_t)n_slots * 3 * sizeof(long long), ctx->stream));   // -1: never touched
    }
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_steps, *ctx->diag_steps_buf.addr()));
    {
        const long long day = 86400;
        if (ctx->diag_interval <= 0) ctx->diag_interval = day;
        HIPCHK(ctx, dev_put(ctx, &DevState::diag_interval, ctx->diag_interval));
    }
    HIPCHK(ctx, dev_put(ctx, &DevState::diag, *ctx->diag_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_rate, n_rate));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_collect, n_collect));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_slots, n_slots));
    HIPCHK(ctx, dev_put(ctx, &DevState::diag_planes, planes));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the sources are stack locals
    return RH_OK;
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
        if (capacity < 1) return fail(ctx, RH_ERR_ARG, "rh_points_configure: capacity = " + std::to_string(capacity) + " (at least one row)");
        if (capacity > (int64_t)1 << 40) return fail(ctx, RH_ERR_ARG, "rh_points_configure: capacity = " + std::to_string(capacity) + " rows is beyond any device");
        for (int j = 0; j < n_planes; ++j) {
            if (planes[j] < 0 || planes[j] >= ctx->planes_held)
                return fail(ctx, RH_ERR_ARG, "rh_points_configure: plane id " + std::to_string(planes[j]) + " is not held by this context");
            if (PLANE_IS_INT[planes[j]])
                return fail(ctx, RH_ERR_ARG, std::string("rh_points_configure: plane ") + PLANE_NAMES[planes[j]] + " is int32 (float64 planes only)");
            plane_list[j] = planes[j];
        }
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
    HIPCHK(ctx, ctx->points_buf.release());
    HIPCHK(ctx, ctx->points_hdr_buf.release());
    ctx->points_ncells = ctx->points_nplanes = 0;
    ctx->points_cap = 0;
    if (!off) {
        const size_t nv = (size_t)n_cells * n_planes;
        HIPCHK(ctx, ctx->points_buf.alloc((size_t)capacity * nv * sizeof(double)));
        HIPCHK(ctx, ctx->points_hdr_buf.alloc((size_t)capacity * 3 * sizeof(long long)));
        ctx->points_ncells = n_cells;
        ctx->points_nplanes = n_planes;
        ctx->points_cap = capacity;
        std::memcpy(ctx->points_planes, plane_list, sizeof(plane_list));
    }
    const long long zero = 0, cap = (long long)ctx->points_cap;
    HIPCHK(ctx, dev_put(ctx, &DevState::points, *ctx->points_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_hdr, *ctx->points_hdr_buf.addr()));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_rows, zero));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_cap, cap));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_ncells, ctx->points_ncells));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_nplanes, ctx->points_nplanes));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_planes, plane_list));
    HIPCHK(ctx, dev_put(ctx, &DevState::points_cells, cell_list));
    return observers_changed(ctx);   // synchronises: the sources above are stack locals
}
static int points_rows(rh_ctx *ctx, const char *who, long long *rows) {
    if (!ctx->points_ncells) return fail(ctx, RH_ERR_STATE, std::string(who) + ": rh_points_configure has not been called");
    HIPCHK(ctx, hipMemcpyAsync(rows, &ctx->dev->points_rows, sizeof(*rows), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_points_count(rh_ctx *ctx, int64_t *rows_total) {
    if (!ctx) return RH_ERR_ARG;
    if (!rows_total) return fail(ctx, RH_ERR_ARG, "rh_points_count: null pointer");
    long long rows = 0;
    if (int rc = points_rows(ctx, "rh_points_count", &rows)) return rc;
    *rows_total = (int64_t)rows;
    return RH_OK;
}
int rh_points_read(rh_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *hdr, double *values, size_t value_bytes) {
    if (!ctx) return RH_ERR_ARG;
    long long total = 0;
    if (int rc = points_rows(ctx, "rh_points_read", &total)) return rc;
    const size_t nv = (size_t)ctx->points_ncells * ctx->points_nplanes;
    if (first_row < 0 || n_rows < 0 || first_row > total || n_rows > total - first_row)
        return fail(ctx, RH_ERR_ARG, "rh_points_read: rows " + std::to_string(first_row) + " ... " + std::to_string(first_row + n_rows - 1) +
                                     " have not been recorded (" + std::to_string(total) + " rows so far)");
    if (n_rows && first_row < total - ctx->points_cap)
        return fail(ctx, RH_ERR_ARG, "rh_points_read: rows " + std::to_string(first_row) + " ... " + std::to_string(total - ctx->points_cap - 1) +
                                     " have been overwritten (the ring holds the last " + std::to_string(ctx->points_cap) + " of " +
                                     std::to_string(total) + " rows)");
    if ((n_rows && (!hdr || !values)) || value_bytes != (size_t)n_rows * nv * sizeof(double))
        return fail(ctx, RH_ERR_ARG, "rh_points_read: size mismatch (n_rows x n_planes x n_cells float64)");
    for (int64_t done = 0; done < n_rows;) {   // at most two pieces: the range may straddle the ring's wrap
        const int64_t slot = (first_row + done) % ctx->points_cap;
        const int64_t m = std::min<int64_t>(n_rows - done, ctx->points_cap - slot);
        HIPCHK(ctx, hipMemcpyAsync(values + (size_t)done * nv, ctx->points_buf + (size_t)slot * nv, (size_t)m * nv * sizeof(double),
                                   hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(hdr + 3 * done, ctx->points_hdr_buf + 3 * slot, (size_t)m * 3 * sizeof(long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
        done += m;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}

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

// rh_pow on the device for n argument pairs (tests: the same bits as the host's compilation of rh_pow.h)
__global__ void k_selftest_rh_pow(const double *x, const double *y, double *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rh_pow(x[i], y[i]);
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

// np_sum144_window for n window starts over one 144-vector, one wavefront per start: out[2 j] by the kernels' function (the rotation path
// where it applies), out[2 j + 1] by the general path (tests: both are numpy's sum over the masked vector, bit for bit)
__global__ void k_selftest_window(const double *v, const int64_t *itd, double *out) {
    const int64_t t = itd[blockIdx.x];
    auto get = [&](int k) { return v[k]; };
    const double a = np_sum144_window(get, t), b = np_sum144_window_general(get, t);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = a;
        out[2 * blockIdx.x + 1] = b;
    }
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

}  // extern "C"
