// rh_context.h -- the context (rh_ctx) and what every host file uses: the environment switches, what the device holds (DeviceHolds) and
// the events that change it, the launch macros, the plane tables.  Part of the one translation unit roger_hip.hip.
#pragma once
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

// The environment switches, read once by rh_create (read_switches) and by nobody else.  Every one selects the reference path of a test or
// of an A/B measurement.
struct Switches {
    bool lazy_ok, sparse_ok, tail_ok, routed_device_ok, defer_select_ok, cell_front_ok;
    int64_t cell_front_max, cell_agg_split_min;
    int pmask_flags, placement_probes;
};
static Switches read_switches(const rh_config &cfg) {
    auto unset = [](const char *name) { return std::getenv(name) == nullptr; };
    auto number = [](const char *name, long long dflt) { const char *v = std::getenv(name); return v ? std::atoll(v) : dflt; };
    Switches s;
    s.lazy_ok = unset("RH_NO_LAZY_ROTATION");
    s.sparse_ok = unset("RH_NO_SPARSE_STORES");
    s.tail_ok = unset("RH_NO_TAIL_CTRL");
    s.routed_device_ok = unset("RH_ROUTED_BY_ROUTINE");     // set: rh_run_steps takes rh_step_routed per step (A/B, tests)
    s.defer_select_ok = unset("RH_NO_DEFERRED_SELECT");     // set: k_select stores the per-cell prec / ta itself (A/B, tests)
    // per-cell forcing takes k_cell_front instead of the five predicate-generation launches ...
    s.cell_front_ok = unset("RH_PER_CELL_OLD_FRONT") && s.defer_select_ok;
    // ... on grids up to this many columns.  Measured, round 4 (profiles/r04_per_cell_front.txt), ms per step with the predicate kernels /
    // with the front: 80 x 53 columns 0.055 / 0.039 (launch-bound: one launch in front of the fused kernel instead of six -- the
    // set_forcing hook rides along), 10^6 columns 0.261 / 0.252, 10^7 columns 2.15 / 2.23 (one thread doing a column's aggregates, plane
    // reads and bits in sequence is latency-bound; two of the five predicate kernels are grid-stride).  Before the slots of the
    // device-wide words and the completion counters had a cache line each, the front took 0.320 ms at 10^6.
    s.cell_front_max = number("RH_CELL_FRONT_MAX", 2097152);
    s.cell_agg_split_min = number("RH_CELL_AGG_SPLIT_MIN", 65536);   // columns from which the per-cell aggregates run as two kernels (tests)
    // DevState::pmask: bit 0: uniform loads, bit 1: derived parameters, bit 2: the catchment mask as a constant
    s.pmask_flags = (unset("RH_NO_PARAM_UNIFORM") ? 1 : 0) | (unset("RH_NO_PARAM_DERIVE") ? 2 : 0) | (unset("RH_NO_MASK_CONSTANT") ? 4 : 0);
    s.placement_probes = (int)number("RH_PLACEMENT_PROBES", cfg.placement_probes);   // (overrides rh_config.placement_probes)
    return s;
}

// A ring of `cap` rows on the device and the rows' headers (3 int64 each; the bands': 2 + 2 per item) beside it: what the points, the
// totals and the zonal totals record into after every step, and the bands after every counted interval.  cap 0: the observer is off.
struct ObsRing {
    DevBuf<double> buf;
    DevBuf<long long> hdr_buf;
    int64_t cap = 0;
    hipError_t release() {
        cap = 0;
        const hipError_t e = buf.release(), h = hdr_buf.release();
        return e != hipSuccess ? e : h;
    }
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
    Switches sw;                     // the environment as rh_create found it
    int n_groups = 1;                // fused kernel: completion groups (about 64 workgroups each, at most RH_DONE_GROUPS)
    bool obs_reads_m1 = false;       // one of the observers was given an X_m1 plane: the fused kernel does not skip those stores
    bool obs_reads_sparse = false;   // an observer was given a plane the sparse kernel leaves out (its KEEP variant stores those); both
                                     // formed by observers_changed from the union of the observers' planes, and by nobody else
    int64_t t_end = -1;              // rh_set_time_limit (host copy of DevState::t_end)
    int64_t call_sparse_steps = 0;   // steps of the most recent rh_run_steps / rh_run_steps_dist call that ran with sparse stores
    DevBuf<double> diag_buf;
    DevBuf<long long> diag_steps_buf;
    long long diag_interval = 86400;
    int diag_n = 0, diag_slots = 0;
    int diag_planes[32] = {};        // host copy of DevState::diag_planes (diag_n of them)
    // time series at observation columns (rh_points_configure): the ring and its headers
    ObsRing points;
    int points_ncells = 0, points_nplanes = 0;   // both 0: not configured, no k_points launch
    int points_planes[RH_POINTS_MAX_PLANES] = {};
    // catchment totals (rh_totals_configure): the ring and its headers, the tiles' partials, the mask (not held: every column)
    ObsRing totals;
    DevBuf<double> totals_part_buf;
    DevBuf<unsigned char> totals_mask_buf;
    int totals_nplanes = 0;          // 0: not configured, no k_totals_* launch
    int64_t totals_ncells = 0;       // columns inside the mask
    int totals_planes[RH_POINTS_MAX_PLANES] = {};
    // zonal totals (rh_zonal_configure): the ring and its headers, the (tile, zone) partials, the zone map and the index over it
    ObsRing zonal;
    DevBuf<double> zonal_part_buf;
    DevBuf<int> zonal_index_buf;     // zone[n], tile_ptr[ntiles + 1], tile_zone[S], acc_ptr[Z * 256 + 1], acc_slot[S] in one allocation
    int zonal_nplanes = 0, zonal_nzones = 0;   // 0: not configured, no k_zonal_* launch
    int zonal_planes[RH_POINTS_MAX_PLANES] = {};
    std::vector<int64_t> zonal_ncells;         // columns of every zone on this rank
    // scores against observed series (rh_scores_configure): the moments, the observations, the series map (not held: every column
    // series 0) and the closed flags
    DevBuf<double> scores_buf, scores_obs_buf;
    DevBuf<int> scores_series_buf;
    DevBuf<unsigned char> scores_closed_buf;
    int scores_nitems = 0;           // 0: not configured, no k_scores launch
    int64_t scores_nintervals = 0;
    int scores_planes[RH_SCORES_MAX_ITEMS] = {};
    // event outputs (rh_events_configure): the slots' maps, their headers and the per-workgroup copies of the slots' ids
    DevBuf<double> events_buf;
    DevBuf<long long> events_hdr_buf, events_ids_buf;
    int events_nitems = 0, events_nslots = 0;   // 0: not configured, no k_events launch
    int events_planes[RH_EVENTS_MAX_ITEMS] = {};
    // duration curves (rh_durations_configure): the counters, the float planes, the spell planes, the edges and the mask (not held:
    // every column)
    DevBuf<unsigned> durations_counts_buf, durations_spells_buf;
    DevBuf<double> durations_vals_buf, durations_edges_buf;
    DevBuf<unsigned char> durations_mask_buf;
    int durations_nitems = 0, durations_nbins = 0;   // 0: not configured, no k_durations launch; nbins: the sum of the items' m + 2
    int durations_planes[RH_DURATIONS_MAX_ITEMS] = {};
    // ensemble bands (rh_bands_configure): the ring and its headers (2 + 2 * bands_nitems int64 a row), the SUM accumulators, the key
    // planes, the digit histograms and the mask (not held: every column)
    ObsRing bands;
    DevBuf<double> bands_acc_buf;
    DevBuf<unsigned long long> bands_keys_buf;
    DevBuf<unsigned> bands_hist_buf;
    DevBuf<unsigned char> bands_mask_buf;
    int bands_nitems = 0, bands_nprobs = 0;   // 0: not configured, no k_bands* launch
    int bands_planes[RH_BANDS_MAX_ITEMS] = {};
    // ... per zone (rh_bands_configure_zonal): the rows' counts (item, zone, 2 int64 a row; the ring's headers are 2 int64 a row then), and
    // zone_off[n_zones + 1] with the zones' column lists behind it in one allocation
    DevBuf<long long> bands_counts_buf;
    DevBuf<int> bands_zone_buf;
    int bands_nzones = 0;            // 0: the plain configuration (k_bands_select); else k_bands_zonal on (bands_nzones, bands_nitems)
    // ... likelihood-weighted (rh_bands_configure_weighted): the weight plane (held: k_bands_select_w takes the place of k_bands_select),
    // the 64-bit digit histograms and the ring of the rows' weight sums (bands_nitems int64 a row)
    DevBuf<unsigned short> bands_weight_buf;
    DevBuf<unsigned long long> bands_whist_buf;
    DevBuf<long long> bands_wsum_buf;
    // ... observations (rh_bands_observations): the series (item, series, interval), the workgroups' partial pairs and the ring of the
    // rows' pairs (bands_nitems x series x 2 int64 a row); held: the k_bands_obs* launches follow the selection's
    DevBuf<double> bands_obs_buf;
    DevBuf<long long> bands_obs_part_buf, bands_obs_ring_buf;
    // carrying the four through a restart (ABI version 18, rh_*_restore): an observer is FRESH from its configure call until the first
    // step that launches the observers -- only then may its state be replaced; scores_interval is the host copy the restore checks a
    // carried t_first against
    unsigned obs_fresh = 0;          // RH_FRESH_SCORES | _EVENTS | _DURATIONS | _BANDS
    int64_t scores_interval = 0;
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
    hipLaunchKernelGGL(k_param_mask, grid, dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, ctx->dev, ctx->pmask_buf, ctx->sw.pmask_flags);
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
