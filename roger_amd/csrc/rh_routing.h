// rh_routing.h -- the routed step on the device (settings.enable_routing_1D): k_routed_*, the halo frame (RouteHalo), the
// gather and the border pack.  The host side is rh_routing_host.h.  Part of the one translation unit roger_hip.hip.
#ifndef RH_ROUTING_H
#define RH_ROUTING_H

// settings.enable_routing_1D: the per-column parts of the D8 routing (rh_physics.h) ...
RH_CELL_KERNEL(k_infiltration_routed, rt_infiltration_routed, rt_infiltration_routed(c, K, X))
RH_CELL_KERNEL(k_route_surface_out, rt_route_surface_out, rt_route_surface_out(c, K, X, (double)D->S.dt_secs))
RH_CELL_KERNEL(k_route_surface_in, rt_route_surface_in, rt_route_surface_in(c))
RH_CELL_KERNEL(k_route_subsurface_out, rt_route_subsurface_out, rt_route_subsurface_out(c))
RH_CELL_KERNEL(k_route_subsurface_in, rt_route_subsurface_in, rt_route_subsurface_in(c))
RH_CELL_KERNEL(k_num_error_routed, rt_num_error_routed, if (rt_num_error_routed(c, K)) atomicOr(&D->words[2], 1ull))
// the step core in three passes, one kernel each (the infiltration's branch conditions come from the adaptive time stepping's
// predicate word: global over the ranks), staged like the fused step (RH_PSTAGE, rh_step.h)
RH_PASS_KERNEL(k_routed_a,
               RH_PSTAGE(routed_a, rt_interception, rt_interception(c, K))
               RH_PSTAGE(routed_a, rt_evapotranspiration, rt_evapotranspiration(c, K))
               RH_PSTAGE(routed_a, rt_snow, rt_snow(c, K, X))
               RH_PSTAGE(routed_a, rt_inf_events, rt_inf_events(c, K, X))
               RH_PSTAGE(routed_a, rt_inf_matrix, rt_inf_matrix(c, K, X))
               RH_PSTAGE(routed_a, rt_inf_macropores, rt_inf_macropores(c, K, X))
               RH_PSTAGE(routed_a, rt_inf_cracks, rt_inf_cracks(c, K, X))
               RH_PSTAGE(routed_a, rt_inf_finish_routed, rt_inf_finish_routed(c, K, X))
               RH_PSTAGE(routed_a, rt_route_surface_out, rt_route_surface_out(c, K, X, (double)D->S.dt_secs)))
RH_PASS_KERNEL(k_routed_b,
               RH_PSTAGE(routed_b, rt_route_surface_in, rt_route_surface_in(c))
               RH_PSTAGE(routed_b, rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X))
               RH_PSTAGE(routed_b, rt_route_subsurface_out, rt_route_subsurface_out(c)))
RH_PASS_KERNEL(k_routed_c,
               RH_PSTAGE(routed_c, rt_route_subsurface_in, rt_route_subsurface_in(c))
               RH_PSTAGE(routed_c, rt_capillary_rise, rt_capillary_rise(c, X))
               RH_PSTAGE(routed_c, rt_storage, rt_storage(c, X))
               RH_PSTAGE(routed_c, rt_num_error_routed, bad = rt_num_error_routed(c, K)))
RH_PASS_KERNEL(k_routed_c_after,
               RH_PSTAGE(routed_c_after, rt_route_subsurface_in, rt_route_subsurface_in(c))
               RH_PSTAGE(routed_c_after, rt_capillary_rise, rt_capillary_rise(c, X))
               RH_PSTAGE(routed_c_after, rt_storage, rt_storage(c, X))
               RH_PSTAGE(routed_c_after, rt_num_error_routed, bad = rt_num_error_routed(c, K))
               RH_PSTAGE(routed_c_after, rt_after_timestep_oned, rt_after_timestep_oned(c)))
// Device-driven stepping (rh_run_steps / rh_run_steps_dist on a routing context): the first pass with the step's forcing selection [and
// the monthly surface parameters, D->monthly] in front, as the fused kernel has them, and the columns' summary bits for the NEXT step's
// control kernel posted as soon as they are final (k_ctrl reads them from sumw: no predicate passes over the arena between two steps).
#define RH_ROUTED_A2_TAIL(seq)                                                                                  \
    RH_PSTAGE_S(seq, rt_interception, rt_interception(c, K))                                                      \
    RH_PSTAGE_S(seq, rt_evapotranspiration, rt_evapotranspiration(c, K))                                          \
    RH_PSTAGE_S(seq, rt_snow, rt_snow(c, K, X))                                                                   \
    q = summary_bits_sw(q, c.swe, c.swe_top);                                                                   \
    post_summary(D, q, dep);                                                                                    \
    RH_PSTAGE_S(seq, rt_inf_events, rt_inf_events(c, K, X))                                                       \
    RH_PSTAGE_S(seq, rt_inf_matrix, rt_inf_matrix(c, K, X))                                                       \
    RH_PSTAGE_S(seq, rt_inf_macropores, rt_inf_macropores(c, K, X))                                               \
    RH_PSTAGE_S(seq, rt_inf_cracks, rt_inf_cracks(c, K, X))                                                       \
    RH_PSTAGE_S(seq, rt_inf_finish_routed, rt_inf_finish_routed(c, K, X))                                         \
    RH_PSTAGE_S(seq, rt_route_surface_out, rt_route_surface_out(c, K, X, (double)D->S.dt_secs))
template <bool SPARSE>
__global__ __launch_bounds__(RH_BLOCK, RH_STEP_WAVES) void k_routed_a2(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const Consts K = D->K;
    const StepCtx X = D->X;
    Col c;
    unsigned long long q = 0;
    unsigned dep = 1;
    double pet_v = X.pet_sel_w, ta_v = X.ta_sel_w;
    if (D->per_cell && X.sel_w >= 0) {
        pet_v = cell_agg(D, a.n, i, 3 * X.sel_w + 2);
        ta_v = cell_agg(D, a.n, i, 3 * X.sel_w + 1);
    }
#ifdef RH_CENSUS   // tools/isa_census.py counts the pipeline a step runs unless the month changes
    if (false) {
#else
    if (D->monthly != 0) {
#endif
        RH_PSTAGE_S(routed_a2_monthly, rt_select_prec, rt_select_prec(c, X, X.prec_sel, X.ta_sel))
        RH_PSTAGE_S(routed_a2_monthly, rt_select_pet, rt_select_pet(c, X, pet_v, ta_v))
        q = summary_bits_pt(c.prec, c.ta, K);
        RH_PSTAGE_S(routed_a2_monthly, rt_params_surface, rt_params_surface(c, D->L, X))
        RH_ROUTED_A2_TAIL(routed_a2_monthly)
    } else {
        RH_PSTAGE_S(routed_a2, rt_select_prec, rt_select_prec(c, X, X.prec_sel, X.ta_sel))
        RH_PSTAGE_S(routed_a2, rt_select_pet, rt_select_pet(c, X, pet_v, ta_v))
        q = summary_bits_pt(c.prec, c.ta, K);
        RH_ROUTED_A2_TAIL(routed_a2)
    }
}
// set_parameters' month-change test was evaluated on the device by the set_forcing hook (D->monthly)
__global__ __launch_bounds__(RH_BLOCK) void k_params_surface_if_monthly(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n || !D->monthly) return;
    const StepCtx X = D->X;
    Col c;
    RH_SET_LOAD_rt_params_surface(LD) rt_params_surface(c, D->L, X);
    RH_SET_STORE_rt_params_surface(ST)
}

// ... and the gather between them: q_in of cell (ix, iy) = np.sum over the eight *_in_d8 entries, in_d8[c, d] = where(flow_dir[s] ==
// code_d, q_out[s], 0) * maskCatch[s] with s = c - (dx_d, dy_d) an interior cell (surface_runoff.py:137-204; the reference scatters
// into shifted slices, a cell next to the edge of the grid receives nothing from outside).  The reference's direction order
// N, NE, E, SE, S, SW, W, NW and numpy's sum of 8 contiguous values, ((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7)).
// Several ranks (the grid split along x and y, num_proc = (px, py)): the neighbour ranks' border cells -- q_out per step, flow
// direction and mask once -- arrive in a one-cell frame around the block.  Frame layout (F = 2 ny + 2 nx + 4 values): [0, ny) the
// west column x = -1, [ny, 2 ny) the east column x = nx, [2 ny, 2 ny + nx) the south row y = -1, [2 ny + nx, 2 ny + 2 nx) the north
// row y = ny, then the corners (-1, -1), (nx, -1), (-1, ny), (nx, ny).  A part without a neighbour holds zeros: the +0.0 contribution
// of a source outside the grid.  Null pointers: no neighbour at all (one domain), nothing outside the block is read.
struct RouteHalo {
    const double *q;
    const int *flow_dir;
    const int *mask;
};
// the frame index of a source cell outside the block (sx in [-1, nx], sy in [-1, ny], not both inside)
RH_DEV int route_frame_index(int nx, int ny, int sx, int sy, bool x_in, bool y_in) {
    if (y_in) return (sx < 0 ? 0 : ny) + sy;
    if (x_in) return 2 * ny + (sy < 0 ? 0 : nx) + sx;
    return 2 * ny + 2 * nx + (sx < 0 ? 0 : 1) + (sy < 0 ? 0 : 2);
}
RH_DEV double route_gather_value(const Arena &a, int nx, int ny, int src_plane, int64_t i, const RouteHalo &H) {
    const int ix = (int)(i / ny), iy = (int)(i % ny);
    const int CODE[8] = {64, 128, 1, 2, 4, 8, 16, 32};
    const int DX[8] = {0, -1, 1, 1, 0, -1, -1, -1};
    const int DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
    double v[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int sx = ix - DX[d], sy = iy - DY[d];
        const bool x_in = sx >= 0 && sx < nx, y_in = sy >= 0 && sy < ny;
        double q = 0.0;
        int fd = 0, mk = 0;
        if (x_in && y_in) {
            const int64_t s = (int64_t)sx * ny + sy;
            q = *rh_cell_any<const double>(a, src_plane, s);
            fd = *rh_cell_any<const int>(a, RH_P_flow_dir_topo, s);
            mk = *rh_cell_any<const int>(a, RH_P_maskCatch, s);
        } else if (H.q) {
            const int f = route_frame_index(nx, ny, sx, sy, x_in, y_in);
            q = H.q[f];
            fd = H.flow_dir[f];
            mk = H.mask[f];
        }
        v[d] = (fd == CODE[d] ? q : 0.0) * (double)mk;
    }
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}
__global__ __launch_bounds__(RH_BLOCK) void k_route_gather(Arena a, int nx, int ny, int src_plane, int dst_plane, RouteHalo H) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    *rh_cell_any<double>(a, dst_plane, i) = route_gather_value(a, nx, ny, src_plane, i, H);
}
// Device-driven routed stepping: the second and third pass with the gather in front of them folded in -- a column reads its eight
// neighbours' q_out (own columns from the arena, the neighbour ranks' border cells from the halo frame) instead of a q_in plane
// that a kernel of its own wrote: 4 launches per step instead of 6 (k_ctrl, k_routed_a2, k_routed_bg, k_routed_cg[_after]).
template <int P, int WHICH, typename T>
RH_DEV void ld_or_gather(const Arena &a, int64_t i, T &dst, int nx, int ny, const RouteHalo &H) {
    if constexpr (P == (WHICH == 0 ? (int)RH_P_q_sur_in : (int)RH_P_q_sub_in))
        dst = route_gather_value(a, nx, ny, WHICH == 0 ? (int)RH_P_q_sur_out : (int)RH_P_q_sub_out, i, H);
    else
        rh_ld(a, P, i, dst);
}
#define RH_PSTAGE_G(which, seq, rt, call)                     \
    RH_SEQ_##seq##_LOAD_##rt(LDG##which) call;                \
    if constexpr (SPARSE) { RH_SEQ_##seq##_SSTORE_##rt(ST) }  \
    else { RH_SEQ_##seq##_STORE_##rt(ST) }
#define LDG0(name) ld_or_gather<RH_P_##name, 0>(a, i, c.name, nx, ny, H);
#define LDG1(name) ld_or_gather<RH_P_##name, 1>(a, i, c.name, nx, ny, H);
template <bool SPARSE>
__global__ __launch_bounds__(RH_BLOCK, RH_STEP_WAVES) void k_routed_bg(Arena a, DevState *D, int nx, int ny, RouteHalo H) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const Consts K = D->K;
    const StepCtx X = D->X;
    Col c;
    RH_PSTAGE_G(0, routed_b, rt_route_surface_in, rt_route_surface_in(c))
    RH_PSTAGE_G(0, routed_b, rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X))
    RH_PSTAGE_G(0, routed_b, rt_route_subsurface_out, rt_route_subsurface_out(c))
}
template <bool AFTER, bool SPARSE>
__global__ __launch_bounds__(RH_BLOCK, RH_STEP_WAVES) void k_routed_cg(Arena a, DevState *D, int nx, int ny, RouteHalo H) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const Consts K = D->K;
    const StepCtx X = D->X;
    Col c;
    bool bad = false;
    if constexpr (AFTER) {
        RH_PSTAGE_G(1, routed_c_after, rt_route_subsurface_in, rt_route_subsurface_in(c))
        RH_PSTAGE_G(1, routed_c_after, rt_capillary_rise, rt_capillary_rise(c, X))
        RH_PSTAGE_G(1, routed_c_after, rt_storage, rt_storage(c, X))
        RH_PSTAGE_G(1, routed_c_after, rt_num_error_routed, bad = rt_num_error_routed(c, K))
        RH_PSTAGE_G(1, routed_c_after, rt_after_timestep_oned, rt_after_timestep_oned(c))
    } else {   // (with the output accumulators between the numerics and the rotation: never sparse)
#define RH_PSTAGE_GF(seq, rt, call) RH_SEQ_##seq##_LOAD_##rt(LDG1) call; RH_SEQ_##seq##_STORE_##rt(ST)
        RH_PSTAGE_GF(routed_c, rt_route_subsurface_in, rt_route_subsurface_in(c))
        RH_PSTAGE_GF(routed_c, rt_capillary_rise, rt_capillary_rise(c, X))
        RH_PSTAGE_GF(routed_c, rt_storage, rt_storage(c, X))
        RH_PSTAGE_GF(routed_c, rt_num_error_routed, bad = rt_num_error_routed(c, K))
#undef RH_PSTAGE_GF
    }
    if (bad) atomicOr(&D->words[2], 1ull);
}
// the rank's own border of one or two planes in the frame layout (what the neighbours' frames take): the columns x = 0 / nx - 1, the
// rows y = 0 / ny - 1 (strided in the arena), the corner cells (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1); only the parts set
// in `parts` (bit p: part p of route_frame_parts).  out1 may be null.
template <typename T>
__global__ void k_route_pack(Arena a, int nx, int ny, unsigned parts, int plane0, T *out0, int plane1, T *out1) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int part, x, y;
    if (t < ny) part = 0, x = 0, y = t;
    else if (t < 2 * ny) part = 1, x = nx - 1, y = t - ny;
    else if (t < 2 * ny + nx) part = 2, x = t - 2 * ny, y = 0;
    else if (t < 2 * ny + 2 * nx) part = 3, x = t - 2 * ny - nx, y = ny - 1;
    else if (t < 2 * ny + 2 * nx + 4) {
        const int k = t - 2 * ny - 2 * nx;
        part = 4 + k, x = (k & 1) ? nx - 1 : 0, y = (k & 2) ? ny - 1 : 0;
    } else
        return;
    if (!((parts >> part) & 1u)) return;
    const int64_t s = (int64_t)x * ny + y;
    out0[t] = *rh_cell_any<const T>(a, plane0, s);
    if (out1) out1[t] = *rh_cell_any<const T>(a, plane1, s);
}

#endif  // RH_ROUTING_H
