// rh_routing_host.h -- host side of settings.enable_routing_1D: the frame layout, the border pack, the halo exchange over RCCL and
// the rh_route_* / rh_*_routing entry points.  Part of the one translation unit roger_hip.hip, behind rh_ctx and rh_rccl.h.
#ifndef RH_ROUTING_HOST_H
#define RH_ROUTING_HOST_H

extern "C" {

// ---- settings.enable_routing_1D -------------------------------------------------------------------------------------------------
static size_t route_frame_size(const rh_ctx *ctx) { return 2 * (size_t)ctx->cfg.ny + 2 * (size_t)ctx->cfg.nx + 4; }
// the eight parts of the frame layout (k_route_pack, route_gather_value): west, east, south, north, then the corners south-west,
// south-east, north-west, north-east -- offset and length of each, and where its neighbour sits in the process grid
static const int ROUTE_PART_DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
static const int ROUTE_PART_DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};
static void route_frame_parts(const rh_ctx *ctx, size_t off[8], size_t len[8]) {
    const size_t nx = (size_t)ctx->cfg.nx, ny = (size_t)ctx->cfg.ny;
    const size_t o[8] = {0, ny, 2 * ny, 2 * ny + nx, 2 * ny + 2 * nx, 2 * ny + 2 * nx + 1, 2 * ny + 2 * nx + 2, 2 * ny + 2 * nx + 3};
    const size_t l[8] = {ny, ny, nx, nx, 1, 1, 1, 1};
    for (int p = 0; p < 8; ++p) off[p] = o[p], len[p] = l[p];
}
// the neighbour rank of every part (-1: none, the edge of the grid) from the communicator's process grid (ranks x-fastest,
// distributed.get_process_neighbors); the bits of the parts that have one
static unsigned route_neighbours(const rh_ctx *ctx, int peer[8]) {
    const int px = ctx->grid_px, py = ctx->grid_py, ix = ctx->comm_rank % px, iy = ctx->comm_rank / px;
    unsigned parts = 0;
    for (int p = 0; p < 8; ++p) {
        const int jx = ix + ROUTE_PART_DX[p], jy = iy + ROUTE_PART_DY[p];
        peer[p] = jx >= 0 && jx < px && jy >= 0 && jy < py ? jx + jy * px : -1;
        if (peer[p] >= 0) parts |= 1u << p;
    }
    return parts;
}
static int route_buffers(rh_ctx *ctx) {
    if (ctx->route_q) return RH_OK;
    const size_t F = route_frame_size(ctx);
    HIPCHK(ctx, ctx->route_q.alloc(2 * F * sizeof(double)));
    HIPCHK(ctx, ctx->route_i.alloc(4 * F * sizeof(int)));
    HIPCHK(ctx, hipMemsetAsync(ctx->route_q, 0, 2 * F * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->route_i, 0, 4 * F * sizeof(int), ctx->stream));
    return RH_OK;
}
static int route_check(rh_ctx *ctx, int which, const char *who) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->cfg.enable_routing_1D) return fail(ctx, RH_ERR_STATE, std::string(who) + ": the context was created without enable_routing_1D");
    if (which != 0 && which != 1) return fail(ctx, RH_ERR_ARG, std::string(who) + ": which must be 0 (surface) or 1 (subsurface)");
    return route_buffers(ctx);
}
// the own border: q_out of the routing (which >= 0) into route_q, or flow direction and mask into route_i -- one launch
static void route_pack(rh_ctx *ctx, int which, unsigned parts) {
    const int ny = (int)ctx->cfg.ny, nx = (int)ctx->cfg.nx;
    const size_t F = route_frame_size(ctx);
    const dim3 grid((unsigned)((F + 255) / 256)), block(256);
    if (which < 0)
        hipLaunchKernelGGL(k_route_pack<int>, grid, block, 0, ctx->stream, ctx->arena, nx, ny, parts, (int)RH_P_flow_dir_topo, ctx->route_i.get(),
                           (int)RH_P_maskCatch, ctx->route_i + F);
    else
        hipLaunchKernelGGL(k_route_pack<double>, grid, block, 0, ctx->stream, ctx->arena, nx, ny, parts,
                           which == 0 ? (int)RH_P_q_sur_out : (int)RH_P_q_sub_out, ctx->route_q.get(), 0, (double *)nullptr);
}
int rh_route_out(rh_ctx *ctx, int which) {
    int rc = route_check(ctx, which, "rh_route_out");
    if (rc) return rc;
    if (which == 0) LAUNCH_CELLS(ctx, k_route_surface_out);
    else LAUNCH_CELLS(ctx, k_route_subsurface_out);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
// the west / east parts of the frame layout: [0, ny) and [ny, 2 ny)
int rh_route_get_edges(rh_ctx *ctx, int which, double *q_lo, double *q_hi) {
    int rc = route_check(ctx, which, "rh_route_get_edges");
    if (rc) return rc;
    if (!q_lo || !q_hi) return fail(ctx, RH_ERR_ARG, "rh_route_get_edges: null pointer");
    const size_t ny = (size_t)ctx->cfg.ny;
    route_pack(ctx, which, 3u);
    CHECK_LAUNCH(ctx);
    HIPCHK(ctx, hipMemcpyAsync(q_lo, ctx->route_q, ny * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q_hi, ctx->route_q + ny, ny * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_route_get_static_edges(rh_ctx *ctx, int32_t *fd_lo, int32_t *fd_hi, int32_t *mk_lo, int32_t *mk_hi) {
    int rc = route_check(ctx, 0, "rh_route_get_static_edges");
    if (rc) return rc;
    if (!fd_lo || !fd_hi || !mk_lo || !mk_hi) return fail(ctx, RH_ERR_ARG, "rh_route_get_static_edges: null pointer");
    const size_t ny = (size_t)ctx->cfg.ny, F = route_frame_size(ctx);
    route_pack(ctx, -1, 3u);
    CHECK_LAUNCH(ctx);
    int32_t *dst[4] = {fd_lo, fd_hi, mk_lo, mk_hi};
    const size_t src[4] = {0, ny, F, F + ny};
    for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipMemcpyAsync(dst[k], ctx->route_i + src[k], ny * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
int rh_route_set_halo(rh_ctx *ctx, int side, const double *q, const int32_t *flow_dir, const int32_t *mask) {
    int rc = route_check(ctx, 0, "rh_route_set_halo");
    if (rc) return rc;
    if (side != 0 && side != 1) return fail(ctx, RH_ERR_ARG, "rh_route_set_halo: side must be 0 (x = -1) or 1 (x = nx)");
    const size_t ny = (size_t)ctx->cfg.ny, F = route_frame_size(ctx);
    if (flow_dir && mask) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->route_i + 2 * F + side * ny, flow_dir, ny * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->route_i + 3 * F + side * ny, mask, ny * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ctx->route_halo[side] = true;
        ctx->route_frame = true;
    }
    if (q) {
        if (!ctx->route_halo[side]) return fail(ctx, RH_ERR_STATE, "rh_route_set_halo: the side's flow direction and mask must be set first");
        HIPCHK(ctx, hipMemcpyAsync(ctx->route_q + F + side * ny, q, ny * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RH_OK;
}
static RouteHalo route_halo_of(rh_ctx *ctx) {
    if (!ctx->route_frame) return RouteHalo{nullptr, nullptr, nullptr};
    const size_t F = route_frame_size(ctx);
    return RouteHalo{ctx->route_q + F, ctx->route_i + 2 * F, ctx->route_i + 3 * F};
}
static int rh_route_gather_only(rh_ctx *ctx, int which) {
    int rc = route_check(ctx, which, "rh_route_in");
    if (rc) return rc;
    const RouteHalo H = route_halo_of(ctx);
    planes_touched(ctx);
    hipLaunchKernelGGL(k_route_gather, dim3(grid_for(ctx->n)), dim3(RH_BLOCK), 0, ctx->stream, ctx->arena, (int)ctx->cfg.nx, (int)ctx->cfg.ny,
                       which == 0 ? (int)RH_P_q_sur_out : (int)RH_P_q_sub_out, which == 0 ? (int)RH_P_q_sur_in : (int)RH_P_q_sub_in, H);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
int rh_route_in(rh_ctx *ctx, int which) {
    int rc = rh_route_gather_only(ctx, which);
    if (rc) return rc;
    if (which == 0) LAUNCH_CELLS(ctx, k_route_surface_in);
    else LAUNCH_CELLS(ctx, k_route_subsurface_in);
    CHECK_LAUNCH(ctx);
    return RH_OK;
}
// the neighbours' border cells over RCCL: one group per exchange, in it a send of the own part and a receive into the frame part per
// present neighbour (west, east, south, north, the corners; counts ny, nx, 1) -- on a (N, 1) grid the west and east columns only.
// Flow direction and mask go once (again after rh_comm_set_grid), q_out of the routing every time.
static int route_exchange(rh_ctx *ctx, int which) {
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, "routing: " + api->why);
    if (int rc = route_buffers(ctx)) return rc;   // (routed_core exchanges before its first gather allocates them)
    const size_t F = route_frame_size(ctx);
    size_t off[8], len[8];
    int peer[8];
    route_frame_parts(ctx, off, len);
    const unsigned parts = route_neighbours(ctx, peer);
    if (!ctx->route_static_done) {
        // a part without a neighbour holds zeros (also what an earlier grid left there)
        HIPCHK(ctx, hipMemsetAsync(ctx->route_q + F, 0, F * sizeof(double), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->route_i + 2 * F, 0, 2 * F * sizeof(int), ctx->stream));
        route_pack(ctx, -1, parts);
        CHECK_LAUNCH(ctx);
        NCCLCHK(ctx, api->GroupStart());
        for (int k = 0; k < 2; ++k) {   // k = 0: flow direction, 1: mask
            int *own = ctx->route_i + (size_t)k * F, *halo = ctx->route_i + (size_t)(2 + k) * F;
            for (int p = 0; p < 8; ++p) {
                if (peer[p] < 0) continue;
                NCCLCHK(ctx, api->Send(own + off[p], len[p], ncclInt32, peer[p], ctx->comm, ctx->stream));
                NCCLCHK(ctx, api->Recv(halo + off[p], len[p], ncclInt32, peer[p], ctx->comm, ctx->stream));
            }
        }
        NCCLCHK(ctx, api->GroupEnd());
        ctx->route_halo[0] = peer[0] >= 0;
        ctx->route_halo[1] = peer[1] >= 0;
        ctx->route_frame = parts != 0;
        ctx->route_static_done = true;
    }
    route_pack(ctx, which, parts);
    CHECK_LAUNCH(ctx);
    NCCLCHK(ctx, api->GroupStart());
    for (int p = 0; p < 8; ++p) {
        if (peer[p] < 0) continue;
        NCCLCHK(ctx, api->Send(ctx->route_q + off[p], len[p], ncclDouble, peer[p], ctx->comm, ctx->stream));
        NCCLCHK(ctx, api->Recv(ctx->route_q + F + off[p], len[p], ncclDouble, peer[p], ctx->comm, ctx->stream));
    }
    NCCLCHK(ctx, api->GroupEnd());
    return RH_OK;
}
static int route_all(rh_ctx *ctx, int which) {
    int rc = rh_route_out(ctx, which);
    if (rc) return rc;
    if (ctx->comm && ctx->comm_nranks > 1) {
        rc = route_exchange(ctx, which);
        if (rc) return rc;
    }
    return rh_route_in(ctx, which);
}
int rh_surface_routing(rh_ctx *ctx) { return route_all(ctx, 0); }
int rh_subsurface_routing(rh_ctx *ctx) { return route_all(ctx, 1); }

}  // extern "C"

#endif  // RH_ROUTING_HOST_H
