// rh_rccl.h -- RCCL resolved at run time (RcclApi / rccl_api) and the rh_comm_* entry points.  Part of the one translation
// unit roger_hip.hip, behind rh_ctx, fail and HIPCHK.
#ifndef RH_RCCL_H
#define RH_RCCL_H

// RCCL, resolved at run time: a single-GPU user needs no librccl, and a process that already holds one (PyTorch ships its own
// copy under the same soname) keeps using that one.
struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*GroupStart)();
    ncclResult_t (*GroupEnd)();
    ncclResult_t (*CommCount)(const ncclComm_t, int *);
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *);
    const char *(*GetErrorString)(ncclResult_t);
    bool ok;
    std::string why;
};
static RcclApi *rccl_api() {
    static RcclApi api = [] {
        RcclApi a{};
        void *h = nullptr;
        // RH_RCCL_LIB: this RCCL build and no other (a site's own build; tests/loopback_nccl.cpp, whose "ranks" are threads on one GPU)
        if (const char *own = std::getenv("RH_RCCL_LIB")) {
            h = dlopen(own, RTLD_NOW | RTLD_LOCAL);
            if (!h) {
                a.why = std::string("RH_RCCL_LIB: ") + (dlerror() ? dlerror() : "cannot be loaded");
                return a;
            }
        }
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if (h) break;
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!h) {
            a.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "");
            return a;
        }
        a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
        a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
        a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
        a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
        a.Send = (decltype(a.Send))dlsym(h, "ncclSend");
        a.Recv = (decltype(a.Recv))dlsym(h, "ncclRecv");
        a.GroupStart = (decltype(a.GroupStart))dlsym(h, "ncclGroupStart");
        a.GroupEnd = (decltype(a.GroupEnd))dlsym(h, "ncclGroupEnd");
        a.CommCount = (decltype(a.CommCount))dlsym(h, "ncclCommCount");
        a.CommUserRank = (decltype(a.CommUserRank))dlsym(h, "ncclCommUserRank");
        a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
        a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce && a.GetErrorString && a.Send && a.Recv && a.GroupStart &&
               a.GroupEnd && a.CommCount && a.CommUserRank;
        if (!a.ok) a.why = "librccl lacks an expected entry point";
        return a;
    }();
    return &api;
}
static void release_comm(rh_ctx *ctx) {
    if (ctx->comm && ctx->own_comm && rccl_api()->ok) (void)rccl_api()->CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->own_comm = false;
    ctx->comm_nranks = 1;
    ctx->comm_rank = 0;
    ctx->grid_px = ctx->grid_py = 1;
    ctx->route_static_done = false;
}
#define NCCLCHK(ctx, call)                                                                                                   \
    do {                                                                                                                     \
        ncclResult_t r_ = (call);                                                                                            \
        if (r_ != ncclSuccess) return fail(ctx, RH_ERR_HIP, std::string(#call) + ": " + rccl_api()->GetErrorString(r_));     \
    } while (0)

extern "C" {

int rh_comm_unique_id(void *id128) {
    if (!id128) return fail(nullptr, RH_ERR_ARG, "rh_comm_unique_id: null pointer");
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(nullptr, RH_ERR_STATE, "rh_comm_unique_id: " + api->why);
    ncclUniqueId id;
    NCCLCHK(nullptr, api->GetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return RH_OK;
}
int rh_comm_init(rh_ctx *ctx, const void *id128, int nranks, int rank) {
    if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return ctx ? fail(ctx, RH_ERR_ARG, "rh_comm_init: bad arguments") : RH_ERR_ARG;
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, "rh_comm_init: " + api->why);
    release_comm(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    NCCLCHK(ctx, api->CommInitRank(&ctx->comm, nranks, id, rank));
    ctx->own_comm = true;
    ctx->comm_nranks = nranks;
    ctx->comm_rank = rank;
    ctx->grid_px = nranks;
    ctx->grid_py = 1;
    return RH_OK;
}
int rh_set_comm(rh_ctx *ctx, void *nccl_comm) {
    if (!ctx) return RH_ERR_ARG;
    release_comm(ctx);
    ctx->comm = (ncclComm_t)nccl_comm;
    if (ctx->comm) {
        RcclApi *api = rccl_api();
        if (!api->ok) return fail(ctx, RH_ERR_STATE, "rh_set_comm: " + api->why);
        NCCLCHK(ctx, api->CommCount(ctx->comm, &ctx->comm_nranks));
        NCCLCHK(ctx, api->CommUserRank(ctx->comm, &ctx->comm_rank));
        ctx->grid_px = ctx->comm_nranks;
        ctx->grid_py = 1;
    }
    return RH_OK;
}
int rh_comm_set_grid(rh_ctx *ctx, int px, int py) {
    if (!ctx) return RH_ERR_ARG;
    if (!ctx->comm) return fail(ctx, RH_ERR_STATE, "rh_comm_set_grid: no communicator (rh_comm_init / rh_set_comm)");
    if (px < 1 || py < 1 || (int64_t)px * py != ctx->comm_nranks)
        return fail(ctx, RH_ERR_ARG, "rh_comm_set_grid: px * py must equal the communicator's " + std::to_string(ctx->comm_nranks) + " ranks");
    ctx->grid_px = px;
    ctx->grid_py = py;
    ctx->route_static_done = false;   // new neighbours: their flow direction and mask are exchanged again
    return RH_OK;
}
int rh_comm_info(rh_ctx *ctx, int *nranks, int *rank) {
    if (!ctx || !nranks || !rank) return ctx ? fail(ctx, RH_ERR_ARG, "rh_comm_info: null pointer") : RH_ERR_ARG;
    *nranks = 1;
    *rank = 0;
    if (!ctx->comm) return RH_OK;
    RcclApi *api = rccl_api();
    if (!api->ok) return fail(ctx, RH_ERR_STATE, "rh_comm_info: " + api->why);
    NCCLCHK(ctx, api->CommCount(ctx->comm, nranks));
    NCCLCHK(ctx, api->CommUserRank(ctx->comm, rank));
    return RH_OK;
}

}  // extern "C"

#endif  // RH_RCCL_H
