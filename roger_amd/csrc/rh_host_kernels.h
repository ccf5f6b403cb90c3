// rh_host_kernels.h -- the small kernels the host code launches itself: setup, transfer, the stand-alone entry points, the selftests.
// Part of the one translation unit roger_hip.hip, behind the device headers.
#pragma once
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

// rh_pow on the device for n argument pairs (tests: the same bits as the host's compilation of rh_pow.h)
extern "C" __global__ void k_selftest_rh_pow(const double *x, const double *y, double *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rh_pow(x[i], y[i]);
}

// np_sum144_window for n window starts over one 144-vector, one wavefront per start: out[2 j] by the kernels' function (the rotation path
// where it applies), out[2 j + 1] by the general path (tests: both are numpy's sum over the masked vector, bit for bit)
extern "C" __global__ void k_selftest_window(const double *v, const int64_t *itd, double *out) {
    const int64_t t = itd[blockIdx.x];
    auto get = [&](int k) { return v[k]; };
    const double a = np_sum144_window(get, t), b = np_sum144_window_general(get, t);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = a;
        out[2 * blockIdx.x + 1] = b;
    }
}
