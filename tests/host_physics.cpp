#define RH_HOST 1
#include "rh_physics.h"
// host_physics.cpp -- the device's own column code (roger_amd/csrc/rh_physics.h, compiled as host functions: RH_HOST) behind a C ABI,
// so that the tests can run every routine the fused step is made of on the CPU, from any state, and compare it with the oracle routine
// by routine (tests/host_physics.py loads it; tests/test_physics_host_vs_oracle.py).  TEST INFRASTRUCTURE: nothing under roger_amd/
// uses it.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -shared -fPIC -I include -I roger_amd/csrc tests/host_physics.cpp -o libhost_physics.so
//
// Every entry point runs over n columns of a structure-of-arrays snapshot: `planes` holds one pointer per plane of
// include/rh_fields.def, in that file's order (host_plane_name), each to n float64 or int32.  A column is loaded into a Col, the routine
// runs, every field is stored back.  Consts, StepCtx and Luts are the structures of rh_col.h, filled by the caller.
// Entry points that end in the numerics return 1 if every column passed the sanity check (the scalar sanity_ok), 0 otherwise; the
// others return 1.
//
// With -DHOST_PHYSICS_MAIN the file is a program of its own: a few hundred columns from a fixed seed through the setup routines and
// both step cores, for a sanitizer pass (-fsanitize=address,undefined) over this file's loads and stores.
#include <stdint.h>
#include <string.h>

struct PlaneInfo {
    const char *name;
    int is_int;
};
static const PlaneInfo PLANES[] = {
#define RH_DECL_F64_1(name) {#name, 0},
#define RH_DECL_F64_2(name) {#name, 0}, {#name "_m1", 0},
#define RH_DECL_I32_1(name) {#name, 1},
#define RH_DECL_I32_2(name) {#name, 1}, {#name "_m1", 1},
#define RH_FIELD(name, type, levels) RH_DECL_##type##_##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_DECL_F64_1
#undef RH_DECL_F64_2
#undef RH_DECL_I32_1
#undef RH_DECL_I32_2
};
static const int NPLANES = (int)(sizeof(PLANES) / sizeof(PLANES[0]));

static void load(Col &c, void *const *planes, int64_t i) {
    int p = 0;
#define RH_DECL_F64_1(name) c.name = ((const double *)planes[p++])[i];
#define RH_DECL_F64_2(name) RH_DECL_F64_1(name) RH_DECL_F64_1(name##_m1)
#define RH_DECL_I32_1(name) c.name = ((const int32_t *)planes[p++])[i];
#define RH_DECL_I32_2(name) RH_DECL_I32_1(name) RH_DECL_I32_1(name##_m1)
#define RH_FIELD(name, type, levels) RH_DECL_##type##_##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_DECL_F64_1
#undef RH_DECL_F64_2
#undef RH_DECL_I32_1
#undef RH_DECL_I32_2
}

static void store(const Col &c, void *const *planes, int64_t i) {
    int p = 0;
#define RH_DECL_F64_1(name) ((double *)planes[p++])[i] = c.name;
#define RH_DECL_F64_2(name) RH_DECL_F64_1(name) RH_DECL_F64_1(name##_m1)
#define RH_DECL_I32_1(name) ((int32_t *)planes[p++])[i] = c.name;
#define RH_DECL_I32_2(name) RH_DECL_I32_1(name) RH_DECL_I32_1(name##_m1)
#define RH_FIELD(name, type, levels) RH_DECL_##type##_##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_DECL_F64_1
#undef RH_DECL_F64_2
#undef RH_DECL_I32_1
#undef RH_DECL_I32_2
}

// one entry point: load, `body` (which may clear `ok`), store
#define HOST_ENTRY(fn, body)                                                                                              \
    extern "C" int host_##fn(void *const *planes, int64_t n, const Consts *Kp, const StepCtx *Xp, const Luts *Lp) {      \
        const Consts &K = *Kp;                                                                                            \
        const StepCtx &X = *Xp;                                                                                           \
        const Luts &L = *Lp;                                                                                              \
        (void)K; (void)X; (void)L;                                                                                        \
        int ok = 1;                                                                                                       \
        for (int64_t i = 0; i < n; ++i) {                                                                                 \
            Col c;                                                                                                        \
            load(c, planes, i);                                                                                           \
            body;                                                                                                         \
            store(c, planes, i);                                                                                          \
        }                                                                                                                 \
        return ok;                                                                                                        \
    }

extern "C" {
int host_num_planes(void) { return NPLANES; }
const char *host_plane_name(int p) { return (p >= 0 && p < NPLANES) ? PLANES[p].name : nullptr; }
int host_plane_is_int(int p) { return (p >= 0 && p < NPLANES) ? PLANES[p].is_int : -1; }
// the sizes of the structures the caller fills, for the binding's own layout check
int64_t host_sizeof(int which) {
    return which == 0 ? (int64_t)sizeof(Consts) : which == 1 ? (int64_t)sizeof(StepCtx) : which == 2 ? (int64_t)sizeof(Luts) : (int64_t)sizeof(Col);
}
}

// the routines of the step, in the order of rt_step_core / rt_step_core_lateral
HOST_ENTRY(rt_interception, rt_interception(c, K))
HOST_ENTRY(rt_evapotranspiration, rt_evapotranspiration(c, K))
HOST_ENTRY(rt_snow, rt_snow(c, K, X))
HOST_ENTRY(rt_infiltration, rt_infiltration(c, K, X))
HOST_ENTRY(rt_subsurface_runoff, rt_subsurface_runoff(c, X))
HOST_ENTRY(rt_subsurface_runoff_lateral, rt_subsurface_runoff_lateral(c, K, X))
HOST_ENTRY(rt_capillary_rise, rt_capillary_rise(c, X))
HOST_ENTRY(rt_storage, rt_storage(c, X))
HOST_ENTRY(rt_num_error, ok &= !rt_num_error(c, K))
HOST_ENTRY(rt_num_error_lateral, ok &= !rt_num_error_lateral(c, K))
HOST_ENTRY(rt_step_core, ok &= !rt_step_core(c, K, X))
HOST_ENTRY(rt_step_core_lateral, ok &= !rt_step_core_lateral(c, K, X))
HOST_ENTRY(rt_after_timestep, rt_after_timestep(c))
HOST_ENTRY(rt_after_timestep_oned, rt_after_timestep_oned(c))
// the setup routines behind rh_topo, rh_params_surface (also the monthly `set_parameters`), rh_params_soil, rh_initial_conditions
HOST_ENTRY(rt_topo, rt_topo(c))
HOST_ENTRY(rt_params_surface, rt_params_surface(c, L, X))
HOST_ENTRY(rt_params_soil, rt_params_soil(c, K, L))
HOST_ENTRY(rt_initial_conditions, rt_initial_conditions(c))

#ifdef HOST_PHYSICS_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }

int main(int argc, char **argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 300;
    std::vector<std::vector<double>> f64(NPLANES);
    std::vector<std::vector<int32_t>> i32(NPLANES);
    std::vector<void *> planes(NPLANES);
    for (int p = 0; p < NPLANES; ++p) {   // exactly n elements each, so that an index past a plane's end is seen
        if (PLANES[p].is_int) { i32[p].assign(n, 0); planes[p] = i32[p].data(); }
        else { f64[p].assign(n, 0.0); planes[p] = f64[p].data(); }
    }
    auto F = [&](const char *nm) -> double * {
        for (int p = 0; p < NPLANES; ++p) if (!strcmp(PLANES[p].name, nm)) return (double *)planes[p];
        abort();
    };
    auto I = [&](const char *nm) -> int32_t * {
        for (int p = 0; p < NPLANES; ++p) if (!strcmp(PLANES[p].name, nm)) return (int32_t *)planes[p];
        abort();
    };
    static const int LU[] = {8, 5, 10, 13, 0, 98, 14, 20, 999, 11, 12, 6, 7, 9, 15, 31, 32, 33, 40, 41, 50, 100, 16, 17};
    static const double ZGW[] = {0.3, 1.5, 2.5, 6.0, 10.0, 1000.0};
    for (int64_t i = 0; i < n; ++i) {
        I("maskCatch")[i] = 1;
        I("lu_id")[i] = LU[i % 24];
        F("ta")[i] = F("ta_m1")[i] = 15.0;
        F("c_int")[i] = F("c_root")[i] = 1.0;
        F("z_soil")[i] = (double)(int64_t)uni(400, 2000);
        F("dmpv")[i] = 25.0 * (double)(i % 4);
        F("lmpv")[i] = fmin(300.0 * (double)(i % 5), 0.9 * F("z_soil")[i]);
        F("theta_ac")[i] = uni(0.05, 0.2); F("theta_ufc")[i] = uni(0.08, 0.25); F("theta_pwp")[i] = uni(0.05, 0.3);
        F("ks")[i] = uni(0.5, 50); F("kf")[i] = 2500.0;
        F("sealing")[i] = LU[i % 24] == 0 ? uni(0.2, 0.8) : 0.0;
        F("S_dep_tot")[i] = (i % 4 == 3) ? 10.0 : 0.0;
        F("z_gw")[i] = F("z_gw_m1")[i] = ZGW[i % 6];
        F("slope")[i] = 0.05; F("dmph")[i] = 50.0;
    }
    Consts K;
    memset(&K, 0, sizeof K);
    K.pi = 3.14159265358979323846; K.r_mp = 2.5; K.l_sc = 10000; K.sf = 3; K.ta_fm = 0; K.rmax = 30; K.transp_water_stress = 0.75;
    K.atol = 1e-2; K.rtol = 1e-2; K.clay_min = 0.01; K.clay_max = 0.71; K.theta_rew_min = 0.02; K.theta_rew_max = 0.24; K.rew_min = 2;
    K.rew_max = 12; K.z_evap_max = 150; K.zroot_to_zsoil_max = 0.7; K.a_bc = 2; K.b_bc = 2; K.end_event = 21600; K.hpi = 5; K.dx = 1; K.dy = 1;
    static Luts L;
    memset(&L, 0, sizeof L);
    for (int r = 0; r < 24; ++r) {   // a row per land use: any plausible numbers do, the point is the indexing
        L.ilu[r * 13] = L.gc[r * 13] = L.gcm[r * 2] = L.rdlu[r * 7] = (double)LU[r];
        for (int m = 1; m < 13; ++m) { L.ilu[r * 13 + m] = 0.2 + 0.1 * m; L.gc[r * 13 + m] = 0.05 * m; }
        L.gcm[r * 2 + 1] = 0.8;
        L.rdlu[r * 7 + 1] = 200.0 + 50.0 * r;
    }
    StepCtx X;
    memset(&X, 0, sizeof X);
    X.month_tau = 5; X.sel_p = X.sel_w = -1;
    host_rt_topo(planes.data(), n, &K, &X, &L);
    host_rt_params_surface(planes.data(), n, &K, &X, &L);
    host_rt_params_soil(planes.data(), n, &K, &X, &L);
    for (int64_t i = 0; i < n; ++i) {
        const double sat = F("theta_ac")[i] + F("theta_ufc")[i] + F("theta_pwp")[i], pwp = F("theta_pwp")[i];
        F("theta_rz")[i] = F("theta_rz_m1")[i] = pwp + uni(0.1, 0.95) * (sat - pwp);
        F("theta_ss")[i] = F("theta_ss_m1")[i] = pwp + uni(0.1, 0.95) * (sat - pwp);
    }
    host_rt_initial_conditions(planes.data(), n, &K, &X, &L);
    int ok = 1;
    long steps = 0;
    const double DT[3] = {1.0 / 6, 1.0, 24.0};
    for (int lateral = 0; lateral < 2; ++lateral)
        for (int k = 0; k < 12; ++k) {   // rain in the first steps of each round (an event begins, pauses, ends), then dry
            X.dt = DT[k % 3];
            X.cond1 = k == 0; X.cond2 = k == 4; X.cond3 = k == 5; X.cond4 = k == 9; X.cond5 = k < 9;
            for (int64_t i = 0; i < n; ++i) {
                F("prec")[i] = (k < 4 || (k >= 5 && k < 8)) ? 4.0 * X.dt : 0.0;
                F("pet")[i] = F("pet_res")[i] = 0.15 * X.dt;
                F("ta")[i] = k == 7 ? -2.0 : 12.0;
            }
            ok &= lateral ? host_rt_step_core_lateral(planes.data(), n, &K, &X, &L) : host_rt_step_core(planes.data(), n, &K, &X, &L);
            (lateral ? host_rt_after_timestep_oned : host_rt_after_timestep)(planes.data(), n, &K, &X, &L);
            ++steps;
        }
    double total = 0;
    for (int64_t i = 0; i < n; ++i) total += I("maskCatch")[i] ? F("S")[i] : 0.0;
    printf("columns %lld steps %ld sanity %d water %.6f\n", (long long)n, steps, ok, total);
    return (total == total) ? 0 : 1;
}
#endif
