// substep_dry_check.cpp -- the dry paths of h_inf_mp / h_inf_sc (rh_physics.h) against the sub-step loops they replace, on the host.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I roger_amd/csrc tools/substep_dry_check.cpp -o substep_dry_check -lm -pthread
//   ./substep_dry_check [number of random states, default 10000000] [threads, default: the machine's, at most 16]
//
// rh_physics.h is compiled as host code (RH_HOST, rh_col.h: a "wavefront" is one column, so the wave-uniform vote is the column's own
// predicate).  Every state runs the macropore and the crack stage twice, with DryPath<false> (the loops) and with DryPath<true> (the dry path
// where its predicate holds, the loops otherwise), and the two columns must agree in every field.  The states: a systematic part -- a
// dry and a wet base state, every input of the two stages replaced in turn by each of a list of special values (zeros of both signs,
// NaN, infinities, denormal, tiny, huge, negative), at the three sub-step counts 1 / 5 / 120 and with the mask on and off -- and a random
// part, drawn from the ranges the model's states live in, with special values mixed in at random.  Prints how many stage calls took
// which path; exit status 1 on the first mismatch, 2 if a path was hardly taken.
// "Agree": the same bits, or both NaN.  Which of two NaN operands an instruction passes on (sign and payload) depends on the operand
// order the compiler happened to choose for a commutative operation, and that differs between two instantiations of the same source.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#define RH_HOST 1
static thread_local unsigned long long rh_dry_taken[2];   // stage calls that ended in the dry path: macropores, cracks
#define RH_DRY_NOTE(k) (++rh_dry_taken[k])
#include "rh_physics.h"

static thread_local uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }

static const double SPECIAL[] = {0.0, -0.0, NAN, INFINITY, -INFINITY, 4.9406564584124654e-324, 1e-300, 1e-160, 1e160, 1e300, -1.0, -1e-300, 1.0, 2.5};
static const int NSPECIAL = sizeof(SPECIAL) / sizeof(SPECIAL[0]);

// the double inputs of the two stages
#define INPUTS(X)                                                                                                                    \
    X(z0) X(theta_d) X(dmpv) X(lmpv) X(ks) X(wfs) X(mp_drain_area) X(y_mp_m1) X(inf_mp_event_csum) X(z_wf) X(z_wf_t1) X(z_wf_t1_m1)   \
    X(z_root) X(S_ac_rz) X(S_ufc_rz) X(S_lp_rz) X(S_fp_rz) X(inf_mat_rz) X(S_ac_ss) X(S_ufc_ss) X(S_lp_ss) X(S_fp_ss) X(z_sc) X(y_sc_m1) \
    X(inf_sc_event_csum)
enum {
#define X(name) IN_##name,
    INPUTS(X)
#undef X
    N_INPUTS
};
static double *input(Col &c, int k) {
    switch (k) {
#define X(name) case IN_##name: return &c.name;
        INPUTS(X)
#undef X
    }
    return nullptr;
}

static void base_state(Col &c, bool wet) {
    memset(&c, 0, sizeof c);
    c.maskCatch = 1; c.no_wf = 1;
    c.z0 = wet ? 1.5 : 0.0;
    c.theta_d = 0.12; c.dmpv = 50.0; c.lmpv = 300.0; c.ks = 5.0; c.wfs = 120.0; c.mp_drain_area = 0.6;
    c.y_mp_m1 = 14.0; c.inf_mp_event_csum = 3.0; c.z_wf = 40.0; c.z_wf_t1 = 40.0; c.z_wf_t1_m1 = 35.0; c.z_root = 400.0;
    c.S_ac_rz = 40.0; c.S_ufc_rz = 40.0; c.S_lp_rz = 5.0; c.S_fp_rz = 20.0; c.inf_mat_rz = 0.5;
    c.S_ac_ss = 160.0; c.S_ufc_ss = 160.0; c.S_lp_ss = 10.0; c.S_fp_ss = 90.0;
    c.z_sc = 150.0; c.y_sc_m1 = 0.002; c.inf_sc_event_csum = 0.4;
}

static void random_state(Col &c) {
    memset(&c, 0, sizeof c);
    c.maskCatch = uni() < 0.95 ? 1 : 0;
    c.no_wf = uni() < 0.8 ? 1 : (uni() < 0.8 ? 2 : 0);
    c.z0 = uni() < 0.6 ? 0.0 : uni(0, 20);
    c.theta_d = uni() < 0.05 ? 0.0 : uni(0, 0.45);
    c.dmpv = uni() < 0.2 ? 0.0 : uni(1, 250);
    c.lmpv = uni() < 0.1 ? 0.0 : uni(1, 1500);
    c.ks = uni(0.01, 150); c.wfs = uni(5, 1500); c.mp_drain_area = uni(0, 1);
    c.y_mp_m1 = uni() < 0.3 ? 0.0 : uni(0, 120);
    c.inf_mp_event_csum = uni() < 0.3 ? 0.0 : uni(0, 60);
    c.z_wf = uni() < 0.3 ? 0.0 : uni(0, 1600);
    c.z_wf_t1 = uni() < 0.3 ? 0.0 : uni(0, 1600);
    c.z_wf_t1_m1 = uni() < 0.5 ? c.z_wf_t1 : uni(0, 1600);
    c.z_root = uni(100, 1500);
    c.S_ac_rz = uni(0, 200); c.S_ufc_rz = uni(0, 200); c.S_lp_rz = uni(0, 200); c.S_fp_rz = uni(0, 200); c.inf_mat_rz = uni(0, 10);
    c.S_ac_ss = uni(0, 400); c.S_ufc_ss = uni(0, 400); c.S_lp_ss = uni(0, 400); c.S_fp_ss = uni(0, 400);
    c.z_sc = uni() < 0.3 ? 0.0 : uni(0, 700);
    c.y_sc_m1 = uni() < 0.3 ? 0.0 : uni(0, 0.01);
    c.inf_sc_event_csum = uni() < 0.3 ? 0.0 : uni(0, 20);
    if (uni() < 0.25) {   // special values in one to three inputs
        for (int k = 1 + (int)(rnd() % 3); k > 0; --k) *input(c, (int)(rnd() % N_INPUTS)) = SPECIAL[rnd() % NSPECIAL];
    }
}

static thread_local unsigned long long n_states, n_loops[2];
static const char *input_name(int k) {
    static const char *names[] = {
#define X(name) #name,
        INPUTS(X)
#undef X
    };
    return names[k];
}

static bool same_f64(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }
static bool same_col(const Col &a, const Col &b) {
    bool same = true;
#define RH_DECL_F64_1(name) same = same && same_f64(a.name, b.name);
#define RH_DECL_F64_2(name) RH_DECL_F64_1(name) RH_DECL_F64_1(name##_m1)
#define RH_DECL_I32_1(name) same = same && a.name == b.name;
#define RH_DECL_I32_2(name) RH_DECL_I32_1(name) RH_DECL_I32_1(name##_m1)
#define RH_FIELD(name, type, levels) RH_DECL_##type##_##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
#undef RH_DECL_F64_1
#undef RH_DECL_F64_2
#undef RH_DECL_I32_1
#undef RH_DECL_I32_2
    return same;
}

static void report(const Col &a, const Col &b, const Col &in, const Consts &K, double dt) {
    printf("MISMATCH at dt = %g, maskCatch = %d, no_wf = %d, r_mp = %g, l_sc = %g\n", dt, in.maskCatch, in.no_wf, K.r_mp, K.l_sc);
    Col in2 = in;
    for (int k = 0; k < N_INPUTS; ++k) printf("  in  %-20s %.17g\n", input_name(k), *input(in2, k));
#define RH_DECL_F64_1(name) if (!same_f64(a.name, b.name)) printf("  out %-20s loops %.17g  dry %.17g\n", #name, a.name, b.name);
#define RH_DECL_F64_2(name) RH_DECL_F64_1(name) RH_DECL_F64_1(name##_m1)
#define RH_DECL_I32_1(name) if (a.name != b.name) printf("  out %-20s loops %d  dry %d\n", #name, a.name, b.name);
#define RH_DECL_I32_2(name) RH_DECL_I32_1(name) RH_DECL_I32_1(name##_m1)
#define RH_FIELD(name, type, levels) RH_DECL_##type##_##levels(name)
#include "rh_fields.def"
#undef RH_FIELD
}

// both stages, as the pipeline runs them one after the other, with the loops and with the dry path
static bool check(const Col &in, const Consts &K, double dt) {
    const int n = h_inf_substeps(dt);
    Col a, b;
    memcpy(&a, &in, sizeof in);
    memcpy(&b, &in, sizeof in);
    h_inf_mp(a, K, dt, n, (double)a.maskCatch, DryPath<false>());
    h_inf_sc(a, K, dt, n, (double)a.maskCatch, DryPath<false>());
    const unsigned long long t0 = rh_dry_taken[0], t1 = rh_dry_taken[1];
    h_inf_mp(b, K, dt, n, (double)b.maskCatch, DryPath<true>());
    h_inf_sc(b, K, dt, n, (double)b.maskCatch, DryPath<true>());
    n_loops[0] += rh_dry_taken[0] == t0;
    n_loops[1] += rh_dry_taken[1] == t1;
    ++n_states;
    if (!same_col(a, b)) {
        report(a, b, in, K, dt);
        return false;
    }
    return true;
}

int main(int argc, char **argv) {
    const unsigned long long n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    Consts K;
    memset(&K, 0, sizeof K);
    K.pi = 3.14159265358979323846; K.r_mp = 2.5; K.l_sc = 10000.0;
    const double DT[3] = {1.0 / 6, 1.0, 24.0};   // hours: 1, 5 and 120 sub-steps
    if (h_inf_substeps(DT[0]) != 1 || h_inf_substeps(DT[1]) != 5 || h_inf_substeps(DT[2]) != 120) return 3;

    // systematic part
    for (int wet = 0; wet < 2; ++wet)
        for (int mask = 0; mask < 2; ++mask)
            for (int nowf = 0; nowf < 3; ++nowf)
                for (int d = 0; d < 3; ++d) {
                    Col c;
                    base_state(c, wet);
                    c.maskCatch = mask; c.no_wf = nowf;
                    if (!check(c, K, DT[d])) return 1;
                    for (int k = 0; k < N_INPUTS; ++k)
                        for (int s = 0; s < NSPECIAL; ++s) {
                            base_state(c, wet);
                            c.maskCatch = mask; c.no_wf = nowf;
                            *input(c, k) = SPECIAL[s];
                            if (!check(c, K, DT[d])) return 1;
                            // ... and with an empty event sum / a radius below the macropore's own besides
                            c.inf_mp_event_csum = k == IN_inf_mp_event_csum ? c.inf_mp_event_csum : 0.0;
                            c.y_mp_m1 = k == IN_y_mp_m1 ? c.y_mp_m1 : 1.0;
                            if (!check(c, K, DT[d])) return 1;
                        }
                }
    // the settings in turn: pi, r_mp, l_sc
    for (int which = 0; which < 3; ++which)
        for (int s = 0; s < NSPECIAL; ++s)
            for (int d = 0; d < 3; ++d) {
                Consts K2 = K;
                (which == 0 ? K2.pi : which == 1 ? K2.r_mp : K2.l_sc) = SPECIAL[s];
                Col c;
                base_state(c, false);
                if (!check(c, K2, DT[d])) return 1;
            }
    const unsigned long long n_systematic = n_states;

    // random part, over the threads: mostly hourly and 10-minute steps (a wet daily state runs 120 sub-steps twice)
    unsigned nt = argc > 2 ? (unsigned)atoi(argv[2]) : std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    struct Part { unsigned long long states, dry[2], loops[2]; bool ok; };
    std::vector<Part> part(nt);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < nt; ++w)
        pool.emplace_back([&, w] {
            rng_state = 0x9E3779B97F4A7C15ull * (2 * w + 3);
            Part &p = part[w];
            p.ok = true;
            for (unsigned long long i = w; i < n_random && p.ok; i += nt) {
                Col c;
                random_state(c);
                const double u = uni();
                p.ok = check(c, K, DT[u < 0.47 ? 0 : (u < 0.95 ? 1 : 2)]);
            }
            p.states = n_states;
            for (int k = 0; k < 2; ++k) p.dry[k] = rh_dry_taken[k], p.loops[k] = n_loops[k];
        });
    for (auto &t : pool) t.join();
    for (const Part &p : part) {
        if (!p.ok) return 1;
        n_states += p.states;
        for (int k = 0; k < 2; ++k) rh_dry_taken[k] += p.dry[k], n_loops[k] += p.loops[k];
    }
    printf("states %llu (systematic %llu, random %llu): all fields equal bit for bit (NaN for NaN)\n", n_states, n_systematic, n_random);
    printf("macropores: dry path %llu, loops %llu\n", rh_dry_taken[0], n_loops[0]);
    printf("cracks:     dry path %llu, loops %llu\n", rh_dry_taken[1], n_loops[1]);
    for (int k = 0; k < 2; ++k)
        if (rh_dry_taken[k] * 10 < n_states || n_loops[k] * 10 < n_states) return 2;
    return 0;
}
