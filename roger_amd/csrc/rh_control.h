// rh_control.h -- the control part of a step (set_forcing hook, predicate words, forcing aggregates in NumPy's order, the dt
// decision, event bookkeeping) in its three forms -- workgroup kernels, one wavefront (k_ctrl, the fused kernel's tail), the per-cell
// front -- with the summary, export and small scalar kernels.  Part of the one translation unit roger_hip.hip.
#ifndef RH_CONTROL_H
#define RH_CONTROL_H

// ---------------------------------------------------------------------------------------------
// adaptive time stepping (adaptive_time_stepping.py:22-381)
// ---------------------------------------------------------------------------------------------
// The benchmark's `set_forcing` and `set_parameters` hooks (benchmarks/SVAT_benchmark.py:105-110,
// 151-171) on the device: at midnight take the next 144 forcing slots and the calendar entry;
// flag a month change.  The two pieces every form of the control part shares: what a new day, beginning at slot i0 of the resident series,
// does to the scalars, and set_parameters' month-change test.  How a form publishes D->monthly / D->per_cell / err_flags (at once, or
// deferred through RH_SIDE_*) stays with the form.
RH_DEV void hook_new_day(const DevState *D, rh_scalars &S, int64_t i0) {
    S.itt_day = 0;
    S.year[1] = D->calendar[0][i0];
    S.month[1] = D->calendar[1][i0];
    S.doy[1] = D->calendar[2][i0];
    S.itt_forc = i0 + RH_SLOTS_PER_DAY;
}
RH_DEV bool month_changed(const rh_scalars *S) { return (S->month[1] != S->month[0]) && (S->itt > 1); }   // (a pointer: hooks_set_forcing's S is D->S in memory, and itt is read only if the months differ)
// Called by one whole workgroup of RH_BLOCK threads.
RH_DEV void hooks_set_forcing(DevState *D) {
    rh_scalars &S = D->S;
    const bool midnight = (S.time % 86400 == 0);
    const int64_t i0 = S.itt_forc;
    const bool have = midnight && (i0 + RH_SLOTS_PER_DAY <= D->nitt_forc);
    __syncthreads();  // everybody has read S before thread 0 changes it
    if (have && threadIdx.x < RH_SLOTS_PER_DAY)
        for (int k = 0; k < 3; ++k) D->forc[k][threadIdx.x] = D->series[k][i0 + threadIdx.x];
    if (have && threadIdx.x == 0) D->day_cache_ok = 0;
    if (have && D->n_stations > 0) {   // the series are (n_stations, nitt_forc): the day of every station
        const int S = D->n_stations;
        for (int q = threadIdx.x; q < 3 * S * RH_SLOTS_PER_DAY; q += RH_BLOCK) {
            const int v = q / (S * RH_SLOTS_PER_DAY), r = q % (S * RH_SLOTS_PER_DAY), st = r / RH_SLOTS_PER_DAY, j = r % RH_SLOTS_PER_DAY;
            D->forc_multi[q] = D->series[v][(size_t)st * D->nitt_forc + i0 + j];
        }
    }
    if (threadIdx.x == 0) {
        if (have) {
            hook_new_day(D, S, i0);
            D->per_cell = D->weights[0] ? 1 : 0;
        }
        D->monthly = month_changed(&S);
        if (midnight && !have) D->err_flags |= RH_DEVERR_FORCING;   // the step would run on yesterday's forcing: reported by rh_sync / rh_get_scalars
    }
    __threadfence();
    __syncthreads();
}
__global__ __launch_bounds__(RH_BLOCK) void k_set_forcing(DevState *D) { hooks_set_forcing(D); }
// Weighted station forcing (eberbaechle/svat_distributed/svat.py:276-296: prec_day = PREC * prec_weight, ta_day = TA +
// ta_offset, pet_day = PET * pet_weight): the day's series stays one 144-vector, staged in LDS, and every column forms
// its own values from its three weights on the fly -- no (n, 144) arrays, 24 bytes of weights per column and step.
struct DaySeries {
    double f[3][RH_SLOTS_PER_DAY];
};
// The day a kernel in front of the fused step works on when the set_forcing hook rides along (k_cell_front): at midnight, with a day left
// in the resident series, that is the NEXT day -- read straight from the series; the kernel's last wavefront then does what the hook does to
// the state (front_ctrl), and nothing has to run in front of the kernel.
struct FreshDay {
    bool fresh;     // the hook finds midnight and a day left: the new day
    bool missing;   // midnight, but the series is exhausted (the step runs on yesterday's forcing and the error is reported)
    int64_t i0;     // first slot of the new day in the series
    int64_t itd;    // itt_day as the hook leaves it
};
RH_DEV FreshDay fresh_day(const DevState *D, int hooks) {
    FreshDay f;
    const bool midnight = hooks && (D->S.time % 86400 == 0);
    f.i0 = D->S.itt_forc;
    f.fresh = midnight && (f.i0 + RH_SLOTS_PER_DAY <= D->nitt_forc);
    f.missing = midnight && !f.fresh;
    f.itd = f.fresh ? 0 : D->S.itt_day;
    return f;
}
RH_DEV void stage_day(const DevState *D, DaySeries &s, const FreshDay *fd = nullptr) {
    const bool fresh = fd && fd->fresh;
    for (int k = threadIdx.x; k < 3 * RH_SLOTS_PER_DAY; k += RH_BLOCK) {
        const int v = k / RH_SLOTS_PER_DAY, j = k % RH_SLOTS_PER_DAY;
        s.f[v][j] = fresh ? D->series[v][fd->i0 + j] : D->forc[v][j];
    }
    __syncthreads();
}
// slot k (uniform) of a variable from a wavefront's registers (ctrl_inputs, k_cell_front) (x0, x1, x2: the lane's slots lane, lane + 64, lane + 128)
RH_DEV double lane_double(double x, int l) {   // lane l's x (l uniform): v_readlane, no trip through the LDS crossbar
    const long long bits = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)bits, l), hi = __builtin_amdgcn_readlane((int)(bits >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
RH_DEV double ctrl_slot(double x0, double x1, double x2, int k) {
    // The register is chosen by a UNIFORM branch, not by a select in front of the read: under a divergent mask a select leaves the
    // switched-off lanes' copy unwritten, and v_readlane reads whatever lane it is told to (the registers themselves were loaded with
    // every lane on).
    const int r = __builtin_amdgcn_readfirstlane(k >> 6), l = k & 63;
    if (r == 0) return lane_double(x0, l);
    if (r == 1) return lane_double(x1, l);
    return lane_double(x2, l);
}
// The day's series as a column sees it: the one shared series staged in LDS, or -- with several stations -- its station's rows of
// forc_multi (a table of 3 x n_stations x 144 values: cache-resident; on a fresh day the rows of the series themselves); a column without
// a station reads zeros.
struct DayView {
    const DaySeries *lds;  // null: the one series is read where it lies (DevState::forc) -- a step that needs six slots of it does not stage the day
    const double *sv[3];   // several stations: slot 0 of station 0, per variable; one series without staging: DevState::forc[v]
    size_t ststride;       // ... and the distance between two stations
    bool multi;
    int st;
    RH_DEV double operator()(int v, int k) const {
        if (!multi) return lds ? lds->f[v][k] : sv[v][k];
        return st < 0 ? 0.0 : sv[v][(size_t)st * ststride + k];
    }
};
RH_DEV DayView day_view(const DevState *D, const DaySeries &lds, int64_t i, const FreshDay *fd = nullptr, bool staged = true) {
    DayView d;
    d.lds = staged ? &lds : nullptr;
    d.multi = D->n_stations > 0;
    d.st = d.multi ? D->station_idx[i] : 0;
    const bool fresh = fd && fd->fresh;

    for (int v = 0; v < 3; ++v)
        d.sv[v] = !d.multi ? (staged ? nullptr : (fresh ? D->series[v] + fd->i0 : &D->forc[v][0]))   // (fresh: the day the hook is about to bring)
                           : (fresh ? D->series[v] + fd->i0 : D->forc_multi + (size_t)v * D->n_stations * RH_SLOTS_PER_DAY);
    d.ststride = fresh ? (size_t)D->nitt_forc : (size_t)RH_SLOTS_PER_DAY;
    return d;
}
// start-of-step predicates over the columns (adaptive_time_stepping.py:38-81), grid-stride
__global__ __launch_bounds__(RH_BLOCK) void k_pred1(Arena a, DevState *D, int force_daily) {
    const Consts K = D->K;
    unsigned long long b = 0;
    const bool per_cell = D->per_cell != 0, weighted = D->weights[0] != nullptr;
    // weighted station forcing: the day's series changes at midnight only, so the forcing bits of a workgroup's columns
    // (the same columns every step: the grid-stride mapping is fixed) are formed once a day and kept
    const bool daily = force_daily || D->S.itt_day == 0;
    __shared__ DaySeries day;
    if (per_cell && weighted && daily) stage_day(D, day);
    for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * RH_BLOCK) {
        double swe, swe_top;
        rh_ld(a, RH_P_swe, i, swe);
        rh_ld(a, RH_P_swe_top, i, swe_top);
        b |= !(swe <= 0) ? BIT(PB_SWE_NOT_LE0) : 0;
        b |= (swe > 0) ? BIT(PB_SWE_GT0) : 0;
        b |= !(swe_top <= 0) ? BIT(PB_SWETOP_NOT_LE0) : 0;
        b |= (swe_top > 0) ? BIT(PB_SWETOP_GT0) : 0;
        if (per_cell && weighted) {
            if (daily) {
                const double pw = D->weights[0][i], toff = D->weights[1][i];
                const DayView F = day_view(D, day, i);
                for (int k = 0; k < RH_SLOTS_PER_DAY; ++k) b |= forcing_bits(F(0, k) * pw, F(1, k) + toff, K);
            }
        } else if (per_cell) {
            const double *p = D->forc_cell[0] + i, *t = D->forc_cell[1] + i;   // (144, n): stride n between the slots
            for (int k = 0; k < RH_SLOTS_PER_DAY; ++k) b |= forcing_bits(p[(size_t)k * a.n], t[(size_t)k * a.n], K);
        }
    }
    if (per_cell && weighted) {   // keep / reuse the day's forcing bits of this workgroup
        const unsigned long long cols = BIT(PB_SWE_NOT_LE0) | BIT(PB_SWE_GT0) | BIT(PB_SWETOP_NOT_LE0) | BIT(PB_SWETOP_GT0);
        __shared__ unsigned long long s_day;
        if (daily) {
            block_or_store(&D->day_bflags[blockIdx.x], b & ~cols);
            __syncthreads();   // block_or_store's scratch is used again below
        } else {
            if (threadIdx.x == 0) s_day = D->day_bflags[blockIdx.x];
            __syncthreads();
            b |= s_day;
        }
    }
    block_or_store(&D->bflags[0][blockIdx.x], b);
}

// word 0 = OR of the workgroup words of k_pred1 (or, summary path, of the fused kernel's summary words: their
// bits 0..3 are word 0's column bits) and the predicates of the shared forcing series.  Returns the OR of the
// workgroup words in thread 0.
RH_DEV unsigned long long finish_word0(DevState *D, const unsigned long long *flags, int nflags, unsigned long long cell_mask) {
    unsigned long long fb = 0;
    if (!D->per_cell && threadIdx.x < RH_SLOTS_PER_DAY) fb = forcing_bits(D->forc[0][threadIdx.x], D->forc[1][threadIdx.x], D->K);
    __shared__ unsigned long long fw[RH_BLOCK / 64];
    for (int off = 32; off; off >>= 1) fb |= __shfl_xor(fb, off);
    if ((threadIdx.x & 63) == 0) fw[threadIdx.x >> 6] = fb;
    const unsigned long long cells = reduce_bflags(flags, nflags);  // contains __syncthreads
    if (threadIdx.x == 0) {
        unsigned long long w = cells & cell_mask;
        for (int k = 0; k < RH_BLOCK / 64; ++k) w |= fw[k];
        D->words[0] = w;
    }
    __threadfence();
    __syncthreads();
    return cells;
}
__global__ __launch_bounds__(RH_BLOCK) void k_reduce(DevState *D, int which) {
    if (which == 0) {
        finish_word0(D, D->bflags[0], D->pred_blocks, ~0ull);
    } else {
        const unsigned long long w = reduce_bflags(D->bflags[1], D->pred_blocks);
        if (threadIdx.x == 0) D->words[1] = w;
    }
}

// Shared forcing: the nine aggregates of the day's 144-slot series in numpy's summation order,
// computed by one workgroup from LDS.  np.sum over 144 contiguous float64 is
// 0 + (half(0..71) + half(72..143)), each half = ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) with
// r_j = a[j] + a[j+8] + ... + a[j+64] accumulated in that order (numpy pairwise_sum, n <= 128).
// Lane j of a 16-lane group owns one r_j; six groups = six sums.
RH_DEV double np_tree8(const double *r) { return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])); }
RH_DEV double np_sum_of_parts(const double *part16) { return 0.0 + (np_tree8(part16) + np_tree8(part16 + 8)); }
RH_DEV bool in_hourly_window(int k, int64_t itd) { return (k >= itd) && (k < itd + 6); }
// r_j of one half of one sum: sum_id 0..2 = the daily sums of prec / ta / pet, 3..5 = those of the hourly window; l16 = (half, j).
// f: the day's three series.  The callers spread the 96 (sum_id, l16) items over their threads and store r in part[sum_id][l16].
RH_DEV double np_partial_sum(const double (*f)[RH_SLOTS_PER_DAY], int sum_id, int l16, int64_t itd) {
    const int half = l16 >> 3, j = l16 & 7;
    const int var = sum_id % 3;          // 0 prec, 1 ta, 2 pet
    const bool hourly = sum_id >= 3;     // sums 0..2 daily, 3..5 hourly window
    double r = 0.0;
    for (int q = 0; q < 9; ++q) {
        const int k = half * 72 + j + 8 * q;
        double v = f[var][k];
        const bool in = !hourly || in_hourly_window(k, itd);
        if (var == 1) v = (in && !isnan(v)) ? v : 0.0;  // nanmean: NaN (and masked) slots count as 0
        else v = in ? v : 0.0;
        r = (q == 0) ? v : r + v;
    }
    return r;
}
// the slot the ten-minute values are taken from: itt_day, wrapped and clamped as the reference's indexing does
RH_DEV int64_t current_slot(int64_t itd) {
    const int64_t k = itd < 0 ? itd + RH_SLOTS_PER_DAY : itd;
    return k > RH_SLOTS_PER_DAY - 1 ? RH_SLOTS_PER_DAY - 1 : k;
}
// The dt decision table on predicate word 0 (adaptive_time_stepping.py:83-190): which aggregate the step takes and its preliminary
// length.  cond_time: the step begins at midnight.
RH_DEV void step_selection(unsigned long long w, bool cond_time, StepCtx &X) {
    const bool all_p_le0 = !bit(w, PB_P_NOT_LE0), any_p_gt0 = bit(w, PB_P_GT0), any_p_gthpi = bit(w, PB_P_GT_HPI);
    const bool all_p_lehpi = !bit(w, PB_P_NOT_LE_HPI), all_ta_gt = !bit(w, PB_TA_NOT_GT), any_ta_gt = bit(w, PB_TA_GT);
    const bool any_pgt0_tale = bit(w, PB_PGT0_TALE), all_ple0_tale = !bit(w, PB_NOT_PLE0_TALE);
    const bool all_swe_le0 = !bit(w, PB_SWE_NOT_LE0), all_swetop_le0 = !bit(w, PB_SWETOP_NOT_LE0);
    const bool snow_any = (bit(w, PB_SWE_GT0) || bit(w, PB_SWETOP_GT0)) && any_ta_gt;
    const bool cond0 = all_p_le0 && all_swe_le0 && all_swetop_le0 && all_ta_gt;
    const bool cond00 = any_pgt0_tale || all_ple0_tale;
    const bool cond1 = any_p_gthpi && any_p_gt0 && any_ta_gt;
    const bool cond2 = all_p_lehpi && any_p_gt0 && any_ta_gt;
    const bool cond3 = any_p_gthpi && any_p_gt0 && snow_any;
    const bool cond4 = all_p_lehpi && any_p_gt0 && snow_any;
    const bool cond5 = all_p_le0 && snow_any;
    X.sel_daily = cond0 || cond00;
    X.sel_hourly = (cond2 || cond4 || cond5) && !cond1 && !cond3;
    X.sel_10min = (cond1 || cond3) && !cond2 && !cond4 && !cond5;
    // :143-144 (the second assignment overwrites the first), :166, :190
    int64_t dts = cond_time ? 86400 : 3600;
    if (X.sel_hourly) dts = 3600;
    if (X.sel_10min) dts = 600;
    X.dt_secs_prelim = dts;
    X.sel_p = X.sel_10min ? 2 : (X.sel_hourly ? 1 : (X.sel_daily ? 0 : -1));
}

RH_DEV void agg_body(DevState *D) {
    __shared__ double f[3][RH_SLOTS_PER_DAY];   // prec, ta, pet of the day
    __shared__ double part[6][16];
    const int tid = threadIdx.x;
    const bool shared_forcing = !D->per_cell;
    const int64_t itd = D->S.itt_day;
    if (shared_forcing && tid < RH_SLOTS_PER_DAY)
        for (int k = 0; k < 3; ++k) f[k][tid] = D->forc[k][tid];
    __syncthreads();
    if (shared_forcing && tid < 96) {
        const int sum_id = tid >> 4, lane = tid & 15;
        part[sum_id][lane] = np_partial_sum(f, sum_id, lane, itd);
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long w = D->words[0];
        StepCtx X = D->X;
        X.cond_time = (D->S.time % 86400 == 0);
        step_selection(w, X.cond_time, X);
        X.itt_day = itd;
        if (shared_forcing) {
            double s[6];
            for (int q = 0; q < 6; ++q) s[q] = np_sum_of_parts(part[q]);
            int cnt_d = 0, cnt_h = 0;
            for (int k = 0; k < RH_SLOTS_PER_DAY; ++k) {
                const bool ok = !isnan(f[1][k]);
                cnt_d += ok;
                cnt_h += ok && in_hourly_window(k, itd);
            }
            X.agg[0] = s[0];
            X.agg[1] = s[1] / (double)cnt_d;
            X.agg[2] = s[2];
            X.agg[3] = s[3];
            X.agg[4] = s[4] / (double)cnt_h;
            X.agg[5] = s[5];
            const int64_t k = current_slot(itd);
            X.agg[6] = f[0][k];
            X.agg[7] = f[1][k];
            X.agg[8] = f[2][k];
            if (X.sel_p >= 0) {
                X.prec_sel = X.agg[3 * X.sel_p];
                X.ta_sel = X.agg[3 * X.sel_p + 1];
            }
        }
        D->X = X;
    }
}
__global__ __launch_bounds__(RH_BLOCK) void k_agg(DevState *D, int do_hooks, int do_reduce) {
    if (do_hooks) hooks_set_forcing(D);   // rh_run_steps: the user hooks ride along
    if (do_reduce) finish_word0(D, D->bflags[0], D->pred_blocks, ~0ull);  // single GPU: no exchange between k_pred1 and here
    agg_body(D);
}

// Per-cell forcing only: aggregates of every column's own 144-slot series, once per step, into
// nine SoA planes (so the per-column kernels stay free of the 144-element loops).
// PART: 0 = everything in one launch; 1 = the hourly window and the current slot only; 2 = the daily sums only (returns at once unless they
// are due).  From 65 536 columns on the host launches 1 and 2: the daily sums' code needs 214 registers, which leaves the hourly part --
// every step's part -- two waves per SIMD for a chain of dependent loads (58 us at 10^6 columns; on its own 25 us).
template <int PART>
__global__ __launch_bounds__(RH_BLOCK) void k_cell_agg(Arena a, DevState *D, int force_daily) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    const bool weighted = D->weights[0] != nullptr;
    // the station series of the day changes at midnight only (device-side hooks): its daily sums are formed once a day,
    // the first step of the day has itt_day == 0; rows uploaded by the host may change at any time
    const bool daily = (PART != 1) && (!weighted || force_daily || D->S.itt_day == 0);
    if (PART == 2 && !daily) return;
    __shared__ DaySeries day;
    if (weighted) stage_day(D, day);
    if (i >= a.n) return;
    double agg[9];
    if (weighted) {
        const double pw = D->weights[0][i], toff = D->weights[1][i], ew = D->weights[2][i];
        const DayView F = day_view(D, day, i);
        forcing_aggregates_of([&](int k) { return F(0, k) * pw; }, [&](int k) { return F(1, k) + toff; },
                              [&](int k) { return F(2, k) * ew; }, D->S.itt_day, agg, daily, PART != 2);
    } else {
        const double *p = D->forc_cell[0] + i, *t = D->forc_cell[1] + i, *e = D->forc_cell[2] + i;
        const size_t n = (size_t)a.n;
        forcing_aggregates_of([&](int k) { return p[k * n]; }, [&](int k) { return t[k * n]; }, [&](int k) { return e[k * n]; },
                              D->S.itt_day, agg, daily, PART != 2);
    }
    if (daily)
        for (int k = 0; k < 3; ++k) D->agg_cell[(size_t)k * a.n + i] = agg[k];
    if (PART != 2)
        for (int k = 3; k < 9; ++k) D->agg_cell[(size_t)k * a.n + i] = agg[k];
}
RH_DEV double cell_agg(const DevState *D, int64_t n, int64_t i, int k) { return D->agg_cell[(size_t)k * n + i]; }


// mode: RH_SELECT_M1_PENDING = the tau -> taum1 copies of the last fused step are still pending (lazy rotation): prec_m1 / swe_m1 are
// the tau planes as they stand; RH_SELECT_DEFER = the selected prec / ta are not stored, the fused kernel applies the selection itself
// (StepCtx.apply_sel = 2) -- the planes stay untouched between two fused steps, so the rotation can stay pending
#define RH_SELECT_M1_PENDING 1
#define RH_SELECT_DEFER 2
__global__ __launch_bounds__(RH_BLOCK) void k_select(Arena a, DevState *D, int mode) {
    const Consts K = D->K;
    const StepCtx X = D->X;
    const bool per_cell = D->per_cell != 0;
    unsigned long long b = 0;
    for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * RH_BLOCK) {
        Col c;
        rh_ld(a, RH_P_prec, i, c.prec);
        rh_ld(a, RH_P_ta, i, c.ta);
        double prec_m1, swe, swe_top, swe_m1;
        rh_ld(a, RH_P_swe, i, swe);
        rh_ld(a, RH_P_swe_top, i, swe_top);
        if (mode & RH_SELECT_M1_PENDING) {
            prec_m1 = c.prec;
            swe_m1 = swe;
        } else {
            rh_ld(a, RH_P_prec_m1, i, prec_m1);
            rh_ld(a, RH_P_swe_m1, i, swe_m1);
        }
        if (X.sel_p >= 0) {
            if (per_cell)
                rt_select_prec_ta(c, X, cell_agg(D, a.n, i, 3 * X.sel_p), cell_agg(D, a.n, i, 3 * X.sel_p + 1));
            else
                rt_select_prec_ta(c, X, X.prec_sel, X.ta_sel);
            if (!(mode & RH_SELECT_DEFER)) {
                rh_st(a, RH_P_prec, i, c.prec);
                rh_st(a, RH_P_ta, i, c.ta);
            }
        }
        const bool warm = c.ta > K.ta_fm;
        b |= ((c.prec > 0) && warm) ? BIT(PC_RAIN) : 0;
        b |= (((swe > 0) || (swe_top > 0)) && warm) ? BIT(PC_SNOWMELT) : 0;
        b |= !(c.prec <= 0) ? BIT(PC_PREC_NOT_LE0) : 0;
        b |= !((c.prec > 0) && (c.ta <= K.ta_fm)) ? BIT(PC_NOT_PGT0_TALE) : 0;
        b |= (swe_m1 > 0) ? BIT(PC_SWEM1_GT0) : 0;
        b |= !(swe <= 0) ? BIT(PC_SWE_NOT_LE0) : 0;
        b |= (c.prec == 0) ? BIT(PC_P_EQ0) : 0;
        b |= (prec_m1 != 0) ? BIT(PC_PM1_NE0) : 0;
        b |= (c.prec != 0) ? BIT(PC_P_NE0) : 0;
        b |= (prec_m1 == 0) ? BIT(PC_PM1_EQ0) : 0;
    }
    block_or_store(&D->bflags[1][blockIdx.x], b);
}

// infiltration.py:2155-2167 from the predicate word and the event ids
RH_DEV void infiltration_conds(const rh_scalars &S, StepCtx &X, unsigned long long w) {
    X.cond1 = (S.event_id[0] == 0) && (S.event_id[1] >= 1);
    X.cond2 = bit(w, PC_P_EQ0) && bit(w, PC_PM1_NE0) && (S.event_id[0] >= 1);
    X.cond3 = bit(w, PC_P_NE0) && bit(w, PC_PM1_EQ0) && (S.event_id[0] == S.event_id[1]);
    X.cond4 = (S.event_id[0] >= 1) && (S.event_id[1] == 0);
    X.cond5 = S.event_id[1] >= 1;
}

// adaptive_time_stepping.py:192-373, scalar part
RH_DEV void scalars_body(DevState *D, unsigned long long w, int do_finish, int apply_sel);
__global__ __launch_bounds__(RH_BLOCK) void k_scalars(DevState *D, int do_reduce, int do_finish, int apply_sel = 0) {
    unsigned long long w = 0;
    if (do_reduce) w = reduce_bflags(D->bflags[1], D->pred_blocks);
    if (threadIdx.x != 0) return;
    if (!do_reduce) w = D->words[1];
    scalars_body(D, w, do_finish, apply_sel);
}
// agg[3 * sel + off] without a dynamic index (which would put the whole step context into scratch memory)
RH_DEV double agg_pick(const StepCtx &X, int sel, int off) {
    const double a0 = off == 0 ? X.agg[0] : (off == 1 ? X.agg[1] : X.agg[2]);
    const double a1 = off == 0 ? X.agg[3] : (off == 1 ? X.agg[4] : X.agg[5]);
    const double a2 = off == 0 ? X.agg[6] : (off == 1 ? X.agg[7] : X.agg[8]);
    return sel == 0 ? a0 : (sel == 1 ? a1 : a2);
}
// the bookkeeping itself, on copies of the scalars and of the step context
RH_DEV int64_t scalars_update(rh_scalars &S, StepCtx &X, unsigned long long w, int do_finish, int apply_sel, bool per_cell, int64_t ee) {
    X.apply_sel = apply_sel;
    X.halt = 0;   // (the time limit is the summary path's, ctrl_wave: it sets `last` after this bookkeeping)
    X.last = 0;
    const bool ev_start = bit(w, PC_RAIN) || bit(w, PC_SNOWMELT);
    const bool ev_end = !bit(w, PC_PREC_NOT_LE0) || !bit(w, PC_NOT_PGT0_TALE) || (bit(w, PC_SWEM1_GT0) && !bit(w, PC_SWE_NOT_LE0));
    int64_t dts = X.dt_secs_prelim;
    if (ev_start) S.time_event0 = 0;
    if (ev_end) S.time_event0 = S.time_event0 + dts;
    const int64_t te0 = S.time_event0, tm = S.time;
    const bool c6 = (te0 <= ee) && (dts == 600), c7 = (te0 <= ee) && (dts == 3600), c8 = (te0 <= ee) && (dts == 86400);
    const bool c9 = (te0 > ee) && (tm % 3600 != 0) && (dts == 600);
    const bool c10 = (te0 > ee) && (tm % 3600 == 0) && ((dts == 600) || (dts == 3600));
    const bool c11 = (te0 > ee) && (tm % 86400 == 0) && (dts == 86400);
    int w_sel = -1;
    double dt = S.dt;
    int64_t itd = S.itt_day;
    if (c6) { w_sel = 2; S.event_id[1] = S.event_id_counter; dt = 1.0 / 6; itd += 1; }
    if (c7) { w_sel = 1; S.event_id[1] = S.event_id_counter; dt = 1; itd += 6; }
    if (c8) { w_sel = 0; dt = 24; itd = 0; }
    if (c9) { w_sel = 2; S.event_id[1] = 0; dt = 1.0 / 6; dts = 600; itd += 1; }
    if (c10) { w_sel = 1; S.event_id[1] = 0; dt = 1; dts = 3600; itd += 6; }
    if (c11) { w_sel = 0; S.event_id[1] = 0; dt = 24; dts = 86400; itd = 0; }
    S.dt = dt;
    S.dt_secs = dts;
    S.itt_day = itd;
    if ((S.event_id[0] > 0) && (S.event_id[1] == 0)) S.event_id_counter += 1;
    X.sel_w = w_sel;
    if (w_sel >= 0 && !per_cell) {
        X.pet_sel_w = agg_pick(X, w_sel, 2);
        X.ta_sel_w = agg_pick(X, w_sel, 1);
    }
    X.dt = dt;
    X.month_tau = S.month[1];
    infiltration_conds(S, X, w);
    if (do_finish) {
        // roger.py:449-450 and the scalar half of after_timestep (svat.py:352-366).  Nothing below
        // this kernel reads these scalars during the step (k_step works from StepCtx), so they are
        // advanced here instead of in a kernel of their own.
        S.itt += 1;
        S.time += S.dt_secs;
        S.event_id[0] = S.event_id[1];
        S.year[0] = S.year[1];
        S.month[0] = S.month[1];
        S.doy[0] = S.doy[1];
    }
    return dts;
}
// rh_enable_timing's step log, on the three values the caller has loaded (the single-wavefront forms request them with their other loads)
RH_DEV void log_dt(DevState *D, int *dt_log, int dt_log_n, int dt_log_cap, int64_t dts) {
    if (dt_log) {
        if (dt_log_n < dt_log_cap) dt_log[dt_log_n] = (int)dts;
        D->dt_log_n = dt_log_n + 1;
    }
}
RH_DEV void log_dt(DevState *D, int64_t dts) {
    if (D->dt_log) log_dt(D, D->dt_log, D->dt_log_n, D->dt_log_cap, dts);   // (the other two are read only when the log is on)
}
// one thread
RH_DEV void scalars_body(DevState *D, unsigned long long w, int do_finish, int apply_sel) {
    // one burst of loads, the bookkeeping in registers, one burst of stores: working on D->S / D->X in place costs a
    // global-memory round trip per field for this single thread (the control kernel took 20 us that way)
    rh_scalars S = D->S;
    StepCtx X = D->X;
    const int64_t dts = scalars_update(S, X, w, do_finish, apply_sel, D->per_cell != 0, D->K.end_event);
    D->words[0] = 0;
    D->words[1] = 0;
    D->words[2] = 0;
    D->S = S;
    D->X = X;
    log_dt(D, dts);
}

// ---- summary path (shared forcing): the whole control part of a step in ONE single-workgroup kernel ----------
// Word 1 of this step from the summary bits the fused kernel left at the end of the previous step and the
// (uniform) selected prec / ta; same terms as k_select evaluates per column.
RH_DEV unsigned long long derive_word1(unsigned long long s, const StepCtx &X, const Consts &K) {
    unsigned long long w = 0;
    if (X.sel_p >= 0) {
        const double P = X.prec_sel, T = X.ta_sel;
        const bool warm = T > K.ta_fm;
        w |= ((P > 0) && warm) ? BIT(PC_RAIN) : 0;
        w |= ((bit(s, QB_SWE_GT0) || bit(s, QB_SWETOP_GT0)) && warm) ? BIT(PC_SNOWMELT) : 0;
        w |= !(P <= 0) ? BIT(PC_PREC_NOT_LE0) : 0;
        w |= !((P > 0) && (T <= K.ta_fm)) ? BIT(PC_NOT_PGT0_TALE) : 0;
        w |= (P == 0) ? BIT(PC_P_EQ0) : 0;
        w |= (P != 0) ? BIT(PC_P_NE0) : 0;
    } else {
        w |= bit(s, QB_RAIN_KEEP) ? BIT(PC_RAIN) : 0;
        w |= bit(s, QB_SNOWMELT_KEEP) ? BIT(PC_SNOWMELT) : 0;
        w |= bit(s, QB_P_NOT_LE0) ? BIT(PC_PREC_NOT_LE0) : 0;
        w |= bit(s, QB_NOT_PGT0_TALE) ? BIT(PC_NOT_PGT0_TALE) : 0;
        w |= bit(s, QB_P_EQ0) ? BIT(PC_P_EQ0) : 0;
        w |= bit(s, QB_P_NE0) ? BIT(PC_P_NE0) : 0;
    }
    w |= bit(s, QB_SWE_GT0) ? BIT(PC_SWEM1_GT0) : 0;       // swe[taum1] of this step = swe the last step left
    w |= bit(s, QB_SWE_NOT_LE0) ? BIT(PC_SWE_NOT_LE0) : 0;
    w |= bit(s, QB_P_NE0) ? BIT(PC_PM1_NE0) : 0;           // prec[taum1] likewise
    w |= bit(s, QB_P_EQ0) ? BIT(PC_PM1_EQ0) : 0;
    return w;
}
// Summary bits of one column (values as they stand in the arena at the start of the next step), in two halves
// so that the fused kernel can sample prec / ta and swe / swe_top where each pair is final: the prec/ta half
// (bit 63 carries `warm` to the second half), then the snow half.
#define QB_WARM_TMP 63
RH_DEV unsigned long long summary_bits_pt(double prec, double ta, const Consts &K) {
    unsigned long long b = 0;
    const bool warm = ta > K.ta_fm;
    b |= warm ? BIT(QB_WARM_TMP) : 0;
    b |= ((prec > 0) && warm) ? BIT(QB_RAIN_KEEP) : 0;
    b |= !(prec <= 0) ? BIT(QB_P_NOT_LE0) : 0;
    b |= !((prec > 0) && (ta <= K.ta_fm)) ? BIT(QB_NOT_PGT0_TALE) : 0;
    b |= (prec == 0) ? BIT(QB_P_EQ0) : 0;
    b |= (prec != 0) ? BIT(QB_P_NE0) : 0;
    return b;
}
RH_DEV unsigned long long summary_bits_sw(unsigned long long b, double swe, double swe_top) {
    const bool warm = bit(b, QB_WARM_TMP);
    b &= ~BIT(QB_WARM_TMP);
    b |= !(swe <= 0) ? BIT(QB_SWE_NOT_LE0) : 0;
    b |= (swe > 0) ? BIT(QB_SWE_GT0) : 0;
    b |= !(swe_top <= 0) ? BIT(QB_SWETOP_NOT_LE0) : 0;
    b |= (swe_top > 0) ? BIT(QB_SWETOP_GT0) : 0;
    b |= (((swe > 0) || (swe_top > 0)) && warm) ? BIT(QB_SNOWMELT_KEEP) : 0;
    return b;
}
RH_DEV unsigned long long summary_bits(double swe, double swe_top, double prec, double ta, const Consts &K) {
    return summary_bits_sw(summary_bits_pt(prec, ta, K), swe, swe_top);
}
// ---- the control part of a step by ONE wavefront (no workgroup barrier): k_ctrl, and the tail of the fused kernel ----------
RH_DEV void wave_sync() {   // LDS written by some lanes of a wavefront, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
RH_DEV unsigned long long wave_or(unsigned long long b) {
    for (int off = 32; off; off >>= 1) b |= __shfl_xor(b, off);
    return b;
}
struct CtrlLds {
    double f[3][RH_SLOTS_PER_DAY];   // prec, ta, pet of the day
    double part[6][16];              // numpy's eight partial sums of both halves, six sums
};
// [Device-side hooks,] predicate word 0, forcing aggregates in numpy's order, dt and event bookkeeping -- what k_agg + k_select +
// k_scalars do for the predicate-kernel generation -- on the copies S / X every lane holds (uniform); `cells` = OR of the
// summary bits of all columns (of all ranks).  The caller stores S / X.  Shared forcing only (the summary path).
#ifdef RH_STEP_PHASES   // measurement builds: cycles of the tail's parts (one wavefront per launch)
__device__ unsigned long long g_tail_phases[8];
#define RH_TPH(k)                                                  \
    if ((threadIdx.x & 63) == 0) {                                 \
        const unsigned long long t_ = clock64();                   \
        atomicAdd(&g_tail_phases[k], t_ - tph);                    \
        tph = t_;                                                  \
    }
#else
#define RH_TPH(k)
#endif
// The day's shared series spread over the wavefront's registers (lane l holds slots l, l + 64, l + 128 of each variable) and the scalars
// the control part needs besides S / X: requested by the caller BEFORE it waits for anything else, so that the tail of the fused kernel
// makes ONE round trip to memory for all its inputs (it made three in sequence: the summary words and S / X, then the constants, then the
// series into LDS -- 19 600 cycles per tail, a tenth of a 10^6-column step and a third of an 80 x 53 one; profiles/r04_tail_phases.txt).
struct CtrlIn {
    double f[3][3];            // f[v][r]: slot lane + 64 r of variable v (slots >= 144: 0)
    double ta_fm;
    int64_t hpi, end_event, nitt_forc;
    long long t_end;
    int cache_ok;
    unsigned long long day_fb;
    double day_agg[3];
    int *dt_log;               // log_dt's three loads, with the others
    int dt_log_n, dt_log_cap;
};
RH_DEV CtrlIn ctrl_inputs(const DevState *D) {
    CtrlIn in;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int k = lane + 64 * r;
            in.f[v][r] = k < RH_SLOTS_PER_DAY ? D->forc[v][k] : 0.0;
        }
    in.ta_fm = D->K.ta_fm;
    in.hpi = D->K.hpi;
    in.end_event = D->K.end_event;
    in.nitt_forc = D->nitt_forc;
    in.t_end = D->t_end;
    in.cache_ok = D->day_cache_ok;
    in.day_fb = D->day_fb;
    in.day_agg[0] = D->day_agg[0]; in.day_agg[1] = D->day_agg[1]; in.day_agg[2] = D->day_agg[2];
    in.dt_log = D->dt_log;
    in.dt_log_n = D->dt_log_n;
    in.dt_log_cap = D->dt_log_cap;
    return in;
}
// The control part in two halves.  ctrl_pre: everything that does not depend on the columns -- the time limit, the set_forcing hook, the
// day's forcing bits (fb) and the aggregates of the day and of the hourly window; it may run while the columns are still being stepped
// (the extra workgroup of a fused launch, pre_tail), so what running wavefronts read (D->monthly, D->per_cell) is NOT written here but
// handed on in `side` (RH_SIDE_*).  ctrl_post: the decisions on word 0 and word 1 (`cells` = OR of the columns' summary bits), dt and the
// event bookkeeping.
#define RH_SIDE_MONTHLY_SET 1   // D->monthly = bit RH_SIDE_MONTHLY
#define RH_SIDE_MONTHLY 2
#define RH_SIDE_PER_CELL_SET 4  // D->per_cell = bit RH_SIDE_PER_CELL
#define RH_SIDE_PER_CELL 8
RH_DEV void ctrl_side_effects(DevState *D, int side) {   // (one lane)
    if (side & RH_SIDE_PER_CELL_SET) D->per_cell = (side & RH_SIDE_PER_CELL) ? 1 : 0;
    if (side & RH_SIDE_MONTHLY_SET) D->monthly = (side & RH_SIDE_MONTHLY) ? 1 : 0;
}
RH_DEV void ctrl_pre(DevState *D, CtrlLds &L, rh_scalars &S, StepCtx &X, int do_hooks, const CtrlIn &in, unsigned long long &fb_out, int &side) {
#ifdef RH_STEP_PHASES
    unsigned long long tph = clock64();
#endif
    const int lane = threadIdx.x & 63;
    Consts Kf;   // forcing_bits reads hpi and ta_fm only
    Kf.hpi = in.hpi;
    Kf.ta_fm = in.ta_fm;
    bool fresh_day = false;
    side = 0;
    fb_out = 0;
    const long long t_end = in.t_end;
    X.halt = (t_end >= 0 && S.time >= t_end) ? 1 : 0;   // the run is over (roger/roger.py:548): nothing is formed, S stays as it is
    X.last = 0;
    if (X.halt) return;
    X.forc_exhausted = 0;
    if (do_hooks) {   // hooks_set_forcing: benchmarks/SVAT_benchmark.py:105-110, 151-171
        const bool midnight = (S.time % 86400 == 0);
        const int64_t i0 = S.itt_forc;
        const bool have = midnight && (i0 + RH_SLOTS_PER_DAY <= in.nitt_forc);
        X.forc_exhausted = (midnight && !have) ? 1 : 0;
        if (have) {
            for (int k = lane; k < 3 * RH_SLOTS_PER_DAY; k += 64) {
                const int v = k / RH_SLOTS_PER_DAY, j = k % RH_SLOTS_PER_DAY;
                const double x = D->series[v][i0 + j];
                L.f[v][j] = x;
                D->forc[v][j] = x;
            }
            hook_new_day(D, S, i0);
            side |= RH_SIDE_PER_CELL_SET | (D->weights[0] ? RH_SIDE_PER_CELL : 0);
            fresh_day = true;
        }
        side |= RH_SIDE_MONTHLY_SET | (month_changed(&S) ? RH_SIDE_MONTHLY : 0);
    }
    const int64_t itd = S.itt_day;
    if (!fresh_day && in.cache_ok) {
        // inside a day whose bits and daily aggregates an earlier control part has formed: the six slots of the hourly window, out of the
        // registers (forcing_aggregates_of: the sums in numpy's order, as the full path forms them)
        RH_TPH(1)
        fb_out = in.day_fb;
        double agg[9];
        // (copies by value: a closure holding a reference to `in` keeps the whole struct in scratch memory)
        const double p0 = in.f[0][0], p1 = in.f[0][1], p2 = in.f[0][2], t0 = in.f[1][0], t1 = in.f[1][1], t2 = in.f[1][2];
        const double e0 = in.f[2][0], e1 = in.f[2][1], e2 = in.f[2][2];
        forcing_aggregates_of([=](int k) { return ctrl_slot(p0, p1, p2, k); }, [=](int k) { return ctrl_slot(t0, t1, t2, k); },
                              [=](int k) { return ctrl_slot(e0, e1, e2, k); }, itd, agg, false, true);
        X.agg[0] = in.day_agg[0]; X.agg[1] = in.day_agg[1]; X.agg[2] = in.day_agg[2];
        X.agg[3] = agg[3]; X.agg[4] = agg[4]; X.agg[5] = agg[5];
        X.agg[6] = agg[6]; X.agg[7] = agg[7]; X.agg[8] = agg[8];
        RH_TPH(2)
    } else {
        if (!fresh_day) {
#pragma unroll
            for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (lane + 64 * r < RH_SLOTS_PER_DAY) L.f[v][lane + 64 * r] = in.f[v][r];
        }
        wave_sync();
        RH_TPH(1)
        // word 0: the columns' bits 0..3 and the predicates of the day's series (adaptive_time_stepping.py:38-81)
        unsigned long long fb = 0;
        int cnt_d = 0, cnt_h = 0;
        for (int k = lane; k < RH_SLOTS_PER_DAY; k += 64) fb |= forcing_bits(L.f[0][k], L.f[1][k], Kf);
        for (int k0 = 0; k0 < RH_SLOTS_PER_DAY; k0 += 64) {   // nanmean's divisors
            const int k = k0 + lane;
            const bool ok = k < RH_SLOTS_PER_DAY && !isnan(L.f[1][k < RH_SLOTS_PER_DAY ? k : 0]);
            cnt_d += __popcll(__ballot(ok));
            cnt_h += __popcll(__ballot(ok && in_hourly_window(k, itd)));
        }
        fb = wave_or(fb);
        fb_out = fb;
        // numpy's partial sums (np_partial_sum): six sums x 16 (half, lane-of-eight) pairs
        for (int item = lane; item < 96; item += 64) {
            const int sum_id = item >> 4, l16 = item & 15;
            L.part[sum_id][l16] = np_partial_sum(L.f, sum_id, l16, itd);
        }
        wave_sync();
        RH_TPH(2)
        X.agg[0] = np_sum_of_parts(L.part[0]);
        X.agg[1] = np_sum_of_parts(L.part[1]) / (double)cnt_d;
        X.agg[2] = np_sum_of_parts(L.part[2]);
        X.agg[3] = np_sum_of_parts(L.part[3]);
        X.agg[4] = np_sum_of_parts(L.part[4]) / (double)cnt_h;
        X.agg[5] = np_sum_of_parts(L.part[5]);
        const int64_t k = current_slot(itd);
        X.agg[6] = L.f[0][k];
        X.agg[7] = L.f[1][k];
        X.agg[8] = L.f[2][k];
        if (lane == 0) {   // the day's part, for the steps until somebody writes forc again
            D->day_fb = fb;
            D->day_agg[0] = X.agg[0]; D->day_agg[1] = X.agg[1]; D->day_agg[2] = X.agg[2];
            D->day_cache_ok = 1;
        }
    }
    X.cond_time = (S.time % 86400 == 0);
    X.itt_day = itd;
}
RH_DEV void ctrl_post(DevState *D, rh_scalars &S, StepCtx &X, unsigned long long cells, unsigned long long fb, double ta_fm, int64_t hpi_i, int64_t end_event,
                      long long t_end, int *dt_log, int dt_log_n, int dt_log_cap) {
#ifdef RH_STEP_PHASES
    unsigned long long tph = clock64();
#endif
    const int lane = threadIdx.x & 63;
    if (X.halt) return;
    Consts Kf;   // derive_word1 reads hpi and ta_fm only
    Kf.hpi = hpi_i;
    Kf.ta_fm = ta_fm;
    const unsigned long long w = (cells & 0xFull) | fb;
    // uniform from here on (every lane computes the same)
    step_selection(w, X.cond_time, X);
    if (X.sel_p >= 0) {
        X.prec_sel = agg_pick(X, X.sel_p, 0);
        X.ta_sel = agg_pick(X, X.sel_p, 1);
    }
    RH_TPH(3)
    const int64_t dts = scalars_update(S, X, derive_word1(cells, X, Kf), 1, 1, false, end_event);
    X.last = (t_end >= 0 && S.time >= t_end) ? 1 : 0;   // (S.time is the END of the step that is being formed)
    RH_TPH(4)
    if (lane == 0) {
        D->words[0] = 0;
        D->words[1] = 0;
        D->words[2] = 0;
        log_dt(D, dt_log, dt_log_n, dt_log_cap, dts);   // (on values requested with the tail's other loads)
    }
    RH_TPH(5)
}
// both halves in one wavefront (the control kernel; a fused launch without the extra workgroup)
RH_DEV void ctrl_wave(DevState *D, CtrlLds &L, rh_scalars &S, StepCtx &X, unsigned long long cells, int do_hooks, const CtrlIn &in) {
    unsigned long long fb;
    int side;
    ctrl_pre(D, L, S, X, do_hooks, in, fb, side);
    if ((threadIdx.x & 63) == 0) ctrl_side_effects(D, side);
    ctrl_post(D, S, X, cells, fb, in.ta_fm, in.hpi, in.end_event, in.t_end, in.dt_log, in.dt_log_n, in.dt_log_cap);
}
RH_DEV unsigned long long dev_load(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RH_DEV void dev_store(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// What pre_tail hands to the tail: S after the hook, X with the aggregates, the day's forcing bits, the deferred writes (RH_SIDE_*) -- one
// 8-byte word per lane (WI: integer fields, WF: doubles), packed by a select chain and taken apart by v_readlane with constant lanes:
// the structs never exist in memory on either side (as aggregates through LDS they cost both kernels a scratch frame).
#define RH_SX_FIELDS(WI, WF)                                                                                                         \
    WI(S.itt) WI(S.time) WI(S.dt_secs) WI(S.itt_day) WI(S.itt_forc) WI(S.time_event0) WI(S.event_id_counter)                         \
    WI(S.event_id[0]) WI(S.event_id[1]) WI(S.year[0]) WI(S.year[1]) WI(S.month[0]) WI(S.month[1]) WI(S.doy[0]) WI(S.doy[1])          \
    WF(S.dt) WI(S.sanity_ok)                                                                                                         \
    WF(X.dt) WF(X.agg[0]) WF(X.agg[1]) WF(X.agg[2]) WF(X.agg[3]) WF(X.agg[4]) WF(X.agg[5]) WF(X.agg[6]) WF(X.agg[7]) WF(X.agg[8])    \
    WI(X.month_tau) WI(X.sel_daily) WI(X.sel_hourly) WI(X.sel_10min) WI(X.sel_p) WF(X.prec_sel) WF(X.ta_sel) WI(X.sel_w)             \
    WF(X.pet_sel_w) WF(X.ta_sel_w) WI(X.cond1) WI(X.cond2) WI(X.cond3) WI(X.cond4) WI(X.cond5) WI(X.cond_time)                       \
    WI(X.dt_secs_prelim) WI(X.itt_day) WI(X.apply_sel) WI(X.forc_exhausted) WI(X.halt) WI(X.last)
#define RH_PRE_FIELDS(WI, WF) RH_SX_FIELDS(WI, WF) WI(fb) WI(side)
static_assert(sizeof(rh_scalars) == 17 * 8, "RH_PRE_FIELDS lists every field of rh_scalars");
static_assert(sizeof(StepCtx) == 200, "RH_PRE_FIELDS lists every field of StepCtx");
RH_DEV unsigned long long lane_word(unsigned long long w, int l) {   // (l: a constant)
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)w, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(w >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
// pw: the lane's word of DevState::pre_words, as pre_tail packed it
RH_DEV void pre_unpack(unsigned long long pw, rh_scalars &S, StepCtx &X, unsigned long long &fb, int &side) {
    int k = 0;
#define RH_WI(f) f = (std::remove_reference_t<decltype((f))>)(long long)lane_word(pw, k); ++k;
#define RH_WF(f) f = __longlong_as_double((long long)lane_word(pw, k)); ++k;
    RH_PRE_FIELDS(RH_WI, RH_WF)
#undef RH_WI
#undef RH_WF
}
// The control kernel of a step that does not find S_next / X_next ready (first step, after the host touched planes or
// scalars, multi-GPU after the exchange): one wavefront.  src: where the columns' summary word is (RH_SRC_*); src64 != null:
// it arrives as 64 int32 (0 / 1) from the exchange between the ranks and is folded here.
__global__ __launch_bounds__(64) void k_ctrl(DevState *D, int do_hooks, int src, const int *src64, int use_pre = 0) {
    __shared__ CtrlLds L;
    const int lane = threadIdx.x & 63;
    const CtrlIn in = ctrl_inputs(D);
    const unsigned long long pw = use_pre ? D->pre_words[lane] : 0ull;   // (written by the launch in front: a plain load)
    unsigned long long cells;
    if (src64) {
        cells = wave_or(src64[lane] ? (1ull << lane) : 0ull);
    } else if (src == RH_SRC_SUMW) {
        cells = wave_or(dev_load(&D->sumw[lane * RH_WSTRIDE]));
        dev_store(&D->sumw[lane * RH_WSTRIDE], 0ull);
    } else {
        cells = D->words[3];
    }
    rh_scalars S;
    StepCtx X;
    if (use_pre) {
        // the columns-independent half was formed by pre_tail of the fused launch in front of the exchange (from the S / X this kernel
        // would read): the decisions on the exchanged word are left
        unsigned long long fb;
        int side;
        pre_unpack(pw, S, X, fb, side);
        if (lane == 0) ctrl_side_effects(D, side);
        ctrl_post(D, S, X, cells, fb, in.ta_fm, in.hpi, in.end_event, in.t_end, in.dt_log, in.dt_log_n, in.dt_log_cap);
    } else {
        S = D->S;
        X = D->X;
        ctrl_wave(D, L, S, X, cells, do_hooks, in);
    }
    if (lane == 0) {
        D->words[3] = cells;
        if (!X.halt) D->sanity_last = 0;
        D->S = S;
        D->X = X;
        if (X.forc_exhausted && !X.halt) D->err_flags |= RH_DEVERR_FORCING;
    }
}
// The tail of the fused kernel, run by the wavefront that finishes last: folds the summary words into words[3] (and, for the
// exchange between ranks, spreads them over 64 int32), latches the sanity word, commits S_next / X_next if the step ran on them,
// and forms the next step's S_next / X_next (the control part of the next step: no control kernel between two fused kernels).
// A workgroup reports itself done; true for the one that is the last of the grid.  Two levels of counters -- workgroup b counts into
// group b mod n_groups, a full group into the top counter --, every counter in a cache line of its own and neighbouring workgroups in
// different groups: device-scope atomics on ONE line are served one after the other (~ 25 ns each; 3 907 workgroups counting into the two
// lines of 62 packed counters kept a 50 us kernel waiting for them, and the fused kernel's waves for their slot).  The counters reset
// themselves.  Called by one lane, after everything the workgroup posted through device-scope atomics has returned.
RH_DEV bool grid_completion(DevState *D, int n_groups) {
    const unsigned nblk = gridDim.x, ng = (unsigned)n_groups < nblk ? (unsigned)n_groups : nblk;
    const unsigned g = blockIdx.x % ng, cnt = nblk / ng + (g < nblk % ng ? 1u : 0u);
    unsigned int *c = &D->done_grp[g * RH_DONE_STRIDE];
    if (__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != cnt - 1) return false;
    __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ng == 1) return true;   // (small grids: one level -- a round trip less in a launch-bound step)
    if (__hip_atomic_fetch_add(&D->done_top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ng - 1) return false;
    __hip_atomic_store(&D->done_top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}
// The first wavefront of a fused launch's extra workgroup (RH_TAIL_PRE), at the START of the launch: commits the running step's S / X
// (nothing of the launch reads D->S / D->X: the columns work from X_next), forms the columns-independent half of the next control part
// and publishes it through returning device-scope atomics (the tail reads it with device-scope loads: sumw's scheme).  `dep`: the wave's
// completion count, made to depend on the atomics' return.
RH_DEV void pre_tail(DevState *D, CtrlLds &L, int flags, unsigned &dep) {
    const int lane = threadIdx.x & 63;
    const CtrlIn in = ctrl_inputs(D);
    const bool use_next = (flags & RH_TAIL_USE_NEXT) != 0;
    rh_scalars S = *(use_next ? &D->S_next : &D->S);   // (one load site: two would leave a copy of the structs in scratch memory)
    StepCtx X = *(use_next ? &D->X_next : &D->X);
    if (use_next && lane == 0) {
        D->S = S;
        D->X = X;
        if (X.forc_exhausted) D->err_flags |= RH_DEVERR_FORCING;
    }
    unsigned long long fb;
    int side;
    ctrl_pre(D, L, S, X, (flags & RH_TAIL_HOOKS) != 0, in, fb, side);
    unsigned long long mine = 0;
    {
        int k = 0;
#define RH_WI(f) if (lane == k) mine = (unsigned long long)(long long)(f); ++k;
#define RH_WF(f) if (lane == k) mine = (unsigned long long)__double_as_longlong(f); ++k;
        RH_PRE_FIELDS(RH_WI, RH_WF)
#undef RH_WI
#undef RH_WF
    }
    const unsigned long long old = __hip_atomic_exchange(&D->pre_words[lane], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" : "+v"(dep) : "v"((unsigned)old));   // (dep is used only after the exchange has returned -- for every lane: one instruction)
}
RH_DEV void step_tail(DevState *D, CtrlLds &L, int flags, int *dst64) {
    const int lane = threadIdx.x & 63;
    const bool pre = (flags & RH_TAIL_PRE) && (flags & RH_TAIL_CTRL);   // (RH_TAIL_PRE alone: the control kernel behind the exchange takes the hand-over)
    CtrlIn in;
    if (!pre) in = ctrl_inputs(D);   // (requested first: one round trip for everything the tail reads)
#ifdef RH_STEP_PHASES
    const unsigned long long tph0 = clock64();
#endif
    // every load of the tail is requested before the first result is used (one round trip)
    const unsigned long long sw = dev_load(&D->sumw[lane * RH_WSTRIDE]);
    const unsigned long long bad = dev_load(&D->words[2]);
    const unsigned long long pw = pre ? dev_load(&D->pre_words[lane]) : 0ull;
    const double ta_fm = D->K.ta_fm;
    const int64_t hpi = D->K.hpi, end_event = D->K.end_event;
    const long long t_end = D->t_end;
    int *const dt_log = D->dt_log;
    const int dt_log_n = D->dt_log_n, dt_log_cap = D->dt_log_cap;
    rh_scalars S;
    StepCtx X;
    unsigned long long fb = 0;
    int side = 0;
    if (!pre) {
        if (flags & RH_TAIL_USE_NEXT) {
            S = D->S_next;
            X = D->X_next;
        } else {
            S = D->S;
            X = D->X;
        }
    }
    const unsigned long long cells = wave_or(sw);
    dev_store(&D->sumw[lane * RH_WSTRIDE], 0ull);
    if (pre) pre_unpack(pw, S, X, fb, side);   // pre_tail has done the commit and its half of the control part
    if (lane == 0) {
        D->words[3] = cells;
        D->sanity_last = bad;
        if (!pre && (flags & RH_TAIL_USE_NEXT)) {
            D->S = S;
            D->X = X;
            if (X.forc_exhausted) D->err_flags |= RH_DEVERR_FORCING;
        }
    }
    if (dst64) dst64[lane] = (int)((cells >> lane) & 1ull);
    if (!(flags & RH_TAIL_CTRL)) return;
#ifdef RH_STEP_PHASES
    if (lane == 0) {
        atomicAdd(&g_tail_phases[0], clock64() - tph0 + (S.time & 0) + (unsigned long long)(X.halt & 0));   // (loads of S / X used)
        atomicAdd(&g_tail_phases[7], 1ull);
    }
#endif
    if (pre) {
        if (lane == 0) ctrl_side_effects(D, side);
        ctrl_post(D, S, X, cells, fb, ta_fm, hpi, end_event, t_end, dt_log, dt_log_n, dt_log_cap);
    } else {
        ctrl_wave(D, L, S, X, cells, (flags & RH_TAIL_HOOKS) != 0, in);
    }
    if (lane == 0) {
        D->S_next = S;
        D->X_next = X;
    }
#ifdef RH_STEP_PHASES
    __threadfence();
    if (lane == 0) atomicAdd(&g_tail_phases[6], clock64() - tph0);
#endif
}
// ---- per-cell forcing: ONE per-column launch in front of the fused kernel (round 4) --------------------------------
// What k_pred1 -> k_agg -> k_cell_agg<1> -> k_select -> k_scalars did in five launches (four of them passes over the columns or
// single-workgroup reductions waiting for each other).  The two global decisions of a step depend on each other -- word 0 (snow state +
// the day's forcing over all columns) decides which aggregate a column takes as its prec / ta, word 1 is formed from THOSE --, so a
// column evaluates word 1's terms for every candidate selection (keep, daily, hourly, ten minutes: 6 bits each) next to its
// aggregates; the wavefront that finishes last folds the words, takes the candidate word 0 selects and does the bookkeeping
// (agg_body's decisions + scalars_update, the same device functions).  The day's forcing bits are formed once a day by the part that
// forms the daily sums and kept in day_word.
enum { FC_RAIN = 0, FC_SNOWMELT, FC_PREC_NOT_LE0, FC_NOT_PGT0_TALE, FC_P_EQ0, FC_P_NE0, FC_PER_CANDIDATE };
#define FC_COMMON 24   // bits 24..: PC_SWEM1_GT0, PC_SWE_NOT_LE0, PC_PM1_NE0, PC_PM1_EQ0, then word 0's four snow bits
RH_DEV unsigned long long front_candidate_bits(double prec, double ta, bool snow, double ta_fm) {
    unsigned long long b = 0;
    const bool warm = ta > ta_fm;
    b |= ((prec > 0) && warm) ? BIT(FC_RAIN) : 0;
    b |= (snow && warm) ? BIT(FC_SNOWMELT) : 0;
    b |= !(prec <= 0) ? BIT(FC_PREC_NOT_LE0) : 0;
    b |= !((prec > 0) && (ta <= ta_fm)) ? BIT(FC_NOT_PGT0_TALE) : 0;
    b |= (prec == 0) ? BIT(FC_P_EQ0) : 0;
    b |= (prec != 0) ? BIT(FC_P_NE0) : 0;
    return b;
}
// the daily part of a column: its daily sums (aggregate planes 0..2) and the forcing bits of its 144 slots
template <class P, class T, class E>
RH_DEV unsigned long long front_daily(P p, T t, E e, double *agg, const Consts &K) {
    forcing_aggregates_of(p, t, e, 0, agg, true, false);
    unsigned long long b = 0;
    for (int k = 0; k < RH_SLOTS_PER_DAY; ++k) b |= forcing_bits(p(k), t(k), K);
    return b;
}
// the control part by the last wavefront: S / X as k_agg's thread 0 and k_scalars form them
// fd: the set_forcing hook rode along with the kernel (fresh_day) -- what it does to the state happens here, once
RH_DEV void front_ctrl(DevState *D, bool daily_due, const FreshDay &fd, int hooks) {
    const int lane = threadIdx.x & 63;
    // everything this wavefront reads is requested before the first result is used (one round trip, as in the fused kernel's tail)
    const unsigned long long fw = dev_load(&D->frontw[lane * RH_WSTRIDE]);
    const unsigned long long dw = daily_due ? dev_load(&D->dayw[lane * RH_WSTRIDE]) : 0ull;
    unsigned long long day = D->day_word;
    const int64_t end_event = D->K.end_event;
    int *const dt_log = D->dt_log;
    const int dt_log_n = D->dt_log_n, dt_log_cap = D->dt_log_cap;
    const unsigned long long cells = wave_or(fw);
    dev_store(&D->frontw[lane * RH_WSTRIDE], 0ull);
    if (daily_due) {
        day = wave_or(dw);
        dev_store(&D->dayw[lane * RH_WSTRIDE], 0ull);
    }
    if (fd.fresh) {   // hooks_set_forcing: the day of the resident series becomes the current one for everybody behind this kernel
        for (int k = lane; k < 3 * RH_SLOTS_PER_DAY; k += 64) D->forc[k / RH_SLOTS_PER_DAY][k % RH_SLOTS_PER_DAY] = D->series[k / RH_SLOTS_PER_DAY][fd.i0 + k % RH_SLOTS_PER_DAY];
        if (lane == 0) D->day_cache_ok = 0;
        const int ns = D->n_stations;
        for (int q = lane; q < 3 * ns * RH_SLOTS_PER_DAY; q += 64) {
            const int v = q / (ns * RH_SLOTS_PER_DAY), r = q % (ns * RH_SLOTS_PER_DAY), st = r / RH_SLOTS_PER_DAY, j = r % RH_SLOTS_PER_DAY;
            D->forc_multi[q] = D->series[v][(size_t)st * D->nitt_forc + fd.i0 + j];
        }
    }
    if (lane != 0) return;
    D->day_word = day;
    rh_scalars S = D->S;   // (hoisted above the folds these two structs end up in scratch memory)
    StepCtx X = D->X;
    if (hooks) {
        if (fd.fresh) {
            hook_new_day(D, S, fd.i0);
            D->per_cell = D->weights[0] ? 1 : 0;
        }
        D->monthly = month_changed(&S);
        if (fd.missing) D->err_flags |= RH_DEVERR_FORCING;
    }
    const unsigned long long w = ((cells >> (FC_COMMON + 4)) & 0xFull) | day;   // word 0: bits 0..3 are the columns' snow bits
    X.cond_time = (S.time % 86400 == 0);
    step_selection(w, X.cond_time, X);
    X.itt_day = S.itt_day;
    // word 1 from the candidate the selection takes (candidate 0: keep; 1 + sel_p otherwise) and the common terms
    const unsigned long long cand = (cells >> (FC_PER_CANDIDATE * (X.sel_p + 1))) & ((1ull << FC_PER_CANDIDATE) - 1);
    unsigned long long w1 = 0;
    w1 |= bit(cand, FC_RAIN) ? BIT(PC_RAIN) : 0;
    w1 |= bit(cand, FC_SNOWMELT) ? BIT(PC_SNOWMELT) : 0;
    w1 |= bit(cand, FC_PREC_NOT_LE0) ? BIT(PC_PREC_NOT_LE0) : 0;
    w1 |= bit(cand, FC_NOT_PGT0_TALE) ? BIT(PC_NOT_PGT0_TALE) : 0;
    w1 |= bit(cand, FC_P_EQ0) ? BIT(PC_P_EQ0) : 0;
    w1 |= bit(cand, FC_P_NE0) ? BIT(PC_P_NE0) : 0;
    w1 |= bit(cells, FC_COMMON + 0) ? BIT(PC_SWEM1_GT0) : 0;
    w1 |= bit(cells, FC_COMMON + 1) ? BIT(PC_SWE_NOT_LE0) : 0;
    w1 |= bit(cells, FC_COMMON + 2) ? BIT(PC_PM1_NE0) : 0;
    w1 |= bit(cells, FC_COMMON + 3) ? BIT(PC_PM1_EQ0) : 0;
    const int64_t dts = scalars_update(S, X, w1, 1, 2, true, end_event);
    D->words[0] = 0;
    D->words[1] = 0;
    D->words[2] = 0;
    D->sanity_last = 0;   // (the fused kernel behind this front has no tail: words[2] is the whole record of its step)
    D->S = S;
    D->X = X;
    log_dt(D, dt_log, dt_log_n, dt_log_cap, dts);
}
// PART 0: every step's part; 1: with the daily part inline (small grids: one launch); 2: the daily part alone (in front of PART 0 on large
// grids, returning at once unless it is due: the daily sums' code needs > 200 registers, which would leave every step's part two waves per
// SIMD).  m1_pending as k_select's RH_SELECT_M1_PENDING.  The column's planes, weights and daily sums are requested FIRST, so that their
// round trips to HBM run under the staging of the day and the window sums.
template <int PART>
__global__ __launch_bounds__(RH_BLOCK) void k_cell_front(Arena a, DevState *D, int force_daily, int m1_pending, int n_groups, int hooks) {
    constexpr bool daily_only = PART == 2, with_daily = PART != 0;
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    const bool weighted = D->weights[0] != nullptr;
    // hooks: the device-side set_forcing hook rides along -- at midnight the kernel works on the day the hook is about to bring, the last
    // wavefront does the hook's bookkeeping (the state is read, not written, until then: PART 2 in front of PART 0 decides the same)
    const FreshDay fd = fresh_day(D, hooks);
    const bool daily_due = !weighted || force_daily || fd.itd == 0;   // (uniform over the grid; k_cell_agg's rule)
    __shared__ unsigned wg_done;
    __shared__ DaySeries day;
    if (daily_only && !daily_due) return;
    const bool in = i < a.n;
    const int64_t ii = in ? i : a.n - 1;
    double prec = 0, ta = 0, swe = 0, swe_top = 0, prec_m1 = 0, swe_m1 = 0, pw = 0, toff = 0, ew = 0, day0 = 0, day1 = 0;
    if (!daily_only) {
        rh_ld(a, RH_P_prec, ii, prec);
        rh_ld(a, RH_P_ta, ii, ta);
        rh_ld(a, RH_P_swe, ii, swe);
        rh_ld(a, RH_P_swe_top, ii, swe_top);
        if (!m1_pending) {
            rh_ld(a, RH_P_prec_m1, ii, prec_m1);
            rh_ld(a, RH_P_swe_m1, ii, swe_m1);
        }
        if (!(with_daily && daily_due)) {   // the daily sums of the day: formed earlier
            day0 = D->agg_cell[ii];
            day1 = D->agg_cell[(size_t)a.n + ii];
        }
    }
    if (weighted) {
        pw = D->weights[0][ii];
        toff = D->weights[1][ii];
        ew = D->weights[2][ii];
    }
    if (threadIdx.x == 0) wg_done = 0;
    // the whole day in LDS only where all of it is walked (the daily part); every step's part reads its window's six slots where they lie
    const bool staged = weighted && with_daily && daily_due;
    if (staged) stage_day(D, day, &fd);
    else __syncthreads();
    const Consts K = D->K;
    const int64_t itd = fd.itd;
    unsigned long long b = 0, db = 0;
    if (in) {
        double agg[9];
        if (weighted) {
            const DayView F = day_view(D, day, i, &fd, staged);
            auto p = [&](int k) { return F(0, k) * pw; };
            auto t = [&](int k) { return F(1, k) + toff; };
            auto e = [&](int k) { return F(2, k) * ew; };
            if (with_daily && daily_due) db = front_daily(p, t, e, agg, K);
            if (!daily_only) forcing_aggregates_of(p, t, e, itd, agg, false, true);
        } else {
            const double *pp = D->forc_cell[0] + i, *tp = D->forc_cell[1] + i, *ep = D->forc_cell[2] + i;
            const size_t n = (size_t)a.n;
            auto p = [&](int k) { return pp[k * n]; };
            auto t = [&](int k) { return tp[k * n]; };
            auto e = [&](int k) { return ep[k * n]; };
            if (with_daily && daily_due) db = front_daily(p, t, e, agg, K);
            if (!daily_only) forcing_aggregates_of(p, t, e, itd, agg, false, true);
        }
        if (with_daily && daily_due)
            for (int k = 0; k < 3; ++k) D->agg_cell[(size_t)k * a.n + i] = agg[k];
        if (!daily_only) {
            for (int k = 3; k < 9; ++k) D->agg_cell[(size_t)k * a.n + i] = agg[k];
            if (!(with_daily && daily_due)) {
                agg[0] = day0;
                agg[1] = day1;
            }
            if (m1_pending) {
                prec_m1 = prec;
                swe_m1 = swe;
            }
            const bool snow = (swe > 0) || (swe_top > 0);
            b |= front_candidate_bits(prec, ta, snow, K.ta_fm);                                   // keep (sel_p < 0)
            b |= front_candidate_bits(agg[0], agg[1], snow, K.ta_fm) << FC_PER_CANDIDATE;        // daily
            b |= front_candidate_bits(agg[3], agg[4], snow, K.ta_fm) << (2 * FC_PER_CANDIDATE);  // hourly
            b |= front_candidate_bits(agg[6], agg[7], snow, K.ta_fm) << (3 * FC_PER_CANDIDATE);  // ten minutes
            b |= (swe_m1 > 0) ? BIT(FC_COMMON + 0) : 0;
            b |= !(swe <= 0) ? BIT(FC_COMMON + 1) : 0;
            b |= (prec_m1 != 0) ? BIT(FC_COMMON + 2) : 0;
            b |= (prec_m1 == 0) ? BIT(FC_COMMON + 3) : 0;
            b |= !(swe <= 0) ? BIT(FC_COMMON + 4 + PB_SWE_NOT_LE0) : 0;
            b |= (swe > 0) ? BIT(FC_COMMON + 4 + PB_SWE_GT0) : 0;
            b |= !(swe_top <= 0) ? BIT(FC_COMMON + 4 + PB_SWETOP_NOT_LE0) : 0;
            b |= (swe_top > 0) ? BIT(FC_COMMON + 4 + PB_SWETOP_GT0) : 0;
        }
    }
    // the wave's bits into the device-wide words (atomics that have RETURNED before the wave counts itself done: k_step's completion scheme)
    unsigned dep = 1;
    b = wave_or(b);
    db = wave_or(db);
    if ((threadIdx.x & 63) == 0) {
        if (db) dep |= (unsigned)(__hip_atomic_fetch_or(&D->dayw[(blockIdx.x & 63) * RH_WSTRIDE], db, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 63);
        if (b) dep |= (unsigned)(__hip_atomic_fetch_or(&D->frontw[(blockIdx.x & 63) * RH_WSTRIDE], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 63);
    }
    if (daily_only) return;   // (the front kernel behind this launch folds dayw)
    bool last = false;
    if ((threadIdx.x & 63) == 0) {
        const unsigned o = atomicAdd(&wg_done, dep);   // LDS; dep == 1 (bit 63 of the words is never set)
        if (o == (RH_BLOCK / 64) - 1) {
            last = grid_completion(D, n_groups);
        }
    }
    if (__shfl((int)last, 0)) {
        front_ctrl(D, daily_due, fd, hooks);
    }
}

// summary bits straight from the arena (first step, or after the host changed planes), OR-ed into sumw (zeroed by the host)
__global__ __launch_bounds__(RH_BLOCK) void k_summary(Arena a, DevState *D) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    unsigned long long b = 0;
    if (i < a.n) {
        double swe, swe_top, prec, ta;
        rh_ld(a, RH_P_swe, i, swe);
        rh_ld(a, RH_P_swe_top, i, swe_top);
        rh_ld(a, RH_P_prec, i, prec);
        rh_ld(a, RH_P_ta, i, ta);
        b = summary_bits(swe, swe_top, prec, ta, D->K);
    }
    b = wave_or(b);
    if ((threadIdx.x & 63) == 0 && b) __hip_atomic_fetch_or(&D->sumw[(blockIdx.x & 63) * RH_WSTRIDE], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Output accumulators: after a step that covered (t0, t1], day = t0 / 86400, slot = day mod diag_slots; the first
// step of a day (t0 on midnight) overwrites.  Rate planes add this step's value (Rate.diagnose, roger/diagnostics/
// rate.py:66-84: `rate += var[..., tau]`), collect planes keep the current one.  S.time / S.dt_secs were advanced by
// the control kernel before the fused kernel ran.  Per slot {steps, t0 of the interval's first step, t1 of its last step}, -1 each
// until a step touches the slot; a slot first touched inside its interval counts from 1 and keeps t0 = -1 (include/roger_hip.h).
// after_fused: the launch follows a fused k_step, whose prologue has just written D->skipped (the step found the run over,
// rh_set_time_limit: nothing to add).  Behind the routine-by-routine step (rh_step_core) and the routed passes there is no such
// launch in front and the flag may be left over from an earlier device run under a limit: they pass 0.
__global__ __launch_bounds__(RH_BLOCK) void k_diag(Arena a, DevState *D, int after_fused) {
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (i >= a.n || (after_fused && D->skipped)) return;
    const int64_t t0 = D->S.time - D->S.dt_secs, iv = D->diag_interval;
    const int64_t slot = (t0 / iv) % D->diag_slots;
    const bool first = (t0 % iv) == 0;   // steps never straddle an interval boundary they do not start on (adaptive_time_stepping)
    const int nr = D->diag_rate, nv = D->diag_rate + D->diag_collect;
    double *base = D->diag + (size_t)slot * nv * a.n;
    if (i == 0) {
        long long *m = D->diag_steps + 3 * slot;
        m[0] = (first || m[0] < 0) ? 1 : m[0] + 1;   // (-1: never touched -- a slot first touched inside its interval counts the steps accumulated)
        if (first) m[1] = t0;
        m[2] = D->S.time;
    }
    for (int j = 0; j < nv; ++j) {
        double v;
        rh_ld(a, D->diag_planes[j], i, v);
        double *p = base + (size_t)j * a.n + i;
        *p = (j < nr && !first) ? *p + v : v;
    }
}
// Time series at observation columns (rh_points_configure): after a step, ONE workgroup gathers planes x cells into row
// points_rows mod points_cap of the ring and writes the row's header {itt, time at the end of the step, dt_secs} from D->S, as the
// control part left them for this step.  The cells lie anywhere in the arena, so the address is formed per lane (rh_cell_any: the
// tiled addressing without the wave-uniform tile of rh_cell).  Every thread reads the row counter, the barrier follows, and thread 0
// writes counter + 1 last: no thread of a launch sees the counter this launch advanced.  after_fused as for k_diag: a fused launch
// that found the run over (rh_set_time_limit) records nothing.
__global__ __launch_bounds__(RH_BLOCK) void k_points(Arena a, DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    const long long row = D->points_rows;
    const int nc = D->points_ncells, nv = nc * D->points_nplanes;
    const long long slot = row % D->points_cap;
    double *dst = D->points + (size_t)slot * nv;
    for (int k = threadIdx.x; k < nv; k += RH_BLOCK) {
        const int j = k / nc, c = k - j * nc;
        dst[k] = __builtin_nontemporal_load(rh_cell_any<const double>(a, D->points_planes[j], D->points_cells[c]));
    }
    const rh_scalars &S = D->S;
    const long long itt = S.itt, time = S.time, dt_secs = S.dt_secs;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long *h = D->points_hdr + 3 * slot;
        h[0] = itt;
        h[1] = time;
        h[2] = dt_secs;
        D->points_rows = row + 1;
    }
}
// Catchment totals (rh_totals_configure): after a step, the sum, minimum and maximum of up to 32 planes over the masked columns, one row
// of a ring per step.  The ORDER of the sum is fixed, so a host restatement (tests/totals_reference.py) gives the same bits:
//   a wavefront:  the tree over its 64 lanes with strides 32 ... 1, lane l < stride becomes x[l] + x[l + stride] (the xor butterfly
//                 gives lane 0 exactly that: every lane of a pair forms the same commutative sum)
//   a workgroup:  (w0 + w1) + (w2 + w3) of its four wavefronts, through LDS
//   the grid:     k_totals_finish, one workgroup: thread t adds the tiles' partials t, t + 256, ... in increasing order to the identity,
//                 then the 256 thread values take the same two levels
// The minimum and the maximum take the same path with fmin / fmax.  A column outside the mask or beyond n contributes the identity
// (+0.0, +inf, -inf).  No floating-point atomics: the tiles' partials are plain stores into totals_part [plane][stat][tile].
RH_DEV double totals_identity(int stat) { return stat == 0 ? 0.0 : (stat == 1 ? __builtin_huge_val() : -__builtin_huge_val()); }   // sum, min, max
RH_DEV double totals_op(int stat, double x, double y) { return stat == 0 ? x + y : (stat == 1 ? fmin(x, y) : fmax(x, y)); }
template <int STAT>
RH_DEV double totals_wave(double x) {
    for (int off = 32; off; off >>= 1) x = totals_op(STAT, x, __shfl_xor(x, off));
    return x;
}
#define RH_TOTALS_CHUNK 8   // planes loaded before the first of them is reduced (memory-level parallelism of the tile kernel)
__global__ __launch_bounds__(RH_BLOCK) void k_totals_tiles(Arena a, DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    __shared__ double part[RH_POINTS_MAX_PLANES * 3][RH_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    const int nv = D->totals_nplanes, wave = threadIdx.x >> 6;
    const unsigned char *mask = D->totals_mask;
    const bool inside = i < a.n;
    const bool counted = inside && (!mask || __builtin_nontemporal_load(mask + i) != 0);
    for (int j0 = 0; j0 < nv; j0 += RH_TOTALS_CHUNK) {
        double v[RH_TOTALS_CHUNK];
#pragma unroll
        for (int k = 0; k < RH_TOTALS_CHUNK; ++k) {
            v[k] = 0.0;
            if (inside && j0 + k < nv) rh_ld(a, D->totals_planes[j0 + k], i, v[k]);
        }
#pragma unroll
        for (int k = 0; k < RH_TOTALS_CHUNK; ++k) {
            if (j0 + k >= nv) break;
            const double s = totals_wave<0>(counted ? v[k] : totals_identity(0));
            const double lo = totals_wave<1>(counted ? v[k] : totals_identity(1));
            const double hi = totals_wave<2>(counted ? v[k] : totals_identity(2));
            if ((threadIdx.x & 63) == 0) {
                part[(j0 + k) * 3 + 0][wave] = s;
                part[(j0 + k) * 3 + 1][wave] = lo;
                part[(j0 + k) * 3 + 2][wave] = hi;
            }
        }
    }
    __syncthreads();
    const int ntiles = D->totals_ntiles;
    for (int q = threadIdx.x; q < nv * 3; q += RH_BLOCK) {
        const int stat = q % 3;
        D->totals_part[(size_t)q * ntiles + blockIdx.x] = totals_op(stat, totals_op(stat, part[q][0], part[q][1]), totals_op(stat, part[q][2], part[q][3]));
    }
}
// ONE workgroup: the tiles' partials into row totals_rows mod totals_cap, values (plane, {sum, min, max}), and the row's header from D->S
// as k_points writes it.  Every thread reads the row counter, the barrier follows, thread 0 writes counter + 1 last.
__global__ __launch_bounds__(RH_BLOCK) void k_totals_finish(DevState *D, int after_fused) {
    if (after_fused && D->skipped) return;
    __shared__ double part[RH_POINTS_MAX_PLANES * 3][RH_BLOCK / 64];
    const long long row = D->totals_rows;
    const long long slot = row % D->totals_cap;
    const int nq = D->totals_nplanes * 3, ntiles = D->totals_ntiles;
    // Four planes x three statistics x four partials per thread are loaded before the first is used: the loads of a thread are
    // independent, only its additions are ordered (one partial per round would cost a memory latency each: 15 x 24 of them in a row at
    // 10^6 columns and eight planes).
    constexpr int PJ = 4, PT = 4;
    for (int j0 = 0; j0 < nq / 3; j0 += PJ) {
        double x[PJ][3];
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int st = 0; st < 3; ++st) x[j][st] = totals_identity(st);
        for (int t0 = threadIdx.x; t0 < ntiles; t0 += PT * RH_BLOCK) {
            double v[PJ][3][PT];
#pragma unroll
            for (int j = 0; j < PJ; ++j)
#pragma unroll
                for (int st = 0; st < 3; ++st)
#pragma unroll
                    for (int k = 0; k < PT; ++k) {
                        const int t = t0 + k * RH_BLOCK;
                        v[j][st][k] = (j0 + j < nq / 3 && t < ntiles) ? D->totals_part[(size_t)((j0 + j) * 3 + st) * ntiles + t] : 0.0;
                    }
#pragma unroll
            for (int k = 0; k < PT; ++k)   // in increasing tile order
                if (t0 + k * RH_BLOCK < ntiles) {
#pragma unroll
                    for (int j = 0; j < PJ; ++j)
#pragma unroll
                        for (int st = 0; st < 3; ++st) x[j][st] = totals_op(st, x[j][st], v[j][st][k]);
                }
        }
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
            if (j0 + j >= nq / 3) break;
            const double s = totals_wave<0>(x[j][0]), lo = totals_wave<1>(x[j][1]), hi = totals_wave<2>(x[j][2]);
            if ((threadIdx.x & 63) == 0) {
                part[(j0 + j) * 3 + 0][threadIdx.x >> 6] = s;
                part[(j0 + j) * 3 + 1][threadIdx.x >> 6] = lo;
                part[(j0 + j) * 3 + 2][threadIdx.x >> 6] = hi;
            }
        }
    }
    const rh_scalars &S = D->S;
    const long long itt = S.itt, time = S.time, dt_secs = S.dt_secs;
    __syncthreads();
    double *dst = D->totals + (size_t)slot * nq;
    for (int q = threadIdx.x; q < nq; q += RH_BLOCK) {
        const int stat = q % 3;
        dst[q] = totals_op(stat, totals_op(stat, part[q][0], part[q][1]), totals_op(stat, part[q][2], part[q][3]));
    }
    if (threadIdx.x == 0) {
        long long *h = D->totals_hdr + 3 * slot;
        h[0] = itt;
        h[1] = time;
        h[2] = dt_secs;
        D->totals_rows = row + 1;
    }
}
// multi-GPU: OR of the summary words into words[3] for the exchange
// dst64 != null: also spread over 64 int32 (0 / 1) for the MAX all-reduce (k_words_expand folded in)
__global__ __launch_bounds__(RH_BLOCK) void k_summary_reduce(DevState *D, int do_hooks, int *dst64, int src) {
    if (do_hooks) hooks_set_forcing(D);
    if (threadIdx.x < 64) {
        unsigned long long w;
        if (src == RH_SRC_SUMW) {
            w = wave_or(dev_load(&D->sumw[threadIdx.x * RH_WSTRIDE]));
            dev_store(&D->sumw[threadIdx.x * RH_WSTRIDE], 0ull);
        } else {
            w = D->words[3];
        }
        if (threadIdx.x == 0) D->words[3] = w;
        if (dst64) dst64[threadIdx.x] = (int)((w >> threadIdx.x) & 1ull);
    }
}

__global__ void k_export(const DevState *D, HostExport *H, unsigned long long seq) {
    H->S = D->S;
    H->bad = D->words[2];
    H->bad_last = D->sanity_last;
    H->err = D->err_flags;
    __threadfence_system();
    __hip_atomic_store(&H->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_advance(DevState *D) {  // roger.py:449-450
    D->S.itt += 1;
    D->S.time += D->S.dt_secs;
}
__global__ void k_rotate_scalars(DevState *D) {
    rh_scalars &S = D->S;
    S.event_id[0] = S.event_id[1];
    S.year[0] = S.year[1];
    S.month[0] = S.month[1];
    S.doy[0] = S.doy[1];
}
__global__ void k_sync_ctx(DevState *D) {
    D->X.dt = D->S.dt;
    D->X.month_tau = D->S.month[1];
    D->X.itt_day = D->S.itt_day;
}
__global__ void k_sanity_to_scalars(DevState *D) { D->S.sanity_ok = D->words[2] ? 0 : 1; }
// Multi-GPU: NCCL/RCCL has no bitwise-OR reduction, so a predicate word is spread over 64 int32
// (0/1) for a MAX all-reduce and folded back afterwards.
__global__ void k_words_expand(DevState *D, int w, int *dst) { dst[threadIdx.x] = (int)((D->words[w] >> threadIdx.x) & 1ull); }
__global__ void k_words_compress(DevState *D, int w, const int *src) {
    unsigned long long b = src[threadIdx.x] ? (1ull << threadIdx.x) : 0ull;
    for (int off = 32; off; off >>= 1) b |= __shfl_xor(b, off);
    if (threadIdx.x == 0) D->words[w] = b;
}

#endif  // RH_CONTROL_H
