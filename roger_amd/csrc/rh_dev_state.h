// rh_dev_state.h -- the device-resident control block (DevState), what the host reads back (HostExport), the launch constants and
// the wavefront / workgroup reductions and NumPy-ordered sums every kernel file builds on.  Part of the one translation unit
// roger_hip.hip.
#ifndef RH_DEV_STATE_H
#define RH_DEV_STATE_H

#define RH_BLOCK 256
// unused slots appended to every tile of the arena (the tile stride in units of 512 bytes decides how the tiles spread over the HBM
// channels; experiments)
#ifndef RH_STRIDE_PAD
#define RH_STRIDE_PAD 0
#endif
#define RH_PRED_BLOCKS 1024  // grid of the grid-stride predicate kernels
#define RH_DONE_GROUPS 256   // completion counters of the fused kernel (two levels: workgroup -> group -> grid), a cache line each
#define RH_DONE_STRIDE 32   // (unsigned ints: 128 bytes)
#define RH_DEVERR_FORCING 1u // a step began a day beyond the end of the resident forcing series
// flags of k_step / sources of k_ctrl
#define RH_TAIL_USE_NEXT 1   // this step runs on S_next / X_next (the previous kernel's tail formed them); its tail commits them
#define RH_TAIL_CTRL 2       // the tail forms the next step's S_next / X_next
#define RH_TAIL_HOOKS 4      // ... including the device-side set_forcing / set_parameters hooks
#define RH_TAIL_PRE 16      // (with RH_TAIL_CTRL) the launch has one workgroup more than the columns need: its first wavefront forms the half of the
                             // next step's control part that does not depend on the columns WHILE they are stepped (pre_tail); the tail does the rest
#define RH_TAIL_SKIP 8       // nobody reads this step's summary word (per-cell forcing behind k_cell_front, which looks at the planes): no summary
                             // bits posted, no completion counting, no tail -- three round trips less at the end of a launch-bound step
#define RH_SRC_WORD3 0       // the summary word sits in words[3] (a fused kernel ran last)
#ifndef RH_WSTRIDE
#define RH_WSTRIDE 16       // words between two slots of the device-wide OR words (sumw, frontw, dayw): 128 bytes -- a slot per cache line
#endif
#define RH_SRC_SUMW 1        // ... in sumw[] (k_summary rebuilt it from the arena)
#define RH_POINTS_MAX_CELLS 256   // rh_points_configure: observation columns and planes per row -- at most 8 192 values, gathered by
#define RH_POINTS_MAX_PLANES 32   // ONE workgroup (k_points)
#ifndef RH_STEP_WAVES
#define RH_STEP_WAVES 2     // waves per SIMD the fused kernel is compiled for (register budget 512 / waves)
#endif

// ---------------------------------------------------------------------------------------------
// device-resident control block
// ---------------------------------------------------------------------------------------------
struct DevState {
    Consts K;
    rh_scalars S;
    StepCtx X;
    unsigned long long words[4];  // predicate words 0,1; word 2 = "sanity violated"; word 3 scratch
    // per-workgroup partial predicate words of k_pred1 / k_select: plain stores, OR-reduced by the
    // single-workgroup kernel that follows (a single word hammered by atomics from every wave
    // costs ~100 us per pass: one address sustains ~90 atomics/us)
    unsigned long long bflags[2][RH_PRED_BLOCKS];
    unsigned long long day_bflags[RH_PRED_BLOCKS];   // k_pred1, weighted station forcing: the forcing bits of the day per workgroup
    int pred_blocks;               // workgroups launched for k_pred1 / k_select
    // summary path: the QB_* bits of every column at the end of a step, OR-ed by the fused kernel's wavefronts into 64 words
    // (device-scope atomics, word = workgroup mod 64: ~250 atomics per address and step at 10^6 columns); the last wavefront
    // to finish folds them into words[3] and runs the control part of the NEXT step on S_next / X_next (step_tail)
    unsigned long long sumw[64 * RH_WSTRIDE];   // 64 slots, one per cache line (RH_WSTRIDE)
    unsigned int done_grp[RH_DONE_GROUPS * RH_DONE_STRIDE];   // workgroups finished per completion group (workgroup b belongs to group b mod n_groups)
    unsigned int done_top;                   // groups finished
    unsigned long long sanity_last;          // words[2] of the last fused step (the tail clears words[2] for the next one)
    // what the control part keeps of the DAY's shared series between two midnights (ctrl_wave): the OR of the slots' forcing bits and the
    // three daily aggregates -- a step inside the day then needs the six slots of its hourly window only.  Everything that writes forc
    // clears day_cache_ok.
    unsigned long long pre_words[64];        // pre_tail -> tail of one fused launch (TailPre, a word per lane)
    int day_cache_ok, day_cache_pad;
    unsigned long long day_fb;
    double day_agg[3];
    unsigned int err_flags;                  // RH_DEVERR_*
    rh_scalars S_next;                       // scalars / step context of the next step, formed by the tail of the last fused kernel;
    StepCtx X_next;                          // committed to S / X by the tail of the kernel that runs that step
    // device-side output accumulators (rh_diag_configure): (diag_slots, diag_rate + diag_collect, n) float64
    double *diag;
    long long *diag_steps;         // per slot: {steps accumulated (the divisor of the "average" diagnostic), start time of the
                                   // interval's first step, end time of its last step}
    long long diag_interval;       // output interval in seconds (86400, 3600 or 600)
    int diag_rate, diag_collect, diag_slots;
    int diag_planes[32];
    // sparse stores with accumulators: the pure-output planes an accumulator was given are stored by the sparse kernel after all
    // (bit p of keep[p / 64]; keep_any = any bit set) -- the other ~70 stay unwritten
    unsigned long long keep[(RH_NPLANES + 63) / 64];
    int keep_any;
    // rh_enable_timing: dt_secs of every step since then (the time-step class of each timed launch)
    int *dt_log;
    int dt_log_cap, dt_log_n;
    double forc[3][RH_SLOTS_PER_DAY];  // shared forcing of the day: prec, ta, pet
    const double *forc_cell[3];        // per-cell forcing, TRANSPOSED on upload to (144, n): slot s of column i at [s * n + i], unit stride over
                                       // the columns (a wave reads 512 contiguous bytes per slot instead of 64 values 1152 bytes apart); or null
    double *agg_cell;                  // per-cell aggregates, 9 planes of n (written by k_cell_agg)
    // per-cell forcing, one launch in front of the fused kernel (k_cell_front): frontw = the waves' column bits of the step (word 0's
    // snow bits, word 1's terms for each candidate selection), dayw = the forcing bits of the DAY over all columns and slots (formed
    // once a day, folded into day_word by the front kernel's last wavefront)
    unsigned long long frontw[64 * RH_WSTRIDE], dayw[64 * RH_WSTRIDE], day_word;
    int per_cell;
    // whole forcing series resident on the device (rh_set_forcing_series): 10-minute PREC/TA/PET
    // and the calendar vectors, as the benchmark's set_forcing_setup holds them in vs.PREC, ...
    const double *series[3];
    const int64_t *calendar[3];
    int64_t nitt_forc;
    long long t_end;                   // rh_set_time_limit: no step begins at or beyond this model time (< 0: no limit)
    int skipped;                       // the last fused launch found its step halted and did nothing (read by k_diag)
    int monthly;                       // set_parameters' month-change test, evaluated on the device
    const double *weights[3];          // per-cell prec_weight, ta_offset, pet_weight (rh_set_forcing_weights) or null
    // several meteorological stations (settings.enable_distributed_input, roger/variables.py:6383-6402): the resident series are
    // (n_stations, nitt_forc) each, a column takes the series of station station_idx[column] (< 0: none, all zeros); the day of
    // every station is staged in forc_multi (3, n_stations, 144) at midnight
    int n_stations;
    const int *station_idx;
    double *forc_multi;

    // Parameter planes of the fused step (RH_PARAM_BITS): one 64-bit word per wavefront's 64 columns.  Bit b: the wave's columns hold
    // ONE value of parameter plane b, so the wave reads one element instead of 512 bytes; bit 63: the planes of RH_DERIVED_FIELDS hold
    // exactly what the stages' rd_* functions compute from the primaries, so they are derived instead of loaded.  Written by
    // k_param_mask whenever somebody other than the fused kernel may have changed planes; all zeros = the plain loads.
    const unsigned long long *pmask;

    const double *mlms;                // lut_mlms rows (oneD model), device copy
    int64_t mlms_rows;
    int max_slope_per;
    Luts L;

    // time series at observation columns (rh_points_configure; k_points): a ring of points_cap rows on the device, row r at r mod
    // points_cap -- points (row, plane, cell) float64 and points_hdr {itt, time at the end of the step, dt_secs} per row.  points_rows
    // counts the rows recorded since the configuration.  (Behind everything else: no member a k_step variant addresses moves.)
    double *points;
    long long *points_hdr;
    long long points_rows, points_cap;
    int points_ncells, points_nplanes;
    int points_planes[RH_POINTS_MAX_PLANES];
    long long points_cells[RH_POINTS_MAX_CELLS];

    // catchment totals (rh_totals_configure; k_totals_tiles, k_totals_finish): a ring of totals_cap rows, row r at r mod totals_cap --
    // totals (row, plane, {sum, min, max}) float64 and totals_hdr as points_hdr.  totals_part [plane][stat][tile]: the partials of the
    // totals_ntiles workgroups of k_totals_tiles.  totals_mask: a byte per column (0: outside the area), or null: every column.
    double *totals;
    long long *totals_hdr;
    double *totals_part;
    const unsigned char *totals_mask;
    long long totals_rows, totals_cap;
    int totals_nplanes, totals_ntiles;
    int totals_planes[RH_POINTS_MAX_PLANES];

    // zonal totals (rh_zonal_configure; k_zonal_tiles, k_zonal_finish in rh_zonal.h): a ring of zonal_cap rows, row r at r mod zonal_cap --
    // zonal (row, zone, plane, {sum, min, max}) float64 and zonal_hdr as points_hdr.  zonal_zone: the zone of every column (-1: outside).
    // The index rh_zonal_configure builds once: tile b holds the zones zonal_tile_zone[zonal_tile_ptr[b] ... zonal_tile_ptr[b + 1]),
    // ascending; that position s is the (tile, zone) pair's SLOT, its partials are zonal_part [slot][plane][stat].  Accumulator t of zone
    // z takes the slots zonal_acc_slot[zonal_acc_ptr[z * 256 + t] ... zonal_acc_ptr[z * 256 + t + 1]), in increasing tile order.
    double *zonal;
    long long *zonal_hdr;
    double *zonal_part;
    const int *zonal_zone, *zonal_tile_ptr, *zonal_tile_zone, *zonal_acc_ptr, *zonal_acc_slot;
    long long zonal_rows, zonal_cap;
    int zonal_nplanes, zonal_nzones;
    int zonal_planes[RH_POINTS_MAX_PLANES];

    // scores against observed series (rh_scores_configure; k_scores in rh_scores.h): scores (item, {acc, m1, m2, m3, m4}, n) float64,
    // scores_obs (item, series, interval) float64 with NaN for a missing observation, scores_series: the series of every column (< 0: not
    // scored) or null (every column series 0), scores_closed: a byte per interval, set when a scored step closed it.  Interval k covers
    // (scores_t_first + k * scores_interval, scores_t_first + (k + 1) * scores_interval].
    double *scores;
    const double *scores_obs;
    const int *scores_series;
    unsigned char *scores_closed;
    long long scores_interval, scores_t_first, scores_nintervals;
    int scores_nitems, scores_nseries;
    int scores_planes[16], scores_kinds[16];   // RH_SCORES_MAX_ITEMS; kinds: 0 SUM, 1 LAST

    // event outputs (rh_events_configure; k_events in rh_events.h): events (slot, item, n) float64, event e in slot e mod events_nslots;
    // events_hdr (slot, 6) {event id, steps, t0 of its first step, t1 of its last step, steps of 600 s, steps of 3600 s}, -1 each until a
    // step touches the slot; events_ids (slot, events_nblk): the slot's event id once per workgroup of the launch (each workgroup reads
    // and writes its own copy only).  events_drained: the highest event id the host has read out; events_running: the id of the event
    // that was running when the observer was configured (0: none) -- it keeps t0 = -1; events_lost: a step found no free slot.
    double *events;
    long long *events_hdr, *events_ids;
    long long events_drained, events_running;
    int events_lost, events_nitems, events_nslots, events_nblk;
    int events_planes[16], events_kinds[16];   // RH_EVENTS_MAX_ITEMS; kinds: 0 SUM, 1 PEAK, 2 FIRST, 3 LAST

    // duration curves (rh_durations_configure; k_durations in rh_durations.h): durations_counts (bin, n) uint32, item j's m_j + 2 bins
    // (the NaN bin last) from durations_bin_off[j]; durations_vals (item, {acc, mn, mx}, n) float64; durations_spells (item, {run,
    // longest, n_spells}, n) uint32; durations_edges: the items' edges one behind the other, item j's durations_nedges[j] from
    // durations_edge_off[j]; durations_mask: a byte per column (0: not counted) or null; durations_thr: NaN for an item without a
    // spell; durations_nsum: SUM items among them.  (Behind everything else: no member another kernel addresses moves.)
    unsigned *durations_counts, *durations_spells;
    double *durations_vals;
    const double *durations_edges;
    const unsigned char *durations_mask;
    long long durations_interval, durations_t_first;
    int durations_nitems, durations_nsum;
    int durations_planes[16], durations_kinds[16], durations_nedges[16], durations_edge_off[16], durations_bin_off[16], durations_sides[16];
    double durations_thr[16];   // RH_DURATIONS_MAX_ITEMS; kinds: 0 SUM, 1 LAST; sides: 0 BELOW, 1 AT_OR_ABOVE

    // ensemble bands (rh_bands_configure; k_bands, k_bands_select in rh_bands.h): a ring of bands_cap rows, row r at r mod bands_cap --
    // bands (row, item, probability) float64 and bands_hdr (row, 2 + 2 * items) int64 {k, t1, then per item m, n_nan}.  bands_acc (item,
    // n) float64: the SUM accumulators; bands_keys (item, n) uint64: the keys of the interval values (~0: masked out, ~0 - 1: NaN);
    // bands_hist [item][8][2048] uint32: the digit histograms of the pass under way, all zeros between two launches; bands_done: the
    // workgroups of the pass that have finished, likewise 0; bands_nan_count: the NaN keys pass 0 met.  Per (item, probability) at
    // [item * 8 + probability]: bands_prefix, the digits picked so far, and bands_rank, the rank that remains among the keys with that
    // prefix; per item bands_m and bands_nan, fixed by pass 0.  (Behind everything else: no member another kernel addresses moves.)
    double *bands, *bands_acc;
    long long *bands_hdr;
    unsigned long long *bands_keys;
    unsigned *bands_hist;
    const unsigned char *bands_mask;
    long long bands_rows, bands_cap, bands_interval, bands_t_first;
    int bands_nitems, bands_nprobs, bands_nsum;
    unsigned bands_done;
    unsigned bands_nan_count[8];
    int bands_planes[8], bands_kinds[8];   // RH_BANDS_MAX_ITEMS; kinds: 0 SUM, 1 LAST
    double bands_probs[8];                 // RH_BANDS_MAX_PROBS
    unsigned long long bands_prefix[64];
    long long bands_rank[64], bands_m[8], bands_nan[8];
    // ... per zone (rh_bands_configure_zonal; k_bands_zonal, k_bands_zonal_row): bands is (row, item, zone, probability), bands_hdr (row,
    // 2) {k, t1} and bands_counts (row, item, zone, 2) int64 {m, n_nan}; bands_mask is zone >= 0.  bands_zone_off [zones + 1] and
    // bands_zone_cols: the columns of every zone, ascending within a zone.  Null without zones: the histograms and the members from
    // bands_done on are the plain selection's alone.
    long long *bands_counts;
    const int *bands_zone_off, *bands_zone_cols;
    // ... likelihood-weighted (rh_bands_configure_weighted; k_bands_select_w): bands_weight (n) uint16, 0: the column takes no part
    // (bands_mask is w != 0); bands_whist [item][8][2048] uint64: the digit histograms as sums of weights, all zeros between two launches;
    // bands_wsum (row, item) int64: W of every row, a ring beside bands_hdr; bands_m_count: the keys of numbers pass 0 met, 0 between two
    // launches; bands_w: W per item, fixed by pass 0.  Null without weights.
    const unsigned short *bands_weight;
    unsigned long long *bands_whist;
    long long *bands_wsum;
    unsigned bands_m_count[8];
    long long bands_w[8];
    // ... observations (rh_bands_observations; k_bands_obs, k_bands_obs_row, k_bands_obs_zonal): bands_obs (item, series, bands_obs_n)
    // float64, NaN: missing, series: 1, or the zones; row interval k reads element k + bands_obs_first.  bands_obs_part (item, workgroup,
    // 2) int64: the workgroups' {below, equal} of the step under way (plain and weighted); bands_obs_ring (row, item, series, 2) int64
    // {below, equal}, a ring beside bands_hdr, -1: no observation.  Null without observations.
    const double *bands_obs;
    long long *bands_obs_part, *bands_obs_ring;
    long long bands_obs_n, bands_obs_first;
};

// What the host reads after a step, in pinned host memory that the device writes directly (hipHostMallocMapped): k_export copies the
// committed scalars and flags and stores `seq` last (system scope), the host waits for its sequence number.  rh_get_scalars used
// four staged copies into pageable memory (>= 40 us); this is one one-thread kernel.
struct HostExport {
    rh_scalars S;
    unsigned long long bad, bad_last;
    unsigned int err, pad;
    unsigned long long seq;
};

// ---------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------
// OR a wavefront's predicate bits into a global word.  The word only ever gains bits during a
// kernel, so a wave whose bits are already present skips the atomic: after the first few waves
// nobody touches the word any more (one address sustains only ~90 atomics/us chip-wide).  The
// pre-check may read a stale (smaller) value, which costs an extra atomic, never a lost bit.
RH_DEV void wave_or_to(unsigned long long *word, unsigned long long bits) {
    for (int off = 32; off; off >>= 1) bits |= __shfl_xor(bits, off);
    if ((threadIdx.x & 63) == 0 && bits) {
        const unsigned long long seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bits & ~seen) atomicOr(word, bits);
    }
}
// OR over the workgroup, then one plain store per workgroup.
RH_DEV void block_or_store(unsigned long long *slot, unsigned long long bits) {
    __shared__ unsigned long long wv[RH_BLOCK / 64];
    for (int off = 32; off; off >>= 1) bits |= __shfl_xor(bits, off);
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0;
        for (int k = 0; k < RH_BLOCK / 64; ++k) b |= wv[k];
        *slot = b;
    }
}
// OR over the wavefront, one plain store per wave: no barrier, so a wave that is done retires at once (the fused
// kernel's waves finish at different times; a closing barrier would hold their registers until the slowest is done)
RH_DEV void wave_or_store(unsigned long long *wave_slots, unsigned long long bits) {
    for (int off = 32; off; off >>= 1) bits |= __shfl_xor(bits, off);
    if ((threadIdx.x & 63) == 0) wave_slots[threadIdx.x >> 6] = bits;
}
// OR-reduce the per-workgroup words (one workgroup of RH_BLOCK threads); result valid in thread 0.
RH_DEV unsigned long long reduce_bflags(const unsigned long long *bf, int nblk) {
    __shared__ unsigned long long wv[RH_BLOCK / 64];
    unsigned long long b = 0;
    // 32 independent loads in flight per thread: the words were written by other CUs (other XCDs' L2s), a single
    // workgroup reading 15 000 of them a few dependent loads at a time is latency-bound (2 us per round trip)
    for (int k = threadIdx.x; k < nblk; k += 32 * RH_BLOCK) {
        unsigned long long v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int idx = k + j * RH_BLOCK;
            v[j] = idx < nblk ? bf[idx] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) b |= v[j];
    }
    for (int off = 32; off; off >>= 1) b |= __shfl_xor(b, off);
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = b;
    __syncthreads();
    b = 0;
    for (int k = 0; k < RH_BLOCK / 64; ++k) b |= wv[k];
    __syncthreads();
    return b;
}
#define BIT(b) (1ull << (b))
RH_DEV bool bit(unsigned long long w, int b) { return (w >> b) & 1ull; }

// numpy's pairwise add.reduce over 144 contiguous float64 (two blocks of 72, eight partial sums
// each) -- the reference aggregates the day's forcing with np.sum / np.nanmean
// (adaptive_time_stepping.py:384-437), so the grouping is part of the result.
RH_DEV double np_sum72(const double *a) {
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    for (int i = 8; i < 72; i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    return ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
}
// ... of values given by an accessor: the eight partial sums run in registers (a staging buffer of 72 doubles per thread lived in scratch
// memory: the daily sums of 10^6 columns with weighted forcing took 1.4 ms, all of it scratch traffic)
template <class Get>
RH_DEV double np_sum72_of(Get get, int base) {
    double r0 = get(base), r1 = get(base + 1), r2 = get(base + 2), r3 = get(base + 3);
    double r4 = get(base + 4), r5 = get(base + 5), r6 = get(base + 6), r7 = get(base + 7);
#pragma unroll 1   // (fully unrolled the 144 loads of a sum are hoisted together: 512 registers and spills)
    for (int i = 8; i < 72; i += 8) {
        r0 += get(base + i); r1 += get(base + i + 1); r2 += get(base + i + 2); r3 += get(base + i + 3);
        r4 += get(base + i + 4); r5 += get(base + i + 5); r6 += get(base + i + 6); r7 += get(base + i + 7);
    }
    return ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
}
template <class Get>
RH_DEV double np_sum144(Get get) {
    const double h0 = np_sum72_of(get, 0);
    return 0.0 + (h0 + np_sum72_of(get, 72));
}

// aggregates {prec, ta, pet} x {daily, hourly, 10 min} of one forcing series (stride between
// consecutive slots given, so the same code serves the shared vector and per-cell rows)
// np.sum over the 144 slots of a series that is 0 outside the hourly window [itd, itd + 6) (the masked sums of
// adaptive_time_stepping.py:400-420), in numpy's pairwise order without walking the 138 zeros: the window's six
// consecutive slots fall into six different lanes of the two 72-blocks (lane = slot mod 8), every lane also receives
// zeros (v + 0.0: a negative zero becomes positive, as in the full sum), and the lanes are combined as np_sum72 does.
// itd is uniform over the grid, so the lane selection is scalar work.
// A window that lies inside one 72-block (every hourly step's: itd a multiple of 6) with a start that is the same over the wavefront
// takes the short way: the six values sit in six of the eight lanes of ONE block in rotated order, r = itd mod 8 says where, and each of
// the eight rotations is the tree ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)) with its two zero lanes written out of it (x + 0.0 = x
// for everything but a negative zero, which `+ 0.0` on the way in has removed; the other block's 0.0 and the leading 0.0 + likewise):
// five additions behind a scalar branch instead of 96 selects per sum (k_cell_agg<1> at 10^6 columns: 39 -> 17 us).
template <class Get>
RH_DEV double np_sum144_window_general(Get get, int64_t itd) {
    double lane[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) lane[h][j] = 0.0;
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        const int64_t k = itd + w;
        if (k < 0 || k >= RH_SLOTS_PER_DAY) continue;
        const double v = get((int)k) + 0.0;
        const int h = k >= 72 ? 1 : 0, j = (int)((k - 72 * h) & 7);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
                if (hh == h && jj == j) lane[hh][jj] = v;
    }
    const double h0 = ((lane[0][0] + lane[0][1]) + (lane[0][2] + lane[0][3])) + ((lane[0][4] + lane[0][5]) + (lane[0][6] + lane[0][7]));
    const double h1 = ((lane[1][0] + lane[1][1]) + (lane[1][2] + lane[1][3])) + ((lane[1][4] + lane[1][5]) + (lane[1][6] + lane[1][7]));
    return 0.0 + (h0 + h1);
}
template <class Get>
RH_DEV double np_sum144_window(Get get, int64_t itd) {
    const int iu = __builtin_amdgcn_readfirstlane((int)itd);
    if (__all((int64_t)iu == itd) && iu >= 0 && iu + 6 <= RH_SLOTS_PER_DAY && !(iu < 72 && iu + 6 > 72)) {
        const double v0 = get(iu) + 0.0, v1 = get(iu + 1) + 0.0, v2 = get(iu + 2) + 0.0, v3 = get(iu + 3) + 0.0, v4 = get(iu + 4) + 0.0,
                     v5 = get(iu + 5) + 0.0;
        switch (iu & 7) {
        case 0: return ((v0 + v1) + (v2 + v3)) + (v4 + v5);
        case 1: return (v0 + (v1 + v2)) + ((v3 + v4) + v5);
        case 2: return (v0 + v1) + ((v2 + v3) + (v4 + v5));
        case 3: return (v5 + v0) + ((v1 + v2) + (v3 + v4));
        case 4: return (v4 + v5) + ((v0 + v1) + (v2 + v3));
        case 5: return ((v3 + v4) + v5) + (v0 + (v1 + v2));
        case 6: return ((v2 + v3) + (v4 + v5)) + (v0 + v1);
        default: return ((v1 + v2) + (v3 + v4)) + (v5 + v0);
        }
    }
    return np_sum144_window_general(get, itd);
}

// aggregates {prec, ta, pet} x {daily, hourly, 10 min} of one forcing series given by accessors (per-cell rows, or the
// weighted station forcing: PREC[k] * w, TA[k] + offset, PET[k] * w).  daily = false leaves a[0..2] alone: the daily
// sums only change with the day.
template <class P, class T, class E>
RH_DEV void forcing_aggregates_of(P p, T t, E e, int64_t itd, double *a, bool daily = true, bool hourly = true);
RH_DEV void forcing_aggregates(const double *p, const double *t, const double *e, int64_t itd, double *a) {
    forcing_aggregates_of([&](int k) { return p[k]; }, [&](int k) { return t[k]; }, [&](int k) { return e[k]; }, itd, a);
}
template <class P, class T, class E>
RH_DEV void forcing_aggregates_of(P p, T t, E e, int64_t itd, double *a, bool daily, bool hourly) {
    if (daily) {
        a[0] = np_sum144([&](int k) { return p(k); });
        int cnt = 0;
        for (int k = 0; k < 144; ++k) cnt += !isnan(t(k));
        a[1] = np_sum144([&](int k) { const double v = t(k); return isnan(v) ? 0.0 : v; }) / (double)cnt;
        a[2] = np_sum144([&](int k) { return e(k); });
    }
    if (!hourly) return;
    a[3] = np_sum144_window([&](int k) { return p(k); }, itd);
    {
        int cnt = 0;
        for (int w = 0; w < 6; ++w) {
            const int64_t k = itd + w;
            cnt += (k >= 0 && k < 144) && !isnan(t((int)k));
        }
        a[4] = np_sum144_window([&](int k) { const double v = t(k); return isnan(v) ? 0.0 : v; }, itd) / (double)cnt;
    }
    a[5] = np_sum144_window([&](int k) { return e(k); }, itd);
    int64_t k = itd < 0 ? itd + 144 : itd;
    k = k > 143 ? 143 : k;
    a[6] = p((int)k);
    a[7] = t((int)k);
    a[8] = e((int)k);
}

RH_DEV unsigned long long forcing_bits(double p, double t, const Consts &K) {
    unsigned long long b = 0;
    const double hpi = (double)K.hpi;
    b |= !(p <= 0) ? BIT(PB_P_NOT_LE0) : 0;
    b |= (p > 0) ? BIT(PB_P_GT0) : 0;
    b |= (p > hpi) ? BIT(PB_P_GT_HPI) : 0;
    b |= !(p <= hpi) ? BIT(PB_P_NOT_LE_HPI) : 0;
    b |= !(t > K.ta_fm) ? BIT(PB_TA_NOT_GT) : 0;
    b |= (t > K.ta_fm) ? BIT(PB_TA_GT) : 0;
    b |= ((p > 0) && (t <= K.ta_fm)) ? BIT(PB_PGT0_TALE) : 0;
    b |= !((p <= 0) && (t <= K.ta_fm)) ? BIT(PB_NOT_PLE0_TALE) : 0;
    return b;
}

#endif  // RH_DEV_STATE_H
