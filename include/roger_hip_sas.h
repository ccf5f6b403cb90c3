/*
 * include/roger_hip_sas.h -- C ABI of the MI355X-native ("hip") backend for RoGeR's offline
 * oxygen-18 transport step with StorAge-selection (SAS) functions, deterministic solver.
 *
 * Replaces, for `enable_offline_transport and enable_oxygen18 and sas_solver == "deterministic"`,
 * the body of `svat_transport_model_deterministic` (roger/core/transport.py:949-991), i.e. the
 * `@roger_kernel`s
 *   calc_infiltration_rz_transport_iso_kernel      core/infiltration.py:2218-2346
 *   calc_evaporation_transport_iso_kernel          core/evapotranspiration.py:653-719
 *   calc_transpiration_transport_iso_kernel        core/evapotranspiration.py:831-901
 *   calc_percolation_rz_transport_iso_kernel       core/subsurface_runoff.py:1531-1626
 *   calc_infiltration_ss_transport_iso_kernel      core/infiltration.py:2441-2512
 *   calc_percolation_ss_transport_iso_kernel       core/subsurface_runoff.py:1753-1820
 *   calc_capillary_rise_rz_transport_iso_kernel    core/capillary_rise.py:404-500
 *   calc_root_zone/subsoil/soil_transport_iso_kernel  core/root_zone.py:189-217, subsoil.py:159-188, soil.py:1036-1090
 *   calculate_age_statistics_*                     core/transport.py:59-312
 *   calc_ageing_sa_msa_iso_kernel                  core/transport.py:682-739, 780-805
 * with the helpers calc_SA, calc_tt, calc_mtt, calc_conc_iso_flux, calc_conc_iso_storage,
 * conc_to_delta, update_sa (transport.py:315-619) and the SAS families of core/sas.py: uniform (code 1),
 * dirac (2), kumaraswami (3, 31-37), gamma (4), exponential (51, 52), power (6, 61, 62).  rh_sas_sync reports a column
 * whose code is none of these (RH_ERR_STATE).
 *
 * With `tracer = RH_SAS_TRACER_BROMIDE` (settings.enable_bromide) the same step runs the reference's anion kernels
 * instead, where msa_* hold solute MASS by age and C_* are concentrations in mg/l:
 *   calc_infiltration_rz/ss_transport_anion_kernel core/infiltration.py:2350-2424, 2516-2566
 *   calc_evaporation_transport_kernel              core/evapotranspiration.py:620-650 (water only)
 *   calc_transpiration_transport_anion_kernel      core/evapotranspiration.py:905-985 (alpha_transp, crop uptake switch)
 *   calc_percolation_rz/ss_transport_anion_kernel  core/subsurface_runoff.py:1630-1716, 1823-1893 (alpha_q)
 *   calc_capillary_rise_rz_transport_anion_kernel  core/capillary_rise.py:503-590
 *   calc_root_zone/subsoil_transport_anion_kernel, calculate_soil_transport_anion_kernel
 *                                                  core/root_zone.py:221-258, subsoil.py:186-223, soil.py:1094-1142
 *   calc_ageing_sa_kernel, calc_ageing_msa_kernel  core/transport.py:623-680, 743-778
 * with calc_mtt's anion branch (transport.py:583-596); RH_SAS_RESCALE then follows rescale_sa_msa_anion_soil_kernel's
 * bromide branch (core/soil.py:1399-1506) or, with RH_SAS_TRACER_CHLORIDE (settings.enable_chloride), its chloride
 * branch (:1507-1640), which RH_SAS_TRACER_VIRTUAL shares.  Nitrate is not implemented.
 *
 * Same conventions as roger_hip.h: plain pointers and sizes, 0 / negative rh_status returns,
 * rh_sas_last_error for the text, one context = one HIP device + one stream, asynchronous
 * launches fenced by rh_sas_sync / rh_sas_download.
 *
 * Data layout.  All arrays are float64 (maskCatch: int32, read as the reference's bool -- roger/variables.py:462-470 --: any non-zero
 * value is 1) over the rank's interior cells in C
 * order (x, y); age-resolved arrays are (n_cells, ages) / (n_cells, ages + 1) with the age axis
 * contiguous, exactly the reference's `vs.sa_rz[2:-2, 2:-2, vs.tau, :]` etc., so that one
 * workgroup streams one column's age vector with unit stride.  Only the prognostic state
 * (sa_rz, msa_rz, sa_ss, msa_ss) has to live in HBM; the per-flux distributions (tt, mtt, TT),
 * sa_s and msa_s are diagnostics that are written only when the context was created with
 * `keep_distributions` (they are 17 more age vectors per column).
 */
#ifndef ROGER_HIP_SAS_H
#define ROGER_HIP_SAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RH_SAS_TRACER_OXYGEN18 0
#define RH_SAS_TRACER_BROMIDE 1
#define RH_SAS_TRACER_CHLORIDE 2 /* the anion kernels as for bromide; RH_SAS_RESCALE scales the solute with the water */
#define RH_SAS_TRACER_VIRTUAL 3  /* settings.enable_virtualtracer: as chloride, and the soil evaporation takes the tracer along
                                    (calc_evaporation_transport_virtualtracer_kernel, core/evapotranspiration.py:722-791) */
/* settings.sas_solver (roger/settings.py:119): "deterministic" (svat_transport_model_deterministic, core/transport.py:949-991) or the
 * explicit "Euler" scheme (svat_transport_model_euler :2064-2414, isotope and anion branches): every sub-step of length settings.h = 1 / substeps
 * evaluates all five fluxes on the StorAge as it stands; "RK4" (svat_transport_model_rk4 :1139-2047, both branches) evaluates them
 * four times per sub-step on trial StorAges and updates with the weighted mean of the four travel time distributions. */
#define RH_SAS_SOLVER_DETERMINISTIC 0
#define RH_SAS_SOLVER_EULER 1
#define RH_SAS_SOLVER_RK4 2
#define RH_SAS_MAX_NAGES 4096 /* ages + 1 <= this (benchmark: ages = 1000, SVATOXYGEN18_benchmark.py:28-44) */

typedef struct rh_sas_config {
    int64_t n_cells;           /* local interior cells (nx * ny of this rank) */
    int32_t ages;              /* settings.ages; nages = ages + 1 */
    int32_t substeps;          /* settings.sas_solver_substeps */
    int32_t device;            /* HIP device ordinal */
    int32_t forcing_days;      /* number of days of daily input resident on the device (>= 1) */
    int32_t age_statistics;    /* settings.enable_age_statistics */
    int32_t keep_distributions;/* also write tt_*, mtt_*, TT_*, sa_s, msa_s (diagnostics) */
    double vsmow, d18O_min, d18O_max; /* settings.VSMOW_conc18O, d18O_min, d18O_max (roger/settings.py:76-78); for
                                       * settings.enable_deuterium: VSMOW_conc2H, d2H_min, d2H_max (:79-81), same kernels */
    int32_t tracer;            /* RH_SAS_TRACER_OXYGEN18 | _BROMIDE | _CHLORIDE | _VIRTUAL (settings.enable_oxygen18 / enable_bromide / enable_chloride / enable_virtualtracer) */
    int32_t solver;            /* RH_SAS_SOLVER_DETERMINISTIC | _EULER | _RK4 (settings.sas_solver) */
} rh_sas_config;

typedef struct rh_sas_ctx rh_sas_ctx;

void rh_sas_default_config(rh_sas_config *cfg);
int rh_sas_create(const rh_sas_config *cfg, rh_sas_ctx **out);
void rh_sas_destroy(rh_sas_ctx *ctx);
const char *rh_sas_last_error(const rh_sas_ctx *ctx); /* ctx may be NULL for rh_sas_create failures */
int rh_sas_set_stream(rh_sas_ctx *ctx, void *hip_stream);
int rh_sas_sync(rh_sas_ctx *ctx);

/* ---- array registry ------------------------------------------------------------------------
 * Names follow the reference variables (roger/variables.py): state `sa_rz msa_rz sa_ss msa_ss`;
 * daily inputs (forcing_days, n) `inf_mat_rz inf_pf_rz inf_pf_ss evap_soil transp q_rz q_ss cpr_rz
 * C_in` (what `set_forcing` assigns, benchmarks/SVATOXYGEN18_benchmark.py:384-437); parameters
 * `maskCatch` (n, int32), `sas_params_<flux>` (n, 8); per-cell results `C_<flux> C_iso_<flux>`,
 * `C_inf_* C_iso_inf_*`, `C_rz C_ss C_s C_iso_rz C_iso_ss C_iso_s`, the age statistics
 * `tt{10,25,50,75,90,avg}_{transp,q_ss}`, `rt{..}_{rz,ss,s}`; diagnostics `tt_<flux> mtt_<flux>`
 * (n, ages), `TT_<flux>` (n, ages + 1), `sa_s msa_s` (n, ages). */
int rh_sas_num_arrays(void);
const char *rh_sas_array_name(int array);
int rh_sas_array_index(const char *name);                  /* -1 if unknown */
int64_t rh_sas_array_elems(const rh_sas_ctx *ctx, int array); /* elements held by this context (0: not allocated) */
int rh_sas_array_is_int(int array);
int rh_sas_upload(rh_sas_ctx *ctx, int array, const void *host, size_t bytes);
int rh_sas_download(rh_sas_ctx *ctx, int array, void *host, size_t bytes); /* synchronises */
/* The same for the rows [first_cell, first_cell + n_cells) of a per-cell array (not for the DAILY inputs):
 * lets a driver stream a state that is larger than it wants to stage on the host (32 GB at 10^6 columns
 * x 1000 ages). */
int rh_sas_upload_cells(rh_sas_ctx *ctx, int array, int64_t first_cell, int64_t n_cells, const void *host, size_t bytes);
int rh_sas_download_cells(rh_sas_ctx *ctx, int array, int64_t first_cell, int64_t n_cells, void *host, size_t bytes);
void *rh_sas_array_device_ptr(rh_sas_ctx *ctx, int array);
/* Row `day_row` of a DAILY input from n_cells float64 already on this device (device-to-device, asynchronous on the
 * context's stream; the caller orders it after the producer): the coupling point for the daily flux sums that the
 * SVAT context accumulates (rh_diag_device_ptr in roger_hip.h). */
int rh_sas_set_daily_from_device(rh_sas_ctx *ctx, int array, int64_t day_row, const double *dev_src);

/* ---- the step --------------------------------------------------------------------------------
 * Stages of one day, in the order of svat_transport_model_deterministic; `stages` is a bit mask so
 * that a driver (and the parity tests) can run the reference's kernels one at a time with the
 * state left in HBM in between.  rh_sas_step == rh_sas_stages(ctx, day, RH_SAS_ALL). */
enum {
    RH_SAS_INF_RZ = 1 << 0,   /* infiltration into the root zone (matrix, then preferential flow) */
    RH_SAS_EVAP = 1 << 1,     /* soil evaporation */
    RH_SAS_TRANSP = 1 << 2,   /* transpiration */
    RH_SAS_Q_RZ = 1 << 3,     /* root zone percolation -> subsoil */
    RH_SAS_INF_SS = 1 << 4,   /* preferential-flow infiltration into the subsoil */
    RH_SAS_Q_SS = 1 << 5,     /* subsoil percolation */
    RH_SAS_CPR = 1 << 6,      /* capillary rise subsoil -> root zone */
    RH_SAS_STORAGE = 1 << 7,  /* root zone / subsoil / soil concentrations (+ age statistics if enabled) */
    RH_SAS_AGEING = 1 << 8,   /* shift by one age class, merge the oldest */
    RH_SAS_ALL = (1 << 9) - 1,
    /* not part of a day: soil.rescale_SA after the transport warm-up (rescale_sa_msa_iso_soil_kernel,
     * core/soil.py:1250-1395): sa_rz, sa_ss scaled to S_rz_init, S_ss_init; storage concentrations recomputed */
    RH_SAS_RESCALE = 1 << 9
};
/* `day` selects the row of the daily inputs: row (day mod forcing_days). */
int rh_sas_stages(rh_sas_ctx *ctx, int64_t day, int stages);
int rh_sas_step(rh_sas_ctx *ctx, int64_t day);
/* `ndays` whole steps for days day0, day0 + 1, ... enqueued back to back. */
int rh_sas_run_days(rh_sas_ctx *ctx, int64_t day0, int64_t ndays);

/* ---- time series at observation columns ("points"), recorded on the device after every day -----------
 * A comparison with a lysimeter -- delta-18O or bromide in its percolate, the concentration in the root zone, the travel time
 * distribution of q_ss -- needs a handful of columns every day, and inside rh_sas_run_days the host cannot look at a column between
 * two days.  After rh_sas_points_configure, rh_sas_step and every day of rh_sas_run_days are followed by ONE launch (k_sas_points,
 * roger_amd/csrc/rh_sas_points.h) that gathers arrays x cells into the next row of a ring on the device.  A pure gather: every value
 * is the bits rh_sas_download returns after that day -- for the prognostic state sa_rz, msa_rz, sa_ss, msa_ss that is the value AFTER
 * the day's ageing.  rh_sas_stages does not record, whatever its mask (a partial one, RH_SAS_ALL, RH_SAS_RESCALE): a driver that
 * steps by stage, or wants the initial values as a row, calls rh_sas_points_record.  A context without points enqueues exactly what
 * it enqueued before these entry points existed.
 *   cells    [n_cells]  local cell indices as in rh_sas_upload_cells, no cell twice; at most RH_SAS_POINTS_MAX_CELLS
 *   arrays   [n_arrays] registry indices (rh_sas_array_index), none twice; at most RH_SAS_POINTS_MAX_ARRAYS.  Per-cell float64
 *                       arrays this context holds: the state, C_*, C_iso_*, M_*, the age statistics, the per-cell parameters
 *                       (S_rz_init, alpha_q, ...) with width 1; tt_*, mtt_*, sa_s, msa_s and the state with width `ages`; TT_* with
 *                       width `ages + 1`
 *   capacity >= 1       rows resident on the device, row r at r mod capacity
 * Row layout (rh_sas_points_row_elems float64): arrays in configured order, within an array the cells in configured order, within a
 * cell the age axis contiguous -- the block of array j is (n_cells, width_j).  Per row one int64 tag, kept on the host: the `day`
 * argument of the step, or the caller's value for rh_sas_points_record.
 * n_cells == 0 or n_arrays == 0 releases the ring and stops the launches.  Every other call starts a new series (row 0).
 * RH_ERR_ARG (rh_sas_last_error names the offender): a cell outside [0, n_cells) or given twice, an unknown array id or an array given
 * twice, an int32 array (maskCatch, lu_id), a daily input or sas_params_* (inputs of the step, not per-cell results), counts above
 * the limits, capacity < 1, a ring above 2 GiB (capacity x row_elems x 8).  RH_ERR_STATE: an array this context does not hold
 * (age_statistics / keep_distributions off, M_* of an isotope context).  A refused call leaves the previous configuration in place.
 *   rh_sas_points_record     one row now, behind what the stream holds, with the caller's tag
 *   rh_sas_points_count      rows recorded since rh_sas_points_configure (the host enqueues every row: no synchronisation)
 *   rh_sas_points_row_elems  float64 per row
 *   rh_sas_points_read       rows [first_row, first_row + n_rows) that are still resident (first_row >= rows_total - capacity): tags
 *                            (n_rows) int64, values (n_rows, row_elems) float64; synchronises.  RH_ERR_ARG for rows that have been
 *                            overwritten (the message says which) or not recorded yet -- never other data.  A range across the
 *                            ring's wrap is two copies.
 * All four: RH_ERR_STATE before rh_sas_points_configure (or after it released the ring). */
#define RH_SAS_POINTS_MAX_CELLS 256
#define RH_SAS_POINTS_MAX_ARRAYS 32
int rh_sas_points_configure(rh_sas_ctx *ctx, const int64_t *cells, int n_cells, const int *arrays, int n_arrays, int64_t capacity);
int rh_sas_points_record(rh_sas_ctx *ctx, int64_t tag);
int rh_sas_points_count(rh_sas_ctx *ctx, int64_t *rows_total);
int rh_sas_points_row_elems(const rh_sas_ctx *ctx, int64_t *elems);
int rh_sas_points_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes);

/* ---- catchment totals, recorded on the device after every day -------------------------------------------------------------------
 * A comparison at the catchment outlet needs the flux-weighted concentration of the percolate, sum(q_ss C_q_ss) / sum(q_ss), the
 * catchment's backward travel time distribution, sum(q_ss tt_q_ss(T)) / sum(q_ss) per age class, and its storage by age, sum(sa_s(T)).
 * After rh_sas_totals_configure, rh_sas_step and every day of rh_sas_run_days are followed by the totals' launches on the context's
 * stream (behind the points' launch if both are on; kernels: roger_amd/csrc/rh_sas_totals.h) that reduce the configured items over
 * the masked cells into the next row of a ring on the device.  rh_sas_stages never records; a context without totals enqueues exactly
 * what it enqueued before these entry points existed.  Stands where the reference has its `tracer_monitor` diagnostic.
 *   mask     [n_cells] bytes, non-zero = inside; NULL: every cell.  A mask with no cell inside is RH_ERR_ARG.
 *   items    [n_items], at most RH_SAS_TOTALS_MAX_ITEMS, each (array, weight):
 *            array   what rh_sas_points_configure accepts -- per-cell float64 arrays this context holds, of width 1, ages or ages + 1 --
 *                    and the nine DAILY inputs, which have width 1: the value is row (day mod forcing_days)
 *            weight  -1 (none) or one of the eight DAILY flux inputs (not C_in): row (day mod forcing_days), the row the day's kernel read
 *   capacity >= 1    rows resident on the device, row r at r mod capacity; capacity x row_elems x 8 at most 2 GiB
 * n_items == 0 releases everything and stops the launches.  Every other call starts a new series (row 0).  RH_ERR_ARG (rh_sas_last_error
 * names the offender): an unknown id, an int32 array, sas_params_*, an array given twice with the same weight, a weight that is not a
 * daily flux input, counts above the limit, capacity < 1, a ring above 2 GiB.  RH_ERR_STATE: an array this context does not hold.  A
 * refused call leaves the previous configuration in place.
 *
 * Which cells count.  Cell c is ELIGIBLE for item j if it is inside the mask and either j has no weight or w[c] > 0 (a NaN or zero
 * weight is not eligible).  With day < 0 (rh_sas_totals_record: "no daily row") an item that has a weight or a DAILY value has no
 * eligible cell.  A term is t = v (no weight) or t = fl(v w): the product is rounded before it is added, never fused.
 *   width 1      a cell is COUNTED if it is eligible and v is not NaN.  Row block [wsum, count, sum, min, max]: wsum = sum of w over the
 *                counted cells (without a weight: = count), count as a double, sum = sum of t, min / max of v itself.  Nothing counted:
 *                [+0.0, 0, +0.0, +inf, -inf].
 *   width W > 1  row block [wsum, count, sum[0 ... W)]: wsum and count over the ELIGIBLE cells; per age class a NaN element contributes
 *                +0.0 (the reference's nansum convention for msa_*, mtt_*).
 * Infinities propagate.  Row layout (rh_sas_totals_row_elems float64): the items' blocks in configured order.  Per row one int64 tag,
 * kept on the host: the `day` argument of the step, or the caller's value for rh_sas_totals_record.
 *
 * The ORDER of the sums is fixed, so that a host restatement (tests/sas_totals_reference.py) gives the same bits.  The result follows
 * the cells of a rank's block: totals of different decompositions differ in the last bits.  No floating-point atomics.
 *   width 1 (sum, wsum, count, min, max; also wsum and count of an age item): the order of rh_totals_* (roger_hip.h).  Cells padded to a
 *       multiple of 256 with the identity (+0.0, +inf, -inf; also where a cell is not counted); per 64 cells the tree with strides
 *       32 ... 1, x[l] = x[l] op x[l + stride]; per 256 cells (w0 + w1) + (w2 + w3); the tiles' partials p: accumulator t of 256 starts
 *       from the identity and takes p[t], p[t + 256], ... in this order; the 256 accumulators go through the same two levels.
 *   width W > 1, per age class: cut the sequence of cells into runs of 256 consecutive cells; sum each run left to right, starting
 *       from +0.0, a skipped cell contributing +0.0; repeat on the sequence of partials (plain sums) until one value is left.  Lanes run
 *       along the age axis, which is contiguous: every global load is unit stride and no butterfly crosses cells.
 * Scratch on the device, sized at configure: items x 5 x ceil(n_cells / 256) float64 for the width-1 partials; for the age rule two
 * buffers of ceil(n_cells / 256) x Wmax and ceil(n_cells / 65536) x Wmax float64, shared by the age items, which are reduced one after
 * another (10^6 cells x 1000 ages: 31 MB + 0.13 MB).
 *   rh_sas_totals_record     one row now, behind what the stream holds, with the caller's tag; day < 0: no daily row
 *   rh_sas_totals_count      rows recorded since rh_sas_totals_configure (no synchronisation) and the cells inside the mask
 *   rh_sas_totals_row_elems  float64 per row
 *   rh_sas_totals_read       as rh_sas_points_read: the resident rows [first_row, first_row + n_rows), RH_ERR_ARG for rows that have been
 *                            overwritten or not recorded yet; synchronises
 * All four: RH_ERR_STATE before rh_sas_totals_configure (or after it released everything). */
#define RH_SAS_TOTALS_MAX_ITEMS 32
typedef struct rh_sas_totals_item {
    int32_t array;
    int32_t weight; /* -1 = none */
} rh_sas_totals_item;
int rh_sas_totals_configure(rh_sas_ctx *ctx, const unsigned char *mask, const rh_sas_totals_item *items, int n_items, int64_t capacity);
int rh_sas_totals_record(rh_sas_ctx *ctx, int64_t tag, int64_t day);
int rh_sas_totals_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells);
int rh_sas_totals_row_elems(const rh_sas_ctx *ctx, int64_t *elems);
int rh_sas_totals_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes);

/* ---- zonal totals: the catchment totals for EVERY zone of a zone map, in one pass ------------------------------------------------------
 * Sub-catchments (one gauge and one isotope series each), land uses, soil classes: after rh_sas_zonal_configure, rh_sas_step and every
 * day of rh_sas_run_days are followed by the zonal launches on the context's stream (behind the points' and the totals' launches where
 * those are on; kernels: roger_amd/csrc/rh_sas_zonal.h) that reduce the configured items over the cells of every zone into the next row
 * of a ring on the device, loading each row of an age-resolved array once whatever the number of zones.  rh_sas_stages never records; a
 * context without the recorder enqueues exactly what it enqueued before these entry points existed.  Points, totals and zonal totals
 * work side by side, configured in any order.
 *   zone     [n_cells] int32: -1 = outside every zone, else 0 ... n_zones - 1; 1 <= n_zones <= RH_SAS_ZONAL_MAX_ZONES
 *   items, capacity   as rh_sas_totals_configure; capacity x row_elems x 8 at most 2 GiB
 * n_items == 0 releases everything and stops the launches.  Every other call starts a new series (row 0).  The refusals of
 * rh_sas_totals_configure, and RH_ERR_ARG for n_zones outside its range, a zone id outside -1 ... n_zones - 1, a map with no cell in any
 * zone, a level-1 buffer (below) above 2 GiB -- the message names the slot count.  A refused call leaves the previous configuration in
 * place.
 *
 * Row layout (rh_sas_zonal_row_elems float64): zone-major; a zone's part holds the items' blocks as a row of rh_sas_totals_* does.  Block
 * (z, j) is, bit for bit, the block that rh_sas_totals_* records for item j with mask = (zone == z): the counting rules, the NaN rules,
 * fl(v w) rounded before it is added, day < 0, and [+0.0, 0, +0.0, +inf, -inf] (sums +0.0) for a zone without a counted cell are the ones
 * stated above.  Per row one int64 tag, kept on the host.
 *
 * The ORDER.  A (tile of 256 cells, zone) pair that exists is a SLOT; the pairs that do not exist are left out, which changes no bit.
 *   width 1: each slot gets the wavefront trees and (w0 op w1) op (w2 op w3) over its tile, the cells of other zones holding the identity;
 *       a zone has 256 accumulators, accumulator t takes the slots of the tiles with tile mod 256 == t in increasing tile order; the 256
 *       accumulators go through the same two levels.  The dense rule would also take the partials of the pairs that do not exist: trees of
 *       identities, and x op identity == x in every bit for an accumulator that starts at the identity (a sum that starts at +0.0 is never
 *       -0.0, a minimum or maximum that starts at an infinity is never NaN).
 *   width W > 1, per age class: a run of the age rule is a tile, so the slots are the same.  Level 1: the cells of z in the run, left to
 *       right from +0.0.  The dense rule then sums 256 consecutive partials left to right, then 256 of those, ...; a run or a group of
 *       runs without a cell of z has the partial +0.0, and adding +0.0 to a running sum that started at +0.0 (never -0.0), or passing a
 *       value through an extra level +0.0 + x, changes no bit.  So the zone's slots are walked once in increasing run order with nested
 *       accumulators: a2 takes the slot partials, is added into a3 and cleared where run / 256 changes, a3 into a4 where run / 65536
 *       changes; both are flushed at the end.
 * Scratch on the device, sized at configure (S slots): S x items x 5 float64 for the width-1 partials; ONE level-1 buffer of S x Wmax
 * float64, shared by the age items, which are reduced one after another; the index over the map (about 2 n_cells + 5 S + 257 n_zones
 * int32).  No floating-point atomics, no counter on the device.
 *   rh_sas_zonal_record     one row now, behind what the stream holds, with the caller's tag; day < 0: no daily row
 *   rh_sas_zonal_count      rows recorded since rh_sas_zonal_configure (no synchronisation) and the cells of every zone, ncells[n_zones]
 *   rh_sas_zonal_row_elems  float64 per row
 *   rh_sas_zonal_read       as rh_sas_totals_read
 * All four: RH_ERR_STATE before rh_sas_zonal_configure (or after it released everything). */
#define RH_SAS_ZONAL_MAX_ZONES 1024
int rh_sas_zonal_configure(rh_sas_ctx *ctx, const int32_t *zone, int n_zones, const rh_sas_totals_item *items, int n_items, int64_t capacity);
int rh_sas_zonal_record(rh_sas_ctx *ctx, int64_t tag, int64_t day);
int rh_sas_zonal_count(rh_sas_ctx *ctx, int64_t *rows_total, int64_t *ncells);
int rh_sas_zonal_row_elems(const rh_sas_ctx *ctx, int64_t *elems);
int rh_sas_zonal_read(rh_sas_ctx *ctx, int64_t first_row, int64_t n_rows, int64_t *tags, double *values, size_t value_bytes);

/* ---- scores against observed tracer samples: per-column moments that stay on the device ---------------------------------------------
 * A SAS parameter study draws its parameters by the thousand -- every column one draw of the same plot -- and judges each draw against
 * delta-18O, delta-2H, bromide or chloride measured in a lysimeter's percolate.  Such samples are BULK samples over irregular windows (a
 * weekly or fortnightly bottle, a gap of a month): what is compared with sample k is the flux-weighted mean over its window,
 * sum(q C) / sum(q).  After rh_sas_scores_configure, rh_sas_step and every day of rh_sas_run_days that lies inside a window are followed
 * by ONE launch (k_sas_scores, roger_amd/csrc/rh_sas_scores.h; behind the points', the totals' and the zonal launches where those are on);
 * a day outside every window launches nothing, rh_sas_stages never scores, and a context without scores enqueues exactly what it enqueued
 * before these entry points existed.  Points, totals, zonal totals and scores work side by side, configured in any order.
 *   items    [n_items], at most RH_SAS_SCORES_MAX_ITEMS, each (value, weight, kind):
 *            value   a per-cell float64 array of width 1 this context holds: C_*, C_iso_*, M_*, the age statistics, the per-cell parameters
 *            weight  -1 (none) or one of the eight DAILY flux inputs (not C_in): row (day mod forcing_days), the row the day's kernel read
 *            kind    RH_SAS_SCORES_BULK (needs a weight), _MEAN or _LAST (take none)
 *   series   [n_cells] int32, the series of every cell, < 0: not scored; NULL: every cell series 0.  1 <= n_series <= RH_SAS_SCORES_MAX_SERIES
 *   obs      [n_items][n_series][n_samples] float64, NaN: missing
 *   first_day, last_day  [n_samples] int64: window k is the days [first_day[k], last_day[k]], inclusive, of the context's DAY COUNT
 * The day count.  The context counts scored days from 0 at configure: day t is the t-th day stepped (rh_sas_step, a day of
 * rh_sas_run_days) or recorded by hand (rh_sas_scores_record) since configure.  The `day` argument of those calls is the row of the daily
 * inputs and nothing else -- a host that keeps one row steps with day 0 throughout.  Windows are strictly increasing and do not overlap:
 * first_day[k] <= last_day[k] < first_day[k + 1].  Window k is OPEN from the day its first day was scored until its last;
 * closed[k] = 1 exactly when the closing day of an open window was scored.  A window whose first day was never scored -- first_day[k] < 0:
 * the series was configured mid-window -- is never open and never compared.
 *
 * The rule (each +, -, *, / one IEEE operation in the order written; the library is built with -ffp-contract=off).  Cell i has
 * s = series[i] (no map: s = 0); s < 0 loads and stores nothing.  Per item, v the value after the day:
 *   BULK: wd = weight[row][i];  MEAN: wd = 1.0.  On the window's first day num and den restart from +0.0.  The day is ELIGIBLE if wd > 0 and
 *         v == v (a NaN weight is not > 0): num = num + fl(v * wd), den = den + wd.  A day that is not eligible leaves both as they are.
 *   LAST: nothing before the closing day.
 *   On the closing day of an open window, o = obs[(j * n_series + s) * n_samples + k]:
 *         BULK / MEAN: the sample is COUNTED if o == o and den > 0; sim = num / den.   LAST: COUNTED if o == o and v == v; sim = v.
 *         A counted sample: n += 1.0; m1 += sim; m2 += sim * sim; m3 += sim * o; d = sim - o; m4 += d * d; so += o; soo += o * o.
 * The simulated concentration is NaN on a day without flux, so a window may hold water for one column and none for its neighbour: the
 * count n and the observation moments so, soo are per-column planes.  Nothing assumes positive sums (delta values are negative).
 * moments [n_items][9][n_cells] float64 = {num, den, n, m1, m2, m3, m4, so, soo}, cleared to +0.0 at configure.  No atomics.
 *
 * n_items == 0 releases everything and stops the launches.  Every other call clears the moments and restarts the day count.  RH_ERR_ARG
 * (rh_sas_last_error names the offender): an unknown id, an int32 array, a DAILY input, sas_params_* or an age-resolved array as value; a
 * weight that is not a daily flux input (or is C_in); BULK without a weight, MEAN / LAST with one; an unknown kind; the same (value,
 * weight, kind) twice; more than 16 items, n_series outside 1 ... 1024; a series id >= n_series; no cell scored; n_samples < 1; windows out
 * of order or overlapping; null pointers.  RH_ERR_STATE: an array this context does not hold.  A refused call leaves the previous
 * configuration in place.
 *   rh_sas_scores_record   scores "now", behind what the stream holds, as the next day of the count, with `day` (>= 0) the daily row:
 *                          for a driver that steps with rh_sas_stages
 *   rh_sas_scores_read     moments (n_items x 9 x n_cells float64), closed (n_samples bytes), days_scored (may be NULL); synchronises
 * Both: RH_ERR_STATE before rh_sas_scores_configure (or after it released everything). */
#define RH_SAS_SCORES_MAX_ITEMS 16
#define RH_SAS_SCORES_MAX_SERIES 1024
#define RH_SAS_SCORES_BULK 0
#define RH_SAS_SCORES_MEAN 1
#define RH_SAS_SCORES_LAST 2
typedef struct rh_sas_scores_item {
    int32_t value;
    int32_t weight; /* -1 = none */
    int32_t kind;
} rh_sas_scores_item;
int rh_sas_scores_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const int32_t *series, int n_series,
                            const double *obs, const int64_t *first_day, const int64_t *last_day, int64_t n_samples);
int rh_sas_scores_record(rh_sas_ctx *ctx, int64_t day);
int rh_sas_scores_read(rh_sas_ctx *ctx, double *moments, size_t moment_bytes, unsigned char *closed, size_t closed_bytes,
                       int64_t *days_scored);

/* ---- transport bands: exact quantiles ACROSS the columns per sample window, and where the observation falls ---------------------------
 * The one figure a GLUE study of the SAS parameters is made for: the 5 - 95 % band of the simulated delta-18O around the bottle samples,
 * and the share of samples the band contains.  After rh_sas_bands_configure, rh_sas_step and every day of rh_sas_run_days enqueue the
 * day's band work behind the scores' launch (kernels, the rule in full and the bytes moved: roger_amd/csrc/rh_sas_bands.h; the numpy twin
 * is tests/sas_bands_reference.py).  rh_sas_stages never records; a context without bands enqueues exactly what it enqueued before these
 * entry points existed.  Points, totals, zonal totals, scores and bands work side by side, configured in any order.
 *   items    [n_items], at most RH_SAS_BANDS_MAX_ITEMS, each (value, weight, kind) as rh_sas_scores_configure takes them
 *   probs    [n_probs] float64, 1 ... RH_SAS_BANDS_MAX_PROBS probabilities within [0, 1], shared by the items
 *   mask     [n_cells] bytes, 0: the cell takes no part; NULL: every cell
 *   weights  [n_cells] uint16 likelihood weights w_i, 0: the cell takes no part; NULL: w_i = 1
 *   obs      [n_items][n_samples] float64, NaN: missing; NULL: no observations, nothing is counted
 *   first_day, last_day  [n_samples] int64: the windows in the context's count of RECORDED days, which starts at 0 at configure -- the
 *            window rules and the clock of rh_sas_scores_configure: a day outside every window launches nothing, a window whose first day
 *            was never recorded is never open
 * The rule.  Per cell that takes part and item, num and den are accumulated over the window's days exactly as k_sas_scores accumulates them
 * (restart from +0.0 on the first day; eligible iff wd > 0 && v == v; num = num + fl(v * wd), den = den + wd).  On the closing day the window
 * value is s = den > 0 ? num / den : NaN (BULK / MEAN) or s = v (LAST), then s = s + 0.0.  m = cells with a number, n_nan = cells with a NaN,
 * W = sum of w_i over the m cells.  For a probability p, T = clamp((int64)ceil(p * (double)W), 1, W) and the result is the smallest s with
 * sum_{s_i <= s} w_i >= T: the bits of np.sort(np.repeat(s, w))[T - 1]; with m == 0 NaN and W = 0.  With observations the int64 pair (below,
 * equal) holds the weights of the members below and equal to o + 0.0; a missing o gives (-1, -1), m == 0 gives (0, 0).
 * Result, no ring (the caller knows n_samples): rows [n_samples][n_items][n_probs] float64, NaN until the window closed; hdr
 * [n_samples][n_items]{m, n_nan, W} int64, 0 until then; obs_pair [n_samples][n_items][2] int64, (-1, -1) until then and without
 * observations; closed [n_samples] bytes, 1 exactly when the closing day of an open window was recorded.
 *
 * n_items == 0 releases everything and stops the launches.  Every other call starts anew (day count 0).  Everything is checked before
 * anything is released or allocated; a refused call leaves the previous configuration in place.  RH_ERR_ARG (rh_sas_last_error names the
 * offender): null pointers; n_items or n_probs beyond the maxima; a probability outside [0, 1] or NaN; the refusals of
 * rh_sas_scores_configure for an item (unknown id, int32, DAILY input, sas_params_*, age-resolved value; a weight that is not a daily flux
 * input; BULK without a weight, MEAN / LAST with one; unknown kind; given twice); n_samples < 1; windows out of order or overlapping; a mask
 * and weights that leave no cell taking part.  RH_ERR_STATE: an array this context does not hold.
 *   rh_sas_bands_record   records "now", behind what the stream holds, as the next day of the count, with `day` (>= 0) the daily row: for
 *                         a driver that steps with rh_sas_stages
 *   rh_sas_bands_read     rows, hdr, obs_pair, closed with their sizes in bytes, days_recorded (may be NULL); synchronises
 * Both: RH_ERR_STATE before rh_sas_bands_configure (or after it released everything). */
#define RH_SAS_BANDS_MAX_ITEMS 8
#define RH_SAS_BANDS_MAX_PROBS 8
int rh_sas_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                           const unsigned char *mask, const uint16_t *weights, const double *obs, const int64_t *first_day,
                           const int64_t *last_day, int64_t n_samples);
int rh_sas_bands_record(rh_sas_ctx *ctx, int64_t day);
int rh_sas_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair, size_t pair_bytes,
                      unsigned char *closed, size_t closed_bytes, int64_t *days_recorded);

/* ---- transport bands per zone: the bands above for every zone of a zone map in one run, each zone with its own observations ---------------
 * The lysimeters of a SAS parameter study, the land uses or sub-catchments of a catchment map (kernels, the rule and the bytes moved:
 * roger_amd/csrc/rh_sas_bands_zonal.h; the numpy twin is tests/sas_bands_zonal_reference.py).
 * The promise, which is the whole specification: block (item, zone z) of window k is bit for bit what rh_sas_bands_configure records for that
 * item with mask = (zone == z) & mask, the same weights, probabilities and windows and obs = obs[item][z].  A zone with m == 0 gives NaN rows,
 * W = 0 and, with an observation that is not missing, the pair (0, 0); a missing observation gives (-1, -1).  A cell with zone == -1,
 * mask == 0 or weight 0 takes no part and is in no zone's counts.
 *   zone     [n_cells] int32: -1 outside every zone, else 0 ... n_zones - 1
 *   n_zones  1 ... RH_SAS_BANDS_MAX_ZONES
 *   obs      [n_items][n_zones][n_samples] float64, NaN: missing; NULL: no observations
 *   everything else as rh_sas_bands_configure takes it
 * Result: rows [n_samples][n_items][n_zones][n_probs] float64, hdr [n_samples][n_items][n_zones]{m, n_nan, W} int64, obs_pair
 * [n_samples][n_items][n_zones][2] int64, closed [n_samples] bytes, read with rh_sas_bands_zonal_read (which synchronises).
 * rh_sas_bands_record, rh_sas_step and rh_sas_run_days serve both configurations; a closing day is 2 launches (3 with an observation)
 * instead of 13 (15).  rh_sas_bands_configure_zonal replaces a plain configuration and rh_sas_bands_configure replaces it; n_items == 0
 * releases.  rh_sas_bands_read is RH_ERR_STATE while the bands are per zone, rh_sas_bands_zonal_read is RH_ERR_STATE while they are not.
 * Everything is checked before anything is released or allocated.  RH_ERR_ARG beyond the refusals of rh_sas_bands_configure: n_zones outside
 * 1 ... RH_SAS_BANDS_MAX_ZONES; a zone index outside -1 ... n_zones - 1 (the message names the cell); rows of n_items x n_zones x n_probs
 * float64 x n_samples beyond 2 GiB; and THE BOUND: one workgroup selects a zone in uint32 LDS bins, which hold at most (participating cells
 * of the zone) x 65535, so with a weight plane a zone of more than 65536 participating cells is refused (the message names the zone): such
 * a zone belongs to the mask of rh_sas_bands_configure.  Without weights any zone size is exact.
 * Load balance: one workgroup walks a zone, so the largest zone sets the time of a closing day. */
#define RH_SAS_BANDS_MAX_ZONES 1024
int rh_sas_bands_configure_zonal(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                                 const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights, const double *obs,
                                 const int64_t *first_day, const int64_t *last_day, int64_t n_samples);
int rh_sas_bands_zonal_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, int64_t *obs_pair,
                            size_t pair_bytes, unsigned char *closed, size_t closed_bytes, int64_t *days_recorded);

/* ---- transport bands by age: the bands above for every age class of an age-resolved array ---------------------------------------------------
 * The other figure a SAS parameter study is made for: the travel time distribution of the percolate, TT_q_ss(T) or tt_q_ss(T), or the storage
 * by age sa_s(T), with its 5 - 50 - 95 % band over the behavioural parameter sets -- without downloading the (n_cells, ages) array (kernels,
 * the rule and the bytes moved: roger_amd/csrc/rh_sas_age_bands.h; the numpy twin is tests/sas_age_bands_reference.py).
 * The promise, which is the whole specification: block (item j, age class a) of window k is bit for bit what rh_sas_bands_configure would
 * record for the width-1 values A_j[:, a] with kind LAST under the same mask, weights, probabilities and windows: s = v + 0.0; a NaN element
 * is counted in that age class's n_nan and takes no further part; +-inf are values; a cell with mask == 0 or weight 0 takes no part;
 * T = clamp((int64)ceil(p * (double)W), 1, W) and the result is the smallest s with sum_{s_i <= s} w_i >= T; m == 0 gives NaN rows and W = 0.
 * m, n_nan and W are per age class.
 *   items    [n_items], at most RH_SAS_AGE_BANDS_MAX_ITEMS, each (value, weight, kind): value a per-cell float64 array of width ages or
 *            ages + 1 this context holds (always: sa_rz, sa_ss, msa_*; with keep_distributions: tt_*, mtt_*, TT_*, sa_s, msa_s); weight -1
 *            and kind RH_SAS_SCORES_LAST.  These calls record the band of a SNAPSHOT and stay LAST-only: BULK and MEAN are refused with a
 *            message that says so; the window means of the same arrays are an observer of their own, rh_sas_age_window_bands_* below
 *   probs, mask, weights, first_day, last_day, n_samples   as rh_sas_bands_configure takes them; the count of recorded days is this
 *            recorder's own and starts at 0 at configure
 * After rh_sas_age_bands_configure, rh_sas_step and every day of rh_sas_run_days that closes an open window enqueue, behind the bands'
 * launches, two launches per item (a transpose of the participating columns into a key plane, the selection of every age class by a
 * workgroup of its own); every other day enqueues nothing.  rh_sas_stages never records; a context without bands by age enqueues exactly
 * what it enqueued before these entry points existed.  Points, totals, zonal totals, scores, either kind of bands and the bands by age
 * work side by side, configured in any order.
 * Result, no ring: rows [n_samples][sum_j W_j][n_probs] float64, item j's block (W_j, n_probs) in configured order, NaN until the window
 * closed; hdr [n_samples][sum_j W_j]{m, n_nan, W} int64, 0 until then; closed [n_samples] bytes.
 * n_items == 0 releases everything and stops the launches.  Every other call starts anew (day count 0).  Everything is checked, and the new
 * buffers are allocated, before the previous configuration is released: a refused call or a failed allocation leaves the previous
 * configuration in place.  RH_ERR_ARG (rh_sas_last_error names the offender): null pointers; n_items or n_probs beyond the maxima; a
 * probability outside [0, 1] or NaN; an unknown id; an int32 array, a DAILY input or sas_params_*; a width-1 array (it belongs to
 * rh_sas_bands_configure); a weight, or a kind other than LAST; an item given twice; n_samples < 1; windows out of order or overlapping; a
 * mask and weights that leave no cell taking part; rows of sum_j W_j x n_probs float64 x n_samples, or hdr of sum_j W_j x 3 int64 x
 * n_samples (the larger buffer below three probabilities), beyond 2 GiB; and THE BOUND: one
 * workgroup selects an age class in uint32 LDS bins, which hold at most (participating cells) x 65535, so with a weight plane more than
 * 65536 participating cells are refused.  Without weights any n_cells < 2^31 is exact.  RH_ERR_STATE: an array this context does not hold.
 * Device memory: one key plane of max_j W_j x (participating cells) x 8 bytes, shared by the items.
 *   rh_sas_age_bands_record     records "now", behind what the stream holds, as the next day of the count; `day` (>= 0) is the daily row
 *                               (unused while every item is LAST): for a driver that steps with rh_sas_stages
 *   rh_sas_age_bands_row_elems  sum_j W_j
 *   rh_sas_age_bands_read       rows, hdr, closed with their sizes in bytes, days_recorded (may be NULL); synchronises
 * All three: RH_ERR_STATE before rh_sas_age_bands_configure (or after it released everything). */
#define RH_SAS_AGE_BANDS_MAX_ITEMS 4
int rh_sas_age_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                               const unsigned char *mask, const uint16_t *weights, const int64_t *first_day, const int64_t *last_day,
                               int64_t n_samples);
int rh_sas_age_bands_record(rh_sas_ctx *ctx, int64_t day);
int rh_sas_age_bands_row_elems(const rh_sas_ctx *ctx, int64_t *ages_total);
int rh_sas_age_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed,
                          size_t closed_bytes, int64_t *days_recorded);

/* ---- transport bands by age per zone: the bands by age above for every zone of a zone map in one run -----------------------------------------
 * Every lysimeter's, land use's or sub-catchment's travel time band from ONE transport run (kernels, the rule and the bytes moved:
 * roger_amd/csrc/rh_sas_age_bands.h; the numpy twin is tests/sas_age_bands_zonal_reference.py).
 * The promise, which is the whole specification: block (item j, zone z, age class a) of window k is bit for bit what
 * rh_sas_age_bands_configure records for item j and age class a with mask = (zone == z) & mask and the same weights, probabilities and
 * windows.  A cell with zone == -1, mask == 0 or weight 0 loads and stores nothing and is in no zone's counts; a zone with m == 0 in an age
 * class gives NaN rows and W = 0 there.  Only kind RH_SAS_SCORES_LAST with weight -1 is accepted, as above.
 *   zone     [n_cells] int32: -1 outside every zone, else 0 ... n_zones - 1
 *   n_zones  1 ... RH_SAS_AGE_BANDS_MAX_ZONES
 *   everything else as rh_sas_age_bands_configure takes it
 * Result: rows [n_samples][sum_j W_j x n_zones][n_probs] float64, item j's block (n_zones, W_j, n_probs) in configured order -- the zone axis
 * stands before the age axis, so a zone's distribution is contiguous --, hdr likewise with {m, n_nan, W} int64, closed [n_samples] bytes,
 * read with rh_sas_age_bands_zonal_read (which synchronises).
 * rh_sas_age_bands_record, rh_sas_age_bands_row_elems (sum_j W_j, without the zone axis), rh_sas_step and rh_sas_run_days serve both
 * configurations; a closing day is at most three launches per item: the transpose, the selection of the zones of more than 256
 * participating cells (six digit passes by a workgroup per zone and age class) and the selection of the zones of 1 ... 256 (one key per
 * thread, no histogram).  Each configure call replaces the other; n_items == 0 releases.  rh_sas_age_bands_read is RH_ERR_STATE while the
 * bands by age are per zone, rh_sas_age_bands_zonal_read is RH_ERR_STATE while they are not.  Everything is checked, and the new buffers are
 * allocated, before the running configuration is released: a refused call leaves it in place.
 * RH_ERR_ARG beyond the refusals of rh_sas_age_bands_configure: n_zones outside 1 ... RH_SAS_AGE_BANDS_MAX_ZONES; a zone index outside
 * -1 ... n_zones - 1 (the message names the cell); rows or headers of n_samples x sum_j W_j x n_zones blocks beyond 2 GiB; and THE BOUND,
 * which is PER ZONE here: one workgroup selects a (zone, age class) in uint32 LDS bins, so with a weight plane a ZONE of more than 65536
 * participating cells is refused (the message names the zone and its size).  A weighted study of more than 65536 participating cells in
 * total is accepted when every zone is within the bound -- the one place where this call accepts more than rh_sas_age_bands_configure,
 * which refuses that total.  Without weights any zone size is exact.
 * Load balance: one workgroup walks a (zone, age class), so the largest zone sets the time of a closing day. */
#define RH_SAS_AGE_BANDS_MAX_ZONES 1024
int rh_sas_age_bands_configure_zonal(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                                     const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights,
                                     const int64_t *first_day, const int64_t *last_day, int64_t n_samples);
int rh_sas_age_bands_zonal_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed,
                                size_t closed_bytes, int64_t *days_recorded);

/* ---- window means of the bands by age: the band of a BULK SAMPLE's age-resolved value, plain or per zone --------------------------------------
 * A bottle is a bulk sample over its window, and its travel time distribution is the flux-weighted mean sum_d q_ss(d) tt_q_ss(T, d) /
 * sum_d q_ss(d) over the window's days.  The bands by age above record the snapshot of the closing day; these record the band of that mean
 * (or of the plain mean over the days), for every age class, without downloading the (n_cells, ages) array on any day (kernels, the rule
 * and the bytes moved: roger_amd/csrc/rh_sas_age_bands.h; the numpy twin is tests/sas_age_window_bands_reference.py).
 * The promise, which is the whole specification: block (item j, [zone z,] age class a) of window k is bit for bit what rh_sas_bands_configure
 * records for the width-1 values A_j[:, a] with the same item weight and kind, under the same mask, weights, probabilities and windows; with
 * zones, mask = (zone == z) & mask.  So per participating cell, age class and recorded day of an open window: wd is the cell's value in row
 * `day` of the daily weight (BULK) or 1.0 (MEAN); the element is eligible iff wd > 0 && v == v; then num = num + fl(v * wd), den = den + wd;
 * both restart from +0.0 on the window's first day; on the closing day s = den > 0 ? num / den : NaN, then s + 0.0; a NaN s is counted in
 * that block's n_nan.  den is per ELEMENT: a NaN in one age class on one day does not touch its neighbours.
 *   items    [n_items], at most RH_SAS_AGE_BANDS_MAX_ITEMS, each (value, weight, kind): value as rh_sas_age_bands_configure takes it; kind
 *            RH_SAS_SCORES_BULK with a daily flux input as weight, or RH_SAS_SCORES_MEAN with weight -1.  LAST is refused: it belongs to
 *            rh_sas_age_bands_configure
 *   zone, n_zones   NULL and 0: the plain form; else as rh_sas_age_bands_configure_zonal takes them
 *   probs, mask, weights, first_day, last_day, n_samples   as rh_sas_age_bands_configure takes them; the count of recorded days is this
 *            observer's own and starts at 0 at configure
 * After the call, rh_sas_step and every day of rh_sas_run_days enqueue, behind the bands by age, on every day of an open window one launch
 * per item that updates the accumulators; on the closing day one launch per item that does the day's update in registers and writes the key
 * plane, and the selection launches of the bands by age.  A day outside every window enqueues nothing; rh_sas_stages never records; a context
 * without this observer enqueues exactly what it enqueued before these entry points existed.  Both observers by age may be configured at once:
 * each has its own key plane, participating set, clock and result.
 * Result, no ring: rows [n_samples][sum_j W_j][n_probs] and hdr [n_samples][sum_j W_j]{m, n_nan, W}, as rh_sas_age_bands_read returns them;
 * with zones rows [n_samples][sum_j W_j x n_zones][n_probs], item j's block (n_zones, W_j, n_probs), as rh_sas_age_bands_zonal_read returns
 * them.  ONE read serves both forms.
 * Device memory: the key plane of the bands by age, and 16 bytes per participating cell and age class of every item (num and den, float64),
 * zero at configure.  They are not part of a restart file.
 * n_items == 0 releases.  Everything is checked, and the new buffers are allocated, before the running configuration is released.  The
 * refusals are those of rh_sas_age_bands_configure and _zonal, word for word behind the function's name -- the array checks, an item given
 * twice, n_samples and the 2 GiB bound of the rows, the windows, no participating cell, the bound of a weight plane (per zone with zones),
 * zone indices and n_zones -- and for the item's weight those of rh_sas_bands_configure (not a daily flux input; BULK without a weight;
 * MEAN with one).
 *   rh_sas_age_window_bands_record     records "now" as the next day of the count, with `day` (>= 0) the row of the daily weights
 *   rh_sas_age_window_bands_row_elems  sum_j W_j
 *   rh_sas_age_window_bands_read       rows, hdr, closed with their sizes in bytes, days_recorded (may be NULL); synchronises
 * All three: RH_ERR_STATE before rh_sas_age_window_bands_configure (or after it released everything). */
int rh_sas_age_window_bands_configure(rh_sas_ctx *ctx, const rh_sas_scores_item *items, int n_items, const double *probs, int n_probs,
                                      const int32_t *zone, int n_zones, const unsigned char *mask, const uint16_t *weights,
                                      const int64_t *first_day, const int64_t *last_day, int64_t n_samples);
int rh_sas_age_window_bands_record(rh_sas_ctx *ctx, int64_t day);
int rh_sas_age_window_bands_row_elems(const rh_sas_ctx *ctx, int64_t *ages_total);
int rh_sas_age_window_bands_read(rh_sas_ctx *ctx, double *rows, size_t row_bytes, int64_t *hdr, size_t hdr_bytes, unsigned char *closed,
                                 size_t closed_bytes, int64_t *days_recorded);

/* HIP-event timing of the step kernel (same protocol as rh_enable_timing / rh_timing_summary). */
int rh_sas_enable_timing(rh_sas_ctx *ctx, int on);
int rh_sas_timing_summary(rh_sas_ctx *ctx, double *total_ms, int64_t *launches);

/* Diagnostic: the kernel's x**k routine (power-law SAS function, core/sas.py:228-231) on n host values,
 * 0 < x <= 1; lets the tests bound its error against the host's pow directly.  Uses the current device. */
int rh_sas_selftest_pow(const double *x, const double *k, double *out, int64_t n);
/* Diagnostic: the kernel's division by a loop-invariant divisor (hoisted refined reciprocal + one residual step),
 * out = a / d, to be compared bit for bit with the host's IEEE division. */
int rh_sas_selftest_div(const double *a, const double *d, double *out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* ROGER_HIP_SAS_H */
