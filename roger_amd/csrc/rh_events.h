// rh_events.h -- event outputs (rh_events_configure): per rainfall event and per column the sum, the peak intensity, the first and the
// last value of up to 16 planes, accumulated after every step on the device; the slot of the accumulators is the EVENT, not the day.
// Part of the one translation unit roger_hip.hip, behind rh_scores.h.
//
// The clock and the event id (uniform over the grid, from D->S as k_diag and k_scores read the clock): t1 = S.time, t0 = t1 - S.dt_secs,
// dt = S.dt (hours, a double: 1.0 / 6, 1 or 24), e = S.event_id[1].  D->S holds the FINISHED step's values whenever the observers run:
//   the one-launch front, the split pair       step_tail / pre_tail (rh_control.h) commit S_next to D->S inside the fused launch that runs the
//                                              step; k_ctrl stores D->S before it.  scalars_update (do_finish = 1) has advanced time and
//                                              copied event_id[1] into event_id[0]: [1] is the step's id.
//   the predicate-kernel front                 k_scalars (do_finish = 1) stores D->S in front of the fused launch, the same bookkeeping.
//   the routine-by-routine step                rh_adaptive_dt_finish: k_scalars (do_finish = 0) sets event_id[1] for the step, k_advance
//   (rh_step_core, rh_step_routed)             advances the time, the observers follow; k_rotate_scalars (rh_after_timestep) comes BEHIND
//                                              them and changes event_id[0] only.
//   the routed passes (routed_step_device)     k_ctrl stores D->S in front of the three passes; the observers sit between the numerics and
//                                              the rotation of the planes.
// So event_id[1] is the id on every front; event_id[0] is not (rotated on some, not yet on others) and is not read.
//   e == 0: the step belongs to no event -- the kernel returns after that one scalar load.
//
// Slots.  Event e uses slot e % n_slots.  Header per slot, int64 {event id, steps, t0 of its first step, t1 of its last step, steps of
// 600 s, steps of 3600 s}, every word -1 until a step touches the slot.  A step is the FIRST of its event in a slot when the slot's
// stored id differs from e.  The event that was running when the observer was configured (events_running: S.event_id[1] then) keeps
// t0 = -1 in its header: its sums start at the configuration, not at the event's start.
//
// Items.  Per item j, v the plane's value after the step, p the slot's element of column i:
//   SUM    p = first ? v : p + v                      (k_diag's rate rule, the same order of additions)
//   PEAK   r = v / dt, ONE IEEE division, mm/h;  p = first ? r : (take ? r : p)  with  take = r > p || (p != p && r == r)
//          -- a NaN r is never taken over a stored value (both comparisons are false); a NaN FIRST value is stored and stays until the
//          first step whose r is a number, which replaces it (the second term: r > NaN alone would keep the NaN to the event's end)
//   FIRST  p = v on the first step only; no load and no store on any other
//   LAST   p = v on every step
// events [slot][item][n] float64, cleared to +0.0; plain loads and stores, no atomics; the library is built with -ffp-contract=off.
//
// No overwrite.  The host publishes events_drained, the highest event id it has read out.  A step of event e with
// e - events_drained > n_slots stores nothing -- its slot still holds an event nobody has read --, and thread 0 of workgroup 0 sets
// events_lost = 1.
//
// Who reads what this launch writes: nobody.  `first` must not come from a word another workgroup of the same launch stores, so the
// slot's id is kept once PER WORKGROUP: events_ids [slot][workgroup].  Every thread of workgroup b loads word b, the barrier follows
// (every wave's load has returned), then thread 0 of workgroup b stores e into word b -- k_points' order, read first and the write
// last, inside one workgroup where a barrier can give it.  The copies of the workgroups that hold columns agree after every launch:
// every launch covers all of them (events_nblk = the columns' workgroups + 1, for the fused launch's grid, which has one workgroup more
// with RH_TAIL_PRE; that one holds no column, so its copy decides nothing).  The other header words are read and written by thread 0
// of workgroup 0 alone; header word 0 mirrors its copy.
// events_drained, events_running and the configuration are written by the host only, between launches.
//
// An event step moves 8 B read per item and column plus up to 16 B read-modify-write (SUM, PEAK; LAST 8 B of store, FIRST nothing
// after the first step); an off-event step is one launch that exits on a scalar.
#pragma once

#define RH_EVENTS_MAX_ITEMS 16
#define RH_EVENTS_SUM 0
#define RH_EVENTS_PEAK 1
#define RH_EVENTS_FIRST 2
#define RH_EVENTS_LAST 3
__global__ __launch_bounds__(RH_BLOCK) void k_events(Arena a, DevState *D, int after_fused) {
    const long long e = D->S.event_id[1];
    if (e == 0) return;
    const int nb = D->events_nblk, ns = D->events_nslots;
    if ((after_fused && D->skipped) || (int)blockIdx.x >= nb) return;   // (uniform over the workgroup: in front of the barrier)
    const long long slot = e % ns;
    long long *const mine = D->events_ids + (size_t)slot * nb + blockIdx.x;
    const bool first = *mine != e;
    const bool lost = e - D->events_drained > ns;
    const long long t1 = D->S.time, dts = D->S.dt_secs, running = D->events_running;
    const double dt = D->S.dt;
    __syncthreads();   // every thread of the workgroup holds `first`; only now the workgroup's copy of the id changes
    if (threadIdx.x == 0) {
        if (lost) {
            if (blockIdx.x == 0) D->events_lost = 1;
        } else {
            *mine = e;
            if (blockIdx.x == 0) {
                long long *h = D->events_hdr + 6 * slot;
                const long long ten = dts == 600 ? 1 : 0, hour = dts == 3600 ? 1 : 0;
                if (first) {
                    h[0] = e;
                    h[1] = 1;
                    h[2] = e == running ? -1 : t1 - dts;
                    h[4] = ten;
                    h[5] = hour;
                } else {
                    h[1] = h[1] + 1;
                    h[4] = h[4] + ten;
                    h[5] = h[5] + hour;
                }
                h[3] = t1;
            }
        }
    }
    const int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (lost || i >= a.n) return;
    const int ni = D->events_nitems;
    const size_t n = (size_t)a.n;
    double *base = D->events + (size_t)slot * ni * n + i;
    for (int j = 0; j < ni; ++j) {
        const int kind = D->events_kinds[j];
        if (kind == RH_EVENTS_FIRST && !first) continue;
        double v;
        rh_ld(a, D->events_planes[j], i, v);
        double *p = base + (size_t)j * n;
        if (kind == RH_EVENTS_SUM) {
            *p = first ? v : *p + v;
        } else if (kind == RH_EVENTS_PEAK) {
            const double r = v / dt;
            if (first) {
                *p = r;
            } else {
                const double q = *p;
                if (r > q || (q != q && r == r)) *p = r;
            }
        } else {
            *p = v;
        }
    }
}
