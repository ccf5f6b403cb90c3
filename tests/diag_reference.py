"""The output accumulators (rh_diag_*, k_diag in roger_amd/csrc/rh_control.h) restated on the host in plain numpy.

Imports nothing from roger_amd: it is the rule of include/roger_hip.h (the accumulator section) and of the comment above k_diag,
written down a second time, so that the device kernel and the CPU double (tests/oracle_context.py) can each be held against it
bit for bit -- an accumulator is a sequence of float64 additions in a fixed operand order, there is nothing to tolerate.

After a step that covered (t_start, t_end]:

    t_start = t_end - dt_secs
    slot    = (t_start // interval) % n_slots
    first   = t_start % interval == 0          (a step never straddles an interval boundary it does not start on)
    rate:     slot value = value               on `first`, otherwise old + value (in that operand order)
    collect:  slot value = value               always

and the slot's bookkeeping: steps = 1 on `first`, otherwise max(steps, 0) + 1 (a slot first touched INSIDE its interval counts the
steps that were actually accumulated); t0 = t_start on `first` only (-1 until then: such a slot never learns where its interval
began, which is how roger_amd/diagnostics.py tells a partial sub-daily interval from a whole one); t1 = t_end.  A slot nobody has
touched holds zeros and (-1, -1, -1)."""
import numpy as np


class HostAccumulator:
    def __init__(self, rate, collect, n_slots, n, interval=86400):
        self.rate, self.collect = list(rate), list(collect)
        self.n_slots, self.n, self.interval = int(n_slots), int(n), int(interval)
        assert self.n_slots >= 1 and self.interval in (86400, 3600, 600)
        self.data = {v: np.zeros((self.n_slots, self.n), dtype=np.float64) for v in self.rate + self.collect}
        self.steps = np.full(self.n_slots, -1, dtype=np.int64)
        self.t0 = np.full(self.n_slots, -1, dtype=np.int64)
        self.t1 = np.full(self.n_slots, -1, dtype=np.int64)
        self.log = []   # (t_start, dt_secs, slot, first) of every step fed

    def set_interval(self, interval):
        """rh_diag_set_interval on a configured context: the values stay, the bookkeeping of every slot starts over."""
        self.interval = int(interval)
        assert self.interval in (86400, 3600, 600)
        self.steps[:], self.t0[:], self.t1[:] = -1, -1, -1

    def add(self, t_end, dt_secs, planes):
        """One step: planes[name] = the (n,) float64 values the step left.  Returns the slot it went into."""
        t_end, dt_secs = int(t_end), int(dt_secs)
        t_start = t_end - dt_secs
        slot = (t_start // self.interval) % self.n_slots
        first = t_start % self.interval == 0
        for v in self.rate:
            x = np.asarray(planes[v], dtype=np.float64).reshape(self.n)
            self.data[v][slot] = x if first else self.data[v][slot] + x
        for v in self.collect:
            self.data[v][slot] = np.asarray(planes[v], dtype=np.float64).reshape(self.n)
        self.steps[slot] = 1 if first else max(int(self.steps[slot]), 0) + 1
        if first:
            self.t0[slot] = t_start
        self.t1[slot] = t_end
        self.log.append((t_start, dt_secs, int(slot), bool(first)))
        return int(slot)

    def reported_steps(self, slot):
        """What rh_diag_steps reports: the divisor of the average diagnostic, 0 for a slot nobody has touched."""
        return max(int(self.steps[int(slot)]), 0)

    # -- what a run has exercised, from the log of the steps fed (tests assert these before they lean on them) ------------------
    def step_classes(self):
        return {dt for _, dt, _, _ in self.log}

    def slots_reused(self):
        """Slots that a later interval took over after the index wrapped."""
        seen, reused = {}, set()
        for t_start, _, slot, _ in self.log:
            k = t_start // self.interval
            if slot in seen and seen[slot] != k:
                reused.add(slot)
            seen[slot] = k
        return reused

    def intervals_never_started(self):
        """Intervals inside the run that no step began in: a longer step covered them (sub-daily intervals only)."""
        if not self.log:
            return set()
        begun = {t_start // self.interval for t_start, _, _, _ in self.log}
        last = max(t_start + dt - 1 for t_start, dt, _, _ in self.log) // self.interval
        return set(range(min(begun), last + 1)) - begun
