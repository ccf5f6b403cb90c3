"""The points recorder (rh_points_*, k_points in roger_amd/csrc/rh_control.h) restated on the host in plain numpy, and the CPU double
with it.

`HostRing` imports nothing from roger_amd: it is the ring rule of include/roger_hip.h written down a second time -- row r lives at
r mod capacity; a range is served only while all of it is resident (first >= count - capacity) and recorded (first + n <= count).
`PointsOracleContext` is tests/oracle_context.py's double with the three points_* methods of `_native.Context`; it records after each
of the double's steps, where the double accumulates its output diagnostics."""
import numpy as np

from oracle_context import OracleContext


class HostRing:
    def __init__(self, capacity, n_planes, n_cells):
        if int(capacity) < 1:
            raise ValueError(f"capacity = {capacity}")
        self.capacity = int(capacity)
        self.hdr = np.zeros((self.capacity, 3), dtype=np.int64)
        self.values = np.zeros((self.capacity, int(n_planes), int(n_cells)), dtype=np.float64)
        self.count = 0

    def add(self, hdr, values):
        slot = self.count % self.capacity
        self.hdr[slot] = hdr
        self.values[slot] = values
        self.count += 1

    def read(self, first, n):
        first, n = int(first), int(n)
        if first < 0 or n < 0 or first + n > self.count:
            raise ValueError(f"rows {first} ... {first + n - 1} have not been recorded ({self.count} rows so far)")
        if n and first < self.count - self.capacity:
            raise ValueError(f"rows {first} ... {self.count - self.capacity - 1} have been overwritten")
        idx = (first + np.arange(n)) % self.capacity
        return self.hdr[idx].copy(), self.values[idx].copy()


class PointsOracleContext(OracleContext):
    """The double with points: `trace` keeps every recorded row whatever the ring's capacity (what the tests compare files with)."""

    _ring = None

    def points_configure(self, cells, names, capacity=4096):
        cells, names = [int(c) for c in cells], list(names)
        if not cells or not names:
            self._ring = None
            return
        if any(not 0 <= c < self.n for c in cells) or len(set(cells)) != len(cells) or len(cells) > 256 or len(names) > 32:
            raise ValueError("points_configure: cells")
        if any(self.st.planes[v].dtype != np.float64 for v in names):
            raise ValueError("points_configure: float64 planes only")
        self._ring = HostRing(capacity, len(names), len(cells))
        self._pcells, self._pnames, self.trace = cells, names, []

    def points_count(self):
        if self._ring is None:
            raise RuntimeError("points_configure has not been called")
        return self._ring.count

    def points_read(self, first, n):
        if self._ring is None:
            raise RuntimeError("points_configure has not been called")
        return self._ring.read(first, n)

    def _accumulate(self):
        super()._accumulate()
        if self._ring is None:
            return
        s = self.st.scal
        hdr = (int(s.itt), int(s.time), int(s.dt_secs))
        values = np.stack([self.st.planes[v][self._pcells] for v in self._pnames])
        self._ring.add(hdr, values)
        self.trace.append((hdr, values.copy()))
