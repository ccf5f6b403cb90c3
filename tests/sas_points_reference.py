"""The SAS context's points recorder (rh_sas_points_*, k_sas_points in roger_amd/csrc/rh_sas_points.h) restated on the host, and the CPU
double with it.

`TagRing` is points_reference.HostRing -- the ring rule written down without roger_amd -- with rows of `row_elems` float64 and one
int64 tag per row.  `PointsOracleSasContext` is the oracle-backed SasContext double (with the row-block transfers the restart path
uses) plus the four points_* methods of `_native.SasContext`: a whole day (`step`) records a row, `stages` never does.  `trace` keeps
every recorded row whatever the ring's capacity."""
import numpy as np

from points_reference import HostRing
from roger_amd._native import DAILY_INPUTS, NativeError
from test_host_package_sas_restart import CellOracleSasContext

MAX_CELLS, MAX_ARRAYS = 256, 32     # include/roger_hip_sas.h


class TagRing(HostRing):
    def __init__(self, capacity, row_elems):
        super().__init__(capacity, 1, row_elems)

    def add(self, tag, row):
        super().add((int(tag), 0, 0), np.asarray(row, dtype=np.float64).reshape(1, -1))

    def read(self, first, n):
        hdr, values = super().read(first, n)
        return hdr[:, 0].copy(), values[:, 0, :]


def row_layout(names, widths, n_cells):
    """{name: (offset, width)}: arrays in configured order, cells within an array, the age axis contiguous within a cell."""
    out, off = {}, 0
    for v, w in zip(names, widths):
        out[v] = (off, w)
        off += n_cells * w
    return out, off


def split_rows(values, names, widths, n_cells):
    """(n, row_elems) -> {name: (n, K) or (n, K, width)}"""
    layout, _ = row_layout(names, widths, n_cells)
    n = values.shape[0]
    return {v: (values[:, off:off + n_cells].copy() if w == 1 else values[:, off:off + n_cells * w].reshape(n, n_cells, w).copy())
            for v, (off, w) in layout.items()}


class PointsOracleSasContext(CellOracleSasContext):
    _ring = None

    def points_configure(self, cells, names, capacity=4096):
        cells, names = [int(c) for c in cells], list(names)
        if len(cells) > MAX_CELLS or len(names) > MAX_ARRAYS:
            raise NativeError("rh_sas_points_configure: counts above the limits")
        if not cells or not names:
            self._ring = None
            return
        if any(not 0 <= c < self.n for c in cells) or len(set(cells)) != len(cells):
            raise NativeError("rh_sas_points_configure: cells")
        held = self._arrays()
        for v in names:
            if names.count(v) > 1 or v not in held or held[v].dtype != np.float64 or v in DAILY_INPUTS or v.startswith("sas_params_"):
                raise NativeError(f"rh_sas_points_configure: array {v}")
        self._pcells, self._pnames = cells, names
        self._pwidths = [int(np.prod(held[v].shape[1:], dtype=np.int64)) for v in names]
        self._ring = TagRing(capacity, row_layout(names, self._pwidths, len(cells))[1])
        self.trace = []

    def _on(self):
        if self._ring is None:
            raise NativeError("rh_sas_points_configure has not been called")
        return self._ring

    def points_record(self, tag=0):
        ring, held = self._on(), self._arrays()
        row = np.concatenate([held[v][self._pcells].reshape(-1) for v in self._pnames])
        ring.add(tag, row)
        self.trace.append((int(tag), split_rows(row[None, :], self._pnames, self._pwidths, len(self._pcells))))

    def points_count(self):
        return self._on().count

    def points_read(self, first, n):
        try:
            tags, values = self._on().read(first, n)
        except ValueError as e:
            raise NativeError(f"rh_sas_points_read: {e}") from None
        return tags, split_rows(values, self._pnames, self._pwidths, len(self._pcells))

    def step(self, day):
        super().step(day)
        if self._ring is not None:
            self.points_record(day)
