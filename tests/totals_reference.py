"""The totals recorder (rh_totals_*, k_totals_tiles / k_totals_finish in roger_amd/csrc/rh_control.h) restated on the host in plain
numpy, and the CPU double with it.

`tree_totals` imports nothing from roger_amd: it is the reduction order of include/roger_hip.h written down a second time.
  1. the columns, padded to a multiple of 256 with the identity (+0.0 / +inf / -inf; also where the mask is clear), as
     (tiles, 4 wavefronts, 64 lanes); per wavefront the tree with strides 32, 16, 8, 4, 2, 1: x[l] = x[l] + x[l + stride] for l < stride;
  2. per tile (w0 + w1) + (w2 + w3);
  3. the tiles' partials p: accumulator t (of 256) starts from the identity and adds p[t], p[t + 256], ... in this order; the 256
     accumulators then go through 1. and 2. as one tile.
`TotalsOracleContext` is tests/oracle_context.py's double with the three totals_* methods of `_native.Context`."""
import numpy as np

from oracle_context import OracleContext
from points_reference import HostRing

IDENTITY = {"sum": 0.0, "min": np.inf, "max": -np.inf}
OP = {"sum": np.add, "min": np.fmin, "max": np.fmax}


def _tile(x, op):
    """x (tiles, 4, 64) -> (tiles,)"""
    x = x.copy()
    for stride in (32, 16, 8, 4, 2, 1):
        x[:, :, :stride] = op(x[:, :, :stride], x[:, :, stride:2 * stride])
    w = x[:, :, 0]
    return op(op(w[:, 0], w[:, 1]), op(w[:, 2], w[:, 3]))


def tree_reduce(values, mask, stat):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    keep = np.ones(v.size, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    assert keep.size == v.size
    op, ident = OP[stat], IDENTITY[stat]
    tiles = (v.size + 255) // 256
    x = np.full(tiles * 256, ident, dtype=np.float64)
    x[:v.size][keep] = v[keep]
    p = _tile(x.reshape(tiles, 4, 64), op)
    acc = np.full(256, ident, dtype=np.float64)
    for t in range(tiles):            # increasing tile order: accumulator t mod 256 takes tile t
        acc[t % 256] = op(acc[t % 256], p[t])
    return float(_tile(acc.reshape(1, 4, 64), op)[0])


def tree_totals(values, mask=None):
    """(sum, min, max) over the masked columns in the device's order."""
    return tuple(tree_reduce(values, mask, s) for s in ("sum", "min", "max"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


class TotalsOracleContext(OracleContext):
    """The double with totals: `trace` keeps every recorded row whatever the ring's capacity (what the tests compare files with)."""

    _tring = None

    def totals_configure(self, names, mask=None, capacity=4096):
        names = list(names)
        if not names:
            self._tring = None
            return
        if len(names) > 32:
            raise ValueError("totals_configure: n_planes")
        if any(self.st.planes[v].dtype != np.float64 for v in names):
            raise ValueError("totals_configure: float64 planes only")
        m = None if mask is None else np.asarray(mask).reshape(-1) != 0
        if m is not None and (m.size != self.n or not m.any()):
            raise ValueError("totals_configure: mask")
        self._tring = HostRing(capacity, len(names), 3)
        self._tnames, self._tmask, self.totals_trace = names, m, []

    def totals_count(self):
        if self._tring is None:
            raise RuntimeError("totals_configure has not been called")
        return self._tring.count, self.n if self._tmask is None else int(self._tmask.sum())

    def totals_read(self, first, n):
        if self._tring is None:
            raise RuntimeError("totals_configure has not been called")
        return self._tring.read(first, n)

    def _accumulate(self):
        super()._accumulate()
        if self._tring is None:
            return
        s = self.st.scal
        hdr = (int(s.itt), int(s.time), int(s.dt_secs))
        values = np.array([tree_totals(self.st.planes[v], self._tmask) for v in self._tnames])
        self._tring.add(hdr, values)
        self.totals_trace.append((hdr, values.copy()))
