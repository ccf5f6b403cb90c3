"""The zonal totals recorder (rh_zonal_*, k_zonal_tiles / k_zonal_finish in roger_amd/csrc/rh_zonal.h) restated on the host in plain
numpy and Python loops, and the CPU double with it.  Imports nothing from roger_amd.

`build_index` is the index rh_zonal_configure builds from a zone map (an int per column, -1 outside, else 0 ... Z - 1):
  tile_ptr[ntiles + 1], tile_zone[S]: per tile of 256 columns the ascending zones present; the position s of a (tile, zone) pair is
                                      its slot
  acc_ptr[Z * 256 + 1], acc_slot[S]:  per (zone, accumulator t) the slots of the tiles with tile mod 256 == t, in increasing tile order
`walk_index` is the two kernels over that index: per slot the wavefront trees (strides 32 ... 1) of the columns of the zone, the identity
elsewhere, and (w0 op w1) op (w2 op w3); per zone 256 accumulators from the identity over their slots in list order, then the same two
levels.  It must give what totals_reference.tree_totals gives with mask = zones == z, bit for bit.
`ZonalOracleContext` is tests/oracle_context.py's double with the three zonal_* methods of `_native.Context`."""
import numpy as np

from oracle_context import OracleContext
from points_reference import HostRing
from totals_reference import IDENTITY, OP, _tile

TILE = 256
STATS = ("sum", "min", "max")


def build_index(zone, n_zones):
    zone = np.asarray(zone).reshape(-1)
    ntiles = (zone.size + TILE - 1) // TILE
    tile_ptr, tile_zone = [0], []
    for b in range(ntiles):
        here = zone[b * TILE:(b + 1) * TILE]
        tile_zone += sorted(set(int(z) for z in here if z >= 0))
        tile_ptr.append(len(tile_zone))
    lists = [[] for _ in range(n_zones * TILE)]
    for b in range(ntiles):
        for s in range(tile_ptr[b], tile_ptr[b + 1]):
            lists[tile_zone[s] * TILE + b % TILE].append(s)
    acc_ptr, acc_slot = [0], []
    for lst in lists:
        acc_slot += lst
        acc_ptr.append(len(acc_slot))
    return (np.array(tile_ptr, dtype=np.int64), np.array(tile_zone, dtype=np.int64), np.array(acc_ptr, dtype=np.int64),
            np.array(acc_slot, dtype=np.int64))


def walk_index(values, zone, n_zones, index=None):
    """(n_zones, 3): sum, min, max per zone by walking the index as the kernels do."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    zone = np.asarray(zone).reshape(-1)
    tile_ptr, tile_zone, acc_ptr, acc_slot = index if index is not None else build_index(zone, n_zones)
    ntiles = len(tile_ptr) - 1
    vp = np.zeros(ntiles * TILE)
    vp[:v.size] = v
    zp = np.full(ntiles * TILE, -1, dtype=np.int64)
    zp[:zone.size] = zone
    out = np.empty((n_zones, 3))
    for k, stat in enumerate(STATS):
        op, ident = OP[stat], IDENTITY[stat]
        part = np.empty(len(tile_zone))
        for b in range(ntiles):                                   # k_zonal_tiles: one workgroup per tile, a round per zone it holds
            cols = slice(b * TILE, (b + 1) * TILE)
            for s in range(tile_ptr[b], tile_ptr[b + 1]):
                x = np.where(zp[cols] == tile_zone[s], vp[cols], ident)
                part[s] = _tile(x.reshape(1, 4, 64), op)[0]
        for z in range(n_zones):                                  # k_zonal_finish: one workgroup per zone, thread t = accumulator t
            acc = np.full(TILE, ident)
            for t in range(TILE):
                for s in acc_slot[acc_ptr[z * TILE + t]:acc_ptr[z * TILE + t + 1]]:
                    acc[t] = op(acc[t], part[s])
            out[z, k] = _tile(acc.reshape(1, 4, 64), op)[0]
    return out


class ZonalOracleContext(OracleContext):
    """The double with zonal totals: `zonal_trace` keeps every recorded row whatever the ring's capacity."""

    _zring = None

    def zonal_configure(self, names, zones=None, n_zones=0, capacity=4096):
        names = list(names)
        if not names:
            self._zring = None
            return
        z = np.asarray(zones).reshape(-1).astype(np.int64)
        if len(names) > 32 or not 1 <= int(n_zones) <= 1024:
            raise ValueError("zonal_configure: counts")
        if any(self.st.planes[v].dtype != np.float64 for v in names):
            raise ValueError("zonal_configure: float64 planes only")
        if z.size != self.n or z.min() < -1 or z.max() >= n_zones or not (z >= 0).any():
            raise ValueError("zonal_configure: zone map")
        self._zring = HostRing(capacity, int(n_zones), len(names) * 3)
        self._znames, self._zmap, self._nz, self.zonal_trace = names, z, int(n_zones), []
        self._zindex = build_index(z, int(n_zones))

    def zonal_count(self):
        if self._zring is None:
            raise RuntimeError("zonal_configure has not been called")
        return self._zring.count, np.bincount(self._zmap[self._zmap >= 0], minlength=self._nz).astype(np.int64)

    def zonal_read(self, first, n):
        if self._zring is None:
            raise RuntimeError("zonal_configure has not been called")
        hdr, values = self._zring.read(first, n)
        return hdr, values.reshape(len(hdr), self._nz, len(self._znames), 3)

    def _accumulate(self):
        super()._accumulate()
        if self._zring is None:
            return
        s = self.st.scal
        hdr = (int(s.itt), int(s.time), int(s.dt_secs))
        values = np.stack([walk_index(self.st.planes[v], self._zmap, self._nz, self._zindex) for v in self._znames], axis=1)   # (Z, V, 3)
        self._zring.add(hdr, values.reshape(self._nz, -1))
        self.zonal_trace.append((hdr, values.copy()))
