"""Child process of tests/test_hip_zonal_ranks.py: two loopback ranks (tests/loopback_ranks_child.py: two threads, one context each, joined
by tests/loopback_nccl.cpp) record the zonal totals of their halves of the heterogeneous 4 x 4 SVAT case over the GLOBAL zone list, write
one file each as the host package does, and `zonal_totals.combine` merges them; the merged file against the single domain's.

    python tests/zonal_ranks_child.py OUT_DIR
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from golden_util import load_case  # noqa: E402
from loopback_ranks_child import run_ranks, svat_ctx  # noqa: E402
from nc_util import netcdf_file  # noqa: E402
from roger_amd import _native as native  # noqa: E402
from roger_amd import zonal_totals as zt  # noqa: E402
from roger_amd.totals import local_mask  # noqa: E402

NAMES = ["theta_rz", "S_rz", "swe", "prec"]
NSTEPS = 60
# ids 3 and 8 lie in both halves, 5 in the first only, 9 in the second only; two columns outside
ZONES = np.array([[3, 3, 5, 8], [5, 0, 3, 8], [8, 9, 3, 3], [9, -1, 8, 3]])


def write(path, hdr, values, ids, ncells):
    zt._write_file(path, zt._file_variables(hdr, values, NAMES, ids, ncells, "2018-01-01 00:00:00"), "GoldenSVAT")


def main(out):
    g, names, forcing = load_case("svat_hetero_combo")
    nx, ny = (int(v) for v in g["nx_ny"])
    assert ZONES.shape == (nx, ny)
    ids, index = zt.zone_ids(ZONES)
    nz = ids.size
    # the single domain: its rows, and the planes after every step (the terms of the bound)
    whole = svat_ctx(g, names, forcing)
    whole.zonal_configure(NAMES, index, nz, capacity=NSTEPS)
    terms = []
    for _ in range(NSTEPS):
        whole.run_steps(1)
        terms.append({v: whole.download(v) for v in NAMES})
    hdr, values = whole.zonal_read(0, NSTEPS)
    one = os.path.join(out, "one.zonal_totals.nc")
    write(one, hdr, values, ids, whole.zonal_count()[1])
    whole.close()
    uid = native.comm_unique_id()

    def rank(r):
        ctx = svat_ctx(g, names, forcing, columns=(r * nx // 2, (r + 1) * nx // 2))
        ctx.comm_init(uid, 2, r)
        local = local_mask(index, nx, ny, (2, 1), r)
        ctx.zonal_configure(NAMES, local, nz, capacity=NSTEPS)
        ctx.run_steps_dist(NSTEPS)
        rows, cells = ctx.zonal_count()
        assert rows == NSTEPS
        h, v = ctx.zonal_read(0, NSTEPS)
        ctx.close()
        path = os.path.join(out, f"two.zonal_totals.{r:04d}.nc")
        write(path, h, v, ids, cells)
        return path, cells

    res = run_ranks(rank, 2)
    assert list(res[0][1]) == [3, 2, 2, 0] and list(res[1][1]) == [3, 0, 2, 2], (res[0][1], res[1][1])
    two = os.path.join(out, "two.zonal_totals.nc")
    zt.combine([res[0][0], res[1][0]], two)
    a, b = netcdf_file(one), netcdf_file(two)
    for key in ("zone", "ncells", "itt", "dt", "Time"):
        np.testing.assert_array_equal(a.variables[key][:], b.variables[key][:], err_msg=key)
    worst = 0.0
    for v in NAMES:
        for stat in ("min", "max"):
            np.testing.assert_array_equal(a.variables[f"{v}_{stat}"][:], b.variables[f"{v}_{stat}"][:], err_msg=f"{v}_{stat}")
        sa, sb = np.asarray(a.variables[f"{v}_sum"][:]), np.asarray(b.variables[f"{v}_sum"][:])
        for k in range(NSTEPS):
            for z in range(nz):
                t = terms[k][v].reshape(-1)[index.reshape(-1) == z]
                bound = t.size * 2.0 ** -52 * math.fsum(np.abs(t))      # reassociating n additions
                assert abs(sa[k, z] - sb[k, z]) <= bound, (v, k, z, sa[k, z], sb[k, z], bound)
                worst = max(worst, abs(sa[k, z] - sb[k, z]) / bound if bound else 0.0)
        assert np.any(sa != 0), v
    print(f"zonal: 2 ranks combined == single domain within n 2^-52 sum|t| over {NSTEPS} steps (largest difference / bound {worst:.3f})")


if __name__ == "__main__":
    main(sys.argv[1])
