"""Child process of tests/test_hip_durations_ranks.py: the duration curves behind rh_run_steps_dist on two loopback ranks, 257 x 1 as
256 + 1 columns (a full tile, and a rank of one column), SVAT with and without lateral flow.  Ranks are threads of this process joined by
the loopback communicator (RH_RCCL_LIB), with the helpers of tests/ranks_observers.py: its single-domain `reference` without observer
and communicator, its `Block` of a rank's columns and `run_ranks`.  Every rank must hold the restatement (tests/durations_reference.py)
over ITS columns of the single-domain record: counters and spell planes exactly, the float planes as bits.  Edges, thresholds and the
mask are those of tests/test_hip_durations.py, defined on the global domain and cut to the block."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from ranks_observers import Block, native, reference, run_ranks  # noqa: E402
from test_hip_durations import KINDS, NAMES, config_of, expected, mask_of  # noqa: E402
from test_hip_points import NDAYS, NSTEPS  # noqa: E402


def main():
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    nx, ny, cutx, iv = 257, 1, 256, 3600
    forcing = combo_forcing(ndays=NDAYS + 4)
    blocks = [np.arange(0, cutx * ny), np.arange(cutx * ny, nx * ny)]
    mask = mask_of(nx * ny)
    assert all(mask[b].any() for b in blocks)
    for lateral in (False, True):
        p = hetero_params(nx * ny, seed=5)
        if lateral:
            p.update(slope=0.05, slope_per=5, dmph=50.0)
            p["z_soil"] = np.maximum(p["z_soil"], 800.0)

        def make(x0, x1, p=p, lateral=lateral):
            ctx = create_svat(x1 - x0, ny, params={k: (v[x0 * ny:x1 * ny] if np.ndim(v) else v) for k, v in p.items()}, lateral=lateral)
            ctx.set_forcing_series(forcing)
            return ctx

        rec = reference(make(0, nx), NSTEPS, NAMES, what=f"257 x 1 lateral={lateral}")
        cfg = config_of(rec.hdr, rec.planes, iv)
        for pieces in ((NSTEPS,), (1, 2, 37, NSTEPS - 40)):
            uid = native.comm_unique_id()

            def rank(r, uid=uid, pieces=pieces):
                ctx = make(int(blocks[r][0]) // ny, int(blocks[r][-1]) // ny + 1)
                ctx.comm_init(uid, 2, r)
                ctx.durations_configure(NAMES, KINDS, cfg[0], cfg[1], mask[blocks[r]], iv, 0)
                for n in pieces:
                    ctx.run_steps_dist(n)
                got = ctx.durations_read()
                ctx.close()
                return got

            held = run_ranks(rank, 2)
            for r, (counts, vals, spells) in enumerate(held):   # (compared in the main thread, after both ranks have returned)
                want = expected(Block(rec, blocks[r]), cfg, iv, mask[blocks[r]])
                for j, c in enumerate(counts):
                    np.testing.assert_array_equal(c, want.counts[j], err_msg=f"rank {r}, pieces {pieces}: counts of item {j}")
                np.testing.assert_array_equal(spells, want.spells, err_msg=f"rank {r}, pieces {pieces}: spell planes")
                assert (vals.view(np.uint64) == want.vals.view(np.uint64)).all(), (r, pieces, "float planes")
                assert want.counts[0].any()
        print(f"durations 257 x 1 lateral={lateral}: blocks of {[len(b) for b in blocks]} columns == restatements of the single domain over "
              f"{NSTEPS} steps, in one call and in pieces")


if __name__ == "__main__":
    main()
