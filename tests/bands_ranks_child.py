"""Child process of tests/test_hip_bands_ranks.py: the ensemble bands behind rh_run_steps_dist on two loopback ranks, 257 x 1 as 256 + 1
columns (a full tile, and a rank of one column).  Ranks are threads of this process joined by the loopback communicator (RH_RCCL_LIB),
with the helpers of tests/ranks_observers.py: its single-domain `reference` without observer and communicator, its `Block` of a rank's
columns and `run_ranks`.  Order statistics of blocks do not merge: every rank must hold the restatement (tests/bands_reference.py) over
ITS columns of the single-domain record, headers exactly and values as bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from bands_reference import LAST, SUM, HostBands  # noqa: E402
from ranks_observers import Block, native, reference, run_ranks  # noqa: E402
from test_hip_points import NDAYS, NSTEPS  # noqa: E402

NAMES, KINDS, PROBS = ("q_ss", "theta_rz"), (SUM, LAST), (0.0, 0.05, 0.5, 0.95, 1.0)


def main():
    from roger_amd.forcing import combo_forcing
    from roger_amd.svat import create_svat, hetero_params

    nx, ny, cutx, iv = 257, 1, 256, 3600
    forcing = combo_forcing(ndays=NDAYS + 4)
    blocks = [np.arange(0, cutx * ny), np.arange(cutx * ny, nx * ny)]
    mask = np.ones(nx * ny, dtype=np.uint8)
    mask[[5, 64, 200]] = 0
    p = hetero_params(nx * ny, seed=5)

    def make(x0, x1):
        ctx = create_svat(x1 - x0, ny, params={k: (v[x0 * ny:x1 * ny] if np.ndim(v) else v) for k, v in p.items()}, lateral=False)
        ctx.set_forcing_series(forcing)
        return ctx

    rec = reference(make(0, nx), NSTEPS, NAMES, what="257 x 1")
    for pieces in ((NSTEPS,), (1, 2, 37, NSTEPS - 40)):
        uid = native.comm_unique_id()

        def rank(r, uid=uid, pieces=pieces):
            ctx = make(int(blocks[r][0]) // ny, int(blocks[r][-1]) // ny + 1)
            ctx.comm_init(uid, 2, r)
            ctx.bands_configure(NAMES, KINDS, PROBS, iv, 0, mask[blocks[r]], NSTEPS)
            for n in pieces:
                ctx.run_steps_dist(n)
            got = ctx.bands_read(0, ctx.bands_count())
            ctx.close()
            return got

        held = run_ranks(rank, 2)
        for r, (hdr, values) in enumerate(held):   # (compared in the main thread, after both ranks have returned)
            blk = Block(rec, blocks[r])
            h = HostBands(KINDS, PROBS, len(blocks[r]), mask[blocks[r]], iv, 0)
            for k in range(NSTEPS):
                t1, dt = int(rec.hdr[k, 1]), int(rec.hdr[k, 2])
                h.add(t1 - dt, t1, [blk.planes[v][k] for v in NAMES])
            whdr, wvalues = h.rows()
            assert len(whdr) > NDAYS and (whdr[:, 2] == int(mask[blocks[r]].sum())).all()
            np.testing.assert_array_equal(hdr, whdr, err_msg=f"rank {r}, pieces {pieces}: headers")
            assert values.shape == wvalues.shape and (values.view(np.uint64) == wvalues.view(np.uint64)).all(), (r, pieces, "values")
    print(f"bands 257 x 1: blocks of {[len(b) for b in blocks]} columns == restatements of the single domain over {NSTEPS} steps, "
          "in one call and in pieces")


if __name__ == "__main__":
    main()
