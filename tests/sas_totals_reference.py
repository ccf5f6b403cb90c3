"""The totals recorder of the SAS context (rh_sas_totals_*, roger_amd/csrc/rh_sas_totals.h) restated on the host in plain numpy: which
cells count, and both orders of summation (include/roger_hip_sas.h).  Imports nothing from roger_amd.

Width 1 (`tree_reduce`): the cells, padded to a multiple of 256 with the identity (+0.0 / +inf / -inf; also where a cell is not counted), as
(tiles, 4 wavefronts, 64 lanes); per wavefront the tree with strides 32 ... 1, x[l] = x[l] op x[l + stride]; per tile (w0 + w1) + (w2 + w3);
accumulator t of 256 starts from the identity and takes the tiles' partials p[t], p[t + 256], ... in this order; the 256 accumulators go
through the same two levels.

Width W > 1 (`run_sums`), per age class: runs of 256 consecutive cells, each summed left to right from +0.0, a skipped cell contributing
+0.0; the same on the sequence of partials until one value is left."""
import numpy as np

RUN = 256
IDENTITY = {"sum": 0.0, "min": np.inf, "max": -np.inf}
OP = {"sum": np.add, "min": np.fmin, "max": np.fmax}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def _tile(x, op):
    """x (tiles, 4, 64) -> (tiles,)"""
    x = x.copy()
    for stride in (32, 16, 8, 4, 2, 1):
        x[:, :, :stride] = op(x[:, :, :stride], x[:, :, stride:2 * stride])
    w = x[:, :, 0]
    return op(op(w[:, 0], w[:, 1]), op(w[:, 2], w[:, 3]))


def tree_reduce(x, stat="sum"):
    """The width-1 order over x (n,), in which the cells that do not count already hold the identity."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    op, ident = OP[stat], IDENTITY[stat]
    tiles = (x.size + 255) // 256
    padded = np.full(tiles * 256, ident, dtype=np.float64)
    padded[:x.size] = x
    p = _tile(padded.reshape(tiles, 4, 64), op)
    acc = np.full(256, ident, dtype=np.float64)
    for t0 in range(0, tiles, 256):       # accumulator t: partials t, t + 256, ... in increasing order
        piece = p[t0:t0 + 256]
        acc[:piece.size] = op(acc[:piece.size], piece)
    return float(_tile(acc.reshape(1, 4, 64), op)[0])


def run_sums(x):
    """The age order over x (n, W), in which skipped cells and NaN elements already hold +0.0: (W,)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    while True:
        runs = (x.shape[0] + RUN - 1) // RUN
        padded = np.zeros((runs * RUN, x.shape[1]), dtype=np.float64)
        padded[:x.shape[0]] = x
        padded = padded.reshape(runs, RUN, x.shape[1])
        acc = np.zeros((runs, x.shape[1]), dtype=np.float64)
        for k in range(RUN):              # left to right
            acc = acc + padded[:, k, :]
        if runs == 1:
            return acc[0]
        x = acc


def eligible(n, weight=None, mask=None, live=True):
    e = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    assert e.size == n
    if not live:
        return np.zeros(n, dtype=bool)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            e = e & (np.asarray(weight, dtype=np.float64).reshape(-1) > 0.0)      # (NaN > 0 is False)
    return e


def item_block(values, weight=None, mask=None, live=True):
    """The row block of one item: [wsum, count, sum, min, max] for values (n,), [wsum, count, sum[0 ... W)] for values (n, W).
    `live` False: day < 0 for an item that has a weight or a DAILY value."""
    v = np.asarray(values, dtype=np.float64)
    n = v.shape[0]
    e = eligible(n, weight, mask, live)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        if v.ndim == 1:
            c = e & ~np.isnan(v)
            t = v if weight is None else v * w                                    # rounded before it is added
            return np.array([tree_reduce(np.where(c, w, 0.0)), tree_reduce(np.where(c, 1.0, 0.0)), tree_reduce(np.where(c, t, 0.0)),
                             tree_reduce(np.where(c, v, np.inf), "min"), tree_reduce(np.where(c, v, -np.inf), "max")])
        t = v if weight is None else v * w[:, None]
        t = np.where(e[:, None] & ~np.isnan(v), t, 0.0)
        return np.concatenate([[tree_reduce(np.where(e, w, 0.0)), tree_reduce(np.where(e, 1.0, 0.0))], run_sums(t)])


def as_block(stats):
    """The dict of SasContext.totals_read for one row as the row block."""
    head = [stats["wsum"], stats["count"]]
    return np.concatenate([head, np.atleast_1d(stats["sum"])] + ([[stats["min"], stats["max"]]] if "min" in stats else []))


def spread_values(rng, shape, binades=20):
    """Mixed signs, exponents spread over +-`binades` binades: sums whose bits depend on the order."""
    shape = tuple(np.atleast_1d(shape))
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(1.0, 2.0, size=shape) * np.exp2(rng.integers(-binades, binades + 1, size=shape))


def make_inputs(n, ages, seed=0):
    """What the pure-reduction tests upload (CPU teeth tests and GPU tests alike): values with NaN sprinkled in, 3-row daily weights
    with NaN, zero and negative entries, a weight that is zero everywhere."""
    rng = np.random.default_rng(1000 * n + ages + seed)
    d = {
        "C_rz": spread_values(rng, n), "C_iso_q_ss": spread_values(rng, n),
        "tt_q_ss": spread_values(rng, (n, ages)), "TT_q_ss": spread_values(rng, (n, ages + 1)), "sa_s": spread_values(rng, (n, ages)),
        "C_in": spread_values(rng, (3, n)), "q_ss": np.abs(spread_values(rng, (3, n), 8)), "transp": np.abs(spread_values(rng, (3, n), 8)),
        "cpr_rz": np.zeros((3, n)), "C_q_ss": spread_values(rng, n),
    }
    if n >= 5:
        d["C_iso_q_ss"][rng.integers(0, n, size=max(1, n // 7))] = np.nan
        d["tt_q_ss"][rng.integers(0, n, size=max(1, n // 5)), rng.integers(0, ages, size=max(1, n // 5))] = np.nan
        d["tt_q_ss"][n // 2] = np.nan                                  # a whole row
        for r in range(3):
            k = rng.permutation(n)[:max(3, n // 4)]
            d["q_ss"][r, k[0::3]] = 0.0
            d["q_ss"][r, k[1::3]] = np.nan
            d["q_ss"][r, k[2::3]] = -d["q_ss"][r, k[2::3]]
    return d


ITEMS = ("C_rz", ("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), ("TT_q_ss", "q_ss"), "sa_s", "C_in", ("C_in", "transp"),
         ("tt_q_ss", "transp"), ("C_q_ss", "cpr_rz"))
DAILY = ("C_in", "q_ss", "transp", "cpr_rz")


def masks(n):
    """none, every third cell, one that empties whole runs of 256 (the first and every other one after it), a single cell"""
    c = np.arange(n)
    out = {"none": None, "third": c % 3 == 0, "runs": (c // 256) % 2 == 1 if n > 256 else c >= n, "one": c == n // 2}
    if not out["runs"].any():
        out["runs"] = c == n - 1
    return out


def want_row(d, items, mask, day):
    """{item: block} for a record with `day` (a negative one: no daily row)."""
    out = {}
    r = day % 3 if day >= 0 else None
    for it in items:
        v, w = (it, None) if isinstance(it, str) else it
        live = day >= 0 or (w is None and v not in DAILY)
        val = d[v][r if r is not None else 0] if v in DAILY else d[v]
        wt = None if w is None else d[w][r if r is not None else 0]
        out[v if w is None else f"{v}_by_{w}"] = item_block(val, wt, mask, live)
    return out
