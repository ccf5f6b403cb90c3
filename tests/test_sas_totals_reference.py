"""CPU: the host restatement of the SAS totals recorder (tests/sas_totals_reference.py) against exact sums, and the teeth of the inputs
that the GPU tests (tests/test_hip_sas_totals.py) upload."""
import math

import numpy as np
import pytest

import sas_totals_reference as R

EPS = 2.0 ** -52


def terms_of(d, v, w, row=1):
    """The terms t of item (v, w) at daily row `row` without a mask, skipped ones as +0.0, and what counts."""
    val = d[v][row] if v in R.DAILY else d[v]
    wt = None if w is None else d[w][row]
    e = R.eligible(val.shape[0], wt)
    with np.errstate(invalid="ignore"):
        t = val if wt is None else (val * wt if val.ndim == 1 else val * wt[:, None])
    keep = (e if val.ndim == 1 else e[:, None]) & ~np.isnan(val)
    return np.where(keep, t, 0.0)


@pytest.mark.parametrize("n,ages", [(5, 30), (300, 63), (300, 1000), (65537, 30)])
def test_both_orders_agree_with_fsum_within_the_derivable_bound(n, ages):
    """Any order of n floating-point additions is within n * 2^-52 * sum|t| of the exact sum."""
    d = R.make_inputs(n, ages)
    t = terms_of(d, "C_iso_q_ss", "q_ss")
    blk = R.item_block(d["C_iso_q_ss"], d["q_ss"][1])
    assert abs(blk[2] - math.fsum(t)) <= n * EPS * math.fsum(np.abs(t))
    assert blk[1] == np.count_nonzero(R.eligible(n, d["q_ss"][1]) & ~np.isnan(d["C_iso_q_ss"]))
    assert abs(blk[0] - math.fsum(np.where(t != 0, d["q_ss"][1], 0.0))) <= n * EPS * blk[0]
    for v, w in (("tt_q_ss", "q_ss"), ("sa_s", None)):
        t = terms_of(d, v, w)
        got = R.item_block(d[v], None if w is None else d[w][1])[2:]
        for a in (0, ages // 2, ages - 1):
            assert abs(got[a] - math.fsum(t[:, a])) <= n * EPS * math.fsum(np.abs(t[:, a])), (v, a)


@pytest.mark.parametrize("n,ages", [(255, 30), (256, 64), (257, 255), (300, 30), (300, 1000), (65537, 30)])
def test_the_inputs_have_teeth(n, ages):
    """For what the GPU tests upload, the restated sums differ in bits from np.sum and from the other rule: a kernel that summed in
    another order, or fused the product into the sum, would not pass at tolerance zero."""
    d = R.make_inputs(n, ages)
    # width 1: one sum is one number, and a single number can agree by chance; of the set's width-1 sums (3 daily rows) some differ
    w1 = [terms_of(d, v, w, row) for row in range(3) for v, w in (("C_rz", None), ("C_iso_q_ss", "q_ss"), ("C_in", None), ("C_in", "transp"))]
    w1 += [np.where(R.eligible(n, d["q_ss"][row]) & ~np.isnan(d["C_iso_q_ss"]), d["q_ss"][row], 0.0) for row in range(3)]
    assert any(not R.same_bits(R.tree_reduce(t), np.sum(t)) for t in w1)
    assert any(not R.same_bits(R.tree_reduce(t), R.run_sums(t[:, None])[0]) for t in w1)
    for v, w in (("tt_q_ss", "q_ss"), ("TT_q_ss", "q_ss"), ("sa_s", None)):
        t = terms_of(d, v, w)
        runs = R.run_sums(t)
        other = np.array([R.tree_reduce(t[:, a]) for a in range(t.shape[1])])
        # (np.sum of one age class as a vector is numpy's pairwise sum; over axis 0 of the matrix it would itself run left to right)
        plain = np.array([np.sum(np.ascontiguousarray(t[:, a])) for a in range(t.shape[1])])
        assert (runs.view(np.uint64) != plain.view(np.uint64)).any(), v
        assert (runs.view(np.uint64) != other.view(np.uint64)).any(), v
    # a contracted build: level 1 of the age rule with acc = fma(v, w, acc), one rounding, emulated exactly; the further levels as they are
    from fractions import Fraction

    val, wt = d["tt_q_ss"][:, :8], d["q_ss"][1]
    keep = R.eligible(n, wt)[:, None] & ~np.isnan(val)
    partials = []
    for r in range(0, n, 256):
        acc = [0.0] * val.shape[1]
        for c in range(r, min(r + 256, n)):
            for a in range(val.shape[1]):
                if keep[c, a]:
                    acc[a] = float(Fraction(acc[a]) + Fraction(val[c, a]) * Fraction(wt[c]))
        partials.append(acc)
    fused = R.run_sums(np.array(partials)) if len(partials) > 1 else np.array(partials[0])
    assert (fused.view(np.uint64) != R.run_sums(terms_of(d, "tt_q_ss", "q_ss")[:, :val.shape[1]]).view(np.uint64)).any()


def test_right_padding_with_skipped_cells_changes_nothing():
    d = R.make_inputs(300, 30)
    for pad in (1, 212, 213, 1000):
        mask = np.arange(300 + pad) < 300
        for v, w in (("C_iso_q_ss", "q_ss"), ("tt_q_ss", "q_ss"), ("sa_s", None), ("C_rz", None)):
            val = np.concatenate([d[v], R.spread_values(np.random.default_rng(pad), (pad,) + d[v].shape[1:])])
            wt = None if w is None else np.concatenate([d[w][1], np.ones(pad)])
            assert R.same_bits(R.item_block(val, wt, mask), R.item_block(d[v], None if w is None else d[w][1])), (v, pad)


@pytest.mark.parametrize("n", [256, 257, 65536, 65537])
def test_run_boundaries(n):
    """The age rule written cell by cell (one run: a plain left-to-right sum; 257 cells: run 0 + the last cell; 65 537: three levels),
    and the width-1 rule's ragged last tile."""
    rng = np.random.default_rng(n)
    x = R.spread_values(rng, (n, 2))

    def level(x):
        out = []
        for r in range(0, x.shape[0], 256):
            acc = np.zeros(x.shape[1])
            for row in x[r:r + 256]:
                acc = acc + row
            out.append(acc)
        return np.array(out)

    y, levels = x, 0
    while True:
        y, levels = level(y), levels + 1
        if y.shape[0] == 1:
            break
    assert levels == {256: 1, 257: 2, 65536: 2, 65537: 3}[n]
    assert R.same_bits(R.run_sums(x), y[0])
    # width 1: the last tile's missing cells are the identity
    v = x[:, 0]
    full = np.concatenate([v, np.zeros(-n % 256)])
    assert R.same_bits(R.tree_reduce(v), R.tree_reduce(full))
    assert R.tree_reduce(v, "min") == v.min() and R.tree_reduce(v, "max") == v.max()


def test_counting_rules():
    nan, inf = np.nan, np.inf
    v = np.array([1.0, nan, 3.0, 4.0, 5.0, 6.0])
    w = np.array([2.0, 2.0, 0.0, nan, -1.0, 0.5])
    assert list(R.item_block(v, w)) == [2.5, 2.0, 5.0, 1.0, 6.0]
    assert list(R.item_block(v)) == [5.0, 5.0, 19.0, 1.0, 6.0]
    assert list(R.item_block(v, w, mask=[0, 1, 1, 1, 1, 0])) == [0.0, 0.0, 0.0, inf, -inf]
    assert list(R.item_block(v, w, live=False)) == [0.0, 0.0, 0.0, inf, -inf]
    V = np.array([[1.0, nan], [nan, nan], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [inf, 1.0]])
    assert list(R.item_block(V, w)) == [4.5, 3.0, inf, 0.5]          # wsum, count over the ELIGIBLE cells 0, 1, 5
    assert list(R.item_block(V)) == [6.0, 6.0, inf, 19.0]
    assert not np.signbit(R.item_block(V, w, live=False)).any()
