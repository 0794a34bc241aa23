"""lash_tree_build_nj (csrc/dist_nj.hip) through the ABI on synthetic matrices: the records (a, b, and the 64 bits of both lengths) must
equal the model's (nj_model.py) exactly.

Sizes.  The kernels' widths (dist_nj.hip): the wave of 64 inside both reductions; NJ_SCAN_THREADS = NJ_UPDATE_THREADS = 256 (one thread
per slot; a scan workgroup strides the columns above a row's diagonal two at a time, 512 per sweep, so row 0 takes a second sweep from
n = 514 on); NJ_SCAN_GRID = 1 024 (workgroups of a scan launch: rows 0 .. n - 2 have columns above them, so from n = 1 026 on a workgroup
takes a second row); NJ_SELECT_THREADS = 1 024 (one workgroup reduces the scan's partial keys).  Hence 2, 3, 4 and 5, one below, at and
one above 64, 256, 512 (and 514), 1 024 (and 1 026), and 1 030 as the size beyond all.  Both parities of n occur, so rows start on both
alignments of the 16-byte loads."""
import numpy as np
import pytest

import nj_model as NJ
import tree_model as T
from test_gpu_tree import _matrix

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 514, 1023, 1024, 1025, 1026, 1030)
KINDS = ("uniform", "eighths", "equal", "duplicates", "saturated", "f32", "additive")
LARGE_KINDS = ("uniform", "saturated", "additive")               # above n = 257: the model costs seconds at n ~ 1 000


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


def _build(ctx, d, blocks=None):
    n = d.shape[0]
    t = T.Tree(ctx, n)
    try:
        for r0, r1 in blocks if blocks is not None else [(0, n)]:
            t.set_rows(r0, r1, d)
        return NJ.njbuild(t)
    finally:
        t.free()


CASES = [(n, kind) for n in SIZES for kind in KINDS if n <= 257 or kind in LARGE_KINDS]


@pytest.mark.parametrize("n,kind", CASES)
def test_joins_equal_the_model_bit_for_bit(ctx, n, kind):
    seed = 1000 * n + KINDS.index(kind)
    d, truth = NJ.additive(n, seed) if kind == "additive" else (_matrix(n, kind, seed), None)
    want = NJ.joins(d)
    got, stats = _build(ctx, d)
    assert NJ.bits(got) == NJ.bits(want), (n, kind)
    assert stats == dict(steps=n - 1, rescanned_rows=0, bytes=8 * n * n)
    assert sorted(x for m in got for x in m[:2]) == list(range(2 * n - 2)) and got[-1][3] == 0.0
    if truth is not None:                                                       # something other than the rule restated
        assert NJ.splits(n, got) == truth


@pytest.mark.parametrize("n", [5, 65, 257])
def test_set_rows_in_any_split_and_order(ctx, n):
    d = _matrix(n, "eighths" if n == 65 else "uniform", 77 + n)
    d[np.diag_indices(n)] = np.arange(n) / 7.0                                  # the diagonal is stored as given and never read
    rng = np.random.default_rng(n)
    cuts = sorted(set([0, n] + rng.integers(1, n, 6).tolist()))
    uneven = list(zip(cuts[:-1], cuts[1:]))
    rng.shuffle(uneven)
    splits = {"one call": [(0, n)], "row by row": [(r, r + 1) for r in range(n)], "row by row, backwards": [(r, r + 1) for r in range(n)][::-1],
              "uneven blocks out of order": uneven}
    want = NJ.bits(NJ.joins(d))
    block = d.copy()
    block[np.triu_indices(n, 1)] = np.nan                                       # everything above the triangle is poisoned
    for what, blocks in splits.items():
        got, _ = _build(ctx, block, blocks)
        assert NJ.bits(got) == want, what


def test_einval_cases(ctx):
    n = 40
    d = _matrix(n, "uniform", 3)
    # a missing row
    t = T.Tree(ctx, n)
    t.set_rows(0, 17, d)
    t.set_rows(18, n, d)
    with pytest.raises(T.TreeError) as e:
        NJ.njbuild(t)
    assert e.value.code == -1 and "row 17" in e.value.text
    t.set_rows(17, 18, d)
    got, _ = NJ.njbuild(t)
    assert NJ.bits(got) == NJ.bits(NJ.joins(d))
    # a second build of either kind, and the matrix is gone
    with pytest.raises(T.TreeError) as e:
        NJ.njbuild(t)
    assert e.value.code == -1 and "built" in e.value.text
    with pytest.raises(T.TreeError) as e:
        t.build(T.AVERAGE)
    assert e.value.code == -1 and "built" in e.value.text
    with pytest.raises(T.TreeError):
        t.get_rows(0, 1)
    with pytest.raises(T.TreeError):
        t.set_rows(0, 1, d)
    t.free()
    # a NaN cell and an infinite cell: the message names them
    for value, word, cell in ((np.nan, "NaN", (23, 9)), (np.inf, "not finite", (31, 2)), (-np.inf, "not finite", (5, 4))):
        bad = d.copy()
        bad[cell] = bad[cell[::-1]] = value
        t = T.Tree(ctx, n)
        t.set_rows(0, n, bad)
        with pytest.raises(T.TreeError) as e:
            NJ.njbuild(t)
        assert e.value.code == -1 and "row %d" % cell[0] in e.value.text and "col %d" % cell[1] in e.value.text and word in e.value.text
        t.free()
    # the linkage builds order an infinite distance like any other, as before
    bad = d.copy()
    bad[31, 2] = bad[2, 31] = np.inf
    t = T.Tree(ctx, n)
    t.set_rows(0, n, bad)
    got, _ = t.build(T.SINGLE)
    assert T.bits(got) == T.bits(T.merges(bad, T.SINGLE))
    t.free()


def test_n_0_and_1(ctx):
    for n in (0, 1):
        t = T.Tree(ctx, n)
        if n:
            t.set_rows(0, 1, np.zeros((1, 1)))
        got, stats = NJ.njbuild(t)
        assert got == [] and stats == dict(steps=0, rescanned_rows=0, bytes=8 * n * n)
        t.free()
