"""lash_tree_* (csrc/dist_tree.hip) through the ABI on synthetic matrices: the merges (a, b, height bits, size) must equal the model's
(tree_model.py) exactly, for all three linkages.

Sizes.  The kernels' widths (dist_tree.hip): TREE_UPDATE_THREADS = TREE_RESCAN_THREADS = 256 (one thread per slot; one workgroup per
rescanned row, striding its columns by 256), the wave of 64 inside both reductions, TREE_RESCAN_GRID = 512 (workgroups of a rescan
launch: above it a workgroup takes more than one listed row, the first fill lists every row), TREE_SELECT_THREADS = 1024 (one
workgroup strides the rows by 1 024).  Hence one below, at and one above 64, 256, 512 and 1 024, and 1 030 as the size beyond all."""
import numpy as np
import pytest

import tree_model as T

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1030)
KINDS = ("uniform", "eighths", "equal", "duplicates", "saturated", "f32")


def _symmetric(upper):
    d = np.triu(upper, 1)
    return d + d.T


def _matrix(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return _symmetric(rng.random((n, n)))
    if kind == "eighths":                                    # multiples of 1/8: many ties, every average exact or not at random
        return _symmetric(rng.integers(0, 9, (n, n)) / 8.0)
    if kind == "equal":
        return _symmetric(np.full((n, n), 0.3))
    if kind == "duplicates":                                 # blocks of exact duplicates (d = 0, identical rows) among random others
        proto = rng.integers(0, max(2, (2 * n) // 3), n)
        base = _symmetric(rng.random((n, n)))
        return base[np.ix_(proto, proto)]
    if kind == "saturated":                                  # 1.0 everywhere except within a few close families
        fam = np.where(rng.random(n) < 0.4, rng.integers(0, max(1, n // 12) + 1, n), -1 - np.arange(n))
        close = _symmetric(rng.random((n, n)) * 0.05)
        return np.where(fam[:, None] == fam[None, :], close, 1.0) * (1 - np.eye(n))
    if kind == "f32":                                        # f32 values widened to f64
        return _symmetric(rng.random((n, n), np.float32).astype(np.float64))
    raise ValueError(kind)


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


def _build(ctx, d, linkage, blocks=None):
    n = d.shape[0]
    t = T.Tree(ctx, n)
    try:
        for r0, r1 in blocks if blocks is not None else [(0, n)]:
            t.set_rows(r0, r1, d)
        return t.build(linkage)
    finally:
        t.free()


# (all entries equal, where every row's nearest slot is the one just merged, at N <= 257 only)
CASES = [(n, kind) for n in SIZES for kind in KINDS if kind != "equal" or n <= 257]


@pytest.mark.parametrize("n,kind", CASES)
def test_merges_equal_the_model_bit_for_bit(ctx, n, kind):
    d = _matrix(n, kind, 1000 * n + KINDS.index(kind))
    for name, linkage in T.LINKAGES.items():
        want = T.merges(d, linkage)
        got, stats = _build(ctx, d, linkage)
        assert T.bits(got) == T.bits(want), (n, kind, name)
        assert stats["steps"] == max(n - 1, 0) and stats["bytes"] == 8 * n * n
        if n > 1:
            assert stats["rescanned_rows"] >= n                                 # the first fill
            heights = [m[2] for m in got]
            assert name == "average" or all(a <= b for a, b in zip(heights, heights[1:]))   # (min / max are exact: sorted merges)
            assert got[-1][3] == n and sorted(x for m in got for x in m[:2]) == list(range(2 * n - 2))
        if n > 1 and (name == "single" or (kind == "equal" and name == "complete")):
            # nothing moves away from a row whose nearest slot was merged (min never grows; max of equals is the same number; an
            # average of equals may round away): only the merged row itself is rescanned
            assert stats["rescanned_rows"] == n + (n - 1)


def test_a_row_whose_nearest_moved_away_is_rescanned(ctx):
    """complete linkage on random distances: a row whose nearest slot was merged sees it move away, and its minimum is somewhere else"""
    d = _matrix(300, "uniform", 5)
    got, stats = _build(ctx, d, T.COMPLETE)
    assert T.bits(got) == T.bits(T.merges(d, T.COMPLETE))
    assert stats["rescanned_rows"] > 300 + 299


@pytest.mark.parametrize("n", [5, 65, 257, 600])
def test_set_rows_in_any_split_and_order(ctx, n):
    d = _matrix(n, "eighths" if n == 65 else "uniform", 77 + n)
    d[np.diag_indices(n)] = np.arange(n) / 7.0                                  # the diagonal is stored as given
    rng = np.random.default_rng(n)
    cuts = sorted(set([0, n] + rng.integers(1, n, 6).tolist()))
    uneven = list(zip(cuts[:-1], cuts[1:]))
    rng.shuffle(uneven)
    splits = {"one call": [(0, n)], "row by row": [(r, r + 1) for r in range(n)], "row by row, backwards": [(r, r + 1) for r in range(n)][::-1],
              "uneven blocks out of order": uneven}
    want = T.bits(T.merges(d, T.AVERAGE))
    for what, blocks in splits.items():
        t = T.Tree(ctx, n)
        for r0, r1 in blocks:
            # everything above the triangle is poisoned: the entry must not read it
            block = d.copy()
            block[np.triu_indices(n, 1)] = np.nan
            t.set_rows(r0, r1, block)
        full = np.concatenate([t.get_rows(0, n // 2), t.get_rows(n // 2, n)])
        assert np.array_equal(full, d), what                                    # the full symmetric matrix: the mirror is there
        got, stats = t.build(T.AVERAGE)
        t.free()
        assert T.bits(got) == want, what


def test_einval_cases(ctx):
    n = 40
    d = _matrix(n, "uniform", 3)
    # a missing row
    t = T.Tree(ctx, n)
    t.set_rows(0, 17, d)
    t.set_rows(18, n, d)
    with pytest.raises(T.TreeError) as e:
        t.build(T.AVERAGE)
    assert e.value.code == -1 and "row 17" in e.value.text
    t.set_rows(17, 18, d)
    # a bad linkage does not consume the matrix
    for bad in (3, -1, 99):
        with pytest.raises(T.TreeError) as e:
            t.build(bad)
        assert e.value.code == -1 and "linkage" in e.value.text
    got, _ = t.build(T.SINGLE)
    assert T.bits(got) == T.bits(T.merges(d, T.SINGLE))
    # a second build, and the matrix is gone
    with pytest.raises(T.TreeError) as e:
        t.build(T.SINGLE)
    assert e.value.code == -1 and "built" in e.value.text
    with pytest.raises(T.TreeError):
        t.get_rows(0, 1)
    with pytest.raises(T.TreeError):
        t.set_rows(0, 1, d)
    t.free()
    # a NaN cell: the message names it
    bad = d.copy()
    bad[23, 9] = bad[9, 23] = np.nan
    t = T.Tree(ctx, n)
    t.set_rows(0, n, bad)
    with pytest.raises(T.TreeError) as e:
        t.build(T.AVERAGE)
    assert e.value.code == -1 and "row 23" in e.value.text and "col 9" in e.value.text and "NaN" in e.value.text
    t.free()
    # rows beyond n
    t = T.Tree(ctx, n)
    with pytest.raises(T.TreeError) as e:
        t._check(t._lib.lash_tree_set_rows(ctx._h, t._h, 0, n + 1, d.ctypes.data))
    assert e.value.code == -1
    t.free()


def test_n_0_and_1(ctx):
    for n in (0, 1):
        t = T.Tree(ctx, n)
        if n:
            t.set_rows(0, 1, np.zeros((1, 1)))
        got, stats = t.build(T.AVERAGE)
        assert got == [] and stats["steps"] == 0
        t.free()
