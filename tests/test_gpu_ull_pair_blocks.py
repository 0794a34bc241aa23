"""Row blocks of lash_sketch_set_pair_block for UltraLogLog — blocks that start at r0 > 0, span several tiles, or are cut by the
triangle's early return — against the 60-digit reference of tests/ullref.py, cell by cell.  test_gpu_ull_pairs.py checks the VALUES
of the three kernels (ull_fgra_fast_kernel, 16 x 16 tiles; ull_pairs_kernel<false>, p <= 15, 16 x 16; ull_pairs_kernel<true>,
p >= 16, 8 x 16) on one tile through the whole-matrix entry; this file checks WHERE they put them: tile rows relative to the block's
first row, tile columns absolute, tiles wholly above the diagonal skipped by each kernel with its own tile height, and the fix-up launch
of the histogram kernel redoing only tiles in which the fast kernel left a NaN.

Images and reference.  83 images (five column tiles and one of 3; partial row tiles for 8 and for 16), each a copy of one of K = 12
kinds taken from U.regime_images(p), see kinds().  kind[i] is drawn from a fixed-seed RNG among the kinds that images i +- 1, i +- 8
and i +- 16 do not have; six images are PINNED (below).  The estimate of cell (i, j) is the reference (U.fgra_ref / U.ml_ref of
U.merge_hist) of kinds (kind[i], kind[j]): 78 kind pairs per p, gathered into 83 x 83 matrices, compared by test_gpu_ull_pairs._worst
under U.fgra_tol(p) / U.ml_tol(p), 0 and +inf exactly.  Cells above the diagonal of a triangular block are undefined and never read.

Preconditions, asserted by reference(p) without a GPU (in tests/: PYTHONPATH=.. python -c "import test_gpu_ull_pair_blocks as T;
T.reference(10); T.reference(16)"):
  distinct values    The estimates are functions of the merged histogram, and kind pairs can share one: (X, empty) merges to X like
                     (X, X), flat 255 swallows every partner, and a flat image of update value 8 swallows a small-range one.  The 78
                     kind pairs fall into 36 histogram classes at p = 10 and 38 at p = 16; "all 78 different" cannot be had together
                     with an empty and a flat kind.  Asserted instead: two kind pairs' FGRA references differ by more than
                     1e6 * U.fgra_tol(p), relatively, exactly when their histograms differ (the smallest gap is 1.05e6 tolerances at
                     p = 16, 2e9 at p = 10), their ML references then by more than 10 * U.ml_tol(p) (smallest gap 20 and 23 tolerances;
                     1e6 ML tolerances would be a factor of 48 at p = 10.  Ten is enough: a cell that carries another pair's estimate,
                     itself within one tolerance of that pair's reference, stays at least eight away), the only exact 0 is
                     empty x empty and the only +inf the flat-255 class.  So a cell that carries the value of another histogram
                     class cannot pass, and the next two conditions are stated on values that are this far apart:
  neighbours         kind[i] != kind[i +- 1], kind[i +- 8], kind[i +- 16].  For s in (1, 8, 16), rows i and i + s differ, for FGRA and
                     for ML, in a printed cell that every triangle holding both has (a column j <= i), and columns j and j + 1,
                     j and j + 16 in a row of every rectangle: a one-row, one-tile or one-column-tile slip changes an expected value.
  mixed tiles        For every block tested, on the fast kernel's 16 x 16 grid and on the histogram kernel's (16 x 16 at p = 10,
                     8 x 16 at p = 16), both anchored at the block's r0: every tile that is not wholly above the diagonal holds a
                     printed pair the fast kernel finishes and a pair that it leaves as NaN (`regular` of test_gpu_ull_pairs._want) —
                     a printed one wherever the tile prints two cells or more.  SEED was chosen for this.  (16, 16), (32, 32), (48, 48),
                     (64, 64), (80, 80) are the ONLY printed cell of a tile of the triangles (15, 17) and (17, 83): those five images are
                     pinned to the flat odd / flat even / half-and-half kinds, and image 15 to a saturated one ((15, 16) is the only
                     other cell of its tile).  Two tiles cannot mix: the blocks rows (82, 83) x 1 column and x 17 columns end in a tile
                     of one cell; they are exempt, and asserted to be the only ones.

Leftover bytes.  The context keeps one statistics buffer and reuses it, so a skipped cell could hold the right answer of an earlier
call, and the fix-up launch decides by isnan() on what it finds.  Every triangular block is therefore preceded, in the same context, by
the block of the same shape (same cell addresses) on the OTHER set, image i replaced by the image of kind OTHER[kind[i]]: a map, not a
permutation (nothing may map onto flat 255, whose pairs are all +inf), found by search, under which every one of the 83 x 83 cells
holds an estimate apart (as above, FGRA and ML) from the one it holds in the set; asserted.  The other set's blocks are checked too.
The same context and not a fresh one, because that is what a `lash dist` run is: one context, one buffer, block after block.

Fast path off: one child process with LASH_ULL_NO_FAST=1 (read once per process) for the triangles (5, 83) and (17, 83) at both p.
Filters: pair_block_within over the same sets, against test_gpu_dist_within._dense / _want.

CPU time of the references: 0.3 to 1.3 s per p depending on the host (78 kind pairs, FGRA and ML; -s prints it), 4 s for both p with
all preconditions.  On an MI355X: the file 6.6 s; test_fast_path_off 2.4 s (the child process), test_blocks 0.54 s (p = 16, fgra),
0.44 s (p = 10, fgra, with the references), 0.13 s and 0.01 s for ml, test_filters_over_the_same_set 0.2 s at p = 16 and 0.01 s at
p = 10, test_two_sets_query_on_the_device 0.02 s.

Mutations, each tried on a scratch build against this file and the UltraLogLog tests of test_gpu_ull_pairs.py, test_gpu_sketch_set.py
and test_gpu_dist_within.py (test_gpu_pair_blocks.py has none; what (a) does to HyperMinHash and HyperLogLog is in its docstring):
  (a) tile_above_diagonal with >= for >          test_blocks (all four; first at (17, 83), cell (32, 32): inf or another value),
                                                 test_fast_path_off; no older UltraLogLog test
  (b) the fast kernel's early return with UQ / 2 test_blocks[10-fgra] ((5, 83), cell (16, 11)), test_blocks[16-fgra],
                                                 test_fast_path_off; also test_gpu_sketch_set's test_row_blocks_...[ull-11-fgra]
  (c) ull_pairs_kernel's with 2 * TR             nothing, as expected: more tiles are computed, none lost
      ull_pairs_kernel's with TR / 2             test_blocks (all four: printed cells left NaN or stale, (5, 83) from (16, 16), p = 16
                                                 (17, 83) from (32, 32)), test_fast_path_off; also test_row_blocks_...[ull-11-fgra, -ml]
  (d) no early return in the fix-up launch       nothing, as expected: it only redoes tiles nobody reads
  (e) rimg without r0 * stride for ULL           all 17 tests of this file; also test_gpu_ull_pairs' test_resident_set (4) and
                                                 test_row_blocks_...[ull-11-fgra, -ml]
  (f) the fix-up's isnan(*dst) dropped           no test of this file (the histogram kernel's value of a finished pair is within the
                                                 tolerance too); test_gpu_ull_pairs' test_fast_path_on_and_off[9, 16] fails, as before
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import test_gpu_dist_within as W
import ullref as U
from test_gpu_ull_pairs import _tiles_are_mixed, _want, _worst

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 83
K = 12
SEED = 474
OTHER = (1, 9, 1, 5, 10, 11, 2, 0, 5, 10, 6, 0)                                            # kind -> kind of the same position in the other set
EMPTY, FLAT255 = 5, 8
# (16, 16), (32, 32), ... are the only printed cell of a tile of the triangles (15, 17) and (17, 83), and (15, 16) the only other cell of
# the first: the former must be pairs the fast kernel finishes (flat odd / even, half-and-half), the latter not (saturated)
PINNED = {15: 3, 16: 6, 32: 7, 48: 9, 64: 6, 80: 7}
P_VALUES = (10, 16)
TRIANGLES = ((0, 83), (5, 83), (7, 9), (8, 24), (15, 17), (16, 48), (17, 83), (23, 25), (82, 83))
SEAM_TRIANGLES = {10: (), 16: ((40, 83),)}                               # r0 % 16 == 8 ((8, 24) is one too): 8-row tiles inside 16-row tiles
RECTANGLES = ((0, 83), (5, 40), (82, 83))
RECT_COLS = (1, 15, 16, 17, 83)
TWO_SETS_ROWS = (9, 70)
NO_FAST_TRIANGLES = ((5, 83), (17, 83))
WITHIN_TRIANGLES = ((0, 83), (17, 83), (82, 83))
WITHIN_D = (0.0, 0.05, 0.3, 1.0)
ONE_CELL_TILES = {(82, 83, 1, False), (82, 83, 17, False)}               # blocks that end in a tile of one cell: nothing to mix
FGRA_APART, ML_APART = 1e6, 10.0                                         # in tolerances (module docstring)


def kinds(p):
    """[12, 8 + 2^p] from U.regime_images(p): regular, small-range n = m/2 and 2m, saturated mu = 0.2 and 0.7, flat 0 (the empty image),
    flat odd, flat even, flat 255, half-and-half, two more regular ones.  (Its small-range n = 3 is left out: three registers away from the
    empty image, so that at p = 16 the two cannot be told apart by a million tolerances.)"""
    ref, qry = U.regime_images(p)
    out = np.concatenate([ref[:1], ref[2:], qry[[2, 8]]])
    assert len(out) == K and not U.regs_of(out[EMPTY]).any() and (U.regs_of(out[FLAT255]) == 255).all()
    assert len({o.tobytes() for o in out}) == K
    return out


def kind_of(seed=SEED):
    rng = np.random.default_rng(seed)
    u = rng.random(N)
    kind = np.empty(N, np.int64)
    for i in range(N):
        banned = {int(kind[i - s]) for s in (1, 8, 16) if i >= s} | {PINNED[i + s] for s in (1, 8, 16) if i + s in PINNED}
        free = [k for k in range(K) if k not in banned]
        kind[i] = PINNED.get(i, free[int(u[i] * len(free))])
    return kind


def members(kind):
    """the two-set test's 21 query members: a fixed-seed draw, the last image and an empty one among them"""
    m = np.random.default_rng(21).permutation(N)[:21]
    if N - 1 not in m:
        m[0] = N - 1
    if not (kind[m] == EMPTY).any():
        m[1] = np.flatnonzero(kind == EMPTY)[0]
    assert len(set(m.tolist())) == 21
    return m


def blocks(p):
    """(r0, r1, n_cols, triangle) of every block of test_blocks"""
    for r0, r1 in TRIANGLES + SEAM_TRIANGLES[p]:
        yield r0, r1, r1, True
    for r0, r1 in RECTANGLES:
        for nc in RECT_COLS:
            yield r0, r1, nc, False


def unmixed_tiles(regular, r0, r1, n_cols, triangle, tile_rows):
    """the tiles of block rows [r0, r1) x `regular`'s first n_cols columns (regular: [N, n_qry], rows by set index), tile_rows x 16 and
    anchored at r0, that are not wholly above the diagonal and lack a printed regular pair or a non-regular one"""
    bad = []
    rows = np.arange(r0, r1)
    for t0 in range(r0, r1, tile_rows):
        for q0 in range(0, n_cols, 16):
            if triangle and q0 > t0 + tile_rows - 1:                     # tile_above_diagonal, restated
                continue
            rr, cc = rows[(rows >= t0) & (rows < t0 + tile_rows)], np.arange(q0, min(q0 + 16, n_cols))
            reg = regular[np.ix_(rr, cc)]
            printed = cc[None, :] <= rr[:, None] if triangle else np.ones(reg.shape, bool)
            nan_among = printed if printed.sum() >= 2 else np.ones(reg.shape, bool)
            if not ((reg & printed).any() and (~reg & nan_among).any()):
                bad.append((t0, q0))
    return bad


def _apart(vals, margin):
    """[K, K, K, K] bool: whether the references of kind pairs (a, b) and (c, d) differ by more than `margin`, relatively; an exact 0 or
    +inf is apart from everything but itself"""
    v = vals.reshape(-1)
    a, b = v[:, None], v[None, :]
    exact = (a == 0) | np.isinf(a) | (b == 0) | np.isinf(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(a - b) / np.maximum(a, b)
    return np.where(exact, a != b, rel > margin).reshape(K, K, K, K)


_TABLES = {}


def kind_tables(p):
    """dict(img [K, bytes]; fgra, ml, regular, hist_class [K, K]; fgra_apart, ml_apart [K, K, K, K]) with the `distinct values`
    precondition asserted; made once per p"""
    if p in _TABLES:
        return _TABLES[p]
    t0 = time.process_time()
    img = kinds(p)
    f, ml, regular = _want(p, img, img)
    hists = {(a, b): U.merge_hist(U.regs_of(img[a]), U.regs_of(img[b])).tobytes() for a in range(K) for b in range(K)}
    ids = {h: n for n, h in enumerate(sorted(set(hists.values())))}
    cls = np.array([[ids[hists[a, b]] for b in range(K)] for a in range(K)])
    print("\n[reference] p = %d: %d kind pairs in %d histogram classes, %.2f s of CPU" % (p, K * (K + 1) // 2, len(ids), time.process_time() - t0))
    assert not np.isnan(f).any() and not np.isnan(ml).any()
    assert np.array_equal(f, f.T) and np.array_equal(ml, ml.T) and np.array_equal(cls, cls.T)
    same = cls[:, :, None, None] == cls[None, None, :, :]
    fa, ma = _apart(f, FGRA_APART * U.fgra_tol(p)), _apart(ml, ML_APART * U.ml_tol(p))
    assert np.array_equal(fa, ~same), ("fgra", p, np.argwhere(fa == same)[:4])     # apart exactly when the histograms differ
    assert not (ma & same).any()
    for v in (f, ml):
        assert (v == 0).sum() == 1 and v[EMPTY, EMPTY] == 0                        # the only exact 0, the only +inf class
        assert np.array_equal(np.isinf(v), cls == cls[FLAT255, FLAT255]) and np.isinf(v[FLAT255]).all()
    out = dict(img=img, fgra=f, ml=ml, regular=regular, hist_class=cls, fgra_apart=fa, ml_apart=ma)
    _TABLES[p] = out
    return out


def set_failures(p, kind, other=OTHER, first_only=False):
    """what the set `kind` (and the other set, kind -> other[kind]) lacks of the `neighbours`, `mixed tiles` and `leftover bytes`
    preconditions, as a list of tuples; empty when all hold"""
    t = kind_tables(p)
    bad = []
    regular = t["regular"][np.ix_(kind, kind)]
    one_cell = set()
    for blk in blocks(p):
        for g in (16, 8 if p >= 16 else 16):
            um = unmixed_tiles(regular, *blk, g)
            if blk[1] - blk[0] == 1 and blk[2] % 16 == 1 and not blk[3]:
                one_cell.add(blk)
                um = [x for x in um if x != (blk[0], blk[2] - 1)]
            if um:
                bad.append(("unmixed", blk, g, um))
                if first_only:
                    return bad
    if one_cell != ONE_CELL_TILES:
        bad.append(("one-cell tiles", one_cell))
    m = members(kind)
    for g in (16, 8 if p >= 16 else 16):
        um = unmixed_tiles(regular[:, m], *TWO_SETS_ROWS, len(m), False, g)
        if um:
            bad.append(("unmixed, two sets", g, um))
    if not _tiles_are_mixed(regular):                                     # (the whole matrix, anchored at 0, as the sibling file asks)
        bad.append(("unmixed", "whole"))
    for s in (1, 8, 16):
        if not (kind[s:] != kind[:-s]).all():
            bad.append(("neighbour kinds", s))
    okind = np.array(other)[kind]
    for est in ("fgra", "ml"):
        apart = t[est + "_apart"]
        for s in (1, 8, 16):
            for i in range(N - s):
                j = np.arange(i + 1)                                      # (the printed cells the two rows share)
                if not apart[kind[i], kind[j], kind[i + s], kind[j]].any():
                    bad.append(("rows", est, i, i + s))
        for r0, r1 in RECTANGLES + (TWO_SETS_ROWS,):
            i = np.arange(r0, r1)
            for s in (1, 16):
                for j in range(N - s):
                    if r1 - r0 > 1 and not apart[kind[i], kind[j], kind[i], kind[j + s]].any():
                        bad.append(("columns", est, j, j + s, (r0, r1)))
        same = ~apart[kind[:, None], kind[None, :], okind[:, None], okind[None, :]]
        if same.any():
            bad.append(("other set", est, np.argwhere(same)[:3].tolist()))
    if kind[N - 1] in (EMPTY, FLAT255) or (kind == EMPTY).sum() < 2 or np.flatnonzero(kind == EMPTY)[-1] < 17:
        bad.append(("empty images", ))                                    # (what test_filters_over_the_same_set wants)
    return bad


_REFERENCE = {}


def reference(p):
    """dict(imgs, other, kind, fgra, ml, other_fgra, other_ml, regular): the set, the other set, and [N, N] references and `regular`
    of every cell; asserts the module docstring's preconditions.  Made once per p, read-only."""
    if p in _REFERENCE:
        return _REFERENCE[p]
    t, kind = kind_tables(p), kind_of()
    bad = set_failures(p, kind)
    assert not bad, bad
    okind = np.array(OTHER)[kind]
    here, there = np.ix_(kind, kind), np.ix_(okind, okind)
    out = dict(imgs=t["img"][kind], other=t["img"][okind], kind=kind, fgra=t["fgra"][here], ml=t["ml"][here], regular=t["regular"][here],
               other_fgra=t["fgra"][there], other_ml=t["ml"][there])
    for arr in out.values():
        arr.setflags(write=False)
    _REFERENCE[p] = out
    return out


def _check(got, want, r0, r1, n_cols, triangle, tol, what):
    """every printed cell of rows [r0, r1) x columns [0, n_cols) (want: [N, >= n_cols], rows by set index) through _worst"""
    assert got.shape == (r1 - r0, n_cols) and got.dtype == np.float64, what
    w, g = np.array(want[r0:r1, :n_cols]), np.array(got)
    if triangle:
        above = np.arange(n_cols)[None, :] > np.arange(r0, r1)[:, None]
        w[above] = np.nan                                                 # not asked for
        g[above] = np.nan                                                 # and never read
    lost = np.isnan(g) & ~np.isnan(w)
    assert not lost.any(), (what, "%d printed cells are NaN, first at (row, col) = %s" % (lost.sum(), tuple(np.argwhere(lost)[0] + (r0, 0))))
    return _worst(g, w, tol, what)


def _tol(p, est):
    return U.fgra_tol(p) if est == "fgra" else U.ml_tol(p)


@pytest.mark.parametrize("est", ["fgra", "ml"])
@pytest.mark.parametrize("p", P_VALUES)
def test_blocks(p, est):
    """every triangle, each after the block of the same shape on the other set (itself checked), and every rectangle"""
    import lash_amd
    ref = reference(p)
    want, other, tol = ref[est], ref["other_" + est], _tol(p, est)
    t0 = time.time()
    with lash_amd.Context(0) as ctx:
        s, z = ctx.sketch_set("ull", p, ref["imgs"]), ctx.sketch_set("ull", p, ref["other"])
        for r0, r1, nc, tri in blocks(p):
            if tri:
                before = z.pair_block(r0, r1, n_cols=nc, triangle=True, estimator=est)["sum_or_union"]
                _check(before, other, r0, r1, nc, True, tol, (p, est, "other set", r0, r1))
            got = s.pair_block(r0, r1, n_cols=nc, triangle=tri, estimator=est)["sum_or_union"]
            _check(got, want, r0, r1, nc, tri, tol, (p, est, r0, r1, nc, tri))
        z.free()
        s.free()
    print("p=%d %s: GPU calls %.2f s" % (p, est, time.time() - t0))


@pytest.mark.parametrize("est", ["fgra", "ml"])
@pytest.mark.parametrize("p", P_VALUES)
def test_two_sets_query_on_the_device(p, est):
    """reference rows (9, 70) against 21 of the images as a second set adopted from device memory: the whole rectangle, and its first
    17 columns"""
    import lash_amd
    import torch
    ref = reference(p)
    m = members(ref["kind"])
    want = np.ascontiguousarray(ref[est][:, m])
    with lash_amd.Context(0) as ctx:
        s = ctx.sketch_set("ull", p, ref["imgs"])
        q_dev = torch.from_numpy(np.ascontiguousarray(ref["imgs"][m])).cuda()
        q = ctx.sketch_set("ull", p, q_dev)
        for nc in (len(m), 17):
            got = s.pair_block(*TWO_SETS_ROWS, qry=q, n_cols=nc, estimator=est)["sum_or_union"]
            _check(got, want, *TWO_SETS_ROWS, nc, False, _tol(p, est), (p, est, "two sets", nc))
        q.free()
        s.free()


CHILD = ("import sys, numpy as np, lash_amd\n"
         "with lash_amd.Context(0) as ctx:\n"
         "    for arg in sys.argv[1:]:\n"
         "        p, path = arg.split(':', 1)\n"
         "        d = np.load(path)\n"
         "        s, z = ctx.sketch_set('ull', int(p), d['imgs']), ctx.sketch_set('ull', int(p), d['other'])\n"
         "        out = {}\n"
         "        for r0, r1 in d['triangles'].tolist():\n"
         "            z.pair_block(r0, r1, n_cols=r1, triangle=True)\n"
         "            out['%d_%d' % (r0, r1)] = s.pair_block(r0, r1, n_cols=r1, triangle=True)['sum_or_union']\n"
         "        np.savez(path + '.out.npz', **out)\n"
         "        z.free()\n"
         "        s.free()\n")


def test_fast_path_off(tmp_path):
    """LASH_ULL_NO_FAST=1 in one child process: the histogram kernel alone on the triangles (5, 83) and (17, 83), p = 10 and 16, FGRA.
    Both routes meet the reference; the cells the fast kernel leaves to the fix-up launch come from the same histogram code on both
    routes: bit-equal."""
    import lash_amd
    args = []
    for p in P_VALUES:
        ref = reference(p)
        np.savez(tmp_path / ("p%d.npz" % p), imgs=ref["imgs"], other=ref["other"], triangles=np.array(NO_FAST_TRIANGLES))
        args.append("%d:%s" % (p, tmp_path / ("p%d.npz" % p)))
    r = subprocess.run([sys.executable, "-c", CHILD] + args, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT, LASH_ULL_NO_FAST="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for p in P_VALUES:
        ref = reference(p)
        slow = np.load(str(tmp_path / ("p%d.npz.out.npz" % p)))
        with lash_amd.Context(0) as ctx:
            s, z = ctx.sketch_set("ull", p, ref["imgs"]), ctx.sketch_set("ull", p, ref["other"])
            for r0, r1 in NO_FAST_TRIANGLES:
                z.pair_block(r0, r1, n_cols=r1, triangle=True)
                fast = s.pair_block(r0, r1, n_cols=r1, triangle=True)["sum_or_union"]
                alone = slow["%d_%d" % (r0, r1)]
                _check(fast, ref["fgra"], r0, r1, r1, True, U.fgra_tol(p), (p, "fast", r0, r1))
                _check(alone, ref["fgra"], r0, r1, r1, True, U.fgra_tol(p), (p, "histogram only", r0, r1))
                left = ~ref["regular"][r0:r1, :r1] & (np.arange(r1)[None, :] <= np.arange(r0, r1)[:, None])
                assert left.sum() > 1000
                assert np.array_equal(fast[left].view(np.uint64), alone[left].view(np.uint64)), (p, r0, r1)
            z.free()
            s.free()


@pytest.mark.parametrize("model,fp32", [(0, False), (1, False), (0, True), (1, True)])
@pytest.mark.parametrize("p", P_VALUES)
def test_filters_over_the_same_set(p, model, fp32):
    """pair_block_within (FGRA, k = 16) on the triangles (0, 83), (17, 83) and (82, 83), each after the same call on the other set:
    exactly the rows, columns and float64 bit patterns of d <= D, d = dist_rows over that block's pair_block statistics with the cells
    above the diagonal replaced by neutral ones (test_gpu_dist_within._dense / _want).  A filter that read a cell above the diagonal —
    a leftover NaN there is a candidate outright — would return a column > row.  empty x empty is NaN under model 0: never kept."""
    import lash_amd
    ref = reference(p)
    empty = np.flatnonzero(ref["kind"] == EMPTY)
    with lash_amd.Context(0) as ctx:
        s, z = ctx.sketch_set("ull", p, ref["imgs"]), ctx.sketch_set("ull", p, ref["other"])
        card, zcard = s.cardinalities("fgra"), z.cardinalities("fgra")
        assert (card[empty] == 0).all() and len(zcard) == N
        for r0, r1 in WITHIN_TRIANGLES:
            d = W._dense(s, card, "ull", p, 16, model, fp32, r0, r1, r1, True)
            rows = np.arange(r0, r1)
            both_empty = np.isin(rows, empty)[:, None] & np.isin(np.arange(r1), empty)[None, :] & (np.arange(r1)[None, :] <= rows[:, None])
            assert both_empty.any() or r1 - r0 == 1
            assert np.isnan(d[both_empty]).all() if model == 0 else not np.isnan(d).any()      # (model 0: flat 255's +inf makes NaN too)
            for D in WITHIN_D:
                z.pair_block_within(r0, r1, 1.0, 16, n_cols=r1, triangle=True, model=model, fp32=fp32)
                row, col, dist = s.pair_block_within(r0, r1, D, 16, n_cols=r1, triangle=True, model=model, fp32=fp32)
                wr, wc, wd = W._want(d, r0, D)
                assert (col <= row).all(), (r0, r1, D)
                assert np.array_equal(row, wr) and np.array_equal(col, wc), (r0, r1, D)
                assert np.array_equal(dist.view(np.uint64), wd.view(np.uint64)), (r0, r1, D)
                assert not np.isnan(dist).any()
            assert len(W._want(d, r0, 1.0)[0]) > len(W._want(d, r0, 0.05)[0]) > 0                # (the cut-offs do cut)
        z.free()
        s.free()
