"""Row blocks of lash_sketch_set_pair_block for HyperMinHash and HyperLogLog — blocks that start at r0 > 0, span several row
workgroups or tiles, or are cut by the triangle's early return — against references that never touch the library: made-up
images, numpy and fractions.Fraction.  Every comparison is exact (integers, f64 bit patterns); cells above the diagonal of a
triangular block are undefined and never read.

What reaches which kernel:
  hmh_pairs_planes_kernel<false,16>   test_hmh_blocks_on_both_routes[general], test_hmh_two_sets_query_on_the_device[general]
                                      (after prepare(); ~10 % zero registers, all-zero and identical images)
  hmh_pairs_planes_kernel<true,32>    the same two tests with [full]: no zero register anywhere, N == 16 384 asserted
  hmh_pairs_kernel (u16 pairs)        the same tests before prepare() (rows at d_images + r0 * stride), and after prepare() in
                                      test_hmh_words_knob_keeps_the_prepared_route_on_the_u16_kernel (LASH_HMH_PAIRS_WORDS=1)
  hll_pairs_bitmap_kernel<W,Z>        test_hll_blocks[p-kind], p = 10 and 12, by the range (lo, lo + band) of the image kind:
      <false,false>  narrow      (5, 30)                              what sketches of genomes look like
      <false,true>   sparse      (0, 11)                              and narrow x sparse, (0, 30): test_hll_two_sets_...
      <true,false>   band        (6, 33..55 at p = 10, 33..53 at 12)  the hot registers reach above 32
      <true,true>    full_range  (0, 55 at p = 10, 53 at p = 12)
  hll_pairs_kernel (byte-wise)        test_hll_blocks[*-flat] ((7, 7): no band), every kind at p = 8, every kind before
                                      prepare() (rows at d_images + r0 * stride), test_hll_bytewise_knob (LASH_HLL_PAIRS_BYTEWISE=1)
_hll_images asserts each kind's range class, so the table cannot go stale silently.

References.  HyperMinHash: the 1 100 images share one base image outside 512 varied positions (one per 32-bit plane word), so
C = k0 + #{equal and non-zero among the 512}, N = k0 + #{either non-zero among the 512} with k0 the non-zero base registers
outside them (an all-zero image: C = 0, N = the other's non-zero count): n * n * 512 comparisons, all cells;
test_hmh_shortcut_is_the_plain_count proves it on 16 pairs over all 16 384 registers.  HyperLogLog: zero = #{max == 0} and two exact
uint64 sums per pair (registers <= 32 in units of 2^-32, above in units of 2^-64), joined as a Fraction and rounded by float();
test_hll_reference_agrees_with_the_per_pair_one holds it against test_gpu_hll_pairs._want.

CPU time of the references (-s prints each): 0.9 to 2.0 s per HyperMinHash set of 1 100 x 1 100 cells (two sets), 0.1 to 1.4 s per
HyperLogLog case (17 cases), 6 to 17 s for the whole file depending on the host; the 512 varied positions are kept.  On an MI355X no
test of the file takes more than 2.5 s (the two child processes; the block tests 0.1 to 0.4 s).

Mutations, each tried on a scratch build against this file, test_gpu_hll_pairs.py, test_gpu_sketch_set.py and test_gpu_dist_within.py:
  tile_above_diagonal with >= for >            test_hmh_blocks_on_both_routes[general, full] (u16 pairs, (513, 1100): cell (576, 576))
                                               and all 15 test_hll_blocks ((65, n): cell (128, 128); p = 8: (17, 49)); nothing else
  the planes' early return with PL_ROWS - 2    test_hmh_blocks_on_both_routes[general, full] ((513, 1100): cell (1024, 1024)); nothing else
  T without + a.row0                           test_hmh_blocks_on_both_routes and test_hmh_two_sets_query_on_the_device, both variants;
                                               also test_gpu_sketch_set's test_planes_and_word_kernels_agree and test_row_blocks_...[hmh-0-fgra]
                                               and test_gpu_dist_within's test_allpairs_two_ranks_equal_the_cli
  the bitmaps without + r0 * per               test_hll_blocks at p = 10 and 12 except flat (8 cases), test_hll_two_sets_with_different_ranges
                                               [10, 12]; also test_gpu_sketch_set's test_row_blocks_...[hll-12-fgra]"""
import os
import subprocess
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_hll_pairs as HP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HMH_M = 16384
HMH_N = 1100
VARIED = 32 * np.arange(512) + (7 * np.arange(512)) % 32                # one register in every plane word, at a moving bit
FIXED = (0x8001, 0x7FFE, 0x0100)                                        # 0x8001 ^ 0x7FFE = 0xFFFF: all 16 planes differ
HMH_TRIANGLES = ((0, 1100), (37, 1100), (511, 513), (512, 1024), (513, 1100), (1031, 1100), (1099, 1100))
HMH_RECTANGLES = ((0, 1100), (37, 600), (1031, 1100))
HMH_RECT_COLS = (1, 17, 65, 1100)
HMH_IDENTICAL = ((3, 1000), (700, 1099), (512, 511))                     # (copy, original)
HMH_EMPTY = (5, 513, 1098)                                               # (general variant only)

HLL_SIZES = {10: 300, 12: 130, 8: 300}                                   # p -> n
HLL_KINDS = ("narrow", "sparse", "band", "full_range", "flat")
HLL_RECT_COLS = (1, 63, 64, 65)                                          # and n


def _timed(what, t0):
    print("\n[reference] %s: %.2f s of CPU" % (what, time.process_time() - t0))


# ---- HyperMinHash -----------------------------------------------------------------------------------------------------------------

def _hmh_images(full):
    rng = np.random.default_rng(1100 + full)
    base = rng.integers(1, 65536, HMH_M).astype(np.uint16)
    if not full:
        base[rng.random(HMH_M) < 0.1] = 0
    alphabet = np.empty((5, 512), np.uint16)                             # per varied position: 0, the base value, three fixed values
    alphabet[0], alphabet[1] = 0, base[VARIED]
    alphabet[2:] = np.array(FIXED, np.uint16)[:, None]
    pick = rng.integers(1 if full else 0, 5, (HMH_N, 512))
    imgs = np.tile(base, (HMH_N, 1))
    imgs[:, VARIED] = alphabet[pick, np.arange(512)[None, :]]
    for dst, src in HMH_IDENTICAL:
        imgs[dst] = imgs[src]
    if not full:
        imgs[list(HMH_EMPTY)] = 0
    assert full == bool((imgs != 0).all())
    return imgs


def _hmh_reference(imgs):
    """(C, N) uint32 [n, n] of every pair by the shortcut of the module docstring"""
    t0 = time.process_time()
    n = len(imgs)
    rest = np.ones(HMH_M, bool)
    rest[VARIED] = False
    empty = ~imgs.any(axis=1)
    common = imgs[np.flatnonzero(~empty)[0]][rest]
    assert (imgs[~empty][:, rest] == common[None, :]).all()             # what the shortcut rests on
    k0 = np.uint32(np.count_nonzero(common))
    v = np.ascontiguousarray(imgs[:, VARIED])
    nzv = v != 0
    c, m = np.empty((n, n), np.uint32), np.empty((n, n), np.uint32)
    for i0 in range(0, n, 32):
        a, za = v[i0:i0 + 32, None, :], nzv[i0:i0 + 32, None, :]
        c[i0:i0 + 32] = np.count_nonzero((a == v[None, :, :]) & za, axis=2) + k0
        m[i0:i0 + 32] = np.count_nonzero(za | nzv[None, :, :], axis=2) + k0
    nz = (k0 + nzv.sum(axis=1)).astype(np.uint32)                       # an all-zero image shares nothing; N = the other's registers
    nz[empty] = 0
    c[empty, :] = 0
    c[:, empty] = 0
    m[empty, :] = nz[None, :]
    m[:, empty] = nz[:, None]
    _timed("HyperMinHash %d x %d" % (n, n), t0)
    return c, m


# ---- HyperLogLog ------------------------------------------------------------------------------------------------------------------

def _hll_images(p, kind, seed=0):
    n = HLL_SIZES[p]
    rng = np.random.default_rng(1000 * p + 10 * HLL_KINDS.index(kind) + seed)
    img = HP._images(rng, n, p, kind)                                    # [n, 33 + 2^p], random header bytes
    if kind == "sparse":
        img[3] = img[2]                                                  # identical sketches
        img[5, 33:] = 0                                                  # an empty one
        img[n - 1, 33:] = 0
    lo, hi = int(img[:, 33:].min()), int(img[:, 33:].max())
    assert {"narrow": (lo, hi) == (5, 30), "sparse": (lo, hi) == (0, 11), "band": lo == 6 and 32 < hi <= 64,
            "full_range": lo == 0 and hi == 64 - p + 1, "flat": lo == hi == 7}[kind], (kind, lo, hi)
    return img


def _hll_weights():
    w1 = np.array([1 << (32 - r) if r <= 32 else 0 for r in range(256)], np.uint64)
    w2 = np.array([1 << (64 - r) if 32 < r <= 64 else 0 for r in range(256)], np.uint64)
    return w1, w2


def _hll_reference(p, ref, qry):
    """(zero uint32, sum float64) [n_ref, n_qry]; m <= 4096: s1 <= m 2^32 and s2 <= m 2^31 fit uint64"""
    t0 = time.process_time()
    assert p <= 12
    w1, w2 = _hll_weights()
    a, b = ref[:, 33:], qry[:, 33:]
    nr, nq = len(a), len(b)
    zero = np.empty((nr, nq), np.uint32)
    s1, s2 = np.empty((nr, nq), np.uint64), np.zeros((nr, nq), np.uint64)
    wide = max(a.max(), b.max()) > 32                                    # (no register above 32: nothing in units of 2^-64)
    step = max(1, (1 << 22) // (nq << p))
    for i0 in range(0, nr, step):
        mx = np.maximum(a[i0:i0 + step, None, :], b[None, :, :])
        zero[i0:i0 + step] = np.count_nonzero(mx == 0, axis=2)
        s1[i0:i0 + step] = w1[mx].sum(axis=2, dtype=np.uint64)
        if wide:
            s2[i0:i0 + step] = w2[mx].sum(axis=2, dtype=np.uint64)
    total = np.array([float(Fraction((int(x) << 32) + int(y), 1 << 64)) for x, y in zip(s1.ravel(), s2.ravel())], np.float64)
    _timed("HyperLogLog p = %d, %d x %d" % (p, nr, nq), t0)
    return zero, total.reshape(nr, nq)


# ---- images and references: made once per module, read-only -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(what, *key):
        k = (what,) + key
        if k not in cache:
            if what == "hmh":                                            # key: (full,)
                imgs = _hmh_images(*key)
                cache[k] = (imgs,) + _hmh_reference(imgs)
            elif what == "hll":                                          # key: (p, kind)
                img = _hll_images(*key)
                cache[k] = (img,) + _hll_reference(key[0], img, img)
            else:                                                        # "hll2", key: (p,): narrow rows x sparse columns
                ref, qry = get("hll", key[0], "narrow")[0], get("hll", key[0], "sparse")[0]
                cache[k] = (ref, qry) + _hll_reference(key[0], ref, qry)
            for arr in cache[k]:
                arr.setflags(write=False)
        return cache[k]
    return get


def _bytes(imgs):
    return np.ascontiguousarray(imgs).view(np.uint8).reshape(len(imgs), -1)


def _check_block(got, want, r0, r1, n_cols, triangle, what):
    """every printed cell of rows [r0, r1) x columns [0, n_cols): col <= row in a triangle, all of a rectangle"""
    printed = np.ones((r1 - r0, n_cols), bool)
    if triangle:
        printed = np.arange(n_cols)[None, :] <= np.arange(r0, r1)[:, None]
    for key, w in want.items():
        g = got[key]
        assert g.shape == (r1 - r0, n_cols) and g.dtype == w.dtype, (what, key)
        g, w = g[printed], w[r0:r1, :n_cols][printed]
        if w.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, key, (r0, r1, n_cols, triangle), "%d wrong cells, first at (row, col) = %s" % (
            bad.size, tuple(int(x) for x in np.argwhere(printed)[bad[0]] + (r0, 0))))


def _blocks(triangles, rectangles, rect_cols):
    for r0, r1 in triangles:
        yield r0, r1, r1, True
    for r0, r1 in rectangles:
        for nc in rect_cols:
            yield r0, r1, nc, False


# ---- HyperMinHash tests -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("full", [False, True], ids=["general", "full"])
def test_hmh_shortcut_is_the_plain_count(data, full):
    """16 pairs over all 16 384 registers the plain way: an identical pair, a zero image against a filled one, itself and another
    zero image, the last image, first x last"""
    imgs, c, m = data("hmh", full)
    pairs = [HMH_IDENTICAL[0], HMH_IDENTICAL[1], (HMH_N - 1, HMH_N - 1), (HMH_N - 1, 0), (0, HMH_N - 1), (0, 0), (1, 2), (2, 1),
             (HMH_EMPTY[0], 7), (7, HMH_EMPTY[0]), (HMH_EMPTY[0], HMH_EMPTY[0]), (HMH_EMPTY[1], HMH_EMPTY[2]), (HMH_N - 1, HMH_EMPTY[2]),
             (511, 512), (1031, 37), (600, 1099)]
    assert len(set(pairs)) == 16
    for i, j in pairs:
        a, b = imgs[i], imgs[j]
        assert c[i, j] == np.count_nonzero((a == b) & (a != 0)), (i, j)
        assert m[i, j] == np.count_nonzero((a != 0) | (b != 0)), (i, j)
    assert c[3, 1000] == m[3, 1000] == c[1000, 1000]                      # identical images: every non-zero register matches
    if not full:
        assert (m[5] == np.diag(m)).all() and m[5, 513] == 0 and not c[5].any()
    assert (m == HMH_M).all() == full
    assert len(np.unique(c)) > 50                                         # (the cells do differ: a shifted block cannot agree)


@pytest.mark.parametrize("full", [False, True], ids=["general", "full"])
def test_hmh_blocks_on_both_routes(data, full):
    """each block first on the unprepared set (hmh_pairs_kernel on d_images + r0 * stride), then after prepare() (bit planes: 512 rows
    per workgroup read at T + r0 + ..., tiles beyond the workgroup's last row skipped)"""
    import lash_amd
    imgs, c, m = data("hmh", full)
    want = dict(c_or_zero=c, n_counts=m)
    with lash_amd.Context(0) as ctx:
        s = ctx.sketch_set("hmh", 0, _bytes(imgs))
        for prepared in (False, True):
            if prepared:
                s.prepare()
            for r0, r1, nc, tri in _blocks(HMH_TRIANGLES, HMH_RECTANGLES, HMH_RECT_COLS):
                got = s.pair_block(r0, r1, n_cols=nc, triangle=tri)
                _check_block(got, want, r0, r1, nc, tri, "planes" if prepared else "u16 pairs")
                if full and not tri:
                    assert (got["n_counts"] == HMH_M).all()
        s.free()


@pytest.mark.parametrize("full", [False, True], ids=["general", "full"])
def test_hmh_two_sets_query_on_the_device(data, full):
    """reference rows (500, 1100) of a set gathered into place through `order`, against a 70-member query set drawn by a permutation
    and adopted from device memory; before and after prepare(q)"""
    import lash_amd
    import torch
    imgs, c, m = data("hmh", full)
    rng = np.random.default_rng(70)
    members = rng.permutation(HMH_N)[:70]
    members[:4] = (HMH_N - 1, 1000, 3, 600)                              # the last image, an identical pair
    if not full:
        members[4:6] = HMH_EMPTY[:2]
    shuffle = rng.permutation(HMH_N)
    order = np.argsort(shuffle).astype(np.uint32)                        # imgs[shuffle][order] == imgs
    want = dict(c_or_zero=np.ascontiguousarray(c[:, members]), n_counts=np.ascontiguousarray(m[:, members]))
    with lash_amd.Context(0) as ctx:
        s = ctx.sketch_set("hmh", 0, _bytes(imgs[shuffle]), order)
        q_dev = torch.from_numpy(_bytes(imgs[members])).cuda()
        q = ctx.sketch_set("hmh", 0, q_dev)
        for prepared in (False, True):
            if prepared:
                s.prepare(q)
            for nc in (70, 33):
                got = s.pair_block(500, 1100, qry=q, n_cols=nc)
                _check_block(got, want, 500, 1100, nc, False, "planes" if prepared else "u16 pairs")
        q.free()
        s.free()


CHILD = ("import sys, numpy as np, lash_amd\n"
         "algo, p, r0, r1 = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])\n"
         "with lash_amd.Context(0) as ctx:\n"
         "    for path in sys.argv[5:]:\n"
         "        s = ctx.sketch_set(algo, p, np.load(path))\n"
         "        s.prepare()\n"
         "        st = s.pair_block(r0, r1, n_cols=r1, triangle=True)\n"
         "        np.savez(path + '.out.npz', **st)\n"
         "        s.free()\n")


def _child(knob, algo, p, r0, r1, paths):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env[knob] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, algo, str(p), str(r0), str(r1)] + [str(x) for x in paths], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [dict(np.load(str(x) + ".out.npz")) for x in paths]


def test_hmh_words_knob_keeps_the_prepared_route_on_the_u16_kernel(data, tmp_path):
    """LASH_HMH_PAIRS_WORDS=1 (read once per process): prepare() builds no planes, the (37, 1100) triangle is the reference's all the same"""
    imgs, c, m = data("hmh", False)
    np.save(tmp_path / "hmh.npy", _bytes(imgs))
    got, = _child("LASH_HMH_PAIRS_WORDS", "hmh", 0, 37, 1100, [tmp_path / "hmh.npy"])
    _check_block(got, dict(c_or_zero=c, n_counts=m), 37, 1100, 1100, True, "LASH_HMH_PAIRS_WORDS=1")


# ---- HyperLogLog tests ------------------------------------------------------------------------------------------------------------

def test_hll_reference_agrees_with_the_per_pair_one(data):
    """the vectorised reference and test_gpu_hll_pairs._want (a histogram and a sum of Fractions per pair) on a 9 x 9 corner"""
    for p, kind in ((10, "band"), (12, "full_range"), (10, "narrow"), (8, "sparse")):
        img, zero, total = data("hll", p, kind)
        n = len(img)
        rows, cols = np.r_[0:5, n - 4:n], np.r_[0:6, n - 3:n]            # (sparse: identical, empty and last members among them)
        wz, ws = HP._want(img[rows], img[cols])
        assert np.array_equal(zero[np.ix_(rows, cols)], wz), (p, kind)
        assert np.array_equal(total[np.ix_(rows, cols)].view(np.uint64), ws.view(np.uint64)), (p, kind)
    ref, qry, zero, total = data("hll2", 10)
    wz, ws = HP._want(ref[291:300], qry[:9])
    assert np.array_equal(zero[291:300, :9], wz) and np.array_equal(total[291:300, :9].view(np.uint64), ws.view(np.uint64))


def _hll_triangles(p, n):
    return ((0, n), (37, n), (63, 65), (64, 128), (65, n), (n - 1, n)) + (((17, 49),) if p == 8 else ())


@pytest.mark.parametrize("kind", HLL_KINDS)
@pytest.mark.parametrize("p", [10, 12, 8])
def test_hll_blocks(data, p, kind):
    """the (37, n) triangle before any prepare() (hll_pairs_kernel on d_images + r0 * stride), then every block after prepare():
    p >= 10 with a band of values through the bitmaps at bm + r0 * per, p = 8 and `flat` through hll_pairs_kernel again"""
    import lash_amd
    img, zero, total = data("hll", p, kind)
    n = len(img)
    want = dict(c_or_zero=zero, sum_or_union=total)
    with lash_amd.Context(0) as ctx:
        s = ctx.sketch_set("hll", p, img)
        _check_block(s.pair_block(37, n, n_cols=n, triangle=True), want, 37, n, n, True, "unprepared")
        s.prepare()
        for r0, r1, nc, tri in _blocks(_hll_triangles(p, n), ((37, n), (64, 65)), HLL_RECT_COLS + (n,)):
            _check_block(s.pair_block(r0, r1, n_cols=nc, triangle=tri), want, r0, r1, nc, tri, "prepared")
        s.free()


@pytest.mark.parametrize("p", [10, 12])
def test_hll_two_sets_with_different_ranges(data, p):
    """narrow rows (5..30) against sparse columns (0..11): prepare(q) settles on the common range (0, 30), hll_pairs_bitmap_kernel<false,true>,
    and rebuilds the row set's bitmaps for it"""
    import lash_amd
    ref, qry, zero, total = data("hll2", p)
    n = len(ref)
    want = dict(c_or_zero=zero, sum_or_union=total)
    with lash_amd.Context(0) as ctx:
        s, q = ctx.sketch_set("hll", p, ref), ctx.sketch_set("hll", p, qry)
        s.prepare()                                                      # (bitmaps for its own range first: they must not survive)
        s.prepare(q)
        for r0, r1 in ((0, n), (37, n), (64, 65), (65, n)):
            for nc in HLL_RECT_COLS + (len(qry),):
                _check_block(s.pair_block(r0, r1, qry=q, n_cols=nc), want, r0, r1, nc, False, "narrow x sparse")
        q.free()
        s.free()


def test_hll_bytewise_knob(data, tmp_path):
    """LASH_HLL_PAIRS_BYTEWISE=1 (read once per process): prepare() builds no bitmaps, the (37, n) triangle is the reference's all the same"""
    cases = ((10, "narrow"), (10, "band"))
    paths = []
    for p, kind in cases:
        paths.append(tmp_path / ("%s.npy" % kind))
        np.save(paths[-1], data("hll", p, kind)[0])
    for (p, kind), got in zip(cases, _child("LASH_HLL_PAIRS_BYTEWISE", "hll", 10, 37, 300, paths)):
        img, zero, total = data("hll", p, kind)
        _check_block(got, dict(c_or_zero=zero, sum_or_union=total), 37, 300, 300, True, "LASH_HLL_PAIRS_BYTEWISE=1 " + kind)
