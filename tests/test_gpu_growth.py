"""lash_sketch_set_prefix_union_cardinalities (csrc/prefix_union.hip, lash_growth_api.hip) through the ABI.

The yardstick is the slow way (growth_model.py): the images folded one at a time with merge_images, every prefix's number from the host
entry for one image (lash_hmh_cardinality / lash_hll_cardinality / lash_ull_estimate); for hll also numpy's maximum of the register bytes
as a fold of its own.  Every comparison is == on the doubles' bits.

The collection: a family with exact duplicates (steps that change nothing), two inputs shorter than k (empty sketches; one of them is
member 0, so order 0 starts with an empty prefix), one genome ten times the others' size, unrelated genomes of 20-60 kbp: 37 in all.
Tables: hmh (8 192 words), hll p 4 (4 words: fewer than a wave has lanes), 10 and 16 (the 64 KiB edge), ull p 3 (2 words), 12 and 16."""
import numpy as np
import pytest

import growth_model as G
import oracle_lib as O
from test_gpu_dist_within import _family

pytestmark = pytest.mark.gpu

K = 16
SLICES = (0, 1, 2, 7, 64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _genomes():
    fam = _family(300, 40_000)
    tiny = [np.frombuffer(b"ACGTACGTAC", np.uint8).copy(), np.frombuffer(b"TTGACA", np.uint8).copy()]
    others = [O.synth_genome(400 + i, 20_000 + 1_600 * i) for i in range(25)]
    g = [tiny[0]] + fam + [fam[0].copy(), fam[2].copy()] + others[:12] + [O.synth_genome(399, 400_000)] + others[12:] + [tiny[1]]
    assert len(g) == 37
    return g


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genomes():
    return _genomes()


_images, _folds = {}, {}


def _sketches(ctx, genomes, algo, p):
    """the collection's images; the 64 KiB tables take 6 of them: an empty one, two relatives, a duplicate, the large one, a stranger"""
    import lash_amd
    if (algo, p) not in _images:
        gs = genomes if p < 16 else [genomes[i] for i in (0, 1, 3, 8, 22, 30)]
        seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in gs])
        _images[(algo, p)] = ctx.sketch_batch(algo, K, p, 42, seq, rec_off, goff)
    return _images[(algo, p)]


def _want(ctx, algo, p, images, rows, estimator="fgra", hll_bias=None):
    from lash_amd.sketch import sketch_cardinality
    out = np.zeros((len(rows), len(rows[0])))
    for o, idx in enumerate(rows):
        key = (algo, p, tuple(int(i) for i in idx))
        if key not in _folds:
            _folds[key] = G.fold(ctx, algo, p, images, key[2])
        for t, img in enumerate(_folds[key]):
            out[o, t] = sketch_cardinality(algo, p, img, estimator=estimator, hll_bias=hll_bias)
    return out


def _bias(algo, p):
    """hll p = 16: 5 * 2^p = 327 680 and linear counting ends at 50 000, so prefixes of a few 40 kbp genomes need the tables; a made-up one serves
    (model and entry read the same): the case is about the 64 KiB table, not the statistics"""
    from lash_amd.sketch import HllBias
    if (algo, p) != ("hll", 16):
        return None
    raw = np.linspace(0.0, 400_000.0, 41)
    return HllBias().set(16, raw, 100.0 + raw / 128.0)


def _orders(n):
    """five orders of the whole set (order 0 = the members as they are), one of one member, one of 2 n with repeats"""
    whole = G.orders(n, 5, 42)
    twice = np.concatenate([G.order(n, 3, 7), G.order(n, 4, 7)]).astype(np.uint32).reshape(1, 2 * n)
    twice[0, 1] = twice[0, 0]                                              # the same member twice in a row
    return whole, np.array([[n - 2]], dtype=np.uint32), twice


CASES = [("hmh", 0, "fgra"), ("hll", 4, "fgra"), ("hll", 10, "fgra"), ("hll", 16, "fgra"), ("ull", 3, "fgra"), ("ull", 3, "ml"),
         ("ull", 12, "fgra"), ("ull", 12, "ml"), ("ull", 16, "fgra"), ("ull", 16, "ml")]


@pytest.mark.parametrize("algo,p,est", CASES)
def test_every_prefix_equals_the_single_image_entry_bit_for_bit(ctx, genomes, algo, p, est):
    images = _sketches(ctx, genomes, algo, p)
    s = ctx.sketch_set(algo, p, images)
    tb = _bias(algo, p)
    try:
        for rows in _orders(s.n):
            want = _want(ctx, algo, p, images, rows, est, tb)
            got = s.prefix_union_cardinalities(rows, estimator=est, hll_bias=tb)
            assert got.shape == rows.shape and _bits(got) == _bits(want), (algo, p, est, rows.shape)
        whole = _orders(s.n)[0]
        want = _want(ctx, algo, p, images, whole, est, tb)
        assert want[0, 0] < 1.0 < want[0, -1]                                             # the empty prefix; the curve goes somewhere
        # the cut of the work changes no bit: slices (clamped to the word count), one order per chunk
        for slices in SLICES:
            assert _bits(s.prefix_union_cardinalities(whole, estimator=est, hll_bias=tb, slices=slices)) == _bits(want), slices
        assert _bits(s.prefix_union_cardinalities(whole, estimator=est, hll_bias=tb, hist_budget_bytes=1)) == _bits(want)
        assert _bits(s.prefix_union_cardinalities(whole, estimator=est, hll_bias=tb, slices=7, hist_budget_bytes=1)) == _bits(want)
        assert _bits(s.prefix_union_cardinalities(whole[:1], estimator=est, hll_bias=tb)) == _bits(want[:1])       # n_orders = 1
    finally:
        s.free()


@pytest.mark.parametrize("p", [4, 10, 16])
def test_hll_against_a_fold_of_its_own(ctx, genomes, p):
    from lash_amd.sketch import sketch_cardinality
    import lash_amd
    images = _sketches(ctx, genomes, "hll", p)
    hdr = lash_amd.header_bytes("hll")
    s = ctx.sketch_set("hll", p, images)
    try:
        rows, tb = _orders(s.n)[0], _bias("hll", p)
        got = s.prefix_union_cardinalities(rows, hll_bias=tb)
        for o, idx in enumerate(rows):
            acc = images[idx[0]].copy()
            for t, i in enumerate(idx):
                acc[hdr:] = np.maximum(acc[hdr:], images[i][hdr:])                         # (the host entry reads the registers only)
                assert _bits([got[o, t]]) == _bits([sketch_cardinality("hll", p, acc, hll_bias=tb)]), (p, o, t)
    finally:
        s.free()


def test_ull_tables_beyond_64_kib_are_refused(ctx):
    import lash_amd
    images = np.zeros((2, ctx.image_bytes("ull", 17)), dtype=np.uint8)
    s = ctx.sketch_set("ull", 17, images)
    try:
        with pytest.raises(lash_amd.LashError) as e:
            s.prefix_union_cardinalities(np.array([[0, 1]], dtype=np.uint32))
        assert e.value.code == lash_amd.EINVAL and "ull is supported up to -p 16" in str(e.value)
    finally:
        s.free()


def test_bad_arguments_are_refused(ctx, genomes):
    import ctypes as C
    import lash_amd
    images = _sketches(ctx, genomes, "ull", 12)
    s = ctx.sketch_set("ull", 12, images)
    try:
        n = s.n
        for rows, at in (([[0, n, 1]], 1), ([[0, 1, 2], [3, 4, 2**32 - 1]], 5), ([[n]], 0)):
            with pytest.raises(lash_amd.LashError) as e:
                s.prefix_union_cardinalities(np.array(rows, dtype=np.uint32))
            assert e.value.code == lash_amd.EINVAL and e.value.index == at
        with pytest.raises(KeyError):
            s.prefix_union_cardinalities(np.array([[0]], dtype=np.uint32), estimator="mle")
        lib, out, bad = ctx._lib, np.zeros(4), C.c_uint64()
        rows = np.array([[0, 1]], dtype=np.uint32)
        call = lib.lash_sketch_set_prefix_union_cardinalities
        assert call(ctx._h, s._h, rows.ctypes.data, 1, 2, 7, None, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL      # estimator
        assert call(ctx._h, s._h, rows.ctypes.data, 1, 0, 0, None, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL      # len == 0
        assert call(ctx._h, s._h, None, 1, 2, 0, None, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
        assert call(ctx._h, s._h, rows.ctypes.data, 1, 2, 0, None, None, None, C.byref(bad)) == lash_amd.EINVAL
        assert call(ctx._h, None, rows.ctypes.data, 1, 2, 0, None, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
        assert call(None, s._h, rows.ctypes.data, 1, 2, 0, None, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
        assert call(ctx._h, s._h, rows.ctypes.data, 0, 0, 0, None, None, None, None) == lash_amd.OK                             # nothing to do
        assert call(ctx._h, s._h, rows.ctypes.data, 1, 2, 0, None, None, out.ctypes.data, None) == lash_amd.OK                  # opts, bad_index NULL
        assert _bits(out[:2]) == _bits(_want(ctx, "ull", 12, images, rows)[0])
    finally:
        s.free()


def test_hll_below_five_m_needs_the_tables(ctx):
    """p = 10: 5 * 2^p = 5 120 and linear counting ends at 900, so a 2-3 kbp genome's sketch sits in the bias-table regime"""
    import lash_amd
    from lash_amd.sketch import HllBias
    small = O.synth_genome(500, 2_500)
    gs = [np.frombuffer(b"ACGT", np.uint8).copy(), small, _family(501, 2_000)[2], O.synth_genome(502, 30_000)]
    seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in gs])
    images = ctx.sketch_batch("hll", K, 10, 42, seq, rec_off, goff)
    s = ctx.sketch_set("hll", 10, images)
    try:
        rows = np.array([[3, 3, 0, 3], [0, 1, 2, 3]], dtype=np.uint32)      # order 0 never leaves the raw regime; order 1 enters the tables' at step 1
        with pytest.raises(lash_amd.LashError) as e:
            s.prefix_union_cardinalities(rows)
        assert e.value.code == lash_amd.ERANGE and e.value.index == 1 * 4 + 1
        with pytest.raises(lash_amd.LashError) as e:
            s.prefix_union_cardinalities(rows[::-1].copy(), slices=3, hist_budget_bytes=1)
        assert e.value.code == lash_amd.ERANGE and e.value.index == 1
        # a made-up table: this checks that the tables reach the estimate, not the statistics
        raw = np.linspace(0.0, 6000.0, 25)
        tb = HllBias().set(10, raw, 40.0 + raw / 64.0)
        want = _want(ctx, "hll", 10, images, rows, hll_bias=tb)
        got = s.prefix_union_cardinalities(rows, hll_bias=tb)
        assert _bits(got) == _bits(want)
        with pytest.raises(lash_amd.LashError):
            _want(ctx, "hll", 10, images, rows)                           # (the host entry refuses the same prefixes)
    finally:
        s.free()


def test_hmh_rare_ranks_take_the_register_order_sum(ctx, genomes):
    """a register with more than 39 leading zeros: from that step on the histogram's sum is not the crate's, and the entry re-folds"""
    from lash_amd.sketch import sketch_cardinality
    images = _sketches(ctx, genomes, "hmh", 0).copy()
    regs = images[20].view("<u2")
    regs[100], regs[9000] = (45 << 10) | 5, (41 << 10) | 1000
    images[28].view("<u2")[16383] = (63 << 10) | 1023
    s = ctx.sketch_set("hmh", 0, images)
    try:
        rows = np.array([G.order(s.n, 1, 11), G.order(s.n, 2, 11), [20] + list(range(1, s.n))], dtype=np.uint32)
        at = [int(np.flatnonzero(r == 20)[0]) for r in rows]
        assert at == [31, 7, 0]                                           # late, early, and from the very first step
        want = _want(ctx, "hmh", 0, images, rows)
        for kw in ({}, {"slices": 7, "hist_budget_bytes": 1}):
            assert _bits(s.prefix_union_cardinalities(rows, **kw)) == _bits(want), kw
        # the planted registers are what the register-order loop is for: with them the histogram route alone would not do
        lz = np.array([2.0 ** -int(r >> 10) for r in images[20].view("<u2")])
        assert sketch_cardinality("hmh", 0, images[20]) == want[2, 0] and lz.min() == 2.0 ** -45
    finally:
        s.free()


def test_the_set_keeps_its_state(ctx, genomes):
    images = _sketches(ctx, genomes, "hmh", 0)
    s = ctx.sketch_set("hmh", 0, images)
    try:
        card = s.cardinalities()
        s.prepare()
        before = s.pair_block(0, s.n, triangle=True)
        ec = s.hmh_expected_collisions(0, s.n)
        s.prefix_union_cardinalities(G.orders(s.n, 3, 5))
        after = s.pair_block(0, s.n, triangle=True)
        low = np.tril(np.ones((s.n, s.n), bool))
        for key in before:
            assert np.array_equal(before[key][low], after[key][low]), key
        ec2 = s.hmh_expected_collisions(0, s.n)                            # (refused without the cardinalities the set took: still there)
        assert (ec is None) == (ec2 is None)
        assert _bits(s.cardinalities()) == _bits(card)
    finally:
        s.free()
