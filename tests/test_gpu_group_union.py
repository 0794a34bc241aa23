"""lash_sketch_set_group_union (csrc/group_union.hip, lash_group_union_api.hip) through the ABI.

The yardstick is the slow way: every group's members folded one at a time on the CPU with the oracle's merge_images, from the image of an
empty sketch.  Every comparison is == on the bytes, header included.

The collection: 24 sketches of synthetic genomes of 2-30 kbp, one of them an input shorter than k (the empty sketch, the fold's start) and
one an exact duplicate.  Tables: hmh (8 192 words), hll p 4 (one 16-byte unit), 10 and 14, ull p 3 (two words: the one table that is
no whole unit), 12 and 18 (256 KiB: with slices = 1 every thread strides over 64 units), and hmh under a layout with big-endian
registers behind a header.  One call holds groups of 0, 1, 2, 3, 17 and all 24 members, two groups that overlap and one that repeats a
member; the bytes must not depend on how the work is cut (segment 1, 2, 5: with 24 members and pairs of partials the fold has five
levels; slices 1 and 7; a scratch budget of one byte: one group per chunk)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

K = 16
N = 24
EMPTY, DUP = 6, 13                                                         # an input shorter than k; a copy of member 2
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
BE = dict(hmh_reg="be", hmh_hdr="l")

GROUPS = [[], [5], [2, 9], [EMPTY, 0, DUP], [3, 4, 5, 6], [5, 6, 7, 8], list(range(7, 24)), list(range(N)), [4, 4, 11, 4], [EMPTY],
          list(range(N - 1, -1, -1))]
PLANS = [{}, {"segment": 1}, {"segment": 2}, {"segment": 5}, {"slices": 1}, {"slices": 7}, {"segment": 2, "scratch_budget": 1},
         {"segment": 5, "slices": 3, "scratch_budget": 1}, {"segment": 1000}]
CASES = [("hmh", 0, None), ("hll", 4, None), ("hll", 10, None), ("hll", 14, None), ("ull", 3, None), ("ull", 12, None), ("ull", 18, None),
         ("hmh", 0, BE)]
IDS = ["hmh", "hll4", "hll10", "hll14", "ull3", "ull12", "ull18", "hmh_be"]


def _genomes():
    g = [O.synth_genome(900 + i, 2_000 + 1_217 * i) for i in range(N)]
    g[EMPTY] = np.frombuffer(b"ACGTTGCA", np.uint8).copy()
    g[DUP] = g[2].copy()
    assert min(len(x) for x in g if len(x) > K) >= 2_000 and max(len(x) for x in g) <= 30_000
    return g


@pytest.fixture(scope="module")
def genomes():
    return _genomes()


_made = {}


def _case(genomes, algo, p, lay):
    """(context, images, the oracle's folds of GROUPS), made once per table"""
    import lash_amd
    key = (algo, p, lay is not None)
    if key not in _made:
        ctx = lash_amd.Context(0)
        layout = O.make_layout(**lay) if lay else None
        if layout is not None:
            ctx.set_layout(layout.spec())
        seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in genomes])
        images = ctx.sketch_batch(algo, K, p, 42, seq, rec_off, goff)
        assert images.shape == (N, O.image_bytes(ALGO[algo], p, layout))
        want = np.zeros((len(GROUPS), images.shape[1]), dtype=np.uint8)
        for g, members in enumerate(GROUPS):
            acc = images[EMPTY].copy()
            for m in members:
                acc = O.merge_images(ALGO[algo], p, acc, images[m], layout=layout)
            want[g] = acc
        _made[key] = (ctx, images, want)
    return _made[key]


def _diff(got, want):
    bad = np.argwhere(got != want)
    return "equal" if not len(bad) else "%d bytes differ, first at image %d byte %d (got %d want %d)" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("algo,p,lay", CASES, ids=IDS)
def test_every_group_equals_the_fold_under_every_plan(genomes, algo, p, lay):
    import torch
    ctx, images, want = _case(genomes, algo, p, lay)
    assert np.array_equal(images[DUP], images[2]) and not np.array_equal(want[7], images[EMPTY])
    assert np.array_equal(want[0], images[EMPTY]) and np.array_equal(want[7], want[10])       # no members; the order of members
    s = ctx.sketch_set(algo, p, images)
    try:
        for plan in PLANS:
            got = s.group_union(GROUPS, **plan)
            assert got.shape == want.shape and np.array_equal(got, want), (algo, p, plan, _diff(got, want))
        d_out = torch.full((want.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        for plan in ({}, {"segment": 2, "slices": 7}):
            assert s.group_union(GROUPS, device_out=d_out, **plan) is d_out
            ctx.synchronize()
            back = d_out.cpu().numpy()
            assert np.array_equal(back[:want.size].reshape(want.shape), want) and (back[want.size:] == 0xA5).all(), (algo, p, plan)
        one = s.group_union([list(range(N))])                                                # n_groups = 1
        assert np.array_equal(one[0], want[7])
        assert s.group_union([]).shape == (0, images.shape[1])
    finally:
        s.free()


@pytest.mark.parametrize("algo,p,lay", [CASES[0], CASES[2], CASES[4], CASES[6]], ids=[IDS[0], IDS[2], IDS[4], IDS[6]])
def test_the_plan_reports_what_runs(genomes, algo, p, lay):
    ctx, images, want = _case(genomes, algo, p, lay)
    words = (32768 if algo == "hmh" else 1 << p) // 4
    units = words // 4 if words % 4 == 0 else words
    s = ctx.sketch_set(algo, p, images)
    try:
        def partials(n, segment):
            """a group of n members: the partial unions its first two levels leave (they bound the two halves of the scratch buffer)"""
            fan = max(segment, 2)
            e = -(-n // segment) if n > segment else 0
            return e + (-(-e // fan) if e > fan else 0)

        def scratch(segment):
            return sum(partials(len(g), segment) for g in GROUPS) * words * 4
        assert partials(24, 2) == 12 + 6 and partials(24, 5) == 5 and partials(5, 5) == 0 and partials(24, 1) == 24 + 12
        for seg, sl in ((5, 7), (1, 1), (2, 3), (1000, 100_000_000)):
            assert s.group_union_plan(GROUPS, segment=seg, slices=sl) == (seg, min(sl, units), scratch(seg)), (seg, sl)
        seg, sl, sc = s.group_union_plan(GROUPS)
        assert 8 <= seg <= 256 and sl == max(1, -(-units // 256)) and sc == scratch(seg)
        # a budget below one group's partials: the largest single group is what a call holds at once
        assert s.group_union_plan(GROUPS, segment=2, scratch_budget=1)[2] == max(partials(len(g), 2) for g in GROUPS) * words * 4
    finally:
        s.free()


def test_bad_arguments_are_refused(genomes):
    import lash_amd
    ctx, images, want = _case(genomes, "ull", 12, None)
    s = ctx.sketch_set("ull", 12, images)
    try:
        for groups, at in (([[0, N, 1]], 1), ([[0, 1], [], [2, 3, 2**32 - 1]], 4), ([[N]], 0)):
            with pytest.raises(lash_amd.LashError) as e:
                s.group_union(groups)
            assert e.value.code == lash_amd.EINVAL and e.value.index == at
        lib, bad = ctx._lib, C.c_uint64(77)
        out = np.zeros((2, images.shape[1]), dtype=np.uint8)
        off = np.array([0, 2, 3], dtype=np.uint64)
        mem = np.array([1, 2, 3], dtype=np.uint32)
        plan = lash_amd._lib.GroupUnionOpts()
        for call in (lib.lash_sketch_set_group_union, lib.lash_sketch_set_group_union_device):
            assert call(None, s._h, off.ctypes.data, mem.ctypes.data, 2, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, None, off.ctypes.data, mem.ctypes.data, 2, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, None, mem.ctypes.data, 2, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, off.ctypes.data, None, 2, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, off.ctypes.data, mem.ctypes.data, 2, None, None, C.byref(bad)) == lash_amd.EINVAL
            for wrong in ([1, 2, 3], [0, 3, 2]):                                              # not from 0; decreasing
                w = np.array(wrong, dtype=np.uint64)
                assert call(ctx._h, s._h, w.ctypes.data, mem.ctypes.data, 2, None, out.ctypes.data, C.byref(bad)) == lash_amd.EINVAL
                assert b"group_off" in lib.lash_ctx_last_error(ctx._h)
                assert lib.lash_sketch_set_group_union_plan(ctx._h, s._h, w.ctypes.data, 2, None, C.byref(plan)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, off.ctypes.data, None, 0, None, None, None) == lash_amd.OK           # nothing to do
        assert bad.value == 77                                                                              # no refusal named a member
        assert lib.lash_sketch_set_group_union_plan(ctx._h, s._h, off.ctypes.data, 2, None, None) == lash_amd.EINVAL
        assert lib.lash_sketch_set_group_union(ctx._h, s._h, off.ctypes.data, mem.ctypes.data, 2, None, out.ctypes.data, None) == lash_amd.OK   # opts, bad_index NULL
        acc = O.merge_images(O.ULL, 12, O.merge_images(O.ULL, 12, images[EMPTY], images[1]), images[2])
        assert np.array_equal(out[0], acc) and np.array_equal(out[1], O.merge_images(O.ULL, 12, images[EMPTY], images[3]))
    finally:
        s.free()


def test_the_set_keeps_its_state(genomes):
    ctx, images, want = _case(genomes, "hmh", 0, None)
    s = ctx.sketch_set("hmh", 0, images)
    try:
        card = s.cardinalities()
        s.prepare()
        before = s.pair_block(0, s.n, triangle=True)
        assert np.array_equal(s.group_union(GROUPS, segment=2), want)
        after = s.pair_block(0, s.n, triangle=True)
        low = np.tril(np.ones((s.n, s.n), bool))
        for key in before:
            assert np.array_equal(before[key][low], after[key][low]), key
        assert s.cardinalities().view(np.uint64).tolist() == card.view(np.uint64).tolist()
    finally:
        s.free()
