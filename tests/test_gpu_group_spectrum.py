"""lash_sketch_set_group_spectrum (csrc/group_spectrum.hip, lash_group_spectrum_api.hip) through the ABI.

The yardstick is tests/spectrum_model.py: max, equality and bincount over the registers of the images.  Every comparison is ==.

The collection is the one the group-union test uses, rebuilt here: 24 sketches of synthetic genomes of 2-30 kbp, one of them an input
shorter than k (the empty sketch) and one an exact duplicate, as HyperMinHash under the default layout and under one with big-endian
registers behind a header.  One call holds groups of 0, 1, 2, 3, 17 and all 24 members, two groups that overlap and one that repeats a
member (it counts as often as it is listed); the bins must not depend on how the work is cut: segment 1, 2, 5 (count tables in scratch
memory and the finishing launch) and 1000 (every group one task, final in registers), slices 1 and 7, a scratch budget of one byte (one
group per chunk)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import spectrum_model as S

pytestmark = pytest.mark.gpu

K = 16
N = 24
EMPTY, DUP = 6, 13                                                         # an input shorter than k; a copy of member 2
BE = dict(hmh_reg="be", hmh_hdr="l")

GROUPS = [[], [5], [2, 9], [EMPTY, 0, DUP], [3, 4, 5, 6], [5, 6, 7, 8], list(range(7, 24)), list(range(N)), [4, 4, 11, 4], [EMPTY],
          list(range(N - 1, -1, -1))]
PLANS = [{}, {"segment": 1}, {"segment": 2}, {"segment": 5}, {"slices": 1}, {"slices": 7}, {"segment": 2, "scratch_budget": 1},
         {"segment": 5, "slices": 3, "scratch_budget": 1}, {"segment": 1000}]
CASES = [None, BE]
IDS = ["hmh", "hmh_be"]


def _genomes():
    g = [O.synth_genome(900 + i, 2_000 + 1_217 * i) for i in range(N)]
    g[EMPTY] = np.frombuffer(b"ACGTTGCA", np.uint8).copy()
    g[DUP] = g[2].copy()
    return g


_made = {}


def _case(lay, algo="hmh", p=0):
    """(context, images, registers as the model reads them), made once per layout and table"""
    import lash_amd
    key = (algo, p, lay is not None)
    if key not in _made:
        ctx = lash_amd.Context(0)
        layout = O.make_layout(**lay) if lay else None
        if layout is not None:
            ctx.set_layout(layout.spec())
        seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in _genomes()])
        images = ctx.sketch_batch(algo, K, p, 42, seq, rec_off, goff)
        regs = None
        if algo == "hmh":
            hdr = lash_amd.header_bytes("hmh", layout.spec() if layout is not None else None)
            assert images.shape == (N, hdr + 2 * S.M) and (hdr > 0) == (lay is not None)
            regs = S.registers(images, hdr, big_endian=lay is not None)
        _made[key] = (ctx, images, regs)
    return _made[key]


@pytest.fixture(scope="module")
def want():
    """the model's bins of GROUPS, per layout: the registers are the same numbers under both, so are the bins"""
    out = {}
    for lay, name in zip(CASES, IDS):
        _, _, regs = _case(lay)
        out[name] = [S.hist(regs, g) for g in GROUPS]
    assert all(np.array_equal(a, b) for a, b in zip(out["hmh"], out["hmh_be"]))
    return out


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("lay", CASES, ids=IDS)
def test_the_bins_equal_the_model_under_every_plan(want, lay):
    import torch
    ctx, images, regs = _case(lay)
    w = want[IDS[CASES.index(lay)]]
    # the collection exercises what it should: empty buckets, shared and private registers, a count above two
    assert [len(h) for h in w] == [len(g) + 1 for g in GROUPS] and all(int(h.sum()) == S.M for h in w)
    assert w[0].tolist() == [S.M] and w[9].tolist() == [S.M, 0] and 0 < int(w[1][0]) < S.M
    assert int(w[7][2]) > 0 and int(w[7][1]) > 0 and int(w[8][3]) > 0 and int(w[8][1]) > 0 and np.array_equal(w[7], w[10])
    s = ctx.sketch_set("hmh", 0, images)
    try:
        unions = s.group_union(GROUPS)
        for plan in PLANS:
            got = s.group_spectrum(GROUPS, **plan)
            assert _same(got, w), (plan, [g.tolist() for g in got], [h.tolist() for h in w])
        for plan in ({}, {"segment": 2, "slices": 7}, {"segment": 5, "scratch_budget": 1}):
            got, img = s.group_spectrum(GROUPS, union_images=True, **plan)
            assert _same(got, w) and img.shape == unions.shape and np.array_equal(img, unions), plan
        # the device form writes its bins and its images and nothing beyond them
        n_bins = sum(len(g) + 1 for g in GROUPS)
        for plan in ({}, {"segment": 2, "slices": 7}):
            d_hist = torch.full((n_bins + 4,), -1515870811, dtype=torch.int32, device="cuda")          # 0xA5A5A5A5
            d_img = torch.full((unions.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            for images_out in (d_img, None):
                d_hist.fill_(-1515870811)
                s.group_spectrum(GROUPS, device_out=(d_hist, images_out), **plan)
                ctx.synchronize()
                back = d_hist.cpu().numpy().view(np.uint32)
                assert np.array_equal(back[:n_bins], np.concatenate(w)) and (back[n_bins:] == 0xA5A5A5A5).all(), plan
            back = d_img.cpu().numpy()
            assert np.array_equal(back[:unions.size].reshape(unions.shape), unions) and (back[unions.size:] == 0xA5).all(), plan
        one = s.group_spectrum([list(range(N))])                                             # n_groups = 1
        assert len(one) == 1 and np.array_equal(one[0], w[7])
        assert s.group_spectrum([]) == []
    finally:
        s.free()


@pytest.mark.parametrize("lay", CASES, ids=IDS)
def test_a_pair_is_the_c_and_n_of_dist(lay):
    ctx, images, regs = _case(lay)
    pairs = [(0, 1), (2, DUP), (2, 9), (EMPTY, 4), (EMPTY, EMPTY), (23, 7), (5, 5)]
    s = ctx.sketch_set("hmh", 0, images)
    try:
        bins = s.group_spectrum([list(p) for p in pairs])
    finally:
        s.free()
    for (i, j), h in zip(pairs, bins):
        c, n = ctx.hmh_pair_counts(images[i:i + 1], images[j:j + 1])
        assert (int(h[2]), S.M - int(h[0])) == (int(c[0, 0]), int(n[0, 0])), (i, j, h.tolist())
    assert int(bins[1][1]) == 0 and int(bins[1][2]) > 0 and bins[4].tolist() == [S.M, 0, 0]


@pytest.mark.parametrize("algo,p", [("hll", 10), ("ull", 12)])
def test_other_sketches_are_refused(algo, p):
    import lash_amd
    ctx, images, _ = _case(None, algo, p)
    s = ctx.sketch_set(algo, p, images)
    try:
        with pytest.raises(lash_amd.LashError) as e:
            s.group_spectrum([[0, 1]])
        assert e.value.code == lash_amd.EINVAL and "not HyperMinHash" in str(e.value)
        hist = np.full(3, 7, dtype=np.uint32)
        off = np.array([0, 2], dtype=np.uint64)
        mem = np.array([0, 1], dtype=np.uint32)
        for call in (ctx._lib.lash_sketch_set_group_spectrum, ctx._lib.lash_sketch_set_group_spectrum_device):
            assert call(ctx._h, s._h, off.ctypes.data, mem.ctypes.data, 1, None, hist.ctypes.data, None, None) == lash_amd.EINVAL
            assert b"not HyperMinHash" in ctx._lib.lash_ctx_last_error(ctx._h)
        assert hist.tolist() == [7, 7, 7]
    finally:
        s.free()


def test_bad_arguments_are_refused(want):
    import lash_amd
    ctx, images, regs = _case(None)
    s = ctx.sketch_set("hmh", 0, images)
    try:
        for groups, at in (([[0, N, 1]], 1), ([[0, 1], [], [2, 3, 2**32 - 1]], 4), ([[N]], 0)):
            with pytest.raises(lash_amd.LashError) as e:
                s.group_spectrum(groups)
            assert e.value.code == lash_amd.EINVAL and e.value.index == at
        lib, bad = ctx._lib, C.c_uint64(77)
        hist = np.zeros(5, dtype=np.uint32)
        off = np.array([0, 2, 3], dtype=np.uint64)
        mem = np.array([1, 2, 3], dtype=np.uint32)
        for call in (lib.lash_sketch_set_group_spectrum, lib.lash_sketch_set_group_spectrum_device):
            assert call(None, s._h, off.ctypes.data, mem.ctypes.data, 2, None, hist.ctypes.data, None, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, None, off.ctypes.data, mem.ctypes.data, 2, None, hist.ctypes.data, None, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, None, mem.ctypes.data, 2, None, hist.ctypes.data, None, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, off.ctypes.data, None, 2, None, hist.ctypes.data, None, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, s._h, off.ctypes.data, mem.ctypes.data, 2, None, None, None, C.byref(bad)) == lash_amd.EINVAL
            for wrong in ([1, 2, 3], [0, 3, 2]):                                              # not from 0; decreasing
                w = np.array(wrong, dtype=np.uint64)
                assert call(ctx._h, s._h, w.ctypes.data, mem.ctypes.data, 2, None, hist.ctypes.data, None, C.byref(bad)) == lash_amd.EINVAL
                assert b"group_off" in lib.lash_ctx_last_error(ctx._h)
            assert call(ctx._h, s._h, off.ctypes.data, None, 0, None, None, None, None) == lash_amd.OK           # nothing to do
        assert bad.value == 77 and not hist.any()                                                               # no refusal named a member
        assert lib.lash_sketch_set_group_spectrum(ctx._h, s._h, off.ctypes.data, mem.ctypes.data, 2, None, hist.ctypes.data, None, None) == lash_amd.OK
        assert hist[:3].tolist() == S.hist(regs, [1, 2]).tolist() and hist[3:].tolist() == S.hist(regs, [3]).tolist()
    finally:
        s.free()


def test_the_set_keeps_its_state(want):
    ctx, images, regs = _case(None)
    s = ctx.sketch_set("hmh", 0, images)
    try:
        card = s.cardinalities()
        s.prepare()
        before = s.pair_block(0, s.n, triangle=True)
        assert _same(s.group_spectrum(GROUPS, segment=2), want["hmh"])
        after = s.pair_block(0, s.n, triangle=True)
        low = np.tril(np.ones((s.n, s.n), bool))
        for key in before:
            assert np.array_equal(before[key][low], after[key][low]), key
        assert s.cardinalities().view(np.uint64).tolist() == card.view(np.uint64).tolist()
    finally:
        s.free()
