"""lash_sketch_set_screen_wta (csrc/screen_wta.hip, lash_screen_api.hip) through the ABI.

The yardstick is tests/screen_model.py: equality, first position and counting over the registers of the images.  Every comparison is ==.

The references are a collection in the style of the group-spectrum test: 24 sketches of synthetic genomes of 2-30 kbp, one of them an
input shorter than k (the empty sketch), one an exact duplicate of another and one a prefix of another.  The queries are three: the
concatenation of several references (the duplicated one, the prefix's parent and strangers among them), one single reference, and an
empty input.  Both as HyperMinHash under the default layout and under one with big-endian registers behind a header.  The lists have 0,
1, 2, 17 and all 24 entries, repeat a row and reverse the priority; the counts must not depend on how the work is cut: segment 1, 2, 5
(winner tables merged with atomic minima) and 1000 (every list one task, stored directly), slices 1 and 7, a scratch budget of one byte
(one query per chunk)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import screen_model as W
import spectrum_model as S

pytestmark = pytest.mark.gpu

K = 16
N = 24
EMPTY, DUP, PREFIX = 6, 13, 17                                             # an input shorter than k; a copy of member 2; the first 40 % of member 20
PARENT = 20
MIX = [2, DUP, PARENT, 4, 9, 11]                                           # query 0: these references, one record each
SINGLE = 2                                                                 # query 1
NQ = 3                                                                     # query 2: an input shorter than k
BE = dict(hmh_reg="be", hmh_hdr="l")

ALL = list(range(N))
SEVENTEEN = [PREFIX, PARENT] + [i for i in range(N) if i not in (PREFIX, PARENT, 2, 4, 5, 7, 8, 10, 12)]   # the prefix before its parent; 2 and 4 left out
assert len(SEVENTEEN) == 17
LISTS = [
    [ALL, SEVENTEEN, []],
    [ALL[::-1], [DUP], [EMPTY, 3]],
    [[PARENT, 2, PARENT, DUP, 2, PREFIX], [], ALL],
    [[], [DUP, SINGLE], [5]],
]
PLANS = [{}, {"segment": 1}, {"segment": 2}, {"segment": 5}, {"slices": 1}, {"slices": 7}, {"segment": 2, "scratch_budget": 1},
         {"segment": 5, "slices": 3, "scratch_budget": 1}, {"segment": 1000}]
CASES = [None, BE]
IDS = ["hmh", "hmh_be"]


def _genomes():
    g = [O.synth_genome(1700 + i, 2_000 + 1_217 * i) for i in range(N)]
    g[EMPTY] = np.frombuffer(b"ACGTTGCA", np.uint8).copy()
    g[DUP] = g[2].copy()
    g[PREFIX] = g[PARENT][:len(g[PARENT]) * 2 // 5].copy()
    return g


def _queries():
    """record lists: the mix, the single reference, the input shorter than k"""
    g = _genomes()
    return [[g[i].tobytes() for i in MIX], [g[SINGLE].tobytes()], [b"ACGTTGCAAC"]]


def exercises(ref_regs, qry_regs):
    """the collection shows what the kernels have to get right (checked with the oracle's CPU sketches before the seeds were committed)"""
    assert not ref_regs[EMPTY].any() and not qry_regs[2].any() and np.array_equal(ref_regs[DUP], ref_regs[2])
    h = W.holds(ref_regs, qry_regs[0], ALL)
    assert int((h.sum(axis=0) >= 2).sum()) > 100                              # contested buckets: two or more holders among the candidates
    s, w = W.wta(ref_regs, qry_regs[0], ALL)
    assert int(w[DUP]) == 0 < int(s[DUP]) == int(s[2]) and int(w[2]) > 1000     # the copy, later in the list, wins nothing
    assert int(w[PREFIX]) > 0 and 0 < int(w[PARENT]) < int(s[PARENT])         # the prefix comes first and takes part of its parent's share
    s, w = W.wta(ref_regs, qry_regs[0], ALL[::-1])
    assert int(w[N - 1 - PREFIX]) == 0 < int(s[N - 1 - PREFIX])               # reversed: the parent comes first and leaves the prefix nothing
    assert int(w[N - 1 - 2]) == 0 < int(s[N - 1 - 2]) == int(s[N - 1 - DUP]) and int(w[N - 1 - DUP]) > 1000
    win = W.winners(ref_regs, qry_regs[0], SEVENTEEN)                         # NONE buckets: empty in the query, and occupied but nobody's
    assert int(((win == W.NONE) & (qry_regs[0] != 0)).sum()) > 100 and int(((win == W.NONE) & (qry_regs[0] == 0)).sum()) > 100
    s, w = W.wta(ref_regs, qry_regs[1], [DUP, SINGLE])
    assert int(s[0]) == int(s[1]) == int(w[0]) == int((qry_regs[1] != 0).sum()) > 1000 and int(w[1]) == 0


_made = {}


def _case(lay, algo="hmh", p=0):
    """(context, reference images, query images, their registers as the model reads them), made once per layout and table"""
    import lash_amd
    key = (algo, p, lay is not None)
    if key not in _made:
        ctx = lash_amd.Context(0)
        layout = O.make_layout(**lay) if lay else None
        if layout is not None:
            ctx.set_layout(layout.spec())
        seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in _genomes()])
        refs = ctx.sketch_batch(algo, K, p, 42, seq, rec_off, goff)
        seq, rec_off, goff = lash_amd.records_to_arrays(_queries())
        qrys = ctx.sketch_batch(algo, K, p, 42, seq, rec_off, goff)
        rr = qr = None
        if algo == "hmh":
            hdr = lash_amd.header_bytes("hmh", layout.spec() if layout is not None else None)
            assert refs.shape == (N, hdr + 2 * S.M) and qrys.shape == (NQ, hdr + 2 * S.M) and (hdr > 0) == (lay is not None)
            rr, qr = S.registers(refs, hdr, big_endian=lay is not None), S.registers(qrys, hdr, big_endian=lay is not None)
        _made[key] = (ctx, refs, qrys, rr, qr)
    return _made[key]


@pytest.fixture(scope="module")
def want():
    """the model's counts of LISTS, per layout: the registers are the same numbers under both, so are the counts"""
    out = {}
    for lay, name in zip(CASES, IDS):
        _, _, _, rr, qr = _case(lay)
        out[name] = [W.screen(rr, qr, lists) for lists in LISTS]
    for (sa, wa), (sb, wb) in zip(out["hmh"], out["hmh_be"]):
        assert all(np.array_equal(a, b) for a, b in zip(sa + wa, sb + wb))
    return out


def _same(got, want):
    return all(len(g) == len(w) and all(x.dtype == np.uint32 and np.array_equal(x, y) for x, y in zip(g, w)) for g, w in zip(got, want))


@pytest.mark.parametrize("lay", CASES, ids=IDS)
def test_the_counts_equal_the_model_under_every_plan(want, lay):
    import torch
    ctx, refs, qrys, rr, qr = _case(lay)
    w = want[IDS[CASES.index(lay)]]
    exercises(rr, qr)
    r, q = ctx.sketch_set("hmh", 0, refs), ctx.sketch_set("hmh", 0, qrys)
    try:
        for lists, model in zip(LISTS, w):
            for plan in PLANS:
                got = r.screen_wta(q, lists, **plan)
                assert _same(got, model), (lists, plan, [x.tolist() for x in got[0] + got[1]], [x.tolist() for x in model[0] + model[1]])
        # the device form writes its counts and nothing beyond them
        lists, model = LISTS[0], w[0]
        n = sum(len(l) for l in lists)
        for plan in ({}, {"segment": 2, "slices": 7}, {"segment": 5, "scratch_budget": 1}):
            d_shared = torch.full((n + 4,), -1515870811, dtype=torch.int32, device="cuda")              # 0xA5A5A5A5
            d_won = torch.full((n + 4,), -1515870811, dtype=torch.int32, device="cuda")
            r.screen_wta(q, lists, device_out=(d_shared, d_won), **plan)
            ctx.synchronize()
            for back, part in ((d_shared.cpu().numpy().view(np.uint32), model[0]), (d_won.cpu().numpy().view(np.uint32), model[1])):
                assert np.array_equal(back[:n], np.concatenate(part)) and (back[n:] == 0xA5A5A5A5).all(), plan
        # every list empty: nothing to do
        s, wn = r.screen_wta(q, [[], [], []])
        assert [len(x) for x in s] == [0, 0, 0] and [len(x) for x in wn] == [0, 0, 0]
        # a set screened against itself
        s, wn = r.screen_wta(r, [[i] for i in range(N)])
        occupied = (rr != 0).sum(axis=1)
        assert [int(x[0]) for x in s] == occupied.tolist() == [int(x[0]) for x in wn]
    finally:
        q.free()
        r.free()


@pytest.mark.parametrize("lay", CASES, ids=IDS)
def test_shared_is_the_c_of_dist(want, lay):
    ctx, refs, qrys, rr, qr = _case(lay)
    c, _ = ctx.hmh_pair_counts(refs, qrys)
    for lists, (shared, _) in zip(LISTS, want[IDS[CASES.index(lay)]]):
        for j, rows in enumerate(lists):
            assert [int(c[i, j]) for i in rows] == shared[j].tolist(), (j, rows)


@pytest.mark.parametrize("algo,p", [("hll", 10), ("ull", 12)])
def test_other_sketches_are_refused(algo, p):
    import lash_amd
    ctx, refs, qrys, _, _ = _case(None, algo, p)
    _, hrefs, hqrys, _, _ = _case(None)
    other_r, other_q = ctx.sketch_set(algo, p, refs), ctx.sketch_set(algo, p, qrys)
    hmh_r, hmh_q = ctx.sketch_set("hmh", 0, hrefs), ctx.sketch_set("hmh", 0, hqrys)
    try:
        for r, q, which in ((other_r, other_q, "reference"), (other_r, hmh_q, "reference"), (hmh_r, other_q, "query")):
            with pytest.raises(lash_amd.LashError) as e:
                r.screen_wta(q, [[0, 1], [], [2]])
            assert e.value.code == lash_amd.EINVAL and "not HyperMinHash" in str(e.value) and which in str(e.value)
            shared, won = np.full(3, 7, dtype=np.uint32), np.full(3, 9, dtype=np.uint32)
            off = np.array([0, 2, 2, 3], dtype=np.uint64)
            mem = np.array([0, 1, 2], dtype=np.uint32)
            for call in (ctx._lib.lash_sketch_set_screen_wta, ctx._lib.lash_sketch_set_screen_wta_device):
                assert call(ctx._h, r._h, q._h, off.ctypes.data, mem.ctypes.data, None, shared.ctypes.data, won.ctypes.data, None) == lash_amd.EINVAL
                assert b"not HyperMinHash" in ctx._lib.lash_ctx_last_error(ctx._h)
            assert shared.tolist() == [7, 7, 7] and won.tolist() == [9, 9, 9]
    finally:
        for s in (other_r, other_q, hmh_r, hmh_q):
            s.free()


def test_bad_arguments_are_refused(want):
    import lash_amd
    ctx, refs, qrys, rr, qr = _case(None)
    r, q = ctx.sketch_set("hmh", 0, refs), ctx.sketch_set("hmh", 0, qrys)
    try:
        for lists, at in (([[0, N, 1], [], []], 1), ([[0, 1], [], [2, 3, 2**32 - 1]], 4), ([[], [N], []], 0)):
            with pytest.raises(lash_amd.LashError) as e:
                r.screen_wta(q, lists)
            assert e.value.code == lash_amd.EINVAL and e.value.index == at and "does not have" in str(e.value)
        lib, bad = ctx._lib, C.c_uint64(77)
        shared, won = np.full(3, 7, dtype=np.uint32), np.full(3, 9, dtype=np.uint32)
        off = np.array([0, 2, 2, 3], dtype=np.uint64)
        mem = np.array([1, 2, 3], dtype=np.uint32)
        sp, wp = shared.ctypes.data, won.ctypes.data
        for call in (lib.lash_sketch_set_screen_wta, lib.lash_sketch_set_screen_wta_device):
            assert call(None, r._h, q._h, off.ctypes.data, mem.ctypes.data, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, None, q._h, off.ctypes.data, mem.ctypes.data, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, r._h, None, off.ctypes.data, mem.ctypes.data, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, r._h, q._h, None, mem.ctypes.data, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, r._h, q._h, off.ctypes.data, None, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, r._h, q._h, off.ctypes.data, mem.ctypes.data, None, None, wp, C.byref(bad)) == lash_amd.EINVAL
            assert call(ctx._h, r._h, q._h, off.ctypes.data, mem.ctypes.data, None, sp, None, C.byref(bad)) == lash_amd.EINVAL
            for wrong in ([1, 2, 2, 3], [0, 3, 2, 3]):                                        # not from 0; decreasing
                w = np.array(wrong, dtype=np.uint64)
                assert call(ctx._h, r._h, q._h, w.ctypes.data, mem.ctypes.data, None, sp, wp, C.byref(bad)) == lash_amd.EINVAL
                assert b"cand_off" in lib.lash_ctx_last_error(ctx._h)
            none = np.zeros(4, dtype=np.uint64)
            assert call(ctx._h, r._h, q._h, none.ctypes.data, None, None, None, None, None) == lash_amd.OK      # nothing to do
        assert bad.value == 77 and shared.tolist() == [7, 7, 7] and won.tolist() == [9, 9, 9]                   # no refusal named a row or wrote
        assert lib.lash_sketch_set_screen_wta(ctx._h, r._h, q._h, off.ctypes.data, mem.ctypes.data, None, sp, wp, None) == lash_amd.OK
        ms, mw = W.screen(rr, qr, [[1, 2], [], [3]])
        assert shared.tolist() == np.concatenate(ms).tolist() and won.tolist() == np.concatenate(mw).tolist()
    finally:
        q.free()
        r.free()


def test_the_sets_keep_their_state(want):
    ctx, refs, qrys, rr, qr = _case(None)
    r, q = ctx.sketch_set("hmh", 0, refs), ctx.sketch_set("hmh", 0, qrys)
    try:
        rcard, qcard = r.cardinalities(), q.cardinalities()
        r.prepare(q)
        before = r.pair_block(0, r.n, qry=q)
        assert _same(r.screen_wta(q, LISTS[0], segment=2), want["hmh"][0])
        after = r.pair_block(0, r.n, qry=q)
        for key in before:
            assert np.array_equal(before[key], after[key]), key
        assert r.cardinalities().view(np.uint64).tolist() == rcard.view(np.uint64).tolist()
        assert q.cardinalities().view(np.uint64).tolist() == qcard.view(np.uint64).tolist()
    finally:
        q.free()
        r.free()
