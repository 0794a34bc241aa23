"""The stand-alone pair entries (lash_hmh_pair_counts, lash_hll_pair_union_stats, lash_ull_pair_union_estimates) bind the
context's two call-scoped sketch sets to each call's images (lash_set_bind, sketch_set.hip).  The host entries stage every call
at the same device address, so a bind that kept anything derived from the previous call's images (planes, `full`, the register
range, the bitmaps) would answer the next call from stale operands.  One context, calls in an order in which each derived
state changes from one call to the next, every result against numpy."""
from fractions import Fraction

import numpy as np
import pytest

import ullref as U

pytestmark = pytest.mark.gpu


def _hll(regs):
    img = np.zeros((len(regs), 33 + regs.shape[1]), np.uint8)
    img[:, 33:] = regs
    return img


def _hll_want(ref, qry):
    """zero = #{max(a, b) == 0}; sum = sum 2^-max(a, b), rounded once from the exact rational"""
    zero = np.zeros((len(ref), len(qry)), np.uint32)
    s = np.zeros((len(ref), len(qry)), np.float64)
    for i in range(len(ref)):
        for j in range(len(qry)):
            mx = np.maximum(ref[i, 33:], qry[j, 33:])
            zero[i, j] = (mx == 0).sum()
            s[i, j] = float(sum(Fraction(int(c), 1 << r) for r, c in enumerate(np.bincount(mx)) if c))
    return zero, s


def _hmh_want(ref, qry):
    c = ((ref[:, None, :] == qry[None, :, :]) & (ref[:, None, :] != 0)).sum(axis=2)
    n = ((ref[:, None, :] != 0) | (qry[None, :, :] != 0)).sum(axis=2)
    return c.astype(np.uint32), n.astype(np.uint32)


def test_rebinding_on_one_context():
    import lash_amd
    import torch
    rng = np.random.default_rng(2024)

    def regs(p, lo, hi):
        return _hll(rng.integers(lo, hi, (3, 1 << p), dtype=np.uint8)), _hll(rng.integers(lo, hi, (2, 1 << p), dtype=np.uint8))

    cases = [("bitmaps, not wide, no zero", 12) + regs(12, 5, 21),
             ("same address, WIDE and ZERO, a band across 32", 12) + regs(12, 0, 41),
             ("hi == lo: byte-wise", 12, _hll(np.full((3, 4096), 9, np.uint8)), _hll(np.full((2, 4096), 9, np.uint8))),
             ("smallest bitmap precision", 10) + regs(10, 3, 30),
             ("byte-wise precision", 9) + regs(9, 0, 25)]
    assert cases[1][2][:, 33:].min() == 0 and cases[1][2][:, 33:].max() == 40
    with lash_amd.Context(0) as ctx:
        for what, p, ref, qry in cases:
            z, s = ctx.hll_pair_union_stats(p, ref, qry)
            wz, ws = _hll_want(ref, qry)
            assert np.array_equal(z, wz) and np.array_equal(s.view(np.uint64), ws.view(np.uint64)), what
        # reference == query: one set on both sides (the device entry; the host entry stages two copies)
        ref = cases[1][2]
        d = torch.from_numpy(ref).cuda()
        dz, ds = torch.zeros((3, 3), dtype=torch.int32, device="cuda"), torch.zeros((3, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.hll_pair_union_stats_device(12, d, 3, d, 3, dz, ds)
        ctx.synchronize()
        wz, ws = _hll_want(ref, ref)
        assert np.array_equal(dz.cpu().numpy().view(np.uint32), wz) and np.array_equal(ds.cpu().numpy().view(np.uint64), ws.view(np.uint64))

        # HyperMinHash on the same context: `full` off, on, then one set on both sides
        a0, b0 = rng.integers(0, 5, (5, 16384), dtype=np.uint16), rng.integers(0, 5, (3, 16384), dtype=np.uint16)
        a1, b1 = rng.integers(1, 5, (5, 16384), dtype=np.uint16), rng.integers(1, 5, (3, 16384), dtype=np.uint16)
        assert (a0 == 0).any() and (a1 != 0).all()
        for a, b in ((a0, b0), (a1, b1), (a0, b0)):
            c, n = ctx.hmh_pair_counts(a.view(np.uint8).reshape(5, -1), b.view(np.uint8).reshape(3, -1))
            wc, wn = _hmh_want(a, b)
            assert np.array_equal(c, wc) and np.array_equal(n, wn)
            assert (n == 16384).all() == (a is a1)
        d = torch.from_numpy(a0[:3].view(np.uint8).reshape(3, -1).copy()).cuda()
        dc, dn = torch.zeros((3, 3), dtype=torch.int32, device="cuda"), torch.zeros((3, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.hmh_pair_counts_device(d, 3, d, 3, dc, dn)
        ctx.synchronize()
        wc, wn = _hmh_want(a0[:3], a0[:3])
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), wc) and np.array_equal(dn.cpu().numpy().view(np.uint32), wn)

        # UltraLogLog on the same context (its operands are the images themselves)
        p = 11
        ur, uq = np.zeros((3, 8 + (1 << p)), np.uint8), np.zeros((2, 8 + (1 << p)), np.uint8)
        ur[:, 8:] = rng.integers(4 * p + 12, 4 * p + 44, (3, 1 << p))
        uq[:, 8:] = rng.integers(4 * p + 12, 4 * p + 44, (2, 1 << p))
        got = ctx.ull_pair_union_estimates(p, ur, uq, "fgra")
        for i in range(3):
            for j in range(2):
                want = float(U.fgra_ref(U.merge_hist(U.regs_of(ur[i]), U.regs_of(uq[j])), p))
                assert abs(got[i, j] - want) <= ((1 << p) + 1024) * 2.0 ** -52 * want, (i, j)
        # and HyperLogLog once more after the others have used the sets
        what, p, ref, qry = cases[0]
        z, s = ctx.hll_pair_union_stats(p, ref, qry)
        wz, ws = _hll_want(ref, qry)
        assert np.array_equal(z, wz) and np.array_equal(s.view(np.uint64), ws.view(np.uint64))
