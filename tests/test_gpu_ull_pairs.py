"""The three UltraLogLog pair kernels of dist_kernels.hip (ull_fgra_fast_kernel, ull_pairs_kernel<false> with 16-bit bins for
p <= 15, ull_pairs_kernel<true> with 32-bit bins above) against the 60-digit reference of tests/ullref.py: the estimate of
pair (i, j) is fgra_ref / ml_ref of the histogram of merge_ref(ref_i, qry_j).  Nothing here goes through ull_estimators.h.

Bounds as in tests/test_ull_reference.py: FGRA relative (m + 1024) 2^-52, ML relative 2 * 0.001 * 0.7608 / sqrt(m), exact
for 0 and +inf.  No entry refuses saturated registers (r >= 252) or any byte, so everything a sketch can hold is given.
One deviation from "all_pairs(p) at p = 3": that is 7442 image pairs of 8 registers, and their 14 884 references take
longer than a test may; test_merge_table_every_pair_of_values estimates every 15th of them, and
test_every_pair_of_values_alone takes all 59 536 ordered pairs of values one register at a time (244 references).

Measured on an MI355X (test_regimes prints these with -s), worst |got - ref| / ref over 11 x 13 images + 3 x 5 dense ones:
  p      3        8        9        10       12       15       16       18       20
  FGRA   4.1e-15  1.1e-14  1.5e-14  1.2e-14  8.8e-14  3.8e-13  1.4e-11  2.0e-11  1.8e-11
  bound  2.3e-13  2.8e-13  3.4e-13  4.6e-13  1.1e-12  7.5e-12  1.5e-11  5.8e-11  2.3e-10
  ML     5.0e-07  2.9e-08  9.3e-10  1.3e-09  1.3e-09  1.4e-09  1.4e-09  1.4e-09  1.4e-09
  bound  5.4e-04  9.5e-05  6.7e-05  4.8e-05  2.4e-05  8.4e-06  5.9e-06  3.0e-06  1.5e-06
The p >= 16 FGRA figures are the almost empty sketches of tests/test_ull_reference.py's docstring (the same on the host).
Wall time per case on that machine (16 s for the file): test_fast_path_on_and_off 2.1 s (p = 9), 3.1 s (p = 16), a child process
each; test_merge_table_every_pair_of_values 0.9 / 2.8 / 0.1 / 0.1 s at p = 3 / 10 / 15 / 16 (p = 10: 46 x 2 references of 200 bins);
test_regimes 0.1 to 0.3 s up to p = 16, 0.6 s at p = 18, 1.6 s at p = 20; test_every_pair_of_values_alone 0.3 s;
test_resident_set 0.01 s at p = 10, 0.1 s at p = 16.

Mutations of the kernels, each tried on a scratch build: one entry of ull_merge_fast's table changed (0x55FAE4 -> 0x55F6E4) fails
every test of this file; UllLaneHist's & 0xFFFF narrowed to 0x7FFF fails test_regimes[15] alone (the bins that hold all 2^15
registers); the fix-up's isnan(*dst) dropped fails test_fast_path_on_and_off at both p.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ullref as U
from ullref import TINY_FILLER, TINY_P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(p, ref, qry, cells=None):
    """(fgra, ml, regular) [n_ref, n_qry]: the references of every merged pair (NaN where not asked for) and whether all
    its registers are regular, i.e. whether ull_fgra_fast_kernel finishes the pair itself"""
    nr, nq = len(ref), len(qry)
    f, ml = np.full((nr, nq), np.nan), np.full((nr, nq), np.nan)
    regular = np.zeros((nr, nq), bool)
    for i, j in (cells if cells is not None else [(i, j) for i in range(nr) for j in range(nq)]):
        hist = U.merge_hist(U.regs_of(ref[i]), U.regs_of(qry[j]))
        f[i, j], ml[i, j] = U.fgra_ref(hist, p), U.ml_ref(hist, p)
        regular[i, j] = hist[:4 * p + 4].sum() == 0 and hist[252:].sum() == 0
    return f, ml, regular


def _worst(got, want, tol, what):
    """largest relative error over the cells `want` has; 0 and +inf exactly; asserts the bound"""
    ask = ~np.isnan(want)
    exact = ask & ((want == 0) | np.isinf(want))
    assert np.array_equal(got[exact], want[exact]), what
    rest = ask & ~exact
    err = np.abs(got[rest] - want[rest]) / want[rest]
    assert not np.isnan(err).any(), what
    worst = float(err.max()) if err.size else 0.0
    assert worst <= tol, (what, worst, tol, np.argwhere(rest)[int(err.argmax())])
    return worst


@pytest.mark.parametrize("p", [3, 10, 15, 16])
def test_merge_table_every_pair_of_values(p):
    """all_pairs(p): position k of image pair i holds one ordered pair of register values; the estimate of that pair of images is
    the reference of the merged histogram.  (p = 3 needs 7442 image pairs of 8 registers: every 15th is estimated here, and
    test_every_pair_of_values_alone takes all 59 536 value pairs one by one.)"""
    import lash_amd
    pairs = U.all_pairs(p)
    if p == 3:
        pairs = pairs[::15]
    ref, qry = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    diag = [(i, i) for i in range(len(pairs))]
    wf, wm, _ = _want(p, ref, qry, diag)
    with lash_amd.Context(0) as ctx:
        for est, want, tol in (("fgra", wf, U.fgra_tol(p)), ("ml", wm, U.ml_tol(p))):
            got = np.full(want.shape, np.nan)
            for c in range(0, len(pairs), 64):                  # the diagonal blocks hold the pairs that belong together
                s = slice(c, c + 64)
                got[s, s] = ctx.ull_pair_union_estimates(p, ref[s], qry[s], est)
            _worst(got, want, tol, (p, est))


def _tiny_images(p, values):
    imgs = np.full((len(values), 1 << p), TINY_FILLER, np.uint8)
    imgs[:, 0] = values
    return np.stack([U.image(r, p) for r in imgs])


def test_every_pair_of_values_alone():
    """p = 3: sketch a = (a, filler x 7), sketch b = (b, filler x 7) for all 244 x 244 ordered pairs of values in one call; the
    merged sketch is (merge(a, b), filler x 7).  test_ull_reference.py shows that any other merge result moves FGRA by more
    than 1e6 tolerances."""
    import lash_amd
    p = TINY_P
    v = np.array(U.valid_values(p), np.uint8)
    imgs = _tiny_images(p, v)
    merged = U.merge_ref(np.repeat(v, len(v)), np.tile(v, len(v))).reshape(len(v), len(v))
    by_value = {}
    for r in np.unique(merged):
        hist = np.zeros(256, np.int64)
        hist[TINY_FILLER] += (1 << p) - 1
        hist[r] += 1
        by_value[int(r)] = (U.fgra_ref(hist, p), U.ml_ref(hist, p))
    with lash_amd.Context(0) as ctx:
        for k, (est, tol) in enumerate((("fgra", U.fgra_tol(p)), ("ml", U.ml_tol(p)))):
            got = ctx.ull_pair_union_estimates(p, imgs, imgs, est)
            want = np.array([[by_value[int(r)][k] for r in row] for row in merged])
            _worst(got, want, tol, est)


P_REGIMES = [3, 8, 9, 10, 12, 15, 16, 18, 20]


@pytest.mark.parametrize("p", P_REGIMES)
def test_regimes(p):
    """11 x 13 images (one partial tile of the fast kernel and of both histogram forms): sampled regular / small-range /
    saturated sketches, flat and half-and-half ones.  The fast kernel's tile holds pairs it finishes and pairs it leaves as
    NaN for the fix-up launch; p = 15 flat x flat puts 32 768 into one 16-bit bin, in the even and in the odd half of a word."""
    import lash_amd
    t0 = time.time()
    ref, qry = U.regime_images(p)
    assert ref.shape[0] == 11 and qry.shape[0] == 13
    rng = np.random.default_rng(p)
    dref, dqry = np.stack([U.dense(rng, p) for _ in range(3)]), np.stack([U.dense(rng, p) for _ in range(5)])
    wf, wm, regular = _want(p, ref, qry)
    df, dm, dregular = _want(p, dref, dqry)
    assert _tiles_are_mixed(regular) and dregular.all()
    if p == 15:
        hists = [U.merge_hist(U.regs_of(ref[i]), U.regs_of(qry[j])) for i in range(11) for j in range(13)]
        full = {int(h.argmax()) for h in hists if h.max() == 1 << p}
        assert any(r & 1 for r in full) and any(not r & 1 for r in full) and 0 in full
    t1 = time.time()
    with lash_amd.Context(0) as ctx:
        gf, gm = ctx.ull_pair_union_estimates(p, ref, qry, "fgra"), ctx.ull_pair_union_estimates(p, ref, qry, "ml")
        hf, hm = ctx.ull_pair_union_estimates(p, dref, dqry, "fgra"), ctx.ull_pair_union_estimates(p, dref, dqry, "ml")
    t2 = time.time()
    worst_f = max(_worst(gf, wf, U.fgra_tol(p), (p, "fgra")), _worst(hf, df, U.fgra_tol(p), (p, "fgra dense")))
    worst_m = max(_worst(gm, wm, U.ml_tol(p), (p, "ml")), _worst(hm, dm, U.ml_tol(p), (p, "ml dense")))
    print("p=%d worst relative error: fgra %.2e (bound %.2e), ml %.2e (bound %.2e); reference %.1f s, GPU calls %.2f s"
          % (p, worst_f, U.fgra_tol(p), worst_m, U.ml_tol(p), t1 - t0, t2 - t1))


def _tiles_are_mixed(regular):
    """every tile of the fast kernel (16 x 16) and of the histogram kernels (16 x 16 for p <= 15, 8 x 16 above) holds a pair
    the fast kernel finishes and a pair it leaves as NaN"""
    for rows in (8, 16):
        for r0 in range(0, regular.shape[0], rows):
            for c0 in range(0, regular.shape[1], 16):
                tile = regular[r0:r0 + rows, c0:c0 + 16]
                if not (tile.any() and not tile.all()):
                    return False
    return True


@pytest.mark.parametrize("p", [9, 16])
def test_fast_path_on_and_off(tmp_path, p):
    """LASH_ULL_NO_FAST=1 (read once per process): the histogram kernel alone.  Both routes meet the reference.  The pairs the
    fast kernel leaves to the fix-up launch come from the same histogram code: bit-equal between the routes.  The pairs it
    finishes must survive the fix-up launch of their (mixed) tile: bit-equal to the same pairs in a call where every pair is
    regular, so that the fix-up returns at once, and not all of them bit-equal to the histogram kernel's values (m terms
    added in register order against at most 256 products: were they all equal, the comparison would show nothing)."""
    import lash_amd
    ref, qry = U.regime_images(p)
    wf, _, regular = _want(p, ref, qry)
    assert _tiles_are_mixed(regular)
    rows = [i for i in range(len(ref)) if regular[i].sum() >= 8]            # the flat and half-and-half images of regular values
    cols = [j for j in range(len(qry)) if regular[rows, j].all()]
    assert len(rows) >= 3 and len(cols) >= 8
    np.save(tmp_path / "ref.npy", ref)
    np.save(tmp_path / "qry.npy", qry)
    with lash_amd.Context(0) as ctx:
        fast = ctx.ull_pair_union_estimates(p, ref, qry, "fgra")
        alone = ctx.ull_pair_union_estimates(p, ref[rows], qry[cols], "fgra")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import lash_amd\n"
            "ref, qry = np.load(%r), np.load(%r)\n"
            "with lash_amd.Context(0) as ctx:\n"
            "    np.save(%r, ctx.ull_pair_union_estimates(%d, ref, qry, 'fgra'))\n"
            % (ROOT, str(tmp_path / "ref.npy"), str(tmp_path / "qry.npy"), str(tmp_path / "slow.npy"), p))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LASH_ULL_NO_FAST="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    slow = np.load(tmp_path / "slow.npy")
    _worst(fast, wf, U.fgra_tol(p), "fast")
    _worst(slow, wf, U.fgra_tol(p), "histogram only")
    assert np.array_equal(fast[~regular].view(np.uint64), slow[~regular].view(np.uint64))
    block = np.ix_(rows, cols)
    assert np.array_equal(fast[block].view(np.uint64), alone.view(np.uint64))
    differ = int((fast[block].view(np.uint64) != slow[block].view(np.uint64)).sum())
    print("p=%d: %d of %d finished pairs differ bitwise between the fast and the histogram kernel" % (p, differ, alone.size))
    assert differ > 0


@pytest.mark.parametrize("p", [10, 16])
@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_resident_set(p, est):
    """the same images as a resident set: cardinalities are the reference of each image alone; row blocks whose bounds are no
    multiples of 8, as triangle and as rectangle, are bit-equal to the whole-matrix entry in the cells they print"""
    import lash_amd
    ref, qry = U.regime_images(p)
    imgs = np.concatenate([ref, qry[[2, 8]]])                   # 13 different images
    n = len(imgs)
    tol = U.fgra_tol(p) if est == "fgra" else U.ml_tol(p)
    alone = np.array([[(U.fgra_ref if est == "fgra" else U.ml_ref)(U.hist_of(U.regs_of(i)), p) for i in imgs]])
    with lash_amd.Context(0) as ctx:
        whole = ctx.ull_pair_union_estimates(p, imgs, imgs, est)
        s = ctx.sketch_set("ull", p, imgs)
        _worst(s.cardinalities(est)[None, :], alone, tol, "cardinalities")
        for r0, r1 in ((0, 3), (3, 10), (10, n)):
            tri = s.pair_block(r0, r1, n_cols=r1, triangle=True, estimator=est)["sum_or_union"]
            rect = s.pair_block(r0, r1, estimator=est)["sum_or_union"]
            assert np.array_equal(rect.view(np.uint64), whole[r0:r1].view(np.uint64))
            for i in range(r0, r1):
                assert np.array_equal(tri[i - r0, :i + 1].view(np.uint64), whole[i, :i + 1].view(np.uint64)), i
        s.free()
    w = _want(p, imgs, imgs)[0 if est == "fgra" else 1]
    _worst(whole, w, tol, "whole")
    _worst(np.diag(whole)[None, :], alone, tol, "a sketch merged with itself")
