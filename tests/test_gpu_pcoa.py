"""lash_tree_build_pcoa (csrc/dist_pcoa.hip) through the ABI on synthetic matrices against the numpy model (pcoa_model.py).

Sizes: n = 2 and 3 (n < m, k' = n - 1 < K), 15, 16, 17 (around one 16-row strip of the product kernel and around m = 16; n <= m for K = 16),
65 (past one 64-row stage of Q and of the Gram chunks), 257 (past the 128 rows of a workgroup and a 256-thread sweep), 1000 (several
workgroups and segments, no multiple of 16 or 64).  K = 1, 3 (m = 9 and 11: 16-column panels) and 16 (m = 32: 32-column panels).

Inputs (pcoa_model.KINDS): euclidean, non_euclidean (a negative eigenvalue larger in size than theta_K: what an iteration by size gets
wrong; a 2 x 2 matrix is always Euclidean, so n = 2 is not in that kind, and 3 points have one positive eigenvalue above the size of
the negative one, so (n = 3, K = 1) cannot have the property and only runs), line (rank 1: every K > 1 is above the rank).

The gap condition is a condition on the input, asserted on the numpy spectrum alone: the axes the input was built around, the first
min(k', 3) of the R^8 kinds (their scales 8, 5, 3 set the leading eigenvalues apart; from the fourth on they lie closer than 0.05
lambda_1 by construction, and K = 16 reaches into the null space of a rank-8 matrix whatever the seed) and the one axis of `line`, lie at
least GAP * lambda_1 from every other eigenvalue of B.  SEEDS were searched on the CPU for that.  On those axes the coordinates must be
within (4 tol lambda_1 / gap_a) sqrt(lambda_a) + 2 tol sqrt(lambda_1) of the model's, and so must those of every other axis whose own gap_a
is at least 100 tol lambda_1 (the bound is then as loose as the gap is small, but it is the derived one).  On the rest (equal eigenvalues
up to rounding, the null space of a low-rank B: any rotation within the eigenspace is a valid answer) what is checked instead is what
holds for every valid answer: the eigenvalue bound, the residual of the axis against numpy's B, and |X - X_model| <= sqrt(theta+) +
sqrt(lambda+) <= 2 sqrt(lambda+ + 2 tol lambda_1).

diagonal_negative (n = 65, 257; K = 1, 3) is the input on which ranking eigenvalues by size fails even with spare vectors: nine negative
eigenvalues, each five times lambda_3 in size, against eight spare vectors, so lambda_3 must come from the positive-definite pass."""
import functools

import numpy as np
import pytest

import pcoa_model as P
import tree_model as T

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 0.05
SIZES, SEEDS = P.SIZES, P.SEEDS
KS = (1, 3, 16)
DESIGNED_AXES = {"euclidean": 3, "non_euclidean": 3, "line": 1, "diagonal_negative": 3}
CASES = [(kind, n, k) for kind in P.KINDS for n in SIZES for k in KS if n in SEEDS[kind] and (kind != "diagonal_negative" or k <= 3)]
DETERMINED = 100 * TOL                                                       # a gap, over lambda_1, above which an axis is held to the model's


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _input(kind, n):
    """(distances, B, every eigenvalue of B descending, its eigenvectors), computed once"""
    d = P.KINDS[kind](n, SEEDS[kind][n])
    b = P.centre(d)
    w, v = np.linalg.eigh(b)
    for x in (d, b, w, v):
        x.setflags(write=False)
    return d, b, w[::-1], v[:, ::-1]


def _build(ctx, d, k, blocks=None, **kw):
    n = d.shape[0]
    t = T.Tree(ctx, n)
    try:
        for r0, r1 in blocks if blocks is not None else [(0, n)]:
            t.set_rows(r0, r1, d)
        return P.pcoabuild(t, k, **kw)
    finally:
        t.free()


@pytest.mark.parametrize("kind,n,k", CASES)
def test_axes_against_the_model(ctx, kind, n, k):
    d, b, lam, _ = _input(kind, n)
    kk = min(k, n - 1)
    lam1 = lam[0]
    checked = min(kk, DESIGNED_AXES[kind])
    gap = np.array([np.min(np.abs(np.delete(lam, a) - lam[a])) for a in range(kk)])
    assert np.all(gap[:checked] >= GAP * lam1), ("the input misses the gap condition", gap[:checked] / lam1)
    if kind == "non_euclidean" and (n, k) != (3, 1):
        assert -lam[-1] > lam[kk - 1]
    if kind == "diagonal_negative" and k == 3:                                                  # more large negatives than spare vectors
        assert np.sum(-lam > 4 * lam[2]) == 9 > max(2 * k, k + 8) - k and np.all(np.abs(lam[3:-9]) < 1e-9 * lam1)
    want_eig, want_x, want_trace = P.pcoa(d, k)
    eig, x, st = _build(ctx, d, k, tol=TOL)
    print(kind, n, k, "iterations", st["iterations"], "worst", st["worst_residual"], "shift / lambda_1", st["shift"] / lam1,
          "eig err / lambda_1", np.max(np.abs(eig[:kk] - lam[:kk])) / lam1)
    # eigenvalues
    assert np.all(np.abs(eig[:kk] - lam[:kk]) <= 2 * TOL * lam1)
    assert np.all(eig[kk:] == 0) and not np.any(np.signbit(eig[kk:]))
    # zeros: beyond n - 1 and where theta <= 0, exactly +0.0
    for a in range(k):
        if a >= kk or not eig[a] > 0:
            assert np.all(x[:, a] == 0) and not np.any(np.signbit(x[:, a])), a
    # the sign rule and the residual, on the output itself
    for a in range(kk):
        if eig[a] > 0:
            col = x[:, a]
            assert col[int(np.argmax(np.abs(col)))] > 0, a
            assert abs(col @ col - eig[a]) <= 1e-12 * lam1, a                                     # |v_a| = 1
            assert np.linalg.norm(b @ col - eig[a] * col) <= 2 * TOL * lam1 * np.sqrt(eig[a]), a
    # coordinates
    for a in range(kk):
        sign = -1.0 if x[:, a] @ want_x[:, a] < 0 else 1.0
        err = np.max(np.abs(sign * x[:, a] - want_x[:, a]))
        if a < checked or gap[a] >= DETERMINED * lam1:
            bound = (4 * TOL * lam1 / gap[a]) * np.sqrt(max(lam[a], 0.0)) + 2 * TOL * np.sqrt(lam1)
        else:
            bound = 2 * np.sqrt(max(lam[a], 0.0) + 2 * TOL * lam1)
        print("  axis", a, "coordinate error", err, "bound", bound)
        assert err <= bound, (a, err, bound)
    # stats
    assert abs(st["trace"] - want_trace) <= 1e-12 * np.linalg.norm(b)
    assert st["worst_residual"] <= TOL and st["bytes"] == 8 * n * n and st["products"] == st["iterations"] >= 1
    assert st["shift"] > 0


@pytest.mark.parametrize("kind,n,k", [("non_euclidean", 65, 3), ("euclidean", 257, 16), ("line", 17, 16)])
def test_the_same_bits_whatever_set_rows_received(ctx, kind, n, k):
    d = _input(kind, n)[0]
    sevens = [(r, min(r + 7, n)) for r in range(0, n, 7)]
    block = np.array(d)
    block[np.triu_indices(n, 1)] = np.nan                                                       # only the triangle is read
    want = None
    for what, blocks in (("whole", [(0, n)]), ("blocks of 7", sevens), ("blocks of 7, reversed", sevens[::-1]), ("a second tree", [(0, n)])):
        eig, x, st = _build(ctx, block, k, blocks=blocks, tol=TOL)
        got = (eig.tobytes(), x.tobytes(), st["iterations"], np.float64(st["trace"]).tobytes())
        if want is None:
            want = got
        assert got == want, what


def test_refusals(ctx):
    n = 40
    d = _input("euclidean", 65)[0][:n, :n]
    # k outside 1..16
    for k in (0, 17):
        with pytest.raises(P.PcoaError) as e:
            _build(ctx, d, k)
        assert e.value.code == -1 and "k must be 1 to 16" in e.value.text
    # a missing row, then the build, then a second build of any kind
    t = T.Tree(ctx, n)
    t.set_rows(0, 17, d)
    t.set_rows(18, n, d)
    with pytest.raises(P.PcoaError) as e:
        P.pcoabuild(t, 2)
    assert e.value.code == -1 and "row 17" in e.value.text
    t.set_rows(17, 18, d)
    eig, _, _ = P.pcoabuild(t, 2)
    assert np.all(np.abs(eig - P.pcoa(d, 2)[0]) <= 2 * TOL * eig[0])
    with pytest.raises(P.PcoaError) as e:
        P.pcoabuild(t, 2)
    assert e.value.code == -1 and "built" in e.value.text
    with pytest.raises(T.TreeError) as e:
        t.build(T.AVERAGE)
    assert e.value.code == -1 and "built" in e.value.text
    t.free()
    t = T.Tree(ctx, n)
    t.set_rows(0, n, d)
    t.build(T.SINGLE)
    with pytest.raises(P.PcoaError) as e:
        P.pcoabuild(t, 2)
    assert e.value.code == -1 and "built" in e.value.text
    t.free()
    # a NaN cell and an infinite cell: the message names them
    for value, word, cell in ((np.nan, "NaN", (23, 9)), (np.inf, "not finite", (31, 2)), (-np.inf, "not finite", (5, 4))):
        bad = np.array(d)
        bad[cell] = bad[cell[::-1]] = value
        with pytest.raises(P.PcoaError) as e:
            _build(ctx, bad, 3)
        assert e.value.code == -1 and "row %d" % cell[0] in e.value.text and "col %d" % cell[1] in e.value.text and word in e.value.text
    # n < 2
    for small in (0, 1):
        t = T.Tree(ctx, small)
        if small:
            t.set_rows(0, 1, np.zeros((1, 1)))
        with pytest.raises(P.PcoaError) as e:
            P.pcoabuild(t, 1)
        assert e.value.code == -1 and "at least 2" in e.value.text
        t.free()


def test_no_convergence_is_an_error_and_leaves_the_outputs_alone(ctx):
    n, k = 257, 3
    d = _input("euclidean", n)[0]
    eig, x = np.full(k, 7.0), np.full((n, k), 7.0)
    with pytest.raises(P.PcoaError) as e:
        _build(ctx, d, k, tol=TOL, max_iter=1, out=(eig, x))
    assert e.value.code == -1 and "1 iterations" in e.value.text and "residual" in e.value.text
    assert np.all(eig == 7.0) and np.all(x == 7.0)
