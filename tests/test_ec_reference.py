"""tests/ecref.py, the long-double reference of hyperminhash's expected_collisions that tests/test_gpu_hmh_ec_tiles.py and
tests/test_gpu_hmh_ec.py hold the GPU's cell sums against, checked here without a GPU: its cell vectors against mpmath at 50 digits,
the vectors' totals, the crate's own f64 loop (tests/pyref.py) against it, and the pool of cardinalities the GPU tests draw from.

Vectors against mpmath (4 cardinalities x 5 rows x 6 cells): worst absolute error 1.6e-23 (2^-75.7; asserted <= 2^-60, the scale
on which the vectors' totals are <= 1), worst relative error 9.2e-19 (2^-59.9) at n = 524288, last cell of row 1, where the
exponent n log1p(-b1) = -32 carries its two roundings of 2^-64 each: asserted <= (n b2 + 3) 2^-63, what a 64-bit mantissa gives.

The crate's loop against the reference, 66 pairs (tiny cardinalities, the 2^19 edge, pool values, random ones): worst
|loop - ref| = 5.0 ulp(ec) = 3.5e-17 (ulp(ec) = 2^-57; at 220400.1 x 485422.3), inside the bound derived for it,
6 * 2^-53 + 65536 * 2^-53 * x (four glibc pow below 1 ulp per cell, 65 536 sequential additions): 6.7e-16 to 2.0e-15.  This is
how far the thing the product imitates is from exact; the GPU's tolerance ecref.tol(x) = 66 * 2^-53 + 2^-39 x = 7.3e-15 is larger.

The pool separates: exchanging one cardinality of a pair for another pool value moves ec by at least 1.7e-11
(measured), 22 times the 100 T = 7.7e-13 asserted, so no index error hides inside T.
"""
import numpy as np
import pytest

import ecref as E
import pyref as R


@pytest.fixture(scope="module")
def table():
    return E.pool_table()


def _cell(mp, i, j):
    if i != 64:
        den = mp.mpf(2) ** (24 + i)
        return (1024 + j) / den, (1025 + j) / den
    den = mp.mpf(2) ** 87
    return j / den, (j + 1) / den


def _mpf(mp, g):
    """a long double as an mpf, exactly"""
    f, e = np.frexp(g)
    return mp.mpf(int(f * np.longdouble(2.0 ** 64))) * mp.mpf(2) ** (int(e) - 64)


def test_vectors_against_mpmath():
    import mpmath as mp
    worst_abs = worst_rel = 0.0
    with mp.workdps(50):
        for n in (2, 1000, 3e5, 524288):
            v = E.vector(n)
            assert v.dtype == np.longdouble and v.shape == (65536,) and (v <= 0).all()
            for i in (1, 2, 32, 63, 64):
                for j in (1, 2, 300, 777, 1023, 1024):
                    b1, b2 = _cell(mp, i, j)
                    want = (1 - b2) ** mp.mpf(n) - (1 - b1) ** mp.mpf(n)
                    err = abs(_mpf(mp, v[(i - 1) * 1024 + j - 1]) - want)
                    rel = err / abs(want)
                    assert err <= mp.mpf(2) ** -60, (n, i, j, float(err))
                    assert rel <= (n * b2 + 3) * mp.mpf(2) ** -63, (n, i, j, float(rel))
                    worst_abs, worst_rel = max(worst_abs, float(err)), max(worst_rel, float(rel))
    print("vectors against mpmath: worst absolute %.2g, worst relative %.2g" % (worst_abs, worst_rel))


def test_cell_bounds_are_the_published_ones_and_exact():
    """b1 / b2 as fractions, exact in long double; the cells are disjoint intervals below 2^-13 (row i ends one cell short of
    where row i - 1 begins: the published rule has it so)"""
    from fractions import Fraction
    b1, b2, inv = E.cell_bounds()
    for i, j in ((1, 1), (1, 1024), (7, 513), (63, 1024), (64, 1), (64, 1024)):
        at = (i - 1) * 1024 + j - 1
        den = Fraction(2) ** (24 + i if i != 64 else 87)
        num = 1024 + j if i != 64 else j
        assert Fraction(float(b1[at])) == num / den and Fraction(float(b2[at])) == (num + 1) / den
    order = np.argsort(b1)
    assert (b2[order][:-1] <= b1[order][1:]).all() and b1[order][0] == inv[-1] and b2[order][-1] < np.ldexp(np.longdouble(1), -13)
    assert ((b2 - b1) == inv).all()


def test_vector_totals(table):
    """the cells are disjoint intervals of the minimum hash: every vector's absolute values sum to <= 1 (ecref.tol uses it)"""
    for n, v in list(zip(table.cards, table.V)) + [(c, E.vector(c)) for c in (1.0, 2.0, 17.0, 524288.0)]:
        total = np.abs(v).sum()
        assert 0 < total <= 1, (n, total)
    # one hash: a cell's factor is its width, and the widths add up to 1024 * (2^-25 + ... + 2^-87) + 1024 * 2^-87 = 2^-14
    assert abs(float(np.abs(E.vector(1.0)).sum()) - 2.0 ** -14) <= 2.0 ** -70


def _loop_pairs(cards):
    rng = np.random.default_rng(19)
    tiny = [1.0, 2.0, 17.0]
    pairs = [(a, b) for a in tiny for b in tiny if a <= b]                                     # 6
    pairs += [(a, b) for a in tiny for b in (1000.0, 524288.0)]                                # 6
    pairs += [(524288.0, 524288.0), (524288.0, 524287.5), (524288.0, 100.0), (300000.0, 524288.0)]
    pairs += [(524288.5, 524288.0), (524288.5, 2.0), (524288.0, 524288.5), (2.0 ** 74, 3.0), (2.0 ** 75, 2.0 ** 75)]   # closed forms
    pool = [(cards[a], cards[b]) for a, b in ((0, 0), (0, 95), (95, 95), (40, 41), (41, 40), (7, 88), (60, 13), (95, 94))]
    rand = [tuple(rng.uniform(1, 524288, 2)) for _ in range(25)] + [tuple(np.exp(rng.uniform(0, np.log(524288), 2))) for _ in range(12)]
    return pairs + pool + rand


def test_the_crates_loop_against_the_reference(table):
    pairs = _loop_pairs(table.cards)
    assert len(pairs) >= 60
    worst, at = 0.0, None
    for n, m in pairs:
        want, got = E.ec(n, m), R.hmh_expected_collisions(float(n), float(m))
        if max(n, m) > 2.0 ** 19:
            assert got == want or abs(got - want) <= 2.0 ** -52 * want, (n, m, got, want)      # (pyref squares with **: pow)
            continue
        x = want - 1 / 28
        bound = 6 * 2.0 ** -53 + 65536 * 2.0 ** -53 * x
        err = abs(got - want)
        assert err <= bound, (n, m, got, want, err, bound)
        if err > worst:
            worst, at = err, (n, m)
    print("the loop against the reference: worst %.1f ulp(ec) = %.2g at %s" % (worst / 2.0 ** -57, worst, at))


def test_the_table_is_the_plain_evaluation(table):
    """the upper-triangle bookkeeping: symmetric, and equal to ecref.ec of the two cardinalities"""
    assert np.array_equal(table.ec, table.ec.T) and np.array_equal(table.x, table.x.T)
    for a, b in ((0, 0), (3, 77), (95, 12), (95, 95)):
        assert table.ec[a, b] == E.ec(table.cards[a], table.cards[b])
    ec, t, small = E.expected(table, [5, 0, 9], [7, 0], [table.cards[5], 3e6, table.cards[9]], [table.cards[7], 2.0 ** 75])
    assert small.tolist() == [[True, False], [False, False], [True, False]]
    assert ec[0, 0] == table.ec[5, 7] and ec[2, 0] == table.ec[9, 7] and t[0, 0] == E.tol(table.x64[5, 7]) and t[1, 0] == 0
    assert ec[1, 0] == E.closed_form(table.cards[7], 3e6) and ec[0, 1] == ec[1, 1] == 1.8446744073709552e19


def test_the_pool_separates(table):
    """at most 96 cardinalities in [100, 2^19], each 2 % from its neighbours, three large images; and for any two different pool
    values a != b against any third c, |ec(a, c) - ec(b, c)| > 100 T: an index error cannot hide inside the tolerance"""
    imgs, cards = E.pool()
    n = len(E.K)
    assert n <= 96 and len(cards) == n + 3 and imgs.shape == (n + 3, 32768)
    small, large = cards[:n], cards[n:]
    assert small.min() >= 100 and small.max() <= 2.0 ** 19 and (small[1:] >= 1.02 * small[:-1]).all()
    assert (large > 2.0 ** 19).all() and len(set(large)) == 3
    t100 = 100 * float(E.tol(table.x64.max()))
    gaps = np.diff(np.sort(table.ec, axis=0), axis=0)                # column c: ec(., c) sorted
    assert gaps.min() > t100, (gaps.min(), t100)
    print("pool: smallest |ec(a, c) - ec(b, c)| %.3g, 100 T %.3g" % (gaps.min(), t100))
    # the rules that spread the pool over rows and columns keep every structural neighbour different
    for rule in (E.row_rule, E.col_rule):
        for shift in (0, 1, 50):
            idx = rule(700, shift)
            assert idx.min() >= 0 and idx.max() < n
            E.assert_alias_free(small[idx])


def test_chunk_reference_separates(table):
    """On the reference alone: in the chunk test's block, taking the ec of a pair that differs in its row's or in its column's
    value (any other of the set's cardinalities: what a wrong index into X fetches) moves the distance by more than 100 times the
    tolerance the test allows.  Both values exchanged at once is not asserted: ec(n, m) is close to a function of n m for small
    cardinalities, so pairs with nearly equal products exist in any pool."""
    order, want, t, small, c, n, d, dt = E.chunk_block_reference(table)
    assert small.sum() == 29 * (E.CHUNK_N - 3) and (c[small] >= E.K[0]).all() and (d[small] < 1).all() and (d[small] > 0).sum() > 0.9 * small.sum()
    r0, r1 = E.CHUNK_ROWS
    ri, ci = np.where(order[r0:r1] < len(E.K), order[r0:r1], 0), np.where(order < len(E.K), order, 0)
    col = np.sort(table.ec, axis=0)                                                    # ec(., b) sorted, per column b
    worst = np.inf
    for i, a in enumerate(ri):
        for b in np.unique(ci):
            cells = small[i] & (ci == b)
            if not cells.any():
                continue
            j = int(np.flatnonzero(cells)[0])
            others = np.array([v for v in E.CHUNK_POOL])
            other = np.concatenate([table.ec[others[others != a], b], table.ec[a, others[others != b]]])       # the row's value exchanged, the column's
            moved = np.abs(E._distance(c[i, j], n[i, j], other) - d[i, j]).min()
            worst = min(worst, moved / dt[i, j])
            assert moved > 100 * dt[i, j], (a, b, moved, dt[i, j])
    print("chunk block: the nearest other pool pair moves the distance by >= %.0f tolerances" % worst)
