"""collision_vectors_kernel / collision_gemm_kernel (dist_kernels.hip) and the index plumbing around them, every cell against the
long-double table of tests/ecref.py (checked on its own in tests/test_ec_reference.py): every tile, wave and MFMA block of the
GEMM, the XCD renumbering with idle workgroups, ragged edges, the gather / scatter of lash_hmh_pair_expected_collisions over
mixed small / large matrices, lash_set_ec_block's small_idx / rbase / cached vectors, and its chunks of 4096 query vectors as
both the host scatter (lash_sketch_set_hmh_expected_collisions) and the device's small_cell() (dist_filter.h) read them.

Every assertion on a small x small cell is |got - ref| <= T(x_ref) = (4 E + 2) 2^-53 + 2^-39 x (ecref.tol; E = 16 ulp is an
allowance for ocml's f64 pow that nobody here has measured), on every cell; closed-form cells are the host's f64 expression and
must be equal.  Rows and columns take pool cardinalities by rules under which structural neighbours (distances 1..4, 8, 12, 16,
32, 48, 64, 128, 256) always differ, and any two pool values differ by > 100 T against any third (test_ec_reference.py), so a
mis-indexed cell cannot pass.

Measured on an MI355X (-s prints them): worst |got - ref| in ulp(ec) = 2^-57 (T is 1056 of them), and pytest's wall time
  test_whole_matrix 300 x 391   9 ulp   0.20 s (+ 2.0 s once for the module's table)
  test_edges  1 x 1: 1,  128 x 128: 9,  129 x 127: 9,  1 x 300: 1,  257 x 5: 7 ulp    0.01 s each
  test_set_route (14 calls)      9 ulp   0.18 s
  test_chunk_route               6 ulp over 128 673 cells (9 889 past the first chunk); 133 200 distances, all within 0.001 of their
                                 tolerance; 0.10 s
  tests/test_gpu_hmh_ec.py's 1000 x 1000: 9 ulp.
The worst error is 1 % of T: ocml's pow is nowhere near the 16 ulp allowed for it, and E was not widened.

Mutations, each tried on a scratch build on that machine, and whether the tests before this file noticed:
  1. collision_gemm_kernel: tile = blockIdx.x instead of the XCD renumbering: every test passes, before and now, and rightly: on
     a grid of 8 per_xcd workgroups the renumbering is a bijection of the tile numbers, so each tile is still computed exactly
     once and X is the same; only L2 reuse changes.  An equivalent mutant.  The neighbouring error that does change values,
     per_xcd = n_tiles / 8 (tiles 9..11 of 12 never computed), fails test_whole_matrix, test_edges[129-127, 1-300, 257-5],
     test_set_route and test_chunk_route; the earlier test_gpu_hmh_ec.py passed with it.
  2. the store's + 4u * i -> + i: fails test_whole_matrix, test_edges[128-128, 129-127, 257-5], test_set_route, test_chunk_route
     (every case with more than one row).  The earlier test_gpu_hmh_ec.py failed too (both value tests).
  3. lash_set_ec_block: X + nrs * q0 -> X + nqs * q0 was NOT run: with nqs > nrs, as in any block against a whole collection,
     it puts chunk 1 far outside ec_x (nrs * nqs doubles), an out-of-bounds write.  The in-bounds error on the same line,
     X + (nrs - 1) * q0, fails test_chunk_route (1): 13 985 cells from column 4098 on.  Nothing before reached q0 > 0.
  4. small_cell(): the nrs * q0 term dropped: fails test_chunk_route (2), 9 878 distances from column 4098 on, while (1) passes.
     Nothing before reached q0 > 0, and the filter tests' dense yardstick does not go through small_cell().
"""
import time

import numpy as np
import pytest

import ecref as E

pytestmark = pytest.mark.gpu
HUGE = (2.0 ** 75, 3.0 * 2.0 ** 74)


@pytest.fixture(scope="module")
def table():
    return E.pool_table()


def _mixed(table, idx, huge_at=None, huge=None, large_every=10):
    """cardinalities for a whole-matrix call: pool values by idx; about one member in ten large (> 2^19, every one different from its
    structural neighbours); optionally one above 2^74"""
    card = table.cards[idx].copy()
    r = np.arange(len(idx))
    big = r % large_every == 3
    card[big] = 6.0e5 * 1.07 ** (r[big] % 89)
    if huge_at is not None:
        card[huge_at] = huge
    E.assert_alias_free(card)
    return card


def _check(got, table, ri, ci, rcard, ccard, what, t0):
    want, t, small = E.expected(table, ri, ci, rcard, ccard)
    assert got.shape == want.shape
    worst = E.worst_in_ulp(got, want, t, small)
    print("%s: %d small cells, worst %.2f ulp(ec) (T = %.0f ulp), %.2f s" % (what, int(small.sum()), worst, E.T0 / 2.0 ** -57, time.perf_counter() - t0))
    return want, small


def test_whole_matrix_every_tile_and_the_gaps(table):
    """300 x 391: 3 x 4 = 12 tiles on a grid of 16 (four idle workgroups, per_xcd = 2), ragged in both directions; a tenth of the
    members large and two above 2^74, so the gather into rs / qs and the scatter back run over gaps"""
    import lash_amd
    t0 = time.perf_counter()
    ri, ci = E.row_rule(300), E.col_rule(391)
    rcard, ccard = _mixed(table, ri, 150, HUGE[0]), _mixed(table, ci, 200, HUGE[1])
    assert (rcard > 2.0 ** 19).sum() == 31 and (ccard > 2.0 ** 19).sum() == 40
    with lash_amd.Context(0) as ctx:
        got = ctx.hmh_pair_expected_collisions(rcard, ccard)
        again = ctx.hmh_pair_expected_collisions(rcard, ccard)                       # same queries: the bound query set's cached vectors
        part = ctx.hmh_pair_expected_collisions(rcard[130:], ccard)                    # other rows against them: 2 x 4 tiles
    want, small = _check(got, table, ri, ci, rcard, ccard, "300 x 391", t0)
    assert (want[~small] > 0.5).all() and (want[150] == 1.8446744073709552e19).all() and (want[:, 200] == 1.8446744073709552e19).all()
    assert np.array_equal(again, got) and np.array_equal(part, got[130:])


@pytest.mark.parametrize("m,n", [(1, 1), (128, 128), (129, 127), (1, 300), (257, 5)])
def test_edges(table, m, n):
    import lash_amd
    t0 = time.perf_counter()
    ri, ci = E.row_rule(m, 5), E.col_rule(n, 9)
    rcard, ccard = table.cards[ri], table.cards[ci]
    E.assert_alias_free(rcard)
    E.assert_alias_free(ccard)
    with lash_amd.Context(0) as ctx:
        got = ctx.hmh_pair_expected_collisions(rcard, ccard)
    _check(got, table, ri, ci, rcard, ccard, "%d x %d" % (m, n), t0)


def test_query_vectors_are_kept_only_for_the_same_cardinalities(table):
    """lash_hmh_pair_expected_collisions keeps the bound query set and its cell vectors while the qry_card values repeat.  A call
    whose queries differ in ONE small cardinality (same length, same smallness) must not be answered from them: bit for bit what a
    fresh context returns, and another value than before in that column."""
    import lash_amd
    t0 = time.perf_counter()
    ri, ci = E.row_rule(40), E.col_rule(30)
    ci2 = ci.copy()
    ci2[17] = 90                                                                     # (col_rule stays below 83)
    r, q, q2 = table.cards[ri], table.cards[ci], table.cards[ci2]
    with lash_amd.Context(0) as ctx:
        first = ctx.hmh_pair_expected_collisions(r, q)
        second = ctx.hmh_pair_expected_collisions(r, q2)
    with lash_amd.Context(0) as ctx:
        fresh = ctx.hmh_pair_expected_collisions(r, q2)
    _check(first, table, ri, ci, r, q, "40 x 30", t0)
    _check(second, table, ri, ci2, r, q2, "40 x 30, column 17 replaced", t0)
    assert np.array_equal(second, fresh)
    assert (second[:, 17] != first[:, 17]).all() and np.array_equal(np.delete(second, 17, axis=1), np.delete(first, 17, axis=1))


def test_row_blocks_past_8192_small_rows(table):
    """lash_hmh_pair_expected_collisions sends at most 8192 small rows (4 GiB of reference vectors) through lash_set_ec_block at a
    time: 8200 small rows x 3 small columns is one full block and one of 8 rows, which are the point.  About 4.3 GB of vectors on
    the device."""
    import lash_amd
    t0 = time.perf_counter()
    ri, ci = E.row_rule(8200), E.col_rule(3)
    r, q = table.cards[ri], table.cards[ci]
    with lash_amd.Context(0) as ctx:
        got = ctx.hmh_pair_expected_collisions(r, q)
    want, small = _check(got, table, ri, ci, r, q, "8200 x 3", t0)
    assert small.all() and len(np.unique(want[8192:], axis=0)) == 8


def _set(ctx, n, rule, shift, large_at):
    """a set of n members drawn from the pool's images through `order` (rule: pool index per member; large_at: members that are one
    of the three large images) -> (set, pool index per member, cardinalities as the set computed them)"""
    imgs, cards = E.pool()
    order = rule(n, shift).astype(np.uint32)
    for b, at in enumerate(large_at):
        order[at] = len(E.K) + b % 3
    s = ctx.sketch_set("hmh", 0, imgs, order)
    got = s.cardinalities()
    assert np.array_equal(got, cards[order])                                           # the reference is built from these numbers
    E.assert_alias_free(got)
    return s, order.astype(np.int64), got


def _small_only(got, want, small):
    """the set entry writes small x small cells and leaves the others alone"""
    out = want.copy()
    out[small] = got[small]
    return out


def test_set_route_blocks_triangle_and_cached_vectors(table):
    """lash_set_ec_block: rows r0 > 0 (rbase != 0) with a large member inside every block, as a triangle (n_cols = r1) and against a
    second set, a column bound that cuts the small columns short, vectors made per block and cached by prepare()"""
    import lash_amd
    t0 = time.perf_counter()
    with lash_amd.Context(0) as ctx:
        a, ai, ac = _set(ctx, 330, E.row_rule, 0, (20, 120, 260))
        b, bi, bc = _set(ctx, 150, E.col_rule, 11, (77,))
        calls = []
        for r0, r1 in ((0, 37), (37, 200), (200, 330)):
            calls += [(r0, r1, None, r1), (r0, r1, b, 150)]
        calls.append((37, 200, b, 78))                                                 # columns end just past the large one
        res = {}
        for prepared in (False, True):
            if prepared:
                a.prepare()
                a.prepare(b)
            for at, (r0, r1, q, nc) in enumerate(calls):
                res[prepared, at] = a.hmh_expected_collisions(r0, r1, qry=q, n_cols=nc)
        worst = 0.0
        for at, (r0, r1, q, nc) in enumerate(calls):
            qi, qc = (ai, ac) if q is None else (bi, bc)
            want, t, small = E.expected(table, ai[r0:r1], qi[:nc], ac[r0:r1], qc[:nc])
            assert small.any() and not small.all()
            for prepared in (False, True):
                worst = max(worst, E.worst_in_ulp(_small_only(res[prepared, at], want, small), want, t, small))
            assert np.array_equal(res[False, at][small], res[True, at][small]), (r0, r1, nc)
        b.free()
        a.free()
    print("set route: %d calls x 2, worst %.2f ulp(ec), %.2f s" % (len(calls), worst, time.perf_counter() - t0))


def test_chunk_route_host_scatter_and_small_cell(table):
    """More than 4096 small columns without prepare(): lash_set_ec_block cuts them into chunks of q_step = 4096, chunk q0 an
    [nrs][nq] matrix at X + nrs * q0, the last one short.  This makes 2 GiB of query vectors in the context's ec_qry buffer.
    (1) the host scatter: every cell of the block within T, the columns past the 4096th small member being the point;
    (2) small_cell(): pair_block_within with max_dist = 1 returns every pair of the block with the distance the host evaluates from
        the cell sum it fetched; it must be lash_dist_rows' distance under the REFERENCE ec within ecref._distance_tol (pairs with a large member: equal);
    (3) is tests/test_ec_reference.py::test_chunk_reference_separates; (4) same rows and columns in the same order as that dense evaluation."""
    import lash_amd
    t0 = time.perf_counter()
    order, want, t, small, c_want, n_want, d_want, d_tol = E.chunk_block_reference(table)
    imgs, cards = E.pool()
    r0, r1 = E.CHUNK_ROWS
    with lash_amd.Context(0) as ctx:
        s = ctx.sketch_set("hmh", 0, imgs, order.astype(np.uint32))
        got_cards = s.cardinalities()
        assert np.array_equal(got_cards, cards[order])
        got = s.hmh_expected_collisions(r0, r1)
        t1 = time.perf_counter()
        stats = s.pair_block(r0, r1)
        rows, cols, dist = s.pair_block_within(r0, r1, 1.0, E.K_MER)
        s.free()
    worst = E.worst_in_ulp(_small_only(got, want, small), want, t, small)
    tail = np.flatnonzero((order < len(E.K)) & (np.cumsum(order < len(E.K)) > 4096))
    assert len(tail) >= 300 and small[:, tail].sum() == 29 * len(tail)
    print("chunk route: %d small cells (%d past the first chunk), worst %.2f ulp(ec), %.2f s" % (int(small.sum()), int(small[:, tail].sum()), worst, t1 - t0))
    # (2), (4): the dense evaluation under the reference's ec
    assert np.array_equal(stats["c_or_zero"][small], c_want[small]) and np.array_equal(stats["n_counts"][small], n_want[small])
    dense = lash_amd.dist_rows("hmh", 0, E.K_MER, 1, got_cards[r0:r1], got_cards, c_or_zero=stats["c_or_zero"], n_counts=stats["n_counts"], hmh_ec=want)
    assert np.abs(dense - d_want)[small].max() <= 2.0 ** -50                                  # (numpy's restatement, used by the separation test)
    kr, kc = np.nonzero(dense <= 1.0)
    assert len(kr) == dense.size and np.array_equal(rows, kr + r0) and np.array_equal(cols, kc)
    err = np.abs(dist - dense[kr, kc])
    bad = ~(err <= d_tol[kr, kc])
    assert not bad.any(), (int(bad.sum()), rows[bad][:6], cols[bad][:6], dist[bad][:6], dense[kr, kc][bad][:6])
    print("chunk route: %d distances, worst %.3f of the tolerance, %.2f s" % (len(dist), float((err / np.maximum(d_tol[kr, kc], 1e-300))[small[kr, kc]].max()), time.perf_counter() - t0))
