"""tests/screen_model.py on register tables made by hand: the rule of lash_sketch_set_screen_wta and what follows from it."""
import numpy as np

import screen_model as W
from spectrum_model import M


def _table(**at):
    """a register table that is 0 except at the given buckets: _table(b3=7) sets bucket 3 to 7"""
    t = np.zeros(M, dtype=np.uint32)
    for key, v in at.items():
        t[int(key[1:])] = v
    return t


# query: buckets 0..5 occupied
Q = _table(b0=10, b1=11, b2=12, b3=13, b4=14, b5=15)
REFS = np.stack([
    _table(b0=10, b1=11, b2=12),            # 0: holds 0, 1, 2
    _table(b1=11, b2=12, b3=13, b9=99),     # 1: holds 1, 2, 3; bucket 9 is empty in the query
    _table(b2=12, b4=77),                   # 2: holds 2; bucket 4 carries another k-mer
    _table(b7=5),                           # 3: holds nothing
    _table(),                               # 4: an empty sketch
])


def test_the_winner_is_the_first_position_that_holds():
    w = W.winners(REFS, Q, [0, 1, 2])
    assert w[:6].tolist() == [0, 0, 0, 1, W.NONE, W.NONE] and (w[6:] == W.NONE).all()
    w = W.winners(REFS, Q, [2, 1, 0])                                        # the same rows, reversed priority
    assert w[:6].tolist() == [2, 1, 0, 1, W.NONE, W.NONE]
    shared, won = W.wta(REFS, Q, [0, 1, 2])
    assert shared.tolist() == [3, 3, 1] and won.tolist() == [3, 1, 0]
    shared, won = W.wta(REFS, Q, [2, 1, 0])
    assert shared.tolist() == [1, 3, 3] and won.tolist() == [1, 2, 1]


def test_the_consequences_of_the_rule():
    rng = np.random.default_rng(5)
    refs = rng.integers(0, 4, size=(9, M)).astype(np.uint32)                 # registers 0..3: plenty of equal ones, plenty of empty ones
    q = rng.integers(0, 4, size=M).astype(np.uint32)
    for rows in ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 3, 3, 0], [4]):
        shared, won = W.wta(refs, q, rows)
        h = W.holds(refs, q, rows)
        assert (won <= shared).all()
        assert int(won.sum()) == int(h.any(axis=0).sum()) <= int((q != 0).sum())
        w = W.winners(refs, q, rows)
        assert ((w == W.NONE) == ~h.any(axis=0)).all() and (w[q == 0] == W.NONE).all()
        for t, r in enumerate(rows):                                         # shared is the C of the pair's register scan
            assert int(shared[t]) == int(((refs[r] == q) & (q != 0)).sum())


def test_a_row_listed_twice_wins_nothing_at_its_later_position():
    shared, won = W.wta(REFS, Q, [1, 0, 1])
    assert shared.tolist() == [3, 3, 3] and won.tolist() == [3, 1, 0]


def test_an_empty_query_gives_zeros():
    shared, won = W.wta(REFS, _table(), [0, 1, 2, 3, 4])
    assert shared.tolist() == [0] * 5 and won.tolist() == [0] * 5
    assert (W.winners(REFS, _table(), [0, 1]) == W.NONE).all()


def test_an_empty_list_gives_nothing():
    shared, won = W.wta(REFS, Q, [])
    assert shared.shape == (0,) and won.shape == (0,) and shared.dtype == np.uint32 and won.dtype == np.uint32
    assert (W.winners(REFS, Q, []) == W.NONE).all()
    s, w = W.screen(REFS, np.stack([Q, _table()]), [[], [0]])
    assert [x.tolist() for x in s] == [[], [0]] and [x.tolist() for x in w] == [[], [0]]


def test_buckets_nobody_holds_stay_none():
    w = W.winners(REFS, Q, [3, 4])
    assert (w == W.NONE).all()
    shared, won = W.wta(REFS, Q, [3, 4])
    assert shared.tolist() == [0, 0] and won.tolist() == [0, 0]


def test_a_single_candidate_wins_what_it_shares():
    for r in range(5):
        shared, won = W.wta(REFS, Q, [r])
        assert shared.tolist() == won.tolist()
    assert W.wta(REFS, Q, [1])[1].tolist() == [3]


def test_priority_is_distance_then_the_larger_reference_then_the_row():
    d = {0: 0.25, 1: 0.125, 2: 0.25, 3: 0.25, 4: 1.0}
    card = {0: 100.0, 1: 5.0, 2: 300.0, 3: 100.0, 4: 1e9}
    assert W.priority([4, 3, 2, 1, 0], d, card) == [1, 2, 0, 3, 4]


def test_the_table_text():
    lists = [[1, 0], [], [2]]
    shared = [[3, 3], [], [1]]
    won = [[3, 1], [], [1]]
    buckets = [[7, 0, 0], [6, 0, 0], [0, 0, 9]]
    dist = [[0.5, 1.0, 1.0], [0.25, 1.0, 1.0], [1.0, 1.0, 0.0]]
    wta_dist = [[0.25, 0.75], [], [float("nan")]]
    q, r = ["s0", "s1", "s2"], ["a", "b", "c"]
    assert W.table(q, r, lists, shared, won, buckets, dist, wta_dist, 0.5) == W.HEADER + "s0\tb\t3\t3\t6\t0.250000\t0.250000\n"
    assert W.table(q, r, lists, shared, won, buckets, dist, wta_dist, 0.5, keep_losers=True) == (
        W.HEADER + "s0\tb\t3\t3\t6\t0.250000\t0.250000\ns0\ta\t3\t1\t7\t0.500000\t0.750000\ns2\tc\t1\t1\t9\t0.000000\tNaN\n")
