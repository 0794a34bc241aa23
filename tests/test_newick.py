"""host/newick.cpp — the Newick renderer and the cut that `lash dist --tree` / `--cluster D --linkage L` write with — on hand-written
merge lists, against the rule as written down here and against the model's renderer (tree_model.py)."""
import math

import pytest

import tree_model as T


def test_labels_are_quoted_when_they_must_be():
    names = ["a b", "x:1-5", "it's", "(p)", "plain_name.fa", "/data/g1.fa", "w[1]", "semi;colon", "com,ma", "tab\there"]
    want = ["'a b'", "'x:1-5'", "'it''s'", "'(p)'", "plain_name.fa", "/data/g1.fa", "'w[1]'", "'semi;colon'", "'com,ma'", "'tab\there'"]
    for name, w in zip(names, want):
        assert T.host_newick([name], []) == w + ";"
        assert T.label(name) == w
    mg = [(0, 1, 0.5, 2), (2, 3, 0.5, 2), (4, 5, 1.0, 4)]
    assert T.host_newick(names[:4], mg) == "(('a b':0.25,'x:1-5':0.25):0.25,('it''s':0.25,'(p)':0.25):0.25);"


def test_n_0_1_2():
    assert T.host_newick([], []) == ";"
    assert T.host_newick(["solo"], []) == "solo;"
    assert T.host_newick(["a", "b"], [(0, 1, 0.125, 2)]) == "(a:0.0625,b:0.0625);"
    assert T.host_newick(["a", "b"], [(1, 0, 0.0, 2)]) == "(b:0,a:0);"          # the merge's order is the children's order


def test_branch_lengths_are_half_the_height_difference_in_10_digits():
    # heights 0.1, 1/3, 1: branches h_parent / 2 - h_child / 2 with %.10g
    third = 1.0 / 3.0
    names = ["a", "b", "c", "d", "e"]
    mg = [(0, 1, 0.1, 2), (5, 2, third, 3), (3, 4, 0.25, 2), (6, 7, 1.0, 5)]
    got = T.host_newick(names, mg)
    b1 = "%.10g" % (0.1 / 2)
    b2 = "%.10g" % (third / 2 - 0.1 / 2)
    b3 = "%.10g" % (third / 2)
    b4 = "%.10g" % (1.0 / 2 - third / 2)
    assert (b1, b2, b3, b4) == ("0.05", "0.1166666667", "0.1666666667", "0.3333333333")
    assert got == "(((a:%s,b:%s):%s,c:%s):%s,(d:0.125,e:0.125):0.375);" % (b1, b1, b2, b3, b4)
    assert got == T.newick(names, mg)
    # small and large magnitudes keep %g's exponent form
    assert T.host_newick(["a", "b"], [(0, 1, 3e-7, 2)]) == "(a:1.5e-07,b:1.5e-07);"
    assert T.host_newick(["a", "b"], [(0, 1, 2.0 ** -40, 2)]) == "(a:%s,b:%s);" % (("%.10g" % 2.0 ** -41,) * 2)


def test_a_deep_chain_is_rendered_without_recursion():
    n = 20000
    names = ["g%d" % i for i in range(n)]
    mg = [(0, 1, 1.0, 2)] + [(n + s - 1, s + 1, float(s + 1), s + 2) for s in range(1, n - 1)]
    got = T.host_newick(names, mg)
    assert got.startswith("(" * (n - 1) + "g0:0.5,g1:0.5):0.5,g2:1)") and got.endswith(",g%d:%s);" % (n - 1, "%.10g" % ((n - 1) / 2)))
    assert got.count(",") == n - 1


def test_a_list_that_is_no_tree_is_refused():
    assert T.host_newick(["a", "b", "c"], [(0, 1, 0.1, 2), (0, 2, 0.2, 3)]) is None     # leaf 0 twice
    assert T.host_newick(["a", "b", "c"], [(0, 4, 0.1, 2), (3, 2, 0.2, 3)]) is None     # a node before its merge
    assert T.host_cut(3, [(0, 1, 0.1, 2), (0, 2, 0.2, 3)], 1.0) is None


def test_cut_at_and_just_below_a_merge_height():
    # leaves 0..5; (1, 4) at 0.1, (0, 2) at 0.25, (6, 3) at 0.25, (7, 8) at 0.5, (9, 5) at 1.0
    mg = [(1, 4, 0.1, 2), (0, 2, 0.25, 2), (6, 3, 0.25, 3), (7, 8, 0.5, 5), (9, 5, 1.0, 6)]
    cases = [(-1.0, [0, 1, 2, 3, 4, 5]), (0.0, [0, 1, 2, 3, 4, 5]), (math.nextafter(0.1, 0.0), [0, 1, 2, 3, 4, 5]), (0.1, [0, 1, 2, 3, 1, 5]),
             (math.nextafter(0.25, 0.0), [0, 1, 2, 3, 1, 5]), (0.25, [0, 1, 0, 1, 1, 5]), (math.nextafter(0.5, 0.0), [0, 1, 0, 1, 1, 5]),
             (0.5, [0, 0, 0, 0, 0, 5]), (math.nextafter(1.0, 0.0), [0, 0, 0, 0, 0, 5]), (1.0, [0] * 6), (7.0, [0] * 6)]
    for D, want in cases:
        assert T.host_cut(6, mg, D) == want, D
        assert T.cut(6, mg, D) == want, D
    assert T.host_cut(6, mg, float("nan")) == [0, 1, 2, 3, 4, 5]
    assert T.host_cut(0, [], 0.5) == [] and T.host_cut(1, [], 0.5) == [0]
    names = ["n%d" % i for i in range(6)]
    assert T.render_clusters(names, T.cut(6, mg, 0.25)) == "Representative\tMember\nn0\tn0\nn0\tn2\nn1\tn1\nn1\tn3\nn1\tn4\nn5\tn5\n"


def test_the_model_on_a_matrix_worked_by_hand():
    import numpy as np
    # 0-1 at 2, 2-3 at 3 (tie with nothing), then average: d({0,1},{2,3}) = (6 + 8 + 7 + 9) / 4 = 7.5
    D = np.array([[0, 2, 6, 8], [2, 0, 7, 9], [6, 7, 0, 3], [8, 9, 3, 0]], float)
    assert T.merges(D, T.AVERAGE) == [(0, 1, 2.0, 2), (2, 3, 3.0, 2), (4, 5, 7.5, 4)]
    assert T.merges(D, T.SINGLE) == [(0, 1, 2.0, 2), (2, 3, 3.0, 2), (4, 5, 6.0, 4)]
    assert T.merges(D, T.COMPLETE) == [(0, 1, 2.0, 2), (2, 3, 3.0, 2), (4, 5, 9.0, 4)]
    # all equal: the smallest (i, j) every time, the new node staying in slot 0
    E = np.full((4, 4), 0.5)
    assert T.merges(E, T.AVERAGE) == [(0, 1, 0.5, 2), (4, 2, 0.5, 3), (5, 3, 0.5, 4)]
    assert T.newick(list("abcd"), T.merges(D, T.AVERAGE)) == "((a:1,b:1):2.75,(c:1.5,d:1.5):2.25);"
