"""`lash dist --tree --nj` without a GPU: the model of the rule (nj_model.py) against trees whose answer is known, the drift of its carried
row sums against the derived bound, host/newick.cpp's NJ renderer against the model's, and the command line's refusals, which are parsed
before any file is read or any device is opened."""
import os
import subprocess

import numpy as np
import pytest

import host_lib as H
import nj_model as NJ
from test_gpu_tree import _matrix


@pytest.mark.parametrize("n", [4, 5, 17, 65, 257])
def test_additive_trees_are_recovered_exactly(n):
    """branch lengths k/64: every number of the rule is a small multiple of 1/128, so nothing rounds, and neighbour joining recovers an
    additive tree: the same splits, every branch length equal"""
    d, truth = NJ.additive(n, 10 + n)
    assert len(truth) == 2 * n - 3 and np.array_equal(d, d.T) and (d[~np.eye(n, dtype=bool)] > 0).all()
    jn = NJ.joins(d)
    assert len(jn) == n - 1 and sorted(x for m in jn for x in m[:2]) == list(range(2 * n - 2))
    assert NJ.splits(n, jn) == truth


def test_the_model_on_a_matrix_worked_by_hand():
    # the five-taxon example of the neighbour-joining literature: a, b join first at 2 and 3, then (ab), c at 3 and 4, then d, e
    D = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], float)
    jn = NJ.joins(D)
    assert jn == [(0, 1, 2.0, 3.0), (5, 2, 3.0, 4.0), (6, 3, 2.0, 2.0), (7, 4, 1.0, 0.0)]
    assert NJ.newick(list("abcde"), jn) == "(((a:2,b:3):3,c:4):2,d:2,e:1);"
    # all equal: the smallest (i, j) every time, the new node staying in slot 0
    E = np.full((4, 4), 0.5)
    assert [m[:2] for m in NJ.joins(E)] == [(0, 1), (4, 2), (5, 3)]
    assert NJ.joins(np.zeros((1, 1))) == [] and NJ.joins(np.zeros((0, 0))) == []
    assert NJ.joins(np.array([[0, 0.25], [0.25, 0]])) == [(0, 1, 0.25, 0.0)]


@pytest.mark.parametrize("kind", ["uniform", "saturated"])
def test_carried_row_sums_stay_within_the_bound(kind):
    """at r = 2 the row sum of a survivor is its distance to the other one.  It was carried through n - 2 steps of three roundings each,
    on magnitudes <= 2 n max|D|: within 6 n^2 2^-53 max(1, max|D|) of the D[i][j] the closing record reports."""
    n = 257
    d = _matrix(n, kind, 41)
    jn, R, D, slots = NJ.joins_state(d)
    i, j = slots
    bound = 6 * n * n * 2.0 ** -53 * max(1.0, float(np.abs(d).max()))
    assert jn[-1][2] == D[i, j]
    for k in (i, j):
        drift = abs(R[k] - D[i, j])
        print("n %d %s: |R[%d] - D[i][j]| = %.3g, bound %.3g" % (n, kind, k, drift, bound))
        assert drift <= bound


CASES = [
    ([], []),
    (["solo"], []),
    (["a", "b"], [(0, 1, 0.125, 0.0)]),
    (["a", "b"], [(1, 0, 0.3, 0.0)]),
    (["a", "b", "c"], [(0, 2, 0.25, 0.5), (3, 1, 1.0 / 3.0, 0.0)]),                                # the other node of the closing record: a leaf
    (["a", "b", "c"], [(1, 2, 0.25, 0.5), (0, 3, 0.1, 0.0)]),                                      # and with node 2n - 3 second
    (["a", "b", "c", "d"], [(0, 1, 0.1, 0.2), (2, 3, 0.3, 0.4), (4, 5, 0.05, 0.0)]),               # an internal node
    (["a", "b", "c", "d"], [(2, 3, 0.1, 0.2), (0, 1, 0.3, 0.4), (5, 4, 3e-7, 0.0)]),
    (["a", "b", "c", "d", "e"], [(0, 1, 2.0, 3.0), (5, 2, 3.0, 4.0), (6, 3, 2.0, 2.0), (7, 4, 1.0, 0.0)]),
    (["a", "b", "c", "d", "e"], [(3, 4, -0.0125, 2.0 ** -40), (0, 1, 1e10, -1.0 / 3.0), (6, 2, 0.5, -0.0), (5, 7, -0.25, 0.0)]),   # negative lengths
    (["a b", "x:1-5", "it's", "(p)"], [(0, 1, 0.1, 0.2), (4, 2, 0.3, 0.4), (5, 3, 0.05, 0.0)]),    # names that need quoting
]


@pytest.mark.parametrize("names,jn", CASES)
def test_the_host_renderer_equals_the_models(names, jn):
    got = NJ.host_newick(names, jn)
    assert got is not None and got == NJ.newick(names, jn)


def test_the_host_renderer_by_hand():
    assert NJ.host_newick(*CASES[2]) == "(a:0.0625,b:0.0625);"
    assert NJ.host_newick(*CASES[3]) == "(b:0.15,a:0.15);"
    assert NJ.host_newick(*CASES[4]) == "(a:0.25,c:0.5,b:0.3333333333);"
    assert NJ.host_newick(*CASES[5]) == "(b:0.25,c:0.5,a:0.1);"
    assert NJ.host_newick(*CASES[6]) == "(c:0.3,d:0.4,(a:0.1,b:0.2):0.05);"
    assert NJ.host_newick(*CASES[7]) == "(a:0.3,b:0.4,(c:0.1,d:0.2):3e-07);"
    assert NJ.host_newick(*CASES[8]) == "(((a:2,b:3):3,c:4):2,d:2,e:1);"
    assert NJ.host_newick(*CASES[9]) == "((a:1e+10,b:-0.3333333333):0.5,c:-0,(d:-0.0125,e:%s):-0.25);" % ("%.10g" % 2.0 ** -40)
    assert NJ.host_newick(*CASES[10]) == "(('a b':0.1,'x:1-5':0.2):0.3,'it''s':0.4,'(p)':0.05);"


def test_a_deep_chain_is_rendered_without_recursion():
    n = 20000
    names = ["g%d" % i for i in range(n)]
    jn = [(0, 1, 1.0, 1.0)] + [(n + s - 1, s + 1, 0.5, 1.0) for s in range(1, n - 2)] + [(2 * n - 3, n - 1, 0.25, 0.0)]
    got = NJ.host_newick(names, jn)
    assert got == NJ.newick(names, jn) and got.count(",") == n - 1 and got.endswith(",g%d:1,g%d:0.25);" % (n - 2, n - 1))


def test_a_list_that_is_no_tree_is_refused():
    abcd = ["a", "b", "c", "d"]
    assert NJ.host_newick(abcd, [(0, 1, 0.1, 0.2), (0, 2, 0.3, 0.4), (5, 3, 0.05, 0.0)]) is None     # leaf 0 joined twice
    assert NJ.host_newick(abcd, [(0, 1, 0.1, 0.2), (4, 2, 0.3, 0.4), (4, 3, 0.05, 0.0)]) is None     # node 4 used twice; no node 2n - 3
    assert NJ.host_newick(abcd, [(0, 1, 0.1, 0.2), (2, 3, 0.3, 0.4), (4, 4, 0.05, 0.0)]) is None     # the closing record without node 2n - 3
    assert NJ.host_newick(abcd, [(0, 5, 0.1, 0.2), (2, 3, 0.3, 0.4), (4, 1, 0.05, 0.0)]) is None     # a node before its join
    assert NJ.host_newick(abcd, [(0, 1, 0.1, 0.2), (4, 2, 0.3, 0.4), (5, 9, 0.05, 0.0)]) is None     # a node that does not exist
    assert NJ.host_newick(["a", "b"], [(0, 0, 0.1, 0.0)]) is None
    assert NJ.host_newick(abcd, [(0, 1, 0.1, 0.2), (4, 2, 0.3, 0.4), (5, 3, 0.05, 0.0)]) is not None


def _dist(tmp_path, *extra):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "dist", "-q", "none", "-r", "none", "-o", "out.tsv"] + list(extra), cwd=tmp_path, capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("args,message", [
    (["--nj"], "--nj needs --tree"),
    (["--nj", "--block-rows", "3"], "--nj needs --tree"),
    (["--tree", "--nj", "--linkage", "average"], "--nj cannot be used with --linkage"),
    (["--linkage", "average", "--nj", "--tree"], "--nj cannot be used with --linkage"),
    (["--nj", "--cluster", "0.1"], "--nj cannot be used with --cluster"),
    (["--cluster", "0.1", "--linkage", "average", "--nj"], "--nj cannot be used with --cluster"),
])
def test_nj_in_a_wrong_combination_is_refused(tmp_path, args, message):
    r = _dist(tmp_path, *args)
    assert r.returncode == 2 and r.stderr.count("\n") == 1 and r.stderr.startswith("error: " + message)
    assert not (tmp_path / "out.tsv").exists()


def test_what_tree_refuses_stays_refused_with_nj(tmp_path):
    for other in (["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"], ["--derep", "0.05"], ["--containment", "query"]):
        r = _dist(tmp_path, "--tree", "--nj", *other)
        assert r.returncode == 2 and "--tree cannot be used with " + other[0] in r.stderr


def test_tree_nj_is_accepted_and_help_names_it(tmp_path):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the options
    want = _dist(tmp_path)
    for args in (["--tree", "--nj"], ["--nj", "--tree", "--fp32", "-m", "0", "--file-order", "--block-rows", "3", "-t", "2", "--devices", "0,0"]):
        r = _dist(tmp_path, *args)
        assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--nj " in r.stdout + r.stderr and "neighbour-joining" in r.stdout + r.stderr
