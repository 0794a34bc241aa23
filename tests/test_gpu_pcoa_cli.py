"""`lash dist --pcoa K` through the command line.  The yardstick is the model (pcoa_model.py) on the exact distances of the same sketches,
taken through the ABI the way test_gpu_dist_tree.py takes them (the doubles, not six-decimal text), in the run's row order.

Bounds: those of test_gpu_pcoa.py with tol = 1e-10, the command line's, each widened by the 0.5e-9 relative rounding of %.10g.  The
coordinate bound divides by the gap of the axis to its nearest other eigenvalue, whatever that gap is: three families give two leading
axes that stand clear, and the bound is as loose as the third is close."""
import numpy as np
import pytest

import oracle_lib as O
import pcoa_model as P
from test_gpu_dist_tree import _Set
from test_gpu_dist_within import _mutated

pytestmark = pytest.mark.gpu

TOL = 1e-10
ROUND = 0.5e-9


def _families(seed, length, sizes=(14, 13, 13)):
    """about 40 genomes in three mutated families: each family a random ancestor and members at rising mutation rates"""
    out = []
    for f, size in enumerate(sizes):
        root = O.synth_genome(seed + f, length)
        out += [root] + [_mutated(root, 0.002 + 0.004 * j, seed + 100 * f + j) for j in range(1, size)]
    return out


def _parse(text, n, k):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == n + 4
    head = [ln.split("\t") for ln in lines[:3]]
    assert head[0][0] == "#Eigenvalue" and head[1][0] == "#Explained" and head[2] == ["Name"] + ["PC%d" % (a + 1) for a in range(k)]
    assert len(head[0]) == len(head[1]) == k + 1
    rows = [ln.split("\t") for ln in lines[3:-1]]
    assert all(len(r) == k + 1 for r in rows)
    return (np.array(head[0][1:], np.float64), np.array(head[1][1:], np.float64), [r[0] for r in rows],
            np.array([r[1:] for r in rows], np.float64).reshape(n, k))


def _check(text, names, d, k):
    n = len(names)
    eig, share, got_names, x = _parse(text, n, k)
    assert got_names == names
    lam = P.spectrum(d)
    lam1, kk = lam[0], min(k, n - 1)
    want_eig, want_x, trace = P.pcoa(d, k)
    assert np.all(np.abs(eig[:kk] - lam[:kk]) <= 2 * TOL * lam1 + ROUND * np.abs(lam[:kk]))
    assert np.all(np.abs(share[:kk] - lam[:kk] / trace) <= (2 * TOL * lam1 + 2 * ROUND * np.abs(lam[:kk])) / abs(trace))
    for a in range(kk):
        gap = np.min(np.abs(np.delete(lam, a) - lam[a]))
        sign = -1.0 if x[:, a] @ want_x[:, a] < 0 else 1.0
        err = np.max(np.abs(sign * x[:, a] - want_x[:, a]))
        bound = (4 * TOL * lam1 / gap) * np.sqrt(max(lam[a], 0.0)) + 2 * TOL * np.sqrt(lam1) + ROUND * np.max(np.abs(want_x[:, a]))
        print("axis", a, "lambda / lambda_1", lam[a] / lam1, "gap / lambda_1", gap / lam1, "error", err, "bound", bound)
        assert err <= bound, (a, err, bound)
        if eig[a] > 0:
            assert x[int(np.argmax(np.abs(want_x[:, a]))), a] > 0
    return lam


@pytest.fixture(scope="module")
def hmh(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pcoa_hmh")
    return _Set(tmp, "X", _families(700, 40_000), "hmh", 16, 0)


def test_hmh_coordinates_against_the_model(hmh):
    _, names = hmh.names(False)
    lam = _check(hmh.text("p.tsv", ["--pcoa", "3"]), names, hmh.dist(), 3)
    assert lam[-1] < 0                                                          # sketch distances are not Euclidean


def test_hmh_bytes_do_not_depend_on_the_run_shape(hmh):
    want = hmh.text("p.tsv", ["--pcoa", "3"])
    for flags in (["--block-rows", "7"], ["-t", "1"], ["-t", "4"], ["--block-rows", "7", "-t", "4"]):
        assert hmh.text("p.tsv", ["--pcoa", "3"] + flags) == want, flags
    # --file-order changes the row order only: the same lines in another order, up to what another summation order does to the digits
    fo = hmh.text("p.tsv", ["--pcoa", "3", "--file-order"])
    assert hmh.text("p.tsv", ["--pcoa", "3", "--file-order", "--block-rows", "7", "-t", "1"]) == fo
    _, names_fo = hmh.names(True)
    _check(fo, names_fo, hmh.dist(file_order=True), 3)
    assert sorted(names_fo) == sorted(hmh.names(False)[1]) and names_fo != hmh.names(False)[1]


def test_hll_p12_with_simulated_bias_tables(tmp_path):
    s = _Set(tmp_path, "X", _families(800, 120_000, sizes=(5, 4, 4)), "hll", 21, 12)
    _, names = s.names(False)
    _check(s.text("p.tsv", ["--pcoa", "3", "--hll-bias-sim"]), names, s.dist(), 3)


def test_ull_p12(tmp_path):
    s = _Set(tmp_path, "X", _families(900, 60_000, sizes=(5, 4, 4)), "ull", 16, 12)
    _, names = s.names(False)
    _check(s.text("p.tsv", ["--pcoa", "3"]), names, s.dist(), 3)


def test_an_undefined_distance_and_one_name_are_refused(tmp_path):
    genomes = [O.synth_genome(1, 30_000), O.synth_genome(2, 30_000), np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]
    s = _Set(tmp_path, "X", genomes, "ull", 16, 12)
    _, names = s.names(False)
    d = s.dist(model=0)
    rows, cols = np.nonzero(np.isnan(np.tril(d, -1)))
    assert len(rows) == 1
    r = s.run("p.tsv", ["--pcoa", "2", "-m", "0"])
    assert r.returncode != 0 and "NaN" in r.stderr and names[rows[0]] in r.stderr and names[cols[0]] in r.stderr
    one = _Set(tmp_path, "Y", genomes[:1], "hmh", 16, 0)
    r = one.run("p.tsv", ["--pcoa", "2"])
    assert r.returncode != 0 and "at least 2 names" in r.stderr
