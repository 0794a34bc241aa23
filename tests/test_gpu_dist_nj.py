"""`lash dist --tree --nj` through the command line.  The yardstick is the model (nj_model.py) on the exact distances of the same sketches,
taken through the ABI as test_gpu_dist_tree.py does, in the run's row order.  The collection holds exact duplicates, so Q ties occur and
the labels decide."""
import os

import numpy as np
import pytest

import host_lib as H
import nj_model as NJ
import oracle_lib as O
from test_gpu_dist_tree import _Set, _collection
from test_gpu_dist_within import _family, _run

pytestmark = pytest.mark.gpu


def _want(s, file_order=False, model=1, fp32=False):
    _, names = s.names(file_order)
    return NJ.newick(names, NJ.joins(s.dist(file_order, model, fp32))) + "\n"


@pytest.fixture(scope="module")
def hmh(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nj_hmh")
    return _Set(tmp, "X", _collection(100, 60_000), "hmh", 16, 0)


def test_hmh_tree_equals_the_model(hmh):
    n = len(hmh.paths)
    got = hmh.text("t.nwk", ["--tree", "--nj"])
    assert got == _want(hmh)
    assert got.count(",") == n - 1 and got.count("(") == n - 2 and got.endswith(";\n") and all(p in got for p in hmh.paths)
    assert hmh.text("t.nwk", ["--nj", "--tree"]) == got
    assert got != hmh.text("t.nwk", ["--tree"])                                 # not the linkage tree
    d = hmh.dist()
    assert sum(np.array_equal(np.delete(d[i], [i, j]), np.delete(d[j], [i, j])) for i in range(n) for j in range(i)) >= 3   # duplicates: ties


def test_hmh_bytes_do_not_depend_on_the_run_shape(hmh):
    n = len(hmh.paths)
    want = _want(hmh)
    for flags in (["--block-rows", "1"], ["--block-rows", "3"], ["--block-rows", str(n)], ["-t", "1"], ["-t", "4"], ["--devices", "0,0", "--block-rows", "3"]):
        assert hmh.text("t.nwk", ["--tree", "--nj"] + flags) == want, flags
    # --file-order: the tree changes only through the labels that break ties, and the model follows
    want_fo = _want(hmh, file_order=True)
    for flags in ([], ["--block-rows", "3", "-t", "1"]):
        assert hmh.text("t.nwk", ["--tree", "--nj", "--file-order"] + flags) == want_fo, flags
    assert H.name_order(hmh.paths) != list(range(n))


def test_hmh_fp32_and_binomial_model(hmh):
    assert hmh.text("t.nwk", ["--tree", "--nj", "--fp32"]) == _want(hmh, fp32=True)
    assert hmh.text("t.nwk", ["--tree", "--nj", "-m", "0"]) == _want(hmh, model=0)
    assert hmh.text("t.nwk", ["--tree", "--nj", "-m", "0", "--fp32", "--block-rows", "3"]) == _want(hmh, model=0, fp32=True)


def test_hmh_timing_line(hmh):
    n = len(hmh.paths)
    r = _run(hmh.tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "t.nwk", "--tree", "--nj"], dict(os.environ, LASH_CLI_TIMING="1"))
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[lash dist] --tree --nj: ")]
    assert len(lines) == 1, r.stderr[-500:]
    words = lines[0].replace(",", " ").split()
    assert words[4:] == [str(n), "names", str(n - 1), "steps", str(8 * n * n), "matrix", "bytes", "build", words[-2], "ms"]
    assert float(words[-2]) > 0


def test_hll_p10(tmp_path):
    genomes = _family(301, 400_000, rates=(0.0, 0.005, 0.03, 0.1)) + [O.synth_genome(302, 300_000), _family(301, 400_000)[0].copy(),
                                                                      O.synth_genome(303, 350_000)]
    s = _Set(tmp_path, "X", genomes, "hll", 21, 10)
    assert s.text("t.nwk", ["--tree", "--nj"]) == _want(s)
    assert s.text("t.nwk", ["--tree", "--nj", "--block-rows", "3", "--fp32", "-m", "0", "--file-order"]) == _want(s, file_order=True, model=0, fp32=True)


def test_ull_p12_and_an_undefined_distance(tmp_path):
    genomes = _family(501, 200_000, rates=(0.0, 0.005, 0.03, 0.1, 0.3)) + [O.synth_genome(503, 150_000), _family(501, 200_000)[1].copy()]
    genomes += [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]     # shorter than k: empty sketches
    s = _Set(tmp_path, "X", genomes, "ull", 16, 12)
    # -m 1: an empty sketch is at distance 1 from everything; the tree is defined
    assert s.text("t.nwk", ["--tree", "--nj"]) == _want(s)
    assert s.text("t.nwk", ["--tree", "--nj", "--block-rows", "3", "--fp32"]) == _want(s, fp32=True)
    # -m 0: the two empty sketches are NaN against each other: refused, the two names in the message
    d = s.dist(model=0)
    rows, cols = np.nonzero(np.isnan(np.tril(d, -1)))
    assert len(rows) == 1
    _, names = s.names(False)
    for flags in (["--tree", "--nj"], ["--tree", "--nj", "--block-rows", "1"]):
        r = s.run("t.nwk", flags + ["-m", "0"])
        assert r.returncode != 0 and "NaN" in r.stderr and names[rows[0]] in r.stderr and names[cols[0]] in r.stderr, (flags, r.stderr)
