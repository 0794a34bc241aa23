"""`lash dist --tree` and `--cluster D --linkage L` through the command line.  The yardstick is the model (tree_model.py) on the exact
distances of the same sketches, taken through the ABI (pair_block + lash_dist_rows: the doubles the list form rounds to six decimals,
not the text) in the run's row order."""
import os

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
import tree_model as T
from test_gpu_dist_cluster import D_VALUES
from test_gpu_dist_within import _dense, _family, _mutated, _run, _sketch, _sketches, _write

pytestmark = pytest.mark.gpu


def _collection(seed, length):
    """a family, exact duplicates of two of its members under other names, a second family, unrelated genomes: 19 files"""
    fam = _family(seed, length)
    return fam[:3] + [O.synth_genome(seed + 1, length)] + fam[3:] + [fam[0].copy(), fam[2].copy()] \
        + _family(seed + 2, length, rates=(0.0, 0.004, 0.02, 0.1)) + [O.synth_genome(seed + 3, length), O.synth_genome(seed + 4, length // 2),
                                                                       fam[0].copy(), _mutated(fam[5], 0.01, seed)]


class _Set:
    """one sketched collection: the command line's files under `prefix`, and the same sketches made in process for the model"""

    def __init__(self, tmp_path, prefix, genomes, algo, k, p, est="fgra", env=None):
        self.tmp_path, self.prefix, self.genomes, self.algo, self.k, self.p, self.est, self.env = tmp_path, prefix, genomes, algo, k, p, est, env
        self.paths = _write(tmp_path, prefix.lower(), genomes)
        sk = ["-k", str(k)] + (["-a", algo, "-p", str(p)] if algo != "hmh" else [])
        _sketch(tmp_path, prefix, self.paths, sk, env)
        self._dist = {}

    def names(self, file_order):
        order = list(range(len(self.paths))) if file_order else H.name_order(self.paths)
        return order, [self.paths[i] for i in order]

    def dist(self, file_order=False, model=1, fp32=False):
        """the symmetric matrix of printed distances in row order"""
        key = (file_order, model, fp32)
        if key not in self._dist:
            order, _ = self.names(file_order)
            ctx, imgs = _sketches(self.algo, self.k, self.p, [self.genomes[i] for i in order])
            s = ctx.sketch_set(self.algo, self.p, imgs)
            card = s.cardinalities(self.est)
            s.prepare()
            n = s.n
            low = np.tril(_dense(s, card, self.algo, self.p, self.k, model, fp32, 0, n, n, True, est=self.est), -1)
            s.free()
            ctx.close()
            self._dist[key] = low + low.T                      # (-0, the distance of identical sketches under -m 1, enters as 0: x + 0 = +0)
        return self._dist[key]

    def run(self, out, flags):
        extra = ["-e", self.est] if self.algo == "ull" else []
        return _run(self.tmp_path, ["dist", "-q", self.prefix, "-r", self.prefix, "-o", out] + extra + flags, self.env)

    def text(self, out, flags):
        r = self.run(out, flags)
        assert r.returncode == 0, (flags, r.stderr)
        return (self.tmp_path / out).read_text()

    def want_tree(self, linkage, file_order=False, model=1, fp32=False):
        _, names = self.names(file_order)
        return T.newick(names, T.merges(self.dist(file_order, model, fp32), T.LINKAGES[linkage])) + "\n"


def _timing(stderr):
    for ln in stderr.split("\n"):
        if "--tree:" in ln:
            return [float(w) for w in ln.replace(",", " ").split() if w.replace(".", "", 1).isdigit()]
    raise AssertionError("no --tree timing line in: " + stderr[-500:])


@pytest.fixture(scope="module")
def hmh(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tree_hmh")
    return _Set(tmp, "X", _collection(100, 60_000), "hmh", 16, 0)


def test_hmh_trees_equal_the_model(hmh):
    n = len(hmh.paths)
    for linkage in ("average", "single", "complete"):
        got = hmh.text("t.nwk", ["--tree", "--linkage", linkage])
        assert got == hmh.want_tree(linkage), linkage
        assert got.count(",") == n - 1 and got.endswith(";\n") and all(p in got for p in hmh.paths)
    assert hmh.text("t.nwk", ["--tree"]) == hmh.want_tree("average")           # the default is UPGMA


def test_hmh_bytes_do_not_depend_on_the_run_shape(hmh):
    n = len(hmh.paths)
    want = hmh.want_tree("average")
    for flags in (["--block-rows", "1"], ["--block-rows", "3"], ["--block-rows", str(n)], ["-t", "1"], ["-t", "4"], ["--devices", "0,0", "--block-rows", "3"],
                  ["--block-rows", "3", "-t", "4"]):
        assert hmh.text("t.nwk", ["--tree"] + flags) == want, flags
    # --file-order: the tree changes only through the row order, and the model follows
    want_fo = hmh.want_tree("average", file_order=True)
    for flags in ([], ["--block-rows", "1"], ["--block-rows", "3", "-t", "1"], ["--block-rows", str(n), "-t", "4"]):
        assert hmh.text("t.nwk", ["--tree", "--file-order"] + flags) == want_fo, flags
    assert H.name_order(hmh.paths) != list(range(n))


def test_hmh_fp32_and_binomial_model(hmh):
    assert hmh.text("t.nwk", ["--tree", "--fp32"]) == hmh.want_tree("average", fp32=True)
    assert hmh.text("t.nwk", ["--tree", "-m", "0"]) == hmh.want_tree("average", model=0)
    assert hmh.text("t.nwk", ["--tree", "-m", "0", "--fp32", "--linkage", "complete", "--block-rows", "3"]) == hmh.want_tree("complete", model=0, fp32=True)
    assert not np.array_equal(hmh.dist(fp32=True), hmh.dist()) and not np.array_equal(hmh.dist(model=0), hmh.dist())


def test_hmh_timing_line(hmh):
    n = len(hmh.paths)
    r = _run(hmh.tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "t.nwk", "--tree"], dict(os.environ, LASH_CLI_TIMING="1"))
    assert r.returncode == 0, r.stderr
    names, steps, rescanned, nbytes, ms = _timing(r.stderr)
    assert (names, steps, nbytes) == (n, n - 1, 8 * n * n) and rescanned >= n and ms > 0


def test_single_linkage_cut_is_what_cluster_prints(hmh):
    """the cross-check against existing behaviour: the single-linkage tree (whose bytes the model gives, above) cut at D is the partition
    of --cluster D; an explicit `--linkage single` is the same route"""
    _, names = hmh.names(False)
    mg = T.merges(hmh.dist(), T.SINGLE)
    assert hmh.text("t.nwk", ["--tree", "--linkage", "single"]) == T.newick(names, mg) + "\n"
    sizes = set()
    for D in D_VALUES:
        alone = hmh.text("c.tsv", ["--cluster", repr(D)])
        assert alone == T.render_clusters(names, T.cut(len(names), mg, D)), D
        assert hmh.text("c.tsv", ["--cluster", repr(D), "--linkage", "single"]) == alone, D
        assert hmh.text("c.tsv", ["--linkage", "single", "--cluster", repr(D), "--block-rows", "3"]) == alone, D
        sizes.add(len(set(T.cut(len(names), mg, D))))
    assert len(sizes) >= 4                                                     # the cutoffs do cut at different places


@pytest.mark.parametrize("linkage", ["average", "complete"])
def test_cluster_with_a_linkage_is_the_cut_of_the_tree(hmh, linkage):
    _, names = hmh.names(False)
    n = len(names)
    mg = T.merges(hmh.dist(), T.LINKAGES[linkage])
    heights = sorted(set(m[2] for m in mg))
    mid = heights[len(heights) // 2]
    for D in D_VALUES + (mid, float(np.nextafter(mid, 0.0))):                  # at a merge height (included) and just below it
        got = hmh.text("c.tsv", ["--cluster", repr(D), "--linkage", linkage])
        assert got == T.render_clusters(names, T.cut(n, mg, D)), D
        assert got.count("\n") == n + 1
    assert T.cut(n, mg, mid) != T.cut(n, mg, float(np.nextafter(mid, 0.0)))
    _, names_fo = hmh.names(True)
    mg_fo = T.merges(hmh.dist(file_order=True), T.LINKAGES[linkage])
    got = hmh.text("c.tsv", ["--cluster", "0.05", "--linkage", linkage, "--file-order", "--block-rows", "3", "--devices", "0,0"])
    assert got == T.render_clusters(names_fo, T.cut(n, mg_fo, 0.05))


def test_hll_p10(tmp_path):
    genomes = _family(301, 400_000, rates=(0.0, 0.005, 0.03, 0.1)) + [O.synth_genome(302, 300_000), _family(301, 400_000)[0].copy(),
                                                                      O.synth_genome(303, 350_000)]
    s = _Set(tmp_path, "X", genomes, "hll", 21, 10)
    for linkage, flags in (("average", []), ("complete", ["--block-rows", "3"]), ("single", ["--block-rows", "1", "-t", "1"])):
        assert s.text("t.nwk", ["--tree", "--linkage", linkage] + flags) == s.want_tree(linkage), linkage
    assert s.text("t.nwk", ["--tree", "--fp32", "-m", "0", "--file-order"]) == s.want_tree("average", file_order=True, model=0, fp32=True)


@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_ull_p12_and_an_undefined_distance(tmp_path, est):
    genomes = _family(501, 200_000, rates=(0.0, 0.005, 0.03, 0.1, 0.3)) + [O.synth_genome(503, 150_000), _family(501, 200_000)[1].copy()]
    genomes += [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]     # shorter than k: empty sketches
    s = _Set(tmp_path, "X", genomes, "ull", 16, 12, est=est)
    # -m 1: an empty sketch is at distance 1 from everything; the tree is defined
    for linkage, flags in (("average", []), ("complete", ["--block-rows", "3", "--fp32"])):
        assert s.text("t.nwk", ["--tree", "--linkage", linkage] + flags) == s.want_tree(linkage, fp32="--fp32" in flags), linkage
    # -m 0: the two empty sketches are NaN against each other: refused, the two names in the message
    d = s.dist(model=0)
    rows, cols = np.nonzero(np.isnan(np.tril(d, -1)))
    assert len(rows) == 1
    _, names = s.names(False)
    for flags in (["--tree"], ["--tree", "--block-rows", "1"], ["--cluster", "0.1", "--linkage", "average"]):
        r = s.run("t.nwk", flags + ["-m", "0"])
        assert r.returncode != 0 and "NaN" in r.stderr and names[rows[0]] in r.stderr and names[cols[0]] in r.stderr, (flags, r.stderr)


def test_hll_bias_regime_is_refused_without_tables(tmp_path):
    """p = 14: two ~9 kbp genomes are each in linear counting, their union is not; without tables the run is refused with the pair named,
    as the unfiltered run is, and --hll-bias-sim lets it through"""
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    genomes = [O.synth_genome(55, 9_000), O.synth_genome(56, 8_000), _mutated(O.synth_genome(55, 9_000), 0.001, 5)]
    s = _Set(tmp_path, "S", genomes, "hll", 21, 14, env=env)
    want = s.run("full.tsv", [])
    assert want.returncode != 0 and "bias tables" in want.stderr and "union of" in want.stderr
    for flags in (["--tree"], ["--tree", "--block-rows", "1"], ["--cluster", "0.1", "--linkage", "complete"]):
        got = s.run("t.nwk", flags)
        assert (got.returncode, got.stderr) == (want.returncode, want.stderr), flags
    ok = s.text("t.nwk", ["--tree", "--hll-bias-sim"])
    assert ok.count(",") == 2 and ok.endswith(";\n") and all(p in ok for p in s.paths)
    assert s.text("t.nwk", ["--tree", "--hll-bias-sim", "--block-rows", "1"]) == ok
