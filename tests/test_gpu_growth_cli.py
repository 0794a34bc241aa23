"""`lash growth` through the command line: the table must equal the model's (growth_model.py) byte for byte — the orders restated in
Python, every prefix folded with merge_images and estimated by the host entry for one image — in the run's row order."""
import os
import re

import numpy as np
import pytest

import growth_model as G
import host_lib as H
import oracle_lib as O
from test_gpu_dist_within import _family, _run, _sketch, _sketches, _write

pytestmark = pytest.mark.gpu

K = 16


def _collection(seed):
    """a 2.5 kbp genome first (under hll p = 10 its sketch needs the bias tables), a family, a duplicate, an input shorter than k, strangers: 15 files"""
    fam = _family(seed, 30_000)
    return [O.synth_genome(seed + 9, 2_500)] + fam + [fam[1].copy(), np.frombuffer(b"ACGTAC", np.uint8).copy()] \
        + [O.synth_genome(seed + 1 + i, 20_000 + 7_000 * i) for i in range(5)]


class _Set:
    def __init__(self, tmp_path, algo, p, est="fgra"):
        self.tmp_path, self.algo, self.p, self.est = tmp_path, algo, p, est
        self.genomes = _collection(700)
        self.paths = _write(tmp_path, "g", self.genomes)
        _sketch(tmp_path, "X", self.paths, ["-k", str(K)] + (["-a", algo, "-p", str(p)] if algo != "hmh" else []))
        self._card = {}

    def want(self, n_orders, seed, file_order=False):
        import lash_amd
        from lash_amd.sketch import HllBias
        order = list(range(len(self.paths))) if file_order else H.name_order(self.paths)
        rows = G.orders(len(order), n_orders, seed)
        key = (file_order, n_orders, seed)
        if key not in self._card:
            ctx, imgs = _sketches(self.algo, K, self.p, [self.genomes[i] for i in order])
            bias = HllBias.simulated(ctx, self.p) if self.algo == "hll" else None      # what --hll-bias-sim makes: the defaults, seed 42
            self._card[key] = G.prefix_cardinalities(ctx, self.algo, self.p, imgs, rows, self.est, bias)
            ctx.close()
        return G.table([self.paths[i] for i in order], rows, self._card[key])

    def run(self, flags, env=None):
        extra = (["-e", self.est] if self.algo == "ull" else []) + (["--hll-bias-sim"] if self.algo == "hll" and "--no-bias" not in flags else [])
        return _run(self.tmp_path, ["growth", "-r", "X", "-o", "g.tsv"] + extra + [f for f in flags if f != "--no-bias"], env)

    def text(self, flags, env=None):
        out = self.tmp_path / "g.tsv"
        if out.exists():
            out.unlink()
        r = self.run(flags, env)
        assert r.returncode == 0, (flags, r.stderr)
        return out.read_text()


@pytest.fixture(scope="module", params=[("hmh", 0, "fgra"), ("hll", 10, "fgra"), ("ull", 12, "ml")], ids=["hmh", "hll10", "ull12"])
def col(request, tmp_path_factory):
    algo, p, est = request.param
    return _Set(tmp_path_factory.mktemp("growth_" + algo), algo, p, est)


def test_the_table_equals_the_model(col):
    n = len(col.paths)
    one = col.text(["--orders", "1"])
    assert one == col.want(1, 42) == col.text([])                                         # one order is the default
    assert one.count("\n") == n + 1 and one.startswith("Order\tStep\tName\tUnion\tNew\n0\t1\t")
    four = col.text(["--orders", "4", "--seed", "7"])
    assert four == col.want(4, 7) and four.count("\n") == 4 * n + 1
    assert four[:len(one)] == one                                                         # order 0 does not depend on the seed
    assert col.text(["--orders", "4"]) == col.want(4, 42) != four


def test_file_order_and_threads(col):
    fo = col.text(["--orders", "2", "--file-order"])
    assert fo == col.want(2, 42, file_order=True)
    assert fo != col.want(2, 42) and H.name_order(col.paths) != list(range(len(col.paths)))
    assert fo.split("\n")[1].split("\t")[2] == col.paths[0]
    for flags in (["-t", "1"], ["-t", "4"]):
        assert col.text(["--orders", "2", "--file-order"] + flags) == fo, flags


def test_the_timing_line(col):
    env = dict(os.environ, LASH_CLI_TIMING="1")
    r = col.run(["--orders", "3"], env)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[lash growth] ") and " names, " in ln]
    assert len(lines) == 1
    m = re.fullmatch(r"\[lash growth\] (\d+) names, (\d+) orders, (\d+) slices, (\d+) histogram bytes, build (\d+\.\d+) ms", lines[0])
    assert m, lines[0]
    n = len(col.paths)
    assert int(m.group(1)) == n and int(m.group(2)) == 3 and int(m.group(3)) >= 1 and int(m.group(4)) == 3 * n * 1024
    assert "[lash growth]" not in col.run(["--orders", "3"]).stderr.replace("[lash growth] --hll-bias-sim", "")


def test_hll_without_tables_names_the_order_the_step_and_the_name(col):
    if col.algo != "hll":
        assert col.text(["--no-bias"]) == col.want(1, 42)                                 # nothing to refuse: hmh and ull need no tables
        return
    out = col.tmp_path / "g.tsv"
    if out.exists():
        out.unlink()
    env = {k: v for k, v in os.environ.items() if k != "LASH_HLL_BIAS"}
    r = col.run(["--no-bias", "--file-order", "--orders", "2"], env)
    assert r.returncode != 0 and not out.exists()
    assert "order 0, step 1 (%s)" % col.paths[0] in r.stderr and "--hll-bias-sim" in r.stderr
