"""`lash merge` through the command line: the merged collection's sketch file must hold, byte for byte and in group order, the oracle's
folds (merge_images from the image of an empty sketch) of the input collection's own images; its names file the group names; its
parameters file the input's bytes.  The groups come from `lash dist --cluster`, whose output goes in unchanged."""
import os
import re

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
from test_gpu_dist_within import _family, _run, _sketch, _write

pytestmark = pytest.mark.gpu

K = 16
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
TINY = 5                                                                   # the file shorter than k: its image is the empty sketch's


def _collection(seed):
    """a family of five (mutation rates up to 3 %: distances up to about 0.025), an input shorter than k, six strangers: 12 files"""
    fam = _family(seed, 20_000, rates=(0.0, 0.002, 0.005, 0.01, 0.03))
    return fam + [np.frombuffer(b"ACGTAC", np.uint8).copy()] + [O.synth_genome(seed + 1 + i, 12_000 + 3_000 * i) for i in range(6)]


class _Col:
    def __init__(self, tmp_path, algo, p):
        self.tmp_path, self.algo, self.p = tmp_path, algo, p
        self.sk = ["-k", str(K)] + (["-a", algo, "-p", str(p)] if algo != "hmh" else [])
        self.bias = ["--hll-bias-sim"] if algo == "hll" else []
        self.paths = _write(tmp_path, "g", _collection(800))
        _sketch(tmp_path, "X", self.paths, self.sk)
        self.images = self.read("X")
        assert self.images.shape[0] == len(self.paths) == 12

    def read(self, prefix):
        raw = np.frombuffer(H.zstd_read(str(self.tmp_path / (prefix + "_sketches.bin"))), dtype=np.uint8)
        return raw.reshape(-1, O.image_bytes(ALGO[self.algo], self.p))

    def fold(self, members):
        acc = self.images[TINY].copy()
        for m in members:
            acc = O.merge_images(ALGO[self.algo], self.p, acc, self.images[m])
        return acc

    def merge(self, out, flags, env=None):
        return _run(self.tmp_path, ["merge", "-r", "X", "-o", out] + flags, env)

    def check(self, out, names, groups):
        """the three files of collection `out` against group names and member lists"""
        want = np.stack([self.fold(g) for g in groups])
        got = self.read(out)
        assert got.shape == want.shape and np.array_equal(got, want), out
        assert (self.tmp_path / (out + "_files.json")).read_text() == H.json_array(names)
        assert (self.tmp_path / (out + "_parameters.json")).read_bytes() == (self.tmp_path / "X_parameters.json").read_bytes()


@pytest.fixture(scope="module", params=[("hmh", 0), ("hll", 10), ("ull", 12)], ids=["hmh", "hll10", "ull12"])
def col(request, tmp_path_factory):
    algo, p = request.param
    return _Col(tmp_path_factory.mktemp("merge_" + algo), algo, p)


def test_clusters_go_in_unchanged(col):
    r = _run(col.tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "clusters.tsv", "--cluster", "0.06"] + col.bias)
    assert r.returncode == 0, r.stderr
    lines = (col.tmp_path / "clusters.tsv").read_text().split("\n")
    assert lines[0] == "Representative\tMember" and lines[-1] == "" and len(lines) == 14
    reps, groups = [], {}
    for ln in lines[1:-1]:
        rep, member = ln.split("\t")
        if rep not in groups:
            reps.append(rep)
        groups.setdefault(rep, []).append(col.paths.index(member))
    family = [g for g in groups.values() if 0 in g][0]
    assert sorted(family) == [0, 1, 2, 3, 4] and len(reps) == 8                              # the family joined, the strangers did not
    r = col.merge("mrg", ["--groups", "clusters.tsv"])
    assert r.returncode == 0 and "dropped" not in r.stderr, r.stderr
    col.check("mrg", reps, [groups[rep] for rep in reps])
    # the result reads like any collection: growth, dist and merge itself
    r = _run(col.tmp_path, ["growth", "-r", "mrg", "-o", "mrg_growth.tsv"] + col.bias)
    assert r.returncode == 0 and (col.tmp_path / "mrg_growth.tsv").read_text().count("\n") == 9, r.stderr
    r = _run(col.tmp_path, ["merge", "-r", "mrg", "-o", "again", "--all", "everything"])
    assert r.returncode == 0, r.stderr
    col.check("again", ["everything"], [list(range(12))])


def test_all_is_the_union_of_everything(col):
    r = col.merge("pan", ["--all", "pan genome"])
    assert r.returncode == 0, r.stderr
    col.check("pan", ["pan genome"], [list(range(12))])


def test_keep_others_in_row_order_and_threads(col):
    (col.tmp_path / "one.tsv").write_text("pair\t%s\r\n\npair\t%s\n" % (col.paths[3], col.paths[0]))
    r = col.merge("drop", ["--groups", "one.tsv"])
    assert r.returncode == 0 and "10 sketches are in no group" in r.stderr, r.stderr
    col.check("drop", ["pair"], [[3, 0]])
    key_order = [i for i in H.name_order(col.paths) if i not in (0, 3)]
    list_order = [i for i in range(12) if i not in (0, 3)]
    assert key_order != list_order
    for out, flags, order in (("ko", [], key_order), ("kf", ["--file-order"], list_order)):
        r = col.merge(out, ["--groups", "one.tsv", "--keep-others"] + flags)
        assert r.returncode == 0 and "in no group" not in r.stderr, r.stderr
        col.check(out, ["pair"] + [col.paths[i] for i in order], [[3, 0]] + [[i] for i in order])
    for t in ("1", "4"):
        r = col.merge("th" + t, ["--groups", "one.tsv", "--keep-others", "--file-order", "-t", t])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(col.read("th" + t), col.read("kf"))


def test_two_files_of_one_sample(col):
    """files A and B as one group against the sketch of one FASTA holding both records: the same bytes, distance 0"""
    a, b = 6, 9
    recs = [open(col.paths[i], "rb").read() for i in (a, b)]
    (col.tmp_path / "both.fa").write_bytes(recs[0] + recs[1])
    _sketch(col.tmp_path, "two", [col.paths[a], col.paths[b]], col.sk)
    _sketch(col.tmp_path, "whole", [str(col.tmp_path / "both.fa")], col.sk)
    r = _run(col.tmp_path, ["merge", "-r", "two", "-o", "sample", "--all", "sample 1"])
    assert r.returncode == 0, r.stderr
    got, want = col.read("sample"), col.read("whole")
    assert got.shape == want.shape == (1, col.images.shape[1])
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("merge %s: %d bytes differ, first at %s (got %d want %d)" % (col.algo, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
    r = _run(col.tmp_path, ["dist", "-q", "sample", "-r", "whole", "-o", "sample_dist.tsv"] + col.bias)
    assert r.returncode == 0, r.stderr
    rows = (col.tmp_path / "sample_dist.tsv").read_text().split("\n")[:-1]
    pair = [ln for ln in rows if "sample 1" in ln and "both.fa" in ln]
    assert len(pair) == 1 and float(pair[0].rsplit("\t", 1)[1]) == 0.0, rows


REFUSALS = [
    ("g\t{0}\nno tab here\n", "line 2", "no tab"),
    ("g\t{0}\n\ng\t{0}\t{1}\n", "line 3", "more than one tab"),
    ("Representative\tMember\n\t{0}\n", "line 2", "empty group"),
    ("g\t{0}\r\ng\t\r\n", "line 2", "empty member"),
    ("g\t{0}\ng\t{1}\ng\tnope.fa\n", "line 3", "nope.fa"),
    ("\n\n", "bad.tsv", "no group"),
]


@pytest.mark.parametrize("text,where,what", REFUSALS, ids=[r[2].replace(" ", "_") for r in REFUSALS])
def test_bad_groups_files_are_refused_with_the_line(col, text, where, what):
    (col.tmp_path / "bad.tsv").write_text(text.format(col.paths[0], col.paths[1]))
    r = col.merge("bad", ["--groups", "bad.tsv"])
    assert r.returncode != 0 and where in r.stderr and what in r.stderr, r.stderr
    assert not (col.tmp_path / "bad_sketches.bin").exists() and not (col.tmp_path / "bad_files.json").exists()


def test_bad_flags_are_refused(col):
    (col.tmp_path / "ok.tsv").write_text("g\t%s\n" % col.paths[0])
    for flags, what in ((["--groups", "ok.tsv", "--all", "x"], "--all"), (["--all", "x", "--keep-others"], "--keep-others"), ([], "--groups"),
                        (["--groups", "missing.tsv"], "missing.tsv"), (["--all", "x", "--orders", "3"], "--orders")):
        r = col.merge("bad", flags)
        assert r.returncode != 0 and what in r.stderr, (flags, r.stderr)
        assert not (col.tmp_path / "bad_sketches.bin").exists()
    r = _run(col.tmp_path, ["merge", "-r", "X", "--all", "x"])
    assert r.returncode != 0 and "--output" in r.stderr
    r = _run(col.tmp_path, ["merge", "-o", "bad", "--all", "x"])
    assert r.returncode != 0 and "--reference" in r.stderr


def test_the_timing_line(col):
    (col.tmp_path / "tm.tsv").write_text("a\t%s\na\t%s\nb\t%s\n" % (col.paths[1], col.paths[2], col.paths[1]))
    r = col.merge("tm", ["--groups", "tm.tsv", "--keep-others"], dict(os.environ, LASH_CLI_TIMING="1"))
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[lash merge] ")]
    assert len(lines) == 1
    m = re.fullmatch(r"\[lash merge\] (\d+) names, (\d+) groups, (\d+) members, segment (\d+), fold (\d+\.\d+) ms", lines[0])
    assert m, lines[0]
    assert [int(m.group(i)) for i in (1, 2, 3)] == [12, 2 + 10, 3 + 10] and int(m.group(4)) >= 1
    assert "[lash merge]" not in col.merge("tm", ["--groups", "tm.tsv"]).stderr
