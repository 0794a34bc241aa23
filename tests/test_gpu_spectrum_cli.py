"""`lash spectrum` through the command line: {OUT}_spectrum.tsv and {OUT}_groups.tsv must be, byte for byte, the text of the numpy model
(tests/spectrum_model.py) over the input collection's own images, with each group's union cardinality taken from `lash merge`'s image of
the same group through the product's own cardinality; {OUT}_curves.tsv within 1e-9 relative of the model (the host's compiler may
contract a multiply-add differently: at most 2 n roundings of 2^-53 at n <= 12; a wrong term is far above that).  The groups come from
`lash dist --cluster`, whose output goes in unchanged.

The collection is the one the merge test uses, built here: a family of five (mutation rates up to 3 %), an input shorter than k, six
strangers: 12 files."""
import subprocess

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
import spectrum_model as S

pytestmark = pytest.mark.gpu

K = 16
TINY = 5


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _collection(seed):
    base = O.synth_genome(seed, 20_000)
    fam = [base if r == 0 else _mutated(base, r, seed * 100 + i) for i, r in enumerate((0.0, 0.002, 0.005, 0.01, 0.03))]
    return fam + [np.frombuffer(b"ACGTAC", np.uint8).copy()] + [O.synth_genome(seed + 1 + i, 12_000 + 3_000 * i) for i in range(6)]


def _run(tmp_path, args):
    return subprocess.run([H.CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)


class _Col:
    def __init__(self, tmp_path):
        self.tmp_path = tmp_path
        self.paths = []
        for i, g in enumerate(_collection(800)):
            f = tmp_path / ("g%d.fa" % i)
            f.write_bytes(b">s\n" + g.tobytes() + b"\n")
            self.paths.append(str(f))
        self.sketch("X", self.paths, [])
        self.regs = S.registers(self.read("X"))
        assert self.regs.shape == (12, S.M) and not self.regs[TINY].any()

    def sketch(self, prefix, paths, flags):
        (self.tmp_path / (prefix + ".txt")).write_text("\n".join(paths) + "\n")
        r = _run(self.tmp_path, ["sketch", "-f", prefix + ".txt", "-o", prefix, "-k", str(K)] + flags)
        assert r.returncode == 0, r.stderr

    def read(self, prefix):
        raw = np.frombuffer(H.zstd_read(str(self.tmp_path / (prefix + "_sketches.bin"))), dtype=np.uint8)
        return raw.reshape(-1, 2 * S.M)

    def unions(self, tag, flags, n_groups):
        """the cardinalities of `lash merge`'s images for the same groups"""
        import lash_amd
        r = _run(self.tmp_path, ["merge", "-r", "X", "-o", tag] + flags)
        assert r.returncode == 0, r.stderr
        images = self.read(tag)
        assert images.shape[0] == n_groups
        return [lash_amd.sketch_cardinality("hmh", 0, img) for img in images]

    def spectrum(self, out, flags):
        return _run(self.tmp_path, ["spectrum", "-r", "X", "-o", out] + flags)

    def text(self, out, which):
        return (self.tmp_path / ("%s_%s.tsv" % (out, which))).read_text()

    def written(self, out):
        return [w for w in ("spectrum", "groups", "curves") if (self.tmp_path / ("%s_%s.tsv" % (out, w))).exists()]


@pytest.fixture(scope="module")
def col(tmp_path_factory):
    return _Col(tmp_path_factory.mktemp("spectrum"))


def _check_curves(text, names, hists, unions):
    lines = text.split("\n")
    assert lines[0] == "Group\tGenomes\tPan\tCore" and lines[-1] == ""
    at = 1
    for name, h, U in zip(names, hists, unions):
        pan, core = S.curves(h, U)
        for m in range(1, len(h)):
            g, genomes, p, c = lines[at].split("\t")
            at += 1
            assert (g, int(genomes)) == (name, m)
            for got, want in ((float(p), pan[m - 1]), (float(c), core[m - 1])):
                assert abs(got - float("%.10g" % want)) <= 1e-9 * abs(want), (name, m, got, want)
    assert at == len(lines) - 1


def test_clusters_go_in_unchanged(col):
    r = _run(col.tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "clusters.tsv", "--cluster", "0.06"])
    assert r.returncode == 0, r.stderr
    lines = (col.tmp_path / "clusters.tsv").read_text().split("\n")
    assert lines[0] == "Representative\tMember" and len(lines) == 14
    reps, groups = [], {}
    for ln in lines[1:-1]:
        rep, member = ln.split("\t")
        if rep not in groups:
            reps.append(rep)
        groups.setdefault(rep, []).append(col.paths.index(member))
    assert sorted([g for g in groups.values() if 0 in g][0]) == [0, 1, 2, 3, 4] and len(reps) == 8   # the family joined, the strangers did not
    members = [sorted(groups[rep]) for rep in reps]
    hists = [S.hist(col.regs, m) for m in members]
    unions = col.unions("mrg", ["--groups", "clusters.tsv"], len(reps))
    r = col.spectrum("cl", ["--groups", "clusters.tsv", "--curves"])
    assert r.returncode == 0 and "Spectrum tables written." in r.stdout, r.stderr
    assert col.text("cl", "spectrum") == S.spectrum_text(reps, hists, unions)
    assert col.text("cl", "groups") == S.groups_text(reps, hists, unions)
    _check_curves(col.text("cl", "curves"), reps, hists, unions)
    # the family shares most of its k-mers, so its line has a core; the group of the input shorter than k has nothing
    fam = [i for i, m in enumerate(members) if 0 in m][0]
    tiny = [i for i, m in enumerate(members) if m == [TINY]][0]
    assert int(hists[fam][5]) > S.M // 4 and hists[tiny].tolist() == [S.M, 0]
    assert ("%s\t1\t0\t0.000\t0.000\t0.000\t0.000\n" % reps[tiny]) in col.text("cl", "groups")
    assert ("\n%s\t" % reps[tiny]) not in col.text("cl", "spectrum")
    # other thresholds move k-mers between the classes, not the spectrum
    r = col.spectrum("th", ["--groups", "clusters.tsv", "--core", "0.6", "--cloud", "0.3"])
    assert r.returncode == 0, r.stderr
    assert col.written("th") == ["spectrum", "groups"]
    assert col.text("th", "spectrum") == col.text("cl", "spectrum")
    assert col.text("th", "groups") == S.groups_text(reps, hists, unions, 0.6, 0.3) != col.text("cl", "groups")


def test_the_default_is_one_group_of_everything(col):
    hists = [S.hist(col.regs, range(12))]
    unions = col.unions("pan", ["--all", "all"], 1)
    r = col.spectrum("dflt", ["--curves"])
    assert r.returncode == 0, r.stderr
    assert col.text("dflt", "spectrum") == S.spectrum_text(["all"], hists, unions)
    assert col.text("dflt", "groups") == S.groups_text(["all"], hists, unions)
    _check_curves(col.text("dflt", "curves"), ["all"], hists, unions)
    r = col.spectrum("named", ["--all", "all", "--curves", "--file-order", "-t", "2"])
    assert r.returncode == 0, r.stderr
    for which in ("spectrum", "groups", "curves"):
        assert col.text("named", which) == col.text("dflt", which), which
    r = col.spectrum("other", ["--all", "pan genome"])
    assert r.returncode == 0 and col.text("other", "groups") == col.text("dflt", "groups").replace("\nall\t", "\npan genome\t"), r.stderr


def test_a_member_listed_twice_counts_once(col):
    a, b, c = col.paths[1], col.paths[3], col.paths[8]
    (col.tmp_path / "once.tsv").write_text("trio\t%s\ntrio\t%s\ntrio\t%s\n" % (a, b, c))
    (col.tmp_path / "twice.tsv").write_text("trio\t%s\r\ntrio\t%s\ntrio\t%s\n\ntrio\t%s\ntrio\t%s\n" % (b, a, b, c, a))
    for out, f in (("once", "once.tsv"), ("twice", "twice.tsv")):
        r = col.spectrum(out, ["--groups", f, "--curves"])
        assert r.returncode == 0, r.stderr
    hists = [S.hist(col.regs, [1, 3, 8])]
    unions = col.unions("trio", ["--groups", "once.tsv"], 1)
    assert col.text("once", "spectrum") == S.spectrum_text(["trio"], hists, unions)
    assert col.text("once", "groups") == S.groups_text(["trio"], hists, unions)
    for which in ("spectrum", "groups", "curves"):
        assert col.text("twice", which) == col.text("once", which), which


def test_an_hll_collection_is_refused(col):
    col.sketch("L", col.paths[:3], ["-a", "hll", "-p", "10"])
    r = _run(col.tmp_path, ["spectrum", "-r", "L", "-o", "refused", "--curves"])
    assert r.returncode != 0 and "hll" in r.stderr and "HyperMinHash" in r.stderr, r.stderr
    assert col.written("refused") == []
    (col.tmp_path / "bad.tsv").write_text("g\t%s\ng\tnope.fa\n" % col.paths[0])
    r = col.spectrum("refused", ["--groups", "bad.tsv"])
    assert r.returncode != 0 and "line 2" in r.stderr and "nope.fa" in r.stderr and col.written("refused") == []
