"""`lash screen` through the command line: the table must be, byte for byte, the text of the numpy model (tests/screen_model.py) built from
the ABI's own numbers for the same sketch files: the candidates and their d from pair_block_within under the reference containment, the
cardinalities, N from pair_block, the expected collisions of small pairs, and the counts of screen_wta (which are also compared with the
model over the registers).

The database is small: a genome, relatives of it at 1 % and 3 % mutations, its first half, an exact copy, an input shorter than k and five
strangers: 11 files.  The samples are three: the genome with two strangers, another stranger alone, and an input shorter than k."""
import subprocess

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
import screen_model as W
import spectrum_model as S

pytestmark = pytest.mark.gpu

K = 16
BASE, NEAR, FAR, HALF, COPY, TINY = 0, 1, 2, 3, 4, 5
DEFAULT_D = float(np.nextafter(1.0, 0.0))


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _database(seed):
    base = O.synth_genome(seed, 20_000)
    strangers = [O.synth_genome(seed + 1 + i, 12_000 + 3_000 * i) for i in range(5)]
    refs = [base, _mutated(base, 0.01, seed * 100 + 1), _mutated(base, 0.03, seed * 100 + 2), base[:10_000].copy(), base.copy(),
            np.frombuffer(b"ACGTAC", np.uint8).copy()] + strangers
    samples = [[base, strangers[0], strangers[1]], [strangers[3]], [np.frombuffer(b"ACGTACGTAC", np.uint8).copy()]]
    return refs, samples


def _run(tmp_path, args):
    return subprocess.run([H.CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)


class _Col:
    """the sketch files, and the model's table for them from the ABI's numbers"""

    def __init__(self, tmp_path):
        import lash_amd
        self.tmp_path = tmp_path
        refs, samples = _database(4100)
        self.rnames, self.qnames = ["r%d.fa" % i for i in range(len(refs))], ["s%d.fa" % i for i in range(len(samples))]
        for name, g in zip(self.rnames, refs):
            (tmp_path / name).write_bytes(b">s\n" + g.tobytes() + b"\n")
        for name, recs in zip(self.qnames, samples):
            (tmp_path / name).write_bytes(b"".join(b">s%d\n" % i + g.tobytes() + b"\n" for i, g in enumerate(recs)))
        self.sketch("DB", self.rnames, [])
        self.sketch("SM", self.qnames, [])
        self.rimg, self.qimg = self.read("DB"), self.read("SM")
        assert self.rimg.shape == (len(refs), 2 * S.M) and self.qimg.shape == (3, 2 * S.M)
        self.ctx = lash_amd.Context(0)

    def sketch(self, prefix, names, flags):
        (self.tmp_path / (prefix + ".txt")).write_text("\n".join(names) + "\n")
        r = _run(self.tmp_path, ["sketch", "-f", prefix + ".txt", "-o", prefix, "-k", str(K)] + flags)
        assert r.returncode == 0, r.stderr

    def read(self, prefix):
        return np.frombuffer(H.zstd_read(str(self.tmp_path / (prefix + "_sketches.bin"))), dtype=np.uint8).reshape(-1, 2 * S.M)

    def screen(self, out, flags):
        return _run(self.tmp_path, ["screen", "-r", "DB", "-q", "SM", "-o", out] + flags)

    def text(self, out):
        return (self.tmp_path / out).read_text()

    def model(self, max_dist=DEFAULT_D, keep_losers=False, file_order=False, model=1):
        """(the table, the candidate lists by reference name) as the command must write them"""
        import lash_amd
        ro = list(range(len(self.rnames))) if file_order else H.name_order(self.rnames)
        qo = list(range(len(self.qnames))) if file_order else H.name_order(self.qnames)
        r = self.ctx.sketch_set("hmh", 0, self.rimg, order=ro)
        q = self.ctx.sketch_set("hmh", 0, self.qimg, order=qo)
        try:
            rcard, qcard = r.cardinalities(), q.cardinalities()
            r.prepare(q)
            rows, cols, d = r.pair_block_within(0, r.n, max_dist, K, qry=q, model=model, containment="reference")
            buckets = r.pair_block(0, r.n, qry=q)["n_counts"]
            ec = r.hmh_expected_collisions(0, r.n, qry=q)
            dist = np.full((r.n, q.n), np.nan)
            dist[rows, cols] = d
            lists = [W.priority([int(i) for i, c in zip(rows, cols) if c == j], dist[:, j], rcard) for j in range(q.n)]
            shared, won = r.screen_wta(q, lists)
        finally:
            q.free()
            r.free()
        rregs, qregs = S.registers(self.rimg[ro]), S.registers(self.qimg[qo])
        ms, mw = W.screen(rregs, qregs, lists)
        assert all(np.array_equal(a, b) for a, b in zip(shared + won, ms + mw))
        wta = [[float(lash_amd.dist_rows("hmh", 0, K, model, [rcard[i]], [qcard[j]], c_or_zero=[[int(won[j][t])]], n_counts=[[int(buckets[i, j])]],
                                         hmh_ec=None if ec is None else [[ec[i, j]]], containment="reference")[0, 0])
                for t, i in enumerate(rows_j)] for j, rows_j in enumerate(lists)]
        rn, qn = [self.rnames[i] for i in ro], [self.qnames[j] for j in qo]
        named = {qn[j]: [rn[i] for i in rows_j] for j, rows_j in enumerate(lists)}
        return W.table(qn, rn, lists, shared, won, buckets, dist, wta, max_dist, keep_losers), named


@pytest.fixture(scope="module")
def col(tmp_path_factory):
    return _Col(tmp_path_factory.mktemp("screen"))


def _rows(text):
    lines = text.split("\n")
    assert lines[0] + "\n" == W.HEADER and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


def test_the_table_is_the_models(col):
    want, named = col.model()
    r = col.screen("dflt.tsv", [])
    assert r.returncode == 0 and "Screen table written." in r.stdout, r.stderr
    assert col.text("dflt.tsv") == want
    rows = _rows(want)
    # the sample that holds the genome: whoever comes first wins all it shares; of the genome and its copy, equal in every register, the
    # later one wins nothing and is left out; the two strangers of the sample are there
    first = [x for x in rows if x[0] == "s0.fa"]
    assert first[0][1] == named["s0.fa"][0] and first[0][2] == first[0][3]
    assert set(named["s0.fa"]) >= {"r%d.fa" % i for i in (BASE, NEAR, FAR, HALF, COPY, 6, 7)}
    printed = {x[1] for x in first}
    assert len({"r%d.fa" % BASE, "r%d.fa" % COPY} & printed) == 1 and {"r6.fa", "r7.fa"} <= printed
    assert named["s2.fa"] == [] and not [x for x in rows if x[0] == "s2.fa"]
    assert all(int(x[3]) <= int(x[2]) <= int(x[4]) for x in rows)
    # the same bytes however the rows are blocked and formatted
    for out, flags in (("b1.tsv", ["--block-rows", "1"]), ("t2.tsv", ["-t", "2"]), ("b3.tsv", ["--block-rows", "3", "-t", "2"])):
        r = col.screen(out, flags)
        assert r.returncode == 0 and col.text(out) == want, (flags, r.stderr)


def test_keep_losers_is_a_superset_in_the_same_order(col):
    want, _ = col.model()
    kept, named = col.model(keep_losers=True)
    r = col.screen("kept.tsv", ["--keep-losers"])
    assert r.returncode == 0 and col.text("kept.tsv") == kept, r.stderr
    all_rows, rows = _rows(kept), _rows(want)
    assert len(all_rows) == sum(len(v) for v in named.values()) > len(rows)
    it = iter(all_rows)
    assert all(any(x == y for y in it) for x in rows)                       # a subsequence: the same rows in the same order
    losers = [x for x in all_rows if x not in rows]
    assert any(int(x[3]) == 0 < int(x[2]) for x in losers) and all(x[6] == "1.000000" or float(x[6]) > float(x[5]) for x in losers)


def test_max_dist_narrows_the_candidates_and_the_rows(col):
    wide, wide_named = col.model(keep_losers=True)
    want, named = col.model(max_dist=0.02, keep_losers=True)
    r = col.screen("d02.tsv", ["--max-dist", "0.02", "--keep-losers"])
    assert r.returncode == 0 and col.text("d02.tsv") == want, r.stderr
    assert "r%d.fa" % FAR in wide_named["s0.fa"] and "r%d.fa" % FAR not in named["s0.fa"] and "r%d.fa" % NEAR in named["s0.fa"]
    assert all(set(named[k]) <= set(wide_named[k]) for k in named) and sum(map(len, named.values())) < sum(map(len, wide_named.values()))
    want, _ = col.model(max_dist=0.02)
    r = col.screen("d02w.tsv", ["--max-dist=0.02"])
    assert r.returncode == 0 and col.text("d02w.tsv") == want, r.stderr
    assert all(float(x[5]) <= 0.02 and float(x[6]) <= 0.02 for x in _rows(want)) and len(_rows(want)) < len(_rows(col.text("d02.tsv")))
    r = col.screen("d0.tsv", ["--max-dist", "0", "-m", "0"])
    assert r.returncode == 0 and col.text("d0.tsv") == col.model(max_dist=0.0, model=0)[0], r.stderr


def test_file_order_reorders_the_queries(col):
    assert H.name_order(col.qnames) != list(range(len(col.qnames)))            # the key order of these names is not their list order
    want, _ = col.model(file_order=True, keep_losers=True)
    r = col.screen("fo.tsv", ["--file-order", "--keep-losers"])
    assert r.returncode == 0 and col.text("fo.tsv") == want, r.stderr
    key, _ = col.model(keep_losers=True)
    assert want != key
    assert [x[0] for x in _rows(want)] == sorted(x[0] for x in _rows(want))


def test_an_hll_collection_is_refused(col):
    col.sketch("L", col.rnames[:3], ["-a", "hll", "-p", "10"])
    for args in (["-r", "L", "-q", "L"], ["-r", "L", "-q", "SM"], ["-r", "DB", "-q", "L"]):
        r = _run(col.tmp_path, ["screen"] + args + ["-o", "refused.tsv"])
        assert r.returncode == 1 and not (col.tmp_path / "refused.tsv").exists(), r.stderr
    r = _run(col.tmp_path, ["screen", "-r", "L", "-q", "L", "-o", "refused.tsv"])
    assert "hll" in r.stderr and "HyperMinHash" in r.stderr, r.stderr
