"""`lash dist --derep D` (lash_sketch_set_pair_block_derep: pair statistics, expected collisions, a mark and a trim kernel on the GPU,
rep[] in HBM, what is left walked exactly on the host).  The contract: names in row order; a name is a representative iff no
representative before it is within D (the run `--max-dist D` with the same other flags prints their pair), else a member of the FIRST
such representative.  The yardstick for every case is the same build's `--max-dist D` output (held against the unfiltered run by
test_gpu_dist_within.py), and for the ABI a dense numpy distance matrix from dist_rows, put through a greedy walk in a few lines of
Python; compared byte for byte."""
import math
import os
import subprocess

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O

pytestmark = pytest.mark.gpu
HEADER = "Representative\tMember\n"
RATES = (0.0, 0.002, 0.01, 0.03, 0.08)
FLAG_SETS = {"m1": [], "m0": ["-m", "0"], "fp32": ["--fp32"]}


# ---- generators (copies: nothing here is imported from another test file) ---------------------------------------------------------------

def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _family(seed, length, rates=RATES):
    base = O.synth_genome(seed, length)
    return [base if r == 0 else _mutated(base, r, seed * 100 + i) for i, r in enumerate(rates)]


def _chain(seed, length, rate=0.04):
    """a - b - c with b mutated from a and c from b: a-c is about twice as far as a-b and b-c"""
    a = O.synth_genome(seed, length)
    b = _mutated(a, rate, seed * 7 + 1)
    c = _mutated(b, rate, seed * 7 + 2)
    return a, b, c


def _big_family(seed, length, members=40, max_rate=0.01):
    base = O.synth_genome(seed, length)
    rng = np.random.default_rng(seed)
    return [base] + [_mutated(base, float(rng.uniform(0.0, max_rate)), seed * 1000 + m) for m in range(members - 1)]


def _collection(seed, length, big=40):
    """In list order: a chain a, b, c far apart (a first: in list order b joins a, and c, within D of b only, stands alone), families
    at the five rates, a dense family of `big` near-identical members, singletons"""
    a, b, c = _chain(seed, length)
    return ([a] + _family(seed + 1, length) + [O.synth_genome(seed + 2, length)] + [b] + _big_family(seed + 3, length, big)
            + _family(seed + 4, length, rates=RATES[:3]) + [O.synth_genome(seed + 5, length), c])


def _write(tmp_path, stem, genomes):
    paths = []
    for i, g in enumerate(genomes):
        f = tmp_path / ("%s%d.fa" % (stem, i))
        f.write_bytes(b">s\n" + g.tobytes() + b"\n")
        paths.append(str(f))
    return paths


def _run(tmp_path, args, env=None):
    return subprocess.run([H.CLI] + args, cwd=tmp_path, capture_output=True, text=True, env=env or dict(os.environ), timeout=600)


def _sketch(tmp_path, prefix, paths, sk_args, env=None):
    (tmp_path / (prefix + ".txt")).write_text("\n".join(paths) + "\n")
    r = _run(tmp_path, ["sketch", "-f", prefix + ".txt", "-o", prefix] + sk_args, env)
    assert r.returncode == 0, r.stderr


def _bias_file(tmp_path, p):
    m = float(1 << p)
    rng = np.random.default_rng(8)
    raw = np.sort(rng.uniform(0.7 * m, 5.0 * m, 200))
    bias = 0.6 * m * np.exp(-(raw - 0.7 * m) / m)
    with open(tmp_path / "bias.txt", "w") as f:
        f.write("# synthetic\np %d %d\n" % (p, len(raw)) + "".join("%r %r\n" % (float(a), float(b)) for a, b in zip(raw, bias)))


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------

def _greedy(n, near):
    """near[i]: the columns j < i within D of i.  rep[i] = the first representative among them in row order, else i."""
    rep = []
    for i in range(n):
        rep.append(next((j for j in sorted(near[i]) if rep[j] == j), i))
    return rep


def _components(n, near):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(n):
        for j in near[i]:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


def _row_names(full_text):
    """names in the order of their first appearance as a row of the unfiltered run"""
    pos, names = {}, []
    for ln in full_text.split("\n")[1:-1]:
        ref = ln.split("\t", 1)[0]
        if ref not in pos:
            pos[ref] = len(names)
            names.append(ref)
    return names, pos


def _near(pos, cut_text):
    near = [set() for _ in pos]
    for ln in cut_text.split("\n")[1:-1]:
        ref, qry, _ = ln.split("\t")
        if ref != qry:                                                   # a name's own pair plays no part
            i, j = pos[ref], pos[qry]
            near[max(i, j)].add(min(i, j))
    return near


def _text(names, rep):
    order = sorted(range(len(names)), key=lambda i: (rep[i], i))
    return HEADER + "".join("%s\t%s\n" % (names[rep[i]], names[i]) for i in order)


def _timing(stderr):
    """the LASH_CLI_TIMING line of --derep -> (pairs, pruned_not_rep, pruned_after_hit, sent, evaluated, representatives)"""
    for ln in stderr.split("\n"):
        if "--derep:" in ln:
            return [int(w) for w in ln.replace(",", " ").split() if w.isdigit()]
    raise AssertionError("no --derep timing line in: " + stderr[-500:])


class _Set:
    """one sketched collection in a directory of its own, with the unfiltered runs it has needed so far"""

    def __init__(self, tmp, genomes, sk_args, dist_args=(), env=None, paths=None):
        self.tmp, self.dist_args, self.full = tmp, list(dist_args), {}
        self.env = dict(env or os.environ, LASH_CLI_TIMING="1")
        self.paths = paths or _write(tmp, "x", genomes)                  # (paths: genomes written before, in list order)
        self.n = len(self.paths)
        self.chain = None                                                # list places of a chain a, b, c, when the maker knows them
        _sketch(tmp, "X", self.paths, sk_args, self.env)

    def list_names(self):
        """the names in list order, which is the row order under --file-order: what `lash sketch` wrote beside the sketches"""
        import json
        names = json.loads((self.tmp / "X_files.json").read_text())
        assert len(names) == self.n == len(set(names))
        return names

    def dist(self, out, args):
        return _run(self.tmp, ["dist", "-q", "X", "-r", "X", "-o", out] + self.dist_args + args, self.env)

    def full_text(self, flags):
        """the unfiltered run with the flags that change rows or distances"""
        key = tuple(f for f in flags if f in ("--file-order", "--fp32", "-m", "0"))
        if key not in self.full:
            r = self.dist("full.tsv", list(key))
            assert r.returncode == 0, r.stderr
            self.full[key] = (self.tmp / "full.tsv").read_text()
        return self.full[key]

    def want(self, D, flags, names=None):
        """(text, rep, near, names) the greedy walk over the rows `--max-dist D` prints with the same flags; names: the row order, when
        the caller knows it without the unfiltered run"""
        if names is None:
            names = _row_names(self.full_text(flags))[0]
        pos = {name: i for i, name in enumerate(names)}
        assert len(names) == self.n
        r = self.dist("cut.tsv", ["--max-dist", repr(D)] + flags)
        assert r.returncode == 0, (D, flags, r.stderr)
        near = _near(pos, (self.tmp / "cut.tsv").read_text())
        rep = _greedy(self.n, near)
        return _text(names, rep), rep, near, names

    def got(self, D, flags):
        r = self.dist("rep.tsv", ["--derep", repr(D)] + flags)
        assert r.returncode == 0, (D, flags, r.stderr)
        return (self.tmp / "rep.tsv").read_text(), _timing(r.stderr)

    def check(self, D, flags, names=None):
        want, rep, near, names = self.want(D, flags, names)
        got, (pairs, not_rep, after_hit, sent, evaluated, reps) = self.got(D, flags)
        assert got == want, (D, flags)
        assert got.count("\n") == self.n + 1
        assert pairs == self.n * (self.n - 1) // 2 and reps == sum(rep[i] == i for i in range(self.n))
        assert evaluated <= sent and not_rep + sent <= pairs
        if D < 0:
            assert reps == self.n
        return got, rep, near

    def a_printed_distance(self, flags):
        """a distance of the set's own, as printed: the middle one of those in (0.005, 0.3)"""
        vals = sorted(float(ln.rsplit("\t", 1)[1]) for ln in self.full_text(flags).split("\n")[1:-1])
        vals = [v for v in vals if 0.005 < v < 0.3]
        assert len(vals) > 10
        return vals[len(vals) // 2]


def _hmh(tmp):
    """12 kbp (2-20 kbp: both sketches <= 2^19 distinct k-mers, the expected-collision term from the GEMM) and a few of 600-700 kbp (the
    closed form), mixed"""
    a, b, c = _chain(200, 650_000)
    large = [a] + _family(201, 600_000) + [b, c]
    small = _collection(100, 12_000)
    s = _Set(tmp, small[:30] + large + small[30:], ["-k", "16"])
    s.chain = (0, 7, s.n - 1)
    return s


def _hll10(tmp):
    s = _Set(tmp, _collection(300, 300_000), ["-k", "21", "-a", "hll", "-p", "10"])
    s.chain = (0, 7, s.n - 1)
    return s


def _hll14(tmp):
    """p = 14 on small genomes: sketches and unions in the HLL++ bias-table regime, which only the host evaluates (synthetic tables)"""
    _bias_file(tmp, 14)
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    s = _Set(tmp, _collection(400, 20_000) + [O.synth_genome(409, 300_000)], ["-k", "21", "-a", "hll", "-p", "14"], ["--hll-bias", "bias.txt"], env)
    s.chain = (0, 7, s.n - 2)
    return s


def _ull(est):
    def make(tmp):
        # two genomes shorter than k have empty sketches: NaN against each other under -m 0 (never within D), 1 under -m 1
        tiny = [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]
        genomes = _collection(500, 200_000)
        s = _Set(tmp, genomes[:20] + tiny[:1] + genomes[20:] + tiny[1:], ["-k", "16", "-a", "ull", "-p", "12"], ["-e", est])
        s.chain = (0, 7, s.n - 2)
        return s
    return make


MAKERS = {"hmh": _hmh, "hll10": _hll10, "hll14": _hll14, "ull-fgra": _ull("fgra"), "ull-ml": _ull("ml")}
_sets = {}


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    def get(algo):
        if algo not in _sets:
            _sets[algo] = MAKERS[algo](tmp_path_factory.mktemp(algo.replace("-", "_")))
        return _sets[algo]
    yield get
    _sets.clear()


# ---- command line -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag_set", list(FLAG_SETS))
@pytest.mark.parametrize("algo", list(MAKERS))
def test_cli_cutoffs(sets, algo, flag_set):
    """cutoffs from the set's own distances (one as printed, the double just below it), 0, 1 and a negative one, in both row orders"""
    s, flags = sets(algo), FLAG_SETS[flag_set]
    if algo.startswith("ull") and flag_set == "m0":
        assert "NaN" in s.full_text(flags)                               # (the plain run: the NaN pair is really there)
    v = s.a_printed_distance(flags)
    for D in (v, math.nextafter(v, -math.inf), 0.0, 1.0, -0.25):
        s.check(D, flags)
    s.check(v, flags + ["--file-order"])


def _chain_cutoff(s):
    """a D between the chain's two links and its ends, from the unfiltered run in list order: d(a, b), d(b, c) <= D < d(a, c)"""
    ia, ib, ic = s.chain
    names, pos = _row_names(s.full_text(["--file-order"]))
    d = {}
    for ln in s.full_text(["--file-order"]).split("\n")[1:-1]:
        ref, qry, v = ln.split("\t")
        if (pos[ref], pos[qry]) in ((ib, ia), (ic, ib), (ic, ia)):
            d[pos[ref], pos[qry]] = float(v)
    links, ends = max(d[ib, ia], d[ic, ib]), d[ic, ia]
    assert links + 2e-3 < ends, d                                        # (the generator: a - c is about twice as far)
    return (links + ends) / 2


@pytest.mark.parametrize("algo", list(MAKERS))
def test_cli_run_shapes_and_the_chain(sets, algo):
    """--block-rows 1, 7, 37, N and the default, -t 1 and -t 4: one output.  In list order the chain a - b - c (a first) gives b to a and
    leaves c alone, where single linkage has one cluster: the result is not the connected components."""
    s = sets(algo)
    D = _chain_cutoff(s)
    want, rep, near = s.check(D, [])
    for shape in (["--block-rows", "1"], ["--block-rows", "7"], ["--block-rows", "37"], ["--block-rows", str(s.n)], ["-t", "1"], ["-t", "4"],
                  ["--block-rows", "7", "-t", "4"]):
        got, counts = s.got(D, shape)
        assert got == want, shape
        if shape == ["--block-rows", "7"]:
            # the dense family: members of earlier blocks pruned; rows trimmed after their sure hit (hll14: every small pair is
            # in the bias-table regime, which the device cannot place, so no hit is sure there)
            assert counts[1] > 0 and (counts[2] > 0 or algo == "hll14")
    want, rep, near = s.check(D, ["--file-order"])
    got, counts = s.got(D, ["--file-order", "--block-rows", "7"])
    assert got == want
    ia, ib, ic = s.chain
    comp = _components(s.n, near)
    assert ia in near[ib] and ib in near[ic] and ia not in near[ic]
    assert rep[ia] == ia and rep[ib] == ia and rep[ic] == ic and comp[ia] == comp[ib] == comp[ic]   # not the connected components
    sizes = {}
    for r in rep:
        sizes[r] = sizes.get(r, 0) + 1
    assert max(sizes.values()) >= 40                                     # the dense family: one representative and its members


def test_cli_rows_of_more_than_one_tile(tmp_path):
    """1 130 tiny genomes in list order: a row spans more than one 1 024-column tile.  X at place 5; Y (place 1030) is a
    representative two steps from X; the Z (the last 60 rows) lie between the two, within D of both: their sure hit X is in tile 0 and Y's bit
    in tile 1, with the in-block Z before them, is what the trim has to clear."""
    x = O.synth_genome(9100, 4_000)
    mid = _mutated(x, 0.03, 91999)
    zs = [_mutated(mid, 0.004, 91000 + i) for i in range(60)]
    y = _mutated(mid, 0.03, 92000)
    genomes = [O.synth_genome(9200 + i, 4_000) for i in range(1130)]
    for f in range(40):                                                  # small families among the singletons
        for m in range(1, 4):
            genomes[100 + f * 20 + m * 3] = _mutated(genomes[100 + f * 20], 0.01 * m, 93000 + f * 10 + m)
    genomes[5], genomes[1030] = x, y
    genomes[1070:] = zs
    s = _Set(tmp_path, genomes, ["-k", "16"])
    order = ["--file-order"]
    names = s.list_names()
    pos = {name: i for i, name in enumerate(names)}
    r = s.dist("cut.tsv", ["--max-dist", "0.2"] + order)                 # (the distances the layout is about, without 638 000 rows)
    assert r.returncode == 0, r.stderr
    d = {}
    for ln in (tmp_path / "cut.tsv").read_text().split("\n")[1:-1]:
        ref, qry, v = ln.split("\t")
        if pos[ref] >= 1070 and pos[qry] in (5, 1030) or (pos[ref], pos[qry]) == (1030, 5):
            d[pos[ref], pos[qry]] = float(v)
    assert len(d) == 121, len(d)
    D = (max(v for (i, j), v in d.items() if i >= 1070) + d[1030, 5]) / 2
    assert max(v for (i, j), v in d.items() if i >= 1070) < D - 1e-3 and d[1030, 5] > D + 1e-3, d   # the layout the docstring says
    want, rep, near = s.check(D, order, names)
    assert rep[1030] == 1030 and all(rep[i] == 5 and 1030 in near[i] for i in range(1070, 1130))
    for shape in (["--block-rows", "37"], ["--block-rows", "1130"]):
        got, counts = s.got(D, order + shape)
        assert got == want, shape
        if shape[1] == "37":
            assert counts[2] >= 60                                       # at least Y's bit of every Z row


def _hll14_without_tables(tmp_path, genomes):
    env = dict(os.environ, LASH_CLI_TIMING="1")
    env.pop("LASH_HLL_BIAS", None)
    return _Set(tmp_path, genomes, ["-k", "21", "-a", "hll", "-p", "14"], ["--file-order"], env)


def test_cli_refused_like_max_dist(tmp_path):
    """hll p = 14 without tables: two unrelated ~9 kbp genomes are each in linear counting, their union is in the bias-table regime.
    They are rows 0 and 1, so the first off-diagonal pair is the one both runs are refused on, whatever D is."""
    a = O.synth_genome(55, 9_000)
    s = _hll14_without_tables(tmp_path, [a, O.synth_genome(56, 8_000), _mutated(a, 0.001, 5)])
    for D in (0.3, -1.0):
        for shape in ([], ["--block-rows", "1"]):
            want = s.dist("cut.tsv", ["--max-dist", repr(D)] + shape)
            assert want.returncode != 0 and "bias tables" in want.stderr and "union of" in want.stderr
            got = s.dist("rep.tsv", ["--derep", repr(D)] + shape)
            assert got.returncode == want.returncode
            err = [ln for ln in want.stderr.split("\n") if "union of" in ln]
            assert err and err == [ln for ln in got.stderr.split("\n") if "union of" in ln], (D, shape, got.stderr)


def test_cli_refused_pairs_beyond_the_first_hit_do_not_matter(tmp_path):
    """Row 0 is a 300 kbp genome: against it every later (9 kbp) genome's union is far above 5 * 2^14, which the device places, at d = 1.
    At D = 1 that pair is within D, so every row stops at column 0.  The pairs of two unrelated small genomes are in the bias-table
    regime (`--max-dist 1` is refused on the first of them), but they lie beyond each row's first hit: the walk of the contract never
    reaches them and the run succeeds.  At D = 0.01 row 0 is no hit, the walk of row 2 reaches (2, 1), and both runs are refused there."""
    a = O.synth_genome(55, 9_000)
    s = _hll14_without_tables(tmp_path, [O.synth_genome(57, 300_000), a, O.synth_genome(56, 8_000), _mutated(a, 0.001, 5), O.synth_genome(58, 7_000)])
    want = s.dist("cut.tsv", ["--max-dist", "1.0"])
    assert want.returncode != 0 and "union of" in want.stderr
    for shape in ([], ["--block-rows", "1"], ["--block-rows", "2"]):
        got = s.dist("rep.tsv", ["--derep", "1.0"] + shape)
        assert got.returncode == 0, got.stderr
        lines = (tmp_path / "rep.tsv").read_text().split("\n")[1:-1]
        assert len(lines) == 5 and len({ln.split("\t")[0] for ln in lines}) == 1 and lines[0].split("\t")[0] == lines[0].split("\t")[1]
        want5 = s.dist("cut.tsv", ["--max-dist", "0.01"] + shape)
        got5 = s.dist("rep.tsv", ["--derep", "0.01"] + shape)
        err = [ln for ln in want5.stderr.split("\n") if "union of" in ln]
        assert got5.returncode == want5.returncode != 0 and err and err == [ln for ln in got5.stderr.split("\n") if "union of" in ln]


def test_cli_rectangular_and_several_workers_are_refused(tmp_path):
    paths = _write(tmp_path, "x", _family(600, 12_000, rates=(0.0, 0.01, 0.05)))
    _sketch(tmp_path, "X", paths, ["-k", "16"])
    _sketch(tmp_path, "Y", paths[:2], ["-k", "16"])
    r = _run(tmp_path, ["dist", "-q", "Y", "-r", "X", "-o", "rep.tsv", "--derep", "0.05"])
    assert r.returncode != 0 and "--derep" in r.stderr and "same sketch files" in r.stderr
    out = tmp_path / "rep.tsv"
    assert not out.exists() or out.read_text().count("\n") <= 1
    r = _run(tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "rep2.tsv", "--derep", "0.05", "--devices", "0,0"])
    assert r.returncode == 2 and "--devices" in r.stderr and "row order" in r.stderr and not (tmp_path / "rep2.tsv").exists()
    r = _run(tmp_path, ["dist", "-q", "X", "-r", "X", "-o", "rep3.tsv", "--derep", "0.05", "--devices", "0"])
    assert r.returncode == 0 and (tmp_path / "rep3.tsv").read_text().count("\n") == 4


def test_cli_randomized_against_the_yardstick(tmp_path_factory):
    """a short fixed-seed run over random N, algorithm, D, --block-rows and flags"""
    rng = np.random.default_rng(20250311)
    algos = {"hmh": (4_000, ["-k", "16"], []), "ull": (20_000, ["-k", "16", "-a", "ull", "-p", "12"], ["-e", "ml"]),
             "hll": (20_000, ["-k", "21", "-a", "hll", "-p", "10"], [])}
    pools = {}
    for it in range(6):
        algo = str(rng.choice(list(algos)))
        length, sk_args, dist_args = algos[algo]
        if algo not in pools:                                            # 300 genomes: families of 1 to 30 at a random spread
            pool = []
            while len(pool) < 300:
                base = O.synth_genome(7000 + len(pool), length)
                top = float(rng.choice([0.005, 0.02, 0.06, 0.12]))
                pool += [base] + [_mutated(base, float(rng.uniform(0.0, top)), 70000 + len(pool) * 40 + m) for m in range(int(rng.integers(0, 30)))]
            pools[algo] = _write(tmp_path_factory.mktemp("pool_" + algo), "g", pool[:300])
        n = int(rng.choice([2, 3, int(rng.integers(4, 65)), int(rng.integers(65, 301))]))
        pick = rng.permutation(300)[:n]
        s = _Set(tmp_path_factory.mktemp("rnd%d" % it), None, sk_args, dist_args, paths=[pools[algo][i] for i in pick])
        D = float(rng.choice([float(rng.uniform(0.0, 0.15)), float(rng.uniform(0.0, 1.0))]))
        flags = ["--block-rows", str(int(rng.integers(1, 80)))] + (["--file-order"] if rng.random() < 0.5 else []) \
            + (["--fp32"] if rng.random() < 0.3 else []) + (["-m", "0"] if rng.random() < 0.3 else []) + ["-t", str(int(rng.integers(1, 5)))]
        s.check(D, flags)


# ---- ABI level: SketchSet.pair_block_derep / derep against pair_block + dist_rows --------------------------------------------------------

def _sketches(algo, k, p, genomes):
    import lash_amd
    ctx = lash_amd.Context(0)
    seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in genomes])
    return ctx, ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff)


def _dense(s, card, algo, p, k, model, fp32, est="fgra", bias=None):
    """the whole triangle's exact distances; +inf above the diagonal"""
    from lash_amd.sketch import dist_rows
    n = s.n
    st = s.pair_block(0, n, n_cols=n, triangle=True, estimator=est)
    if algo == "hmh":
        ec = s.hmh_expected_collisions(0, n, n_cols=n)
        if ec is not None:
            st["hmh_ec"] = ec
    above = np.arange(n)[None, :] > np.arange(n)[:, None]                # undefined there: neutral statistics
    for key, v in st.items():
        st[key] = np.where(above, 0 if v.dtype != np.float64 else 1e-300, v).astype(v.dtype)
    d = dist_rows(algo, p, k, model, card, card, fp32=fp32, hll_bias=bias, **st)
    d[above] = np.inf
    return d


def _rep_from_dense(d, D):
    n = d.shape[0]
    return np.array(_greedy(n, [np.nonzero(d[i, :i] <= D)[0].tolist() for i in range(n)]), np.uint32)


def _blocks(n, step, start=0):
    edges = [0] + list(range(start or step, n, step)) + [n]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _run_blocks(s, blocks, D, k, acc, **kw):
    total = dict(pairs=0, pruned_not_rep=0, pruned_after_hit=0, sent_to_host=0, evaluated=0)
    for r0, r1 in blocks:
        st = {}
        s.pair_block_derep(r0, r1, D, k, acc, stats=st, **kw)
        for key in total:
            total[key] += st[key]
        total["representatives"] = st["representatives"]
    return total


def _sent_bound(d, rep, blocks, D, margin):
    """How many pairs the device may hand to the host, from the exact distances.  The device knows rep[] of the columns of earlier blocks
    (q < r0) and nothing of its own block's: in-block columns are decided by the host walk of the same call, so each of them counts
    whether it turns out a representative or not; a column of an earlier block counts only if it is a representative.
      a row with a sure hit in an earlier block (a representative q < r0 with d <= D - margin; f = the first): 1 + the counting columns
        before f within margin of D;
      any other row: the counting columns with d <= D + margin.
    (hmh with finite cardinalities: there is no pair the device cannot place.)"""
    bound = 0
    for r0, r1 in blocks:
        earlier = np.nonzero(rep[:r0] == np.arange(r0))[0]
        for i in range(r0, r1):
            sure = earlier[d[i, earlier] <= D - margin]
            if len(sure):
                before = earlier[earlier < sure[0]]
                bound += 1 + int(np.count_nonzero(np.abs(d[i, before] - D) <= margin))
            else:
                bound += int(np.count_nonzero(d[i, earlier] <= D + margin)) + int(np.count_nonzero(d[i, r0:i] <= D + margin))
    return bound


@pytest.fixture(scope="module")
def hmh_derep_set():
    # 330 sketches in a fixed shuffled order: families, a dense family of 40, a chain, a few large genomes
    import lash_amd
    genomes = []
    rng = np.random.default_rng(5)
    for f in range(25):
        base = O.synth_genome(8000 + f, 12_000)
        genomes += [base] + [_mutated(base, float(rng.uniform(0.0, 0.25)), 80000 + f * 10 + m) for m in range(9)]
    genomes += _big_family(8200, 12_000, 40) + list(_chain(8300, 20_000)) + _family(8400, 600_000, rates=(0.0, 0.01, 0.04))
    genomes += [O.synth_genome(8500 + i, 8_000) for i in range(34)]
    perm = np.random.default_rng(6).permutation(len(genomes))
    ctx, imgs = _sketches("hmh", 16, 0, [genomes[i] for i in perm])
    s = ctx.sketch_set("hmh", 0, imgs)
    card = s.cardinalities()
    s.prepare()
    family = np.sort(np.argsort(perm)[250:290])                         # where the 40-member family went
    yield ctx, s, card, family, lash_amd
    s.free()
    ctx.close()


@pytest.mark.parametrize("model,fp32", [(1, False), (0, True)])
def test_abi_derep_equals_the_greedy_walk(hmh_derep_set, model, fp32):
    ctx, s, card, family, lash_amd = hmh_derep_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, model, fp32)
    kw = dict(model=model, fp32=fp32)
    # D = a pair's exact distance is within; one ulp below is not.  A pair on which the walk turns: the first of a few where it does
    vals = d[np.isfinite(d) & (d > 0.01) & (d < 0.5)]
    edge = next(float(v) for v in vals[:: max(1, len(vals) // 60)]
                if not np.array_equal(_rep_from_dense(d, float(v)), _rep_from_dense(d, math.nextafter(float(v), -math.inf))))
    for D in (0.0, 0.02, 0.05, 0.25, 1.0, -0.25, edge, math.nextafter(edge, -math.inf)):
        want = _rep_from_dense(d, D)
        for step in (n, 64, 7):
            assert np.array_equal(s.derep(D, 16, block_rows=step, **kw), want), (D, step)
        acc = lash_amd.Derep(ctx, n)
        blocks = _blocks(n, 100, start=37)                               # unaligned blocks
        tot = _run_blocks(s, blocks, D, 16, acc, **kw)
        assert np.array_equal(acc.result(), want), D
        acc.free()
        assert tot["pairs"] == n * (n - 1) // 2 and tot["representatives"] == int(np.count_nonzero(want == np.arange(n)))
        assert tot["evaluated"] <= tot["sent_to_host"] <= _sent_bound(d, want, blocks, D, 2.0 ** -16 if fp32 else 2.0 ** -40), (D, tot)
    assert not np.array_equal(_rep_from_dense(d, edge), _rep_from_dense(d, math.nextafter(edge, -math.inf)))


def test_abi_blocks_out_of_order_and_an_early_result(hmh_derep_set):
    ctx, s, card, family, lash_amd = hmh_derep_set
    n = s.n
    acc = lash_amd.Derep(ctx, n)

    def refused(*a, **kw):
        with pytest.raises(lash_amd.LashError) as e:
            s.pair_block_derep(*a, **kw)
        assert e.value.code == -1

    refused(5, 10, 0.05, 16, acc)                                        # not from 0
    s.pair_block_derep(0, 5, 0.05, 16, acc)
    refused(6, 10, 0.05, 16, acc)                                        # a gap
    refused(0, 5, 0.05, 16, acc)                                         # again
    refused(5, 10, float("nan"), 16, acc)
    refused(5, n + 1, 0.05, 16, acc, n_cols=n)                           # beyond n
    with pytest.raises(lash_amd.LashError) as e:
        acc.result()                                                     # rows 5 .. n are undecided
    assert e.value.code == -1
    s.pair_block_derep(5, n, 0.05, 16, acc)                              # the refused calls changed nothing
    d = _dense(s, card, "hmh", 0, 16, 1, False)
    assert np.array_equal(acc.result(), _rep_from_dense(d, 0.05))
    refused(n, n, 0.05, 16, lash_amd.Derep(ctx, n))                      # an empty block is still out of order
    acc.free()


def test_abi_a_dense_family_is_pruned_and_trimmed(hmh_derep_set):
    ctx, s, card, family, lash_amd = hmh_derep_set
    n = s.n
    D, margin = 0.05, 2.0 ** -40
    d = _dense(s, card, "hmh", 0, 16, 1, False)
    sub = d[np.ix_(family, family)]
    assert np.nanmax(np.tril(sub, -1)) < D                               # every pair of the family is within D
    want = _rep_from_dense(d, D)
    assert len(set(want[family].tolist())) == 1
    for step in (16, 1):                                                 # (1: no in-block columns, only representatives ever count)
        blocks = _blocks(n, step)
        acc = lash_amd.Derep(ctx, n)
        tot = _run_blocks(s, blocks, D, 16, acc)
        assert np.array_equal(acc.result(), want)
        acc.free()
        print("dense family, blocks of", step, tot, "bound", _sent_bound(d, want, blocks, D, margin))
        assert tot["sent_to_host"] <= _sent_bound(d, want, blocks, D, margin)
        assert tot["pruned_not_rep"] > 0 and tot["pruned_after_hit"] > 0
        assert tot["evaluated"] <= tot["sent_to_host"]
        assert tot["representatives"] == int(np.count_nonzero(want == np.arange(n)))
