"""`lash dist --cluster D` (lash_sketch_set_pair_block_cluster: pair statistics, expected collisions and a mark-and-join kernel on the
GPU, a label array in HBM, undecided pairs evaluated exactly on the host).  The contract: two names are linked iff the run
`--max-dist D` with the same other flags prints their pair; clusters are the connected components; the output is one line per name
under its cluster's first name in row order.  The yardstick for every case is the same build's `--max-dist D` output (held against the
unfiltered run by test_gpu_dist_within.py) put through a plain Python union-find, compared byte for byte."""
import math
import os

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
from test_gpu_dist_within import _bias_file, _dense, _family, _mutated, _run, _sketch, _sketches, _write

pytestmark = pytest.mark.gpu
D_VALUES = (0.0, 0.01, 0.05, 0.2, 1.0, -0.25)
HEADER = "Representative\tMember\n"


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------

def _components(n, edges):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


def _render(full_text, cut_text):
    """names in the order of their first appearance as a row of the unfiltered run; links = the --max-dist rows of two different names"""
    pos, names = {}, []
    for ln in full_text.split("\n")[1:-1]:
        ref = ln.split("\t", 1)[0]
        if ref not in pos:
            pos[ref] = len(names)
            names.append(ref)
    edges = []
    for ln in cut_text.split("\n")[1:-1]:
        ref, qry, _ = ln.split("\t")
        if ref != qry:
            edges.append((pos[ref], pos[qry]))
    lab = _components(len(names), edges)
    order = sorted(range(len(names)), key=lambda i: (lab[i], i))
    return HEADER + "".join("%s\t%s\n" % (names[lab[i]], names[i]) for i in order), lab, edges


def _timing(stderr):
    """the LASH_CLI_TIMING line of --cluster -> (pairs, pruned, joined, sent, clusters)"""
    for ln in stderr.split("\n"):
        if "--cluster:" in ln:
            return [int(w) for w in ln.replace(",", " ").split() if w.isdigit()]
    raise AssertionError("no --cluster timing line in: " + stderr[-500:])


def _close_rows(full_text, D, fp32, nan_too):
    """How many pairs the device may hand to the host, from the unfiltered run with the same distance flags.  The device's d is within
    one margin of the host's and a pair is undecided only within one margin of D, so a returned pair has |d_host - D| <= 2 x margin;
    the text has 6 decimals, hence + 5e-7.  NaN counts only where the design sends it back (hll).  The ABI hands back no pairs, only
    their number: every pair outside this band has to be decided on the device for the number to stay within the count, and for the
    cutoffs used here the band is empty or a handful of rows, so the count is as strict as looking at each pair."""
    tol = 2 * (2.0 ** -16 if fp32 else 2.0 ** -40) + 5e-7
    n = 0
    for ln in full_text.split("\n")[1:-1]:
        ref, qry, v = ln.split("\t")
        v = float(v)
        if ref != qry and (abs(v - D) <= tol or (nan_too and v != v)):
            n += 1
    return n


def _cli_case(tmp_path, prefix, D, flags, env=None, full_cache=None, algo="hmh", sent_bound=True):
    """one --cluster run against the yardstick with the same flags; returns (labels, edges, timing counts).  sent_bound=False: the
    set has pairs the device cannot place (hll bias-table regime), whose number the text does not show."""
    env = dict(env or os.environ, LASH_CLI_TIMING="1")
    dist_flags = [f for f in flags if f in ("--file-order", "--fp32")] + (["-m", "0"] if "-m" in flags else [])
    order_key = tuple(dist_flags)
    if full_cache is None or order_key not in full_cache:
        r = _run(tmp_path, ["dist", "-q", prefix, "-r", prefix, "-o", "full.tsv"] + dist_flags + _passthrough(flags), env)
        assert r.returncode == 0, r.stderr
        text = (tmp_path / "full.tsv").read_text()
        if full_cache is not None:
            full_cache[order_key] = text
    else:
        text = full_cache[order_key]
    r = _run(tmp_path, ["dist", "-q", prefix, "-r", prefix, "-o", "cut.tsv", "--max-dist", repr(D)] + flags, env)
    assert r.returncode == 0, (D, flags, r.stderr)
    want, lab, edges = _render(text, (tmp_path / "cut.tsv").read_text())
    r = _run(tmp_path, ["dist", "-q", prefix, "-r", prefix, "-o", "clu.tsv", "--cluster", repr(D)] + flags, env)
    assert r.returncode == 0, (D, flags, r.stderr)
    got = (tmp_path / "clu.tsv").read_text()
    assert got == want, (D, flags)
    n = len(lab)
    assert got.count("\n") == n + 1
    pairs, pruned, joined, sent, clusters = _timing(r.stderr)
    assert pairs == n * (n - 1) // 2 and clusters == len(set(lab))
    assert joined <= (n - 1) * 3                                         # at most n - 1 per worker (up to three workers here)
    assert pruned + joined + sent <= pairs
    if sent_bound:
        assert sent <= _close_rows(text, D, "--fp32" in flags, algo == "hll"), (D, flags, sent)
    if D < 0:
        assert clusters == n and all(ln.split("\t")[0] == ln.split("\t")[1] for ln in got.split("\n")[1:-1])
    return lab, edges, (pairs, pruned, joined, sent, clusters)


def _passthrough(flags):
    """the flags that change names or bias tables in the unfiltered run (distances are not read from it, only the row order)"""
    out = []
    for i, f in enumerate(flags):
        if f in ("--hll-bias", "-e"):
            out += [f, flags[i + 1]]
    return out


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


def _collection(seed, length, big=40, fam_rates=(0.0, 0.002, 0.01, 0.03, 0.08)):
    """a chain whose three members sit far apart in list order (their links are found in different blocks), families, a large close
    family, singletons"""
    a, b, c = _chain(seed, length)
    return ([a] + _family(seed + 1, length, rates=fam_rates) + [O.synth_genome(seed + 2, length)] + [b] + _big_family(seed + 3, length, big)
            + _family(seed + 4, length, rates=fam_rates[:3]) + [O.synth_genome(seed + 5, length), c])


def _has_chain(lab, edges):
    """some cluster holds two names that are not linked themselves: single linkage is visible"""
    linked = {(min(a, b), max(a, b)) for a, b in edges}
    size = {}
    for l in lab:
        size[l] = size.get(l, 0) + 1
    inside = {}
    for a, b in linked:
        inside[lab[a]] = inside.get(lab[a], 0) + 1
    return any(inside.get(l, 0) < s * (s - 1) // 2 for l, s in size.items() if s > 2)


VARIANTS = [["--block-rows", "1"], ["--block-rows", "7"], ["--devices", "0,0"], ["--devices", "0,0,0", "--block-rows", "5"], ["-t", "1"],
            ["--file-order"], ["--file-order", "--block-rows", "7", "--devices", "0,0"], ["-m", "0"], ["--fp32"],
            ["-m", "0", "--fp32", "--block-rows", "7"]]


def test_hmh_small_genomes_all_cutoffs_and_run_shapes(tmp_path):
    """60 kbp: both sketches <= 2^19 distinct k-mers, the expected-collision term from the GEMM; the 40-member family is mostly pruned"""
    genomes = _collection(100, 60_000)
    _sketch(tmp_path, "X", _write(tmp_path, "x", genomes), ["-k", "16"])
    cache = {}
    for D in D_VALUES:
        lab, edges, (pairs, pruned, joined, sent, clusters) = _cli_case(tmp_path, "X", D, [], full_cache=cache)
        if D == 0.05:
            assert _has_chain(lab, edges)
            assert 2 <= clusters <= len(lab) - 39                            # the 40-member family is one cluster
        if D >= 1:
            assert clusters == 1
    for flags in VARIANTS:
        lab, edges, (pairs, pruned, joined, sent, clusters) = _cli_case(tmp_path, "X", 0.05, flags, full_cache=cache)
        if flags == ["--block-rows", "7"]:
            # the family's later rows meet members that earlier blocks of the same worker have joined: no distance for those
            assert pruned > 0
        _cli_case(tmp_path, "X", 0.2, flags, full_cache=cache)


def test_hmh_large_and_mixed_genomes(tmp_path):
    """> 2^19 distinct 16-mers per genome (the closed-form expected collisions), alone and mixed with small genomes"""
    a, b, c = _chain(200, 700_000)
    large = [a] + _family(201, 650_000, rates=(0.0, 0.005, 0.03)) + [b, O.synth_genome(202, 600_000), c]
    _sketch(tmp_path, "L", _write(tmp_path, "l", large), ["-k", "16"])
    cache = {}
    for D in D_VALUES:
        lab, edges, _ = _cli_case(tmp_path, "L", D, [], full_cache=cache)
        if D == 0.05:
            assert _has_chain(lab, edges)
    _cli_case(tmp_path, "L", 0.05, ["--block-rows", "2", "--devices", "0,0"], full_cache=cache)
    mixed = large[:5] + _collection(210, 40_000, big=12) + large[5:]
    _sketch(tmp_path, "M", _write(tmp_path, "m", mixed), ["-k", "16"])
    cache = {}
    for D, flags in ((0.05, []), (0.2, ["--block-rows", "7"]), (0.05, ["--fp32", "-m", "0", "--file-order"])):
        _cli_case(tmp_path, "M", D, flags, full_cache=cache)


def test_hll_p10_large(tmp_path):
    a, b, c = _chain(300, 500_000)
    genomes = [a] + _family(301, 500_000) + [b] + _big_family(302, 400_000, 12) + [O.synth_genome(303, 400_000), c]
    _sketch(tmp_path, "X", _write(tmp_path, "x", genomes), ["-k", "21", "-a", "hll", "-p", "10"])
    cache = {}
    for D in D_VALUES:
        _cli_case(tmp_path, "X", D, [], full_cache=cache, algo="hll")
    for flags in (["--block-rows", "1"], ["--block-rows", "7", "--devices", "0,0"], ["--fp32", "-m", "0"], ["--file-order"]):
        _cli_case(tmp_path, "X", 0.05, flags, full_cache=cache, algo="hll")


def test_hll_p14_small_with_and_without_tables(tmp_path):
    """p = 14 on small genomes: sketches and unions in the HLL++ bias-table regime, which only the host evaluates: never pruned.  Without
    tables the run fails with the text of the --max-dist run."""
    _bias_file(tmp_path, 14)
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    genomes = _collection(400, 40_000, big=10, fam_rates=(0.0, 0.01, 0.05)) + [O.synth_genome(409, 300_000)]
    sk = ["-k", "21", "-a", "hll", "-p", "14"]
    _sketch(tmp_path, "X", _write(tmp_path, "x", genomes), sk, env)
    cache = {}
    for D, flags in ((0.05, []), (0.2, ["--block-rows", "7"]), (1.0, ["--devices", "0,0"]), (0.0, []), (0.05, ["--fp32", "--file-order"])):
        _cli_case(tmp_path, "X", D, flags + ["--hll-bias", "bias.txt"], env, full_cache=cache, algo="hll", sent_bound=False)
    # without the tables: X fails on its sketches' own estimates; two ~9 kbp genomes are each in linear counting, their union is not
    paths = _write(tmp_path, "n", [O.synth_genome(55, 9_000), O.synth_genome(56, 8_000), _mutated(O.synth_genome(55, 9_000), 0.001, 5)])
    _sketch(tmp_path, "S", paths, sk, env)
    for prefix in ("X", "S"):
        for D in (0.0, 0.3, 1.0, -1.0):
            for flags in ([], ["--block-rows", "1"]):
                want = _run(tmp_path, ["dist", "-q", prefix, "-r", prefix, "-o", "cut.tsv", "--max-dist", repr(D)] + flags, env)
                assert want.returncode != 0 and "bias tables" in want.stderr
                got = _run(tmp_path, ["dist", "-q", prefix, "-r", prefix, "-o", "clu.tsv", "--cluster", repr(D)] + flags, env)
                assert (got.returncode, got.stderr) == (want.returncode, want.stderr), (prefix, D, flags)
    assert "union of" in want.stderr                                     # (S: a block's pair, not a sketch)


@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_ull_p12(tmp_path, est):
    """two genomes shorter than k have empty sketches: NaN against each other under -m 0 (never linked), 1 under -m 1"""
    a, b, c = _chain(500, 300_000)
    genomes = [a] + _family(501, 300_000, rates=(0.0, 0.005, 0.03, 0.1, 0.3)) + [b] + _big_family(502, 200_000, 12) + [O.synth_genome(503, 200_000), c]
    genomes += [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]
    _sketch(tmp_path, "X", _write(tmp_path, "x", genomes), ["-k", "16", "-a", "ull", "-p", "12"])
    cache = {}
    for D in D_VALUES:
        for flags in ([], ["-m", "0", "--block-rows", "7"]):
            _cli_case(tmp_path, "X", D, flags + ["-e", est], full_cache=cache, algo="ull")
    _cli_case(tmp_path, "X", 0.05, ["--fp32", "--devices", "0,0", "--block-rows", "1", "-e", est], full_cache=cache, algo="ull")


def test_a_rectangular_run_is_refused(tmp_path):
    genomes = _family(600, 50_000, rates=(0.0, 0.01, 0.05))
    paths = _write(tmp_path, "x", genomes)
    _sketch(tmp_path, "X", paths, ["-k", "16"])
    _sketch(tmp_path, "Y", paths[:2], ["-k", "16"])
    r = _run(tmp_path, ["dist", "-q", "Y", "-r", "X", "-o", "clu.tsv", "--cluster", "0.05"])
    assert r.returncode != 0 and "--cluster" in r.stderr
    out = tmp_path / "clu.tsv"
    assert not out.exists() or out.read_text().count("\n") <= 1


def test_randomized_against_the_yardstick(tmp_path):
    rng = np.random.default_rng(20240607)
    genomes = []
    for f in range(9):
        base = O.synth_genome(700 + f, int(rng.integers(30_000, 90_000)))
        top = float(rng.choice([0.005, 0.02, 0.06, 0.12]))
        genomes += [base] + [_mutated(base, float(rng.uniform(0.0, top)), 7000 + f * 100 + m) for m in range(int(rng.integers(0, 14)))]
    perm = rng.permutation(len(genomes))
    _sketch(tmp_path, "X", _write(tmp_path, "x", [genomes[i] for i in perm]), ["-k", "16"])
    cache = {}
    for _ in range(6):
        D = float(rng.choice([float(rng.uniform(0.0, 0.15)), float(rng.uniform(0.0, 1.0))]))
        flags = ["--block-rows", str(int(rng.integers(1, 40)))] + (["--file-order"] if rng.random() < 0.5 else []) \
            + (["--devices", "0,0,0"] if rng.random() < 0.5 else []) + (["--fp32"] if rng.random() < 0.3 else [])
        _cli_case(tmp_path, "X", D, flags, full_cache=cache)


# ---- ABI level: SketchSet.pair_block_cluster against pair_block + lash_dist_rows ------------------------------------------------------

def _labels_from_dense(d, D):
    """components of the links d <= D over the strict lower triangle of a dense distance matrix"""
    n = d.shape[0]
    rows, cols = np.nonzero(np.tril(d <= D, -1))
    return np.array(_components(n, zip(rows.tolist(), cols.tolist())), np.uint32)


def _blocks(n, step, start=0):
    edges = [0] + list(range(start or step, n, step)) + [n]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _run_blocks(s, blocks, D, k, acc, **kw):
    total = dict(pairs=0, pruned=0, joined_on_device=0, sent_to_host=0)
    for r0, r1 in blocks:
        st = {}
        s.pair_block_cluster(r0, r1, D, k, acc, stats=st, **kw)
        for key in total:
            total[key] += st[key]
        total["clusters"] = st["clusters"]
    return total


def _unsure_bound(d, D, margin, unplaceable=None, nan_too=False):
    """how many off-diagonal pairs the device may hand to the host: those whose exact d lies within 2 x margin of D (the device's d is
    within one margin of the host's, and undecided only within one margin of D), the pairs it cannot place, and NaN only where the
    design sends it back (hll; an hmh / ull NaN is decided on the device).  The ABI hands back no pairs, only their number; every
    pair outside the band must be decided on the device for the number to stay within this count (see _close_rows)."""
    low = np.tril(np.ones(d.shape, bool), -1)
    close = np.abs(d - D) <= 2 * margin
    if nan_too:
        close |= np.isnan(d)
    if unplaceable is not None:
        close |= unplaceable
    return int(np.count_nonzero(close & low))


@pytest.fixture(scope="module")
def hmh_cluster_set():
    # 1 100 sketches (rows of more than one 1 024-column tile): many small families, a 40-member family, chains, a few large genomes
    import lash_amd
    genomes = []
    rng = np.random.default_rng(5)
    for f in range(100):
        base = O.synth_genome(8000 + f, 12_000)
        genomes += [base] + [_mutated(base, float(rng.uniform(0.0, 0.25)), 80000 + f * 10 + m) for m in range(9)]
    genomes += _big_family(8200, 12_000, 40) + list(_chain(8300, 20_000)) + _family(8400, 600_000, rates=(0.0, 0.01, 0.04))
    genomes += [O.synth_genome(8500 + i, 30_000) for i in range(54)]
    perm = np.random.default_rng(6).permutation(len(genomes))
    ctx, imgs = _sketches("hmh", 16, 0, [genomes[i] for i in perm])
    s = ctx.sketch_set("hmh", 0, imgs)
    card = s.cardinalities()
    s.prepare()
    family = np.sort(np.argsort(perm)[1000:1040])                       # where the 40-member family went
    yield ctx, s, card, family, lash_amd
    s.free()
    ctx.close()


@pytest.mark.parametrize("model,fp32", [(1, False), (0, True)])
def test_abi_labels_blocks_orders_and_merge(hmh_cluster_set, model, fp32):
    ctx, s, card, family, lash_amd = hmh_cluster_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, model, fp32, 0, n, n, True)
    margin = 2.0 ** -16 if fp32 else 2.0 ** -40
    kw = dict(model=model, fp32=fp32)
    for D in (0.0, 0.02, 0.05, 0.1, 0.25, 1.0, -0.25):
        want = _labels_from_dense(d, D)
        blocks = _blocks(n, 300, start=37)                               # unaligned triangle blocks
        acc = lash_amd.Clusters(ctx, n)
        tot = _run_blocks(s, blocks, D, 16, acc, **kw)
        got = acc.labels()
        acc.free()
        assert np.array_equal(got, want), D
        # the smallest index of each cluster
        for lab in np.unique(got):
            assert lab == np.nonzero(got == lab)[0].min()
        assert tot["pairs"] == n * (n - 1) // 2 and tot["clusters"] == len(np.unique(want))
        assert tot["joined_on_device"] <= n - 1
        assert tot["sent_to_host"] <= _unsure_bound(d, D, margin), (D, tot)
        assert tot["pruned"] + tot["joined_on_device"] + tot["sent_to_host"] <= tot["pairs"]
        # reverse order; two accumulators merged; the whole-set walk
        acc = lash_amd.Clusters(ctx, n)
        tot_r = _run_blocks(s, blocks[::-1], D, 16, acc, **kw)
        assert np.array_equal(acc.labels(), want), D
        assert tot_r["clusters"] == len(np.unique(want)) and tot_r["pairs"] == tot["pairs"]
        acc.free()
        a0, a1 = lash_amd.Clusters(ctx, n), lash_amd.Clusters(ctx, n)
        _run_blocks(s, blocks[0::2], D, 16, a0, **kw)
        _run_blocks(s, blocks[1::2], D, 16, a1, **kw)
        before = a1.labels()
        a0.merge(a1)
        assert np.array_equal(a0.labels(), want), D
        assert np.array_equal(a1.labels(), before)                       # merge leaves its source alone
        st = {}
        s.pair_block_cluster(0, 1, D, 16, a0, stats=st, **kw)            # (a block without pairs: the merged accumulator's count)
        assert st["pairs"] == 0 and st["clusters"] == len(np.unique(want))
        a0.free()
        a1.free()
    assert np.array_equal(s.clusters(0.05, 16, block_rows=211, **kw), _labels_from_dense(d, 0.05))


def test_abi_a_dense_family_is_pruned_not_sent(hmh_cluster_set):
    ctx, s, card, family, lash_amd = hmh_cluster_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, 1, False, 0, n, n, True)
    sub = d[np.ix_(family, family)]
    assert np.nanmax(np.tril(sub, -1)) < 0.05                            # every pair of the family is a link at D = 0.05
    acc = lash_amd.Clusters(ctx, n)
    tot = _run_blocks(s, _blocks(n, 64), 0.05, 16, acc)
    got = acc.labels()
    acc.free()
    assert len(set(got[family].tolist())) == 1 and got[family[0]] == family[0]
    # all 780 pairs of the family are links and 39 joins are enough.  A row is new when its block runs, so its first pairs are
    # evaluated; the pairs the same wave looks at afterwards find the row already joined with the column's cluster.
    print("dense family:", tot)
    assert tot["pruned"] > 0 and tot["joined_on_device"] <= n - 1
    assert tot["sent_to_host"] <= _unsure_bound(d, 0.05, 2.0 ** -40)


def test_abi_edge_of_the_cutoff(hmh_cluster_set):
    """D = a pair's exact distance links it; one ulp below does not (as test_gpu_dist_within.py does for --max-dist)"""
    ctx, s, card, family, lash_amd = hmh_cluster_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, 1, False, 0, n, n, True)
    vals = d[np.isfinite(d) & (d > 0.01) & (d < 0.5)]
    assert len(vals) > 100
    for D in vals[:: max(1, len(vals) // 7)][:7]:
        D = float(D)
        lo = math.nextafter(D, -math.inf)
        assert np.array_equal(s.clusters(D, 16), _labels_from_dense(d, D))
        assert np.array_equal(s.clusters(lo, 16, block_rows=100), _labels_from_dense(d, lo))
        # the pair alone: its two sketches as the only off-diagonal pair of a 2 x 2 triangle
        i, j = (int(x) for x in np.argwhere(d == D)[0])
        assert j < i
        row, col, dist = s.pair_block_within(i, i + 1, D, 16, n_cols=i + 1, triangle=True)
        assert ((col == j) & (dist == D)).sum() == 1
        for cut, linked in ((D, True), (lo, False)):
            acc = lash_amd.Clusters(ctx, n)
            s.pair_block_cluster(i, i + 1, cut, 16, acc)
            got = acc.labels()
            acc.free()
            near = np.nonzero(d[i, :i] <= cut)[0]                        # row i alone: i with every column it links
            assert (j in near) == linked
            assert got[i] == (near.min() if len(near) else i) and (got[j] == got[i]) == linked


def _hll_unplaceable(st, p):
    """pairs the device hands to the host whatever D is: the raw estimate at or below 5m (bias-table regime), or a linear-counting
    estimate at its threshold"""
    thr = {10: 900.0, 14: 11500.0}[p]
    m = float(1 << p)
    zero, usum = st["c_or_zero"].astype(np.float64), st["sum_or_union"]
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(zero > 0, m * np.log(m / np.where(zero > 0, zero, 1.0)), np.inf)
        raw = (0.7213 / (1.0 + 1.079 / m)) * m * m / usum
    near = np.abs(lin - thr) <= thr * 2.0 ** -39                           # (numpy's log against the device's: a band twice as wide)
    bias = ~(lin <= thr) & (raw <= 5.0 * m)
    return bias & ~near, bias | near                                     # surely handed over, possibly handed over


def test_abi_hll_and_ull():
    import lash_amd
    a, b, c = _chain(900, 40_000)
    genomes = [a] + _big_family(901, 40_000, 12) + [b] + _family(902, 40_000, rates=(0.0, 0.01, 0.05, 0.2)) + [O.synth_genome(903, 400_000), c]
    genomes += [O.synth_genome(904, 3_000), _mutated(O.synth_genome(904, 3_000), 0.01, 9)]       # p = 14: linear counting
    p = 14
    m = float(1 << p)
    rng = np.random.default_rng(8)
    raw = np.sort(rng.uniform(0.7 * m, 5.0 * m, 200))
    bias = lash_amd.HllBias().set(p, raw, 0.6 * m * np.exp(-(raw - 0.7 * m) / m))
    ctx, imgs = _sketches("hll", 21, p, genomes)
    s = ctx.sketch_set("hll", p, imgs)
    card = s.cardinalities(hll_bias=bias)
    s.prepare()
    n = s.n
    surely, unplaceable = _hll_unplaceable(s.pair_block(0, n, n_cols=n, triangle=True), p)
    assert np.tril(surely, -1).any() and not np.tril(unplaceable, -1)[-1, -2]
    for model, fp32 in ((1, False), (0, True)):
        d = _dense(s, card, "hll", p, 21, model, fp32, 0, n, n, True, bias=bias)
        for D in (0.0, 0.05, 0.3, 1.0):
            for step in (n, 5):
                acc = lash_amd.Clusters(ctx, n)
                tot = _run_blocks(s, _blocks(n, step), D, 21, acc, model=model, fp32=fp32, hll_bias=bias)
                assert np.array_equal(acc.labels(), _labels_from_dense(d, D)), (model, fp32, D, step)
                acc.free()
                # pairs the device cannot place are never pruned; nothing else comes back unless it is at the cutoff
                assert int(np.count_nonzero(np.tril(surely, -1))) <= tot["sent_to_host"] \
                    <= _unsure_bound(d, D, 2.0 ** -16 if fp32 else 2.0 ** -40, unplaceable, nan_too=True), (model, fp32, D, tot)
    # without the tables: refused, at the pair pair_block_within refuses
    acc = lash_amd.Clusters(ctx, n)
    # (rows from 1 on: the first pair of row 1 is (1, 0), two 40 kbp genomes whose union is in the bias-table regime)
    with pytest.raises(lash_amd.LashError) as e:
        s.pair_block_cluster(1, n, 0.1, 21, acc, n_cols=n)
    with pytest.raises(lash_amd.LashError) as w:
        s.pair_block_within(1, n, 0.1, 21, n_cols=n, triangle=True)
    assert e.value.code == w.value.code == -6
    assert e.value.pair == w.value.pair == 0 and bool(np.tril(surely, -1)[1, 0])
    acc.free()
    s.free()
    # ull: empty sketches (genomes shorter than k) are NaN against each other under model 0
    genomes = [a] + _big_family(911, 200_000, 8) + [b, c] + [np.frombuffer(b"ACGTAC", np.uint8).copy()] * 2
    ctx2, imgs = _sketches("ull", 16, 12, genomes)
    s = ctx2.sketch_set("ull", 12, imgs)
    for est in ("fgra", "ml"):
        card = s.cardinalities(est)
        for model in (0, 1):
            d = _dense(s, card, "ull", 12, 16, model, False, 0, s.n, s.n, True, est=est)
            assert np.isnan(d).any() == (model == 0)
            for D in (0.01, 0.05, 1.0):
                st = {}
                acc = lash_amd.Clusters(ctx2, s.n)
                s.pair_block_cluster(0, s.n, D, 16, acc, model=model, estimator=est, stats=st)
                assert np.array_equal(acc.labels(), _labels_from_dense(d, D)), (est, model, D)
                assert st["sent_to_host"] <= _unsure_bound(d, D, 2.0 ** -40)   # (a ull NaN is decided on the device)
                acc.free()
    s.free()
    ctx.close()
    ctx2.close()


def test_abi_hll_p10_large_is_decided_on_the_device():
    """p = 10 with genomes of several hundred kbp: every union is in the raw-estimate regime (above 5 * 2^p), which the device places
    itself; two 600 bp genomes are in linear counting, where the device brackets the host's union estimate.  Nothing comes back unless
    it lies at the cutoff."""
    import lash_amd
    a, b, c = _chain(950, 400_000)
    genomes = [a] + _big_family(951, 300_000, 10) + [b] + _family(952, 500_000, rates=(0.0, 0.01, 0.05, 0.2)) + [O.synth_genome(953, 350_000), c]
    genomes += [O.synth_genome(954, 600), _mutated(O.synth_genome(954, 600), 0.01, 3)]
    p = 10
    ctx, imgs = _sketches("hll", 21, p, genomes)
    s = ctx.sketch_set("hll", p, imgs)
    card = s.cardinalities()
    s.prepare()
    n = s.n
    surely, unplaceable = _hll_unplaceable(s.pair_block(0, n, n_cols=n, triangle=True), p)
    assert not np.tril(unplaceable, -1).any()
    for model, fp32 in ((1, False), (0, False), (1, True)):
        d = _dense(s, card, "hll", p, 21, model, fp32, 0, n, n, True)
        assert np.isfinite(np.tril(d, -1)).all()
        for D in (0.0, 0.01, 0.05, 0.2, 1.0, -0.25):
            for step in (n, 4):
                acc = lash_amd.Clusters(ctx, n)
                tot = _run_blocks(s, _blocks(n, step), D, 21, acc, model=model, fp32=fp32)
                assert np.array_equal(acc.labels(), _labels_from_dense(d, D)), (model, fp32, D, step)
                acc.free()
                assert tot["sent_to_host"] <= _unsure_bound(d, D, 2.0 ** -16 if fp32 else 2.0 ** -40), (model, fp32, D, tot)
    s.free()
    ctx.close()
