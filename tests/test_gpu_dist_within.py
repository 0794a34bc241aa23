"""`lash dist --max-dist D` (lash_sketch_set_pair_block_within: pair statistics, expected collisions and a filter kernel on the GPU,
survivors evaluated exactly on the host).  The contract: the same header and the same rows, in the same order, as the run without the
option, minus every row whose distance fails d <= D.  The reference for every case is the unfiltered output of the same build."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_VALUES = (0.0, 0.01, 0.05, 0.2, 1.0, -0.25)
RATES = (0.0, 0.002, 0.01, 0.03, 0.08, 0.15, 0.3)


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _family(seed, length, rates=RATES):
    base = O.synth_genome(seed, length)
    return [base if r == 0 else _mutated(base, r, seed * 100 + i) for i, r in enumerate(rates)]


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


def _expected(text, D):
    """the unfiltered text with the rows that fail d <= D dropped, judged on the printed value.  Rows whose printed value lies within
    1.5e-6 of D are ambiguous at 6 decimals: returned separately (the exact edge is the ABI test's business)."""
    lines = text.split("\n")
    keep, unsure = [lines[0]], []
    for ln in lines[1:-1]:
        v = float(ln.rsplit("\t", 1)[1])                     # NaN -> fails every comparison
        if abs(v - D) <= 1.5e-6:
            unsure.append(ln)
        elif v <= D:
            keep.append(ln)
    return keep, unsure


def _check(text, got, D):
    keep, unsure = _expected(text, D)
    if not unsure:
        assert got == "\n".join(keep) + "\n"                 # byte for byte, order included
        return
    # ambiguous rows: the output is the unfiltered rows in order, every sure row present, nothing else
    all_lines = text.split("\n")[:-1]
    got_lines = got.split("\n")[:-1]
    it = iter(all_lines)
    assert all(any(g == a for a in it) for g in got_lines)  # an ordered subsequence
    assert [g for g in got_lines if g not in unsure] == keep


def _compare_all(tmp_path, q, r, flags, env=None, d_values=D_VALUES):
    base = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "full.tsv"] + flags, env)
    assert base.returncode == 0, base.stderr
    text = (tmp_path / "full.tsv").read_text()
    assert text.count("\n") > 3
    for D in d_values:
        res = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "cut.tsv", "--max-dist", repr(D)] + flags, env)
        assert res.returncode == 0, (D, res.stderr)
        got = (tmp_path / "cut.tsv").read_text()
        _check(text, got, D)
        if D >= 1 and "NaN" not in text:
            assert got == text
        if D < 0:
            assert got == "Reference\tQuery\tDistance\n"
    return text


FLAG_SETS = [
    ([], True),
    (["-m", "0", "--block-rows", "7", "--file-order"], False),
    (["--fp32", "--block-rows", "1", "--devices", "0,0"], True),
    (["-m", "0", "--fp32", "--file-order", "--devices", "0,0"], False),
    (["--block-rows", "7", "--devices", "0,0"], False),
]


def _triangle_and_rectangle(tmp_path, genomes, sk_args, extra_flags=(), env=None, flag_sets=FLAG_SETS):
    """X = all genomes; Y = a few of them plus one file whose NAME is in X but whose sequence is different (it is rewritten between
    the two `lash sketch` runs): the same-name -> 0 rule must hold in the filtered output too."""
    paths = _write(tmp_path, "x", genomes)
    _sketch(tmp_path, "X", paths, sk_args, env)
    renamed = paths[2]
    ypaths = [paths[0], renamed, paths[-1]]
    with open(renamed, "wb") as f:
        f.write(b">s\n" + _mutated(genomes[2], 0.05, 999).tobytes() + b"\n")
    _sketch(tmp_path, "Y", ypaths, sk_args, env)
    texts = []
    for flags, tri in flag_sets:
        q = "X" if tri else "Y"
        texts.append(_compare_all(tmp_path, q, "X", list(flags) + list(extra_flags), env))
    return texts


def test_hmh_large_genomes(tmp_path):
    """> 2^19 distinct 16-mers per genome: the closed-form expected collisions"""
    genomes = _family(11, 700_000) + [O.synth_genome(12, 650_000)]
    texts = _triangle_and_rectangle(tmp_path, genomes, ["-k", "16"])
    ds = [float(ln.rsplit("\t", 1)[1]) for ln in texts[0].split("\n")[1:-1]]
    assert min(d for d in ds if d > 0) < 0.01 and any(0.05 < d < 0.2 for d in ds) and max(ds) == 1.0


def test_hmh_small_genomes(tmp_path):
    """20-300 kbp: both sketches <= 2^19 distinct k-mers, the expected-collision term from the GEMM kept on the device"""
    genomes = _family(21, 60_000) + _family(22, 250_000, rates=(0.0, 0.01, 0.05, 0.2)) + [O.synth_genome(23, 20_000), O.synth_genome(24, 300_000)]
    _triangle_and_rectangle(tmp_path, genomes, ["-k", "16"])


def test_hmh_mixed_sizes(tmp_path):
    genomes = _family(31, 40_000, rates=(0.0, 0.01, 0.1)) + _family(32, 700_000, rates=(0.0, 0.005, 0.05, 0.3)) + [O.synth_genome(33, 120_000)]
    _triangle_and_rectangle(tmp_path, genomes, ["-k", "16"], flag_sets=FLAG_SETS[:3])


def test_hll_p10_large(tmp_path):
    genomes = _family(41, 500_000) + [O.synth_genome(42, 400_000)]
    _triangle_and_rectangle(tmp_path, genomes, ["-k", "21", "-a", "hll", "-p", "10"])


def _bias_file(tmp_path, p):
    m = float(1 << p)
    rng = np.random.default_rng(8)
    raw = np.sort(rng.uniform(0.7 * m, 5.0 * m, 200))
    bias = 0.6 * m * np.exp(-(raw - 0.7 * m) / m)
    with open(tmp_path / "bias.txt", "w") as f:
        f.write("# synthetic\np %d %d\n" % (p, len(raw)) + "".join("%r %r\n" % (float(a), float(b)) for a, b in zip(raw, bias)))
    return raw, bias


def test_hll_p14_small_with_and_without_tables(tmp_path):
    """p = 14 on small genomes: sketches and unions in the HLL++ bias-table regime.  With (synthetic) tables every such pair is
    evaluated on the host; without them the filtered run fails exactly like the unfiltered one, whatever D is."""
    _bias_file(tmp_path, 14)
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    genomes = _family(51, 40_000, rates=(0.0, 0.01, 0.05, 0.2)) + [O.synth_genome(52, 30_000), O.synth_genome(53, 300_000)]
    _triangle_and_rectangle(tmp_path, genomes, ["-k", "21", "-a", "hll", "-p", "14"], ["--hll-bias", "bias.txt"], env, flag_sets=FLAG_SETS[:3])
    # without the tables: X fails on its sketches' own estimates; two ~9 kbp genomes are each in linear counting, their union is not
    paths = _write(tmp_path, "n", [O.synth_genome(55, 9_000), O.synth_genome(56, 8_000)])
    _sketch(tmp_path, "N", paths[:1], ["-k", "21", "-a", "hll", "-p", "14"], env)
    _sketch(tmp_path, "M", paths[1:], ["-k", "21", "-a", "hll", "-p", "14"], env)
    _sketch(tmp_path, "S", paths, ["-k", "21", "-a", "hll", "-p", "14"], env)
    for q, r in (("X", "X"), ("M", "N"), ("S", "S")):
        want = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "full.tsv"], env)
        assert want.returncode != 0 and "bias tables" in want.stderr
        assert (q == "X") != ("union of" in want.stderr)                               # (a block's pair, not a sketch)
        for D in (0.0, 0.3, 1.0, -1.0):
            got = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "cut.tsv", "--max-dist", repr(D)], env)
            assert (got.returncode, got.stderr) == (want.returncode, want.stderr), (q, r, D)


@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_ull_with_an_empty_sketch(tmp_path, est):
    """a genome shorter than k has an empty sketch: NaN against another empty one under -m 0 (never passes), 1 under -m 1"""
    genomes = _family(61, 300_000, rates=(0.0, 0.005, 0.03, 0.1, 0.3)) + [O.synth_genome(62, 200_000)]
    genomes += [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]
    texts = _triangle_and_rectangle(tmp_path, genomes, ["-k", "16", "-a", "ull", "-p", "12"], ["-e", est])
    assert "NaN" in texts[1] and "NaN" not in texts[0]


# ---- ABI level: SketchSet.pair_block_within against pair_block + lash_dist_rows -------------------------------------------------------

def _sketches(algo, k, p, genomes):
    import lash_amd
    ctx = lash_amd.Context(0)
    seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in genomes])
    return ctx, ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff)


def _dense(s, card, algo, p, k, model, fp32, r0, r1, n_cols, triangle, est="fgra", bias=None):
    from lash_amd.sketch import dist_rows
    st = s.pair_block(r0, r1, n_cols=n_cols, triangle=triangle, estimator=est)
    if algo == "hmh":
        ec = s.hmh_expected_collisions(r0, r1, n_cols=n_cols)
        if ec is not None:
            st["hmh_ec"] = ec
    if triangle:                                   # entries above the diagonal are undefined: neutral statistics for them
        above = np.arange(n_cols)[None, :] > (r0 + np.arange(r1 - r0))[:, None]
        for key, v in st.items():
            st[key] = np.where(above, 0 if v.dtype != np.float64 else 1e-300, v).astype(v.dtype)
    d = dist_rows(algo, p, k, model, card[r0:r1], card[:n_cols], fp32=fp32, hll_bias=bias, **st)
    if triangle:
        d[above] = np.inf
    return d


def _want(d, r0, D):
    rows, cols = np.nonzero(d <= D)
    return rows.astype(np.uint32) + np.uint32(r0), cols.astype(np.uint32), d[rows, cols]


def _families(n_fam, per, length, seed):
    out = []
    rng = np.random.default_rng(seed)
    for f in range(n_fam):
        base = O.synth_genome(seed + f, length)
        out += [base] + [_mutated(base, float(rng.uniform(0.0, 0.3)), seed * 1000 + f * 10 + m) for m in range(per - 1)]
    return out


@pytest.fixture(scope="module")
def hmh_set():
    # 1 300 sketches: rows of more than one 1 024-column filter tile; small genomes (GEMM expected collisions) and a few large ones
    genomes = _families(125, 10, 12_000, 7000) + _families(3, 10, 600_000, 8000) + [O.synth_genome(9000 + i, 30_000) for i in range(20)]
    ctx, imgs = _sketches("hmh", 16, 0, genomes)
    s = ctx.sketch_set("hmh", 0, imgs)
    card = s.cardinalities()
    s.prepare()
    yield ctx, s, card
    s.free()
    ctx.close()


@pytest.mark.parametrize("model,fp32", [(1, False), (0, True)])
@pytest.mark.parametrize("r0,r1,triangle", [(0, 1300, True), (37, 1100, True), (1031, 1300, True), (5, 300, False)])
def test_abi_matches_dense_hmh(hmh_set, model, fp32, r0, r1, triangle):
    ctx, s, card = hmh_set
    n_cols = min(r1, s.n) if triangle else s.n
    d = _dense(s, card, "hmh", 0, 16, model, fp32, r0, r1, n_cols, triangle)
    for D in (0.0, 0.02, 0.1, 0.25, 1.0):
        st = {}
        row, col, dist = s.pair_block_within(r0, r1, D, 16, n_cols=n_cols, triangle=triangle, model=model, fp32=fp32, stats=st)
        wr, wc, wd = _want(d, r0, D)
        assert np.array_equal(row, wr) and np.array_equal(col, wc) and np.array_equal(dist.view(np.uint64), wd.view(np.uint64)), D
        assert st["n_kept"] == len(wr)
        # margin: the kernel passes to the host at most the pairs within the stated margin of D (or NaN)
        slack = int(np.count_nonzero((d > D) & (d <= D + (2.0 ** -16 if fp32 else 2.0 ** -40)))) + int(np.count_nonzero(np.isnan(d)))
        assert st["n_kept"] <= st["n_candidates"] <= st["n_kept"] + slack, (D, st, slack)


def test_abi_exact_edge_and_capacity(hmh_set):
    ctx, s, card = hmh_set
    d = _dense(s, card, "hmh", 0, 16, 1, False, 0, s.n, s.n, True)
    vals = d[np.isfinite(d) & (d > 0.01) & (d < 0.5)]
    assert len(vals) > 100
    for D in vals[:: max(1, len(vals) // 7)][:7]:
        i, j = np.argwhere(d == D)[0]
        row, col, dist = s.pair_block_within(0, s.n, float(D), 16, n_cols=s.n, triangle=True)
        hit = (row == i) & (col == j)
        assert hit.sum() == 1 and dist[hit][0] == D                                   # d <= D: kept at the exact double
        lo = math.nextafter(float(D), -math.inf)
        row, col, dist = s.pair_block_within(0, s.n, lo, 16, n_cols=s.n, triangle=True)
        assert not ((row == i) & (col == j)).any()                                     # one ulp below: dropped
        assert np.array_equal(row, _want(d, 0, lo)[0])
    # capacity: a tiny cap reports the full count, a second call with room gives what one large call gives
    st = {}
    row, col, dist = s.pair_block_within(0, s.n, 0.2, 16, n_cols=s.n, triangle=True, cap=3, stats=st)
    full = st["n_kept"]
    assert full > 3 and len(row) == 3
    r2, c2, d2 = s.pair_block_within(0, s.n, 0.2, 16, n_cols=s.n, triangle=True, cap=full)
    r3, c3, d3 = s.pair_block_within(0, s.n, 0.2, 16, n_cols=s.n, triangle=True)
    assert np.array_equal(r2, r3) and np.array_equal(c2, c3) and np.array_equal(d2, d3) and len(r3) == full
    assert np.array_equal(row, r3[:3]) and np.array_equal(col, c3[:3])


def test_abi_hll_with_tables_and_ull_empty():
    import lash_amd
    genomes = _families(6, 6, 40_000, 3000) + [O.synth_genome(3900, 400_000)]
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
    for model, fp32 in ((1, False), (0, True)):
        d = _dense(s, card, "hll", p, 21, model, fp32, 3, n, n, False, bias=bias)
        for D in (0.0, 0.05, 0.3, 1.0):
            row, col, dist = s.pair_block_within(3, n, D, 21, model=model, fp32=fp32, hll_bias=bias)
            wr, wc, wd = _want(d, 3, D)
            assert np.array_equal(row, wr) and np.array_equal(col, wc) and np.array_equal(dist, wd)
    # without the tables: refused, and at the first pair lash_dist_rows refuses
    with pytest.raises(lash_amd.LashError) as e:
        s.pair_block_within(0, n, 0.1, 21)
    assert e.value.code == -6
    s.free()
    # ull: an empty sketch (genome shorter than k) — NaN against itself under model 0, never kept
    genomes = _families(4, 5, 200_000, 4000) + [np.frombuffer(b"ACGTAC", np.uint8).copy()] * 2
    ctx2, imgs = _sketches("ull", 16, 12, genomes)
    s = ctx2.sketch_set("ull", 12, imgs)
    for est in ("fgra", "ml"):
        card = s.cardinalities(est)
        for model in (0, 1):
            d = _dense(s, card, "ull", 12, 16, model, False, 0, s.n, s.n, True, est=est)
            assert np.isnan(d).any() == (model == 0)
            for D in (0.01, 0.1, 1.0):
                st = {}
                row, col, dist = s.pair_block_within(0, s.n, D, 16, n_cols=s.n, triangle=True, model=model, estimator=est, stats=st)
                wr, wc, wd = _want(d, 0, D)
                assert np.array_equal(row, wr) and np.array_equal(col, wc) and np.array_equal(dist, wd)
    s.free()
    ctx.close()
    ctx2.close()


# ---- the multi-rank driver ---------------------------------------------------------------------------------------------------------

def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def test_allpairs_two_ranks_equal_the_cli(tmp_path):
    genomes = _family(71, 200_000) + [O.synth_genome(72, 150_000)]
    paths = _write(tmp_path, "g", genomes)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    args = ["-f", "list.txt", "-a", "hmh", "-k", "16"]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), "-m", "lash_amd.allpairs", "--backend", "gloo", "--device", "0", "-o", "multi.tsv",
                        "--max-dist", "0.05"] + args, cwd=tmp_path, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    r = _run(tmp_path, ["sketch", "-o", "one"] + args, env)
    assert r.returncode == 0, r.stderr
    r = _run(tmp_path, ["dist", "-q", "one", "-r", "one", "-o", "one.tsv", "--file-order", "--max-dist", "0.05"], env)
    assert r.returncode == 0, r.stderr
    one = (tmp_path / "one.tsv").read_text()
    assert (tmp_path / "multi.tsv").read_text() == one
    assert 8 < one.count("\n") < 1 + 8 * 9 // 2
