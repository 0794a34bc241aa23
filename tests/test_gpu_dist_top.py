"""`lash dist --top K` (lash_sketch_set_pair_block_top: pair statistics and a per-name selection on the GPU, candidates evaluated
exactly on the host, per-name lists in lash_top).  The contract: the same header and the same rows, in the same order, as the run
without the option, minus every row that is in no name's K nearest.  Rank = (distance at full precision, position in the unfiltered
output); a rectangular run ranks each query's pairs, a triangle run each name's row and column.  The expected rows come from the
unfiltered output of the same build and full-precision distances from SketchSet.pair_block + lash_amd.dist_rows on the same sketches."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _family(seed, length, rates=(0.0, 0.002, 0.01, 0.03, 0.08)):
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


def _sketch_files(tmp_path, prefix):
    """(names in list-file order, parameters, images [n, image_bytes]) of a `lash sketch` output"""
    import lash_amd
    files = {os.path.basename(f) for f in glob.glob(str(tmp_path / (prefix + "*")))}
    names = json.loads((tmp_path / next(f for f in files if f.endswith("files.json"))).read_text())
    prm = json.loads((tmp_path / next(f for f in files if f.endswith("parameters.json"))).read_text())
    raw = H.zstd_read(str(tmp_path / next(f for f in files if f.endswith(".bin"))))
    algo = prm["algorithm"]
    p = int(prm.get("precision", 0)) if algo != "hmh" else 0
    ib = lash_amd.image_bytes(algo, p)
    return names, prm, np.frombuffer(raw[: len(names) * ib], np.uint8).reshape(len(names), ib)


def _full_distances(tmp_path, q, r, model, fp32, est):
    """{(reference name, query name): d} at full precision for every pair of the two sketch files (same-name pairs: 0)"""
    import lash_amd
    from lash_amd.sketch import dist_rows
    rn, prm, rimg = _sketch_files(tmp_path, r)
    qn, _, qimg = _sketch_files(tmp_path, q)
    algo, k = prm["algorithm"], int(prm["k"])
    p = int(prm.get("precision", 0)) if algo != "hmh" else 0
    ctx = lash_amd.Context(0)
    rs = ctx.sketch_set(algo, p, rimg)
    qs = ctx.sketch_set(algo, p, qimg)
    rc, qc = rs.cardinalities(est), qs.cardinalities(est)
    rs.prepare(qs)
    st = rs.pair_block(0, rs.n, qry=qs, estimator=est)
    if algo == "hmh":
        ec = rs.hmh_expected_collisions(0, rs.n, qry=qs)
        if ec is not None:
            st["hmh_ec"] = ec
    d = dist_rows(algo, p, k, model, rc, qc, fp32=fp32, **st)
    rs.free()
    qs.free()
    ctx.close()
    return {(a, b): (0.0 if a == b else float(d[i, j])) for i, a in enumerate(rn) for j, b in enumerate(qn)}


def _select(names_of, d, K, n_names):
    """which pairs are in N_K of one of their names: rank (d, position), NaN never ranked"""
    keep = np.zeros(len(d), bool)
    seen = np.zeros(n_names, np.int64)
    for i in np.lexsort((np.arange(len(d)), d)):
        if np.isnan(d[i]):
            continue
        for x in names_of[i]:
            if seen[x] < K:
                keep[i] = True
            seen[x] += 1
    return keep


def _expected(text, full, K, triangle, D=None):
    lines = text.split("\n")
    rows = [ln.split("\t") for ln in lines[1:-1]]
    ids = {}
    names_of = []
    for a, b, _ in rows:
        ia, ib = ids.setdefault(("n", a) if triangle else ("r", a), len(ids)), ids.setdefault(("n", b) if triangle else ("q", b), len(ids))
        names_of.append(tuple(sorted({ia, ib})) if triangle else (ib,))
    d = np.array([full[(a, b)] for a, b, _ in rows], np.float64)
    keep = _select(names_of, d, K, len(ids))
    if D is not None:
        keep &= d <= D
    return "\n".join([lines[0]] + [ln for ln, k in zip(lines[1:-1], keep) if k]) + "\n"


def _compare(tmp_path, q, r, flags, ks, env=None, max_dist=(None,)):
    base = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "full.tsv"] + flags, env)
    assert base.returncode == 0, base.stderr
    text = (tmp_path / "full.tsv").read_text()
    model = 0 if "0" in [flags[i + 1] for i, f in enumerate(flags) if f == "-m"] else 1
    est = flags[flags.index("-e") + 1] if "-e" in flags else "fgra"
    full = _full_distances(tmp_path, q, r, model, "--fp32" in flags, est)
    for K in ks:
        for D in max_dist:
            extra = ["--top", str(K)] + ([] if D is None else ["--max-dist", repr(D)])
            res = _run(tmp_path, ["dist", "-q", q, "-r", r, "-o", "top.tsv"] + extra + flags, env)
            assert res.returncode == 0, (K, D, res.stderr)
            got = (tmp_path / "top.tsv").read_text()
            assert got == _expected(text, full, K, q == r, D), (flags, K, D)
            if K >= text.count("\n") and D is None and "NaN" not in text:
                assert got == text
    return text


FLAG_SETS = [
    [],
    ["-m", "0", "--fp32"],
    ["--block-rows", "3"],
    ["--block-rows", "3", "--devices", "0,0", "--file-order"],
    ["-m", "0", "--block-rows", "2", "--file-order"],
]


def _triangle_and_rectangle(tmp_path, genomes, sk_args, extra=(), ks=(1, 2, 7, 1000), env=None, flag_sets=FLAG_SETS):
    """X = all genomes (triangle runs); Y = a few of them plus one file whose NAME is in X but whose sequence is different: in the
    rectangular X x Y run that pair prints 0 whatever its sketches say"""
    paths = _write(tmp_path, "x", genomes)
    _sketch(tmp_path, "X", paths, sk_args, env)
    ypaths = [paths[0], paths[2], paths[-1], paths[5]]
    with open(paths[2], "wb") as f:
        f.write(b">s\n" + _mutated(genomes[2], 0.05, 999).tobytes() + b"\n")
    _sketch(tmp_path, "Y", ypaths, sk_args, env)
    texts = []
    for i, flags in enumerate(flag_sets):
        for q in ("X", "Y"):
            texts.append(_compare(tmp_path, q, "X", list(flags) + list(extra), ks, env, max_dist=(None, 0.05) if i == 0 else (None,)))
    return texts


def _fixture_genomes(length, seed):
    """a family of mutated genomes, two exact copies of its base under other names (d = 0 ties), unrelated genomes (d = 1 ties)"""
    fam = _family(seed, length)
    return fam + [fam[0].copy(), fam[0].copy()] + [O.synth_genome(seed + 1 + i, length) for i in range(4)]


def test_hmh_large_genomes(tmp_path):
    texts = _triangle_and_rectangle(tmp_path, _fixture_genomes(600_000, 110), ["-k", "16"])
    assert "1.000000" in texts[0] and "\t0.000000" in texts[0]


def test_hmh_small_genomes(tmp_path):
    """both sketches <= 2^19 distinct k-mers: the expected collisions from the GEMM on the device"""
    _triangle_and_rectangle(tmp_path, _fixture_genomes(60_000, 210), ["-k", "16"], flag_sets=FLAG_SETS[:3])


def test_hll_p10(tmp_path):
    _triangle_and_rectangle(tmp_path, _fixture_genomes(400_000, 310), ["-k", "21", "-a", "hll", "-p", "10"], flag_sets=FLAG_SETS[:4])


@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_ull_with_empty_sketches(tmp_path, est):
    """genomes shorter than k have empty sketches: NaN against each other under -m 0, never ranked nor printed"""
    genomes = _fixture_genomes(200_000, 410) + [np.frombuffer(b"ACGTACG", np.uint8).copy(), np.frombuffer(b"TTGCA", np.uint8).copy()]
    texts = _triangle_and_rectangle(tmp_path, genomes, ["-k", "16", "-a", "ull", "-p", "12"], ["-e", est], flag_sets=[[], ["-m", "0"]])
    assert "NaN" in texts[2]


def test_hll_bias_regime_refused_like_the_unfiltered_run(tmp_path):
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    paths = _write(tmp_path, "n", [O.synth_genome(55, 9_000), O.synth_genome(56, 8_000)])
    _sketch(tmp_path, "S", paths, ["-k", "21", "-a", "hll", "-p", "14"], env)
    want = _run(tmp_path, ["dist", "-q", "S", "-r", "S", "-o", "full.tsv"], env)
    assert want.returncode != 0 and "union of" in want.stderr
    for K in ("1", "5"):
        got = _run(tmp_path, ["dist", "-q", "S", "-r", "S", "-o", "top.tsv", "--top", K], env)
        assert (got.returncode, got.stderr) == (want.returncode, want.stderr)


# ---- ABI level: SketchSet.pair_block_top against pair_block + lash_dist_rows ------------------------------------------------------------

def _sketches(algo, k, p, genomes):
    import lash_amd
    ctx = lash_amd.Context(0)
    seq, rec_off, goff = lash_amd.records_to_arrays([[g.tobytes()] for g in genomes])
    return ctx, ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff)


def _dense(s, card, algo, p, k, model, fp32, est="fgra"):
    from lash_amd.sketch import dist_rows
    st = s.pair_block(0, s.n, estimator=est)
    if algo == "hmh":
        ec = s.hmh_expected_collisions(0, s.n)
        if ec is not None:
            st["hmh_ec"] = ec
    return dist_rows(algo, p, k, model, card, card, fp32=fp32, **st)


def _families(n_fam, per, length, seed):
    out = []
    rng = np.random.default_rng(seed)
    for f in range(n_fam):
        base = O.synth_genome(seed + f, length)
        out += [base] + [_mutated(base, float(rng.uniform(0.0, 0.3)), seed * 1000 + f * 10 + m) for m in range(per - 1)]
    return out


@pytest.fixture(scope="module")
def hmh_set():
    # 1 100 sketches: rows longer than one 1 024-column tile; small genomes (GEMM expected collisions), a few large ones, identical copies
    genomes = _families(100, 10, 12_000, 7100) + _families(3, 10, 600_000, 8100) + [O.synth_genome(9100 + i, 30_000) for i in range(60)]
    genomes += [genomes[0].copy() for _ in range(10)]
    ctx, imgs = _sketches("hmh", 16, 0, genomes)
    s = ctx.sketch_set("hmh", 0, imgs)
    card = s.cardinalities()
    s.prepare()
    yield ctx, s, card
    s.free()
    ctx.close()


def _keys_less_equal(d, row, col, b):
    return (d < b["d"]) | ((d == b["d"]) & ((row < b["row"]) | ((row == b["row"]) & (col <= b["col"]))))


@pytest.mark.parametrize("model,fp32", [(1, False), (0, True)])
def test_abi_superset_of_the_block_contribution(hmh_set, model, fp32):
    import lash_amd
    ctx, s, card = hmh_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, model, fp32)
    rng = np.random.default_rng(5 + model)
    for trial in range(12):
        tri = trial % 2 == 0
        r0 = int(rng.integers(0, n - 2))
        r1 = int(rng.integers(r0 + 1, min(n, r0 + 400) + 1))
        nc = r1 if tri else n
        K = int(rng.choice([1, 2, 3, 10, 40]))
        D = None if trial % 3 else float(rng.choice([0.02, 0.1, 0.3]))
        same = np.full(r1 - r0, 0xFFFFFFFF, np.uint32)
        same[:: 7] = np.minimum(np.arange(r0, r1, 7), nc - 1)            # some rows carry the name of some column
        rows = np.arange(r0, r1)[:, None]
        cols = np.arange(nc)[None, :]
        blk = d[r0:r1, :nc].copy()
        blk[same[:, None] == cols] = 0.0
        printed = (cols <= rows) if tri else np.ones_like(blk, bool)
        R, Cc = np.broadcast_to(rows, blk.shape), np.broadcast_to(cols, blk.shape)
        # random caller bounds: +inf, or the key of a random pair of that name
        def bound(m):
            b = np.zeros(m, lash_amd.TOP_KEY)
            b["d"] = np.inf
            b["row"] = b["col"] = 0xFFFFFFFF
            pick = rng.random(m) < 0.5
            b["d"][pick] = rng.choice([0.0, 0.05, 0.2, 0.6, 1.0], size=int(pick.sum()))
            b["row"][pick] = rng.integers(0, n, size=int(pick.sum()))
            b["col"][pick] = rng.integers(0, n, size=int(pick.sum()))
            return b
        cb, rb = bound(nc), bound(r1 - r0)
        st = {}
        row, col, dist = s.pair_block_top(r0, r1, K, 16, n_cols=nc, triangle=tri, max_dist=D, same_col=same, col_bound=cb,
                                          row_bound=rb if tri else None, model=model, fp32=fp32, stats=st)
        assert np.all(np.diff(row.astype(np.int64) * nc + col) > 0)                         # (row, col) order, each once
        assert np.array_equal(dist.view(np.uint64), blk[row - r0, col].view(np.uint64))      # exact values
        valid = printed & ~np.isnan(blk)
        # the exact K-th key of each name over the block's pairs of that name, capped by the caller's bound
        got = set(zip(row.tolist(), col.tolist()))

        def kth(mask_rows):
            out = []
            for dd, rr, cc in mask_rows:
                o = np.lexsort((cc, rr, dd))
                out.append((dd[o[K - 1]], rr[o[K - 1]], cc[o[K - 1]]) if len(o) >= K else (np.inf, 0xFFFFFFFF, 0xFFFFFFFF))
            return out
        col_parts = [(blk[:, c][valid[:, c]], R[:, c][valid[:, c]], Cc[:, c][valid[:, c]]) for c in range(nc)]
        if tri:
            # a name's pairs in a triangle block: its column part and, for the block's rows, its row part
            parts = []
            for c in range(nc):
                dd, rr, cc = col_parts[c]
                if r0 <= c < r1:
                    m = valid[c - r0]
                    keep = ~((rr == c) & (cc == c))                                                # the diagonal is in both parts
                    dd, rr, cc = np.concatenate([dd[keep], blk[c - r0][m]]), np.concatenate([rr[keep], R[c - r0][m]]), np.concatenate([cc[keep], Cc[c - r0][m]])
                parts.append((dd, rr, cc))
        else:
            parts = col_parts
        T = kth(parts)
        T = [min(t, (b["d"], b["row"], b["col"])) for t, b in zip(T, cb)]
        if tri:
            for i in range(r1 - r0):
                x = r0 + i
                T[x] = min(T[x], (rb[i]["d"], rb[i]["row"], rb[i]["col"]))
        Tarr = np.array([(t[0], t[1], t[2]) for t in T], dtype=lash_amd.TOP_KEY)
        want = valid & _keys_less_equal(blk, R, Cc, Tarr[Cc])
        if tri:
            want |= valid & (R < nc) & _keys_less_equal(blk, R, Cc, Tarr[np.minimum(R, nc - 1)])
        if D is not None:
            want &= blk <= D
        wr, wc = np.nonzero(want)
        missing = set(zip((wr + r0).tolist(), wc.tolist())) - got
        assert not missing, (trial, sorted(missing)[:5])
        assert st["n_candidates"] >= len(row)


def test_top_pairs_matches_numpy(hmh_set):
    """SketchSet.top_pairs (row blocks + TopK) against the rank rule in numpy, one block and many"""
    ctx, s, card = hmh_set
    n = s.n
    d = _dense(s, card, "hmh", 0, 16, 1, False)
    tri_r, tri_c = np.tril_indices(n)
    dd = d[tri_r, tri_c].copy()
    dd[tri_r == tri_c] = 0.0
    names = [tuple(sorted({a, b})) for a, b in zip(tri_r.tolist(), tri_c.tolist())]
    for K in (1, 3, 12):
        keep = _select(names, dd, K, n)
        want = (tri_r[keep], tri_c[keep], dd[keep])
        for br in (None, 97):
            row, col, dist = s.top_pairs(K, 16, block_rows=br, same_col=np.arange(n))
            assert np.array_equal(row, want[0]) and np.array_equal(col, want[1]) and np.array_equal(dist, want[2]), (K, br)


def test_abi_tight_on_unrelated_genomes():
    """mostly unrelated genomes, K above the family size: nearly every pair is saturated at d = 1.0 and only the first few of them
    per name (the exact-pair tie-break) come back"""
    genomes = _families(60, 2, 20_000, 12000) + [O.synth_genome(13000 + i, 20_000) for i in range(180)]
    ctx, imgs = _sketches("hmh", 16, 0, genomes)
    s = ctx.sketch_set("hmh", 0, imgs)
    s.cardinalities()
    s.prepare()
    K = 3
    for r0, r1, tri in ((0, s.n, True), (100, 250, True), (0, 120, False), (200, s.n, False)):
        nc = r1 if tri else s.n
        st = {}
        s.pair_block_top(r0, r1, K, 16, n_cols=nc, triangle=tri, stats=st)
        assert st["n_candidates"] <= 2 * K * ((r1 - r0) + nc), (r0, r1, tri, st)
    s.free()
    ctx.close()


def test_abi_hll_bias_regime_like_within():
    import lash_amd
    genomes = _families(4, 4, 40_000, 3100) + [O.synth_genome(3950, 400_000)]
    ctx, imgs = _sketches("hll", 21, 14, genomes)
    s = ctx.sketch_set("hll", 14, imgs)
    m = float(1 << 14)
    rng = np.random.default_rng(8)
    raw = np.sort(rng.uniform(0.7 * m, 5.0 * m, 200))
    bias = lash_amd.HllBias().set(14, raw, 0.6 * m * np.exp(-(raw - 0.7 * m) / m))
    s.cardinalities(hll_bias=bias)
    s.prepare()
    for r0, r1 in ((0, s.n), (3, s.n), (5, 9)):
        with pytest.raises(lash_amd.LashError) as w:
            s.pair_block_within(r0, r1, 0.1, 21)
        with pytest.raises(lash_amd.LashError) as t:
            s.pair_block_top(r0, r1, 2, 21)
        assert t.value.code == w.value.code == -6 and t.value.pair == w.value.pair
    # with the tables the bias-regime pairs are evaluated on the host: the result is the rank rule on exact distances
    from lash_amd.sketch import dist_rows
    card = s.cardinalities(hll_bias=bias)
    st = s.pair_block(0, s.n)
    d = dist_rows("hll", 14, 21, 1, card, card, hll_bias=bias, **st)
    n = s.n
    R, Cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    flat_d, flat_r, flat_c = d.ravel(), R.ravel(), Cc.ravel()
    keep = _select([(c,) for c in flat_c.tolist()], flat_d, 2, n)
    row, col, dist = s.top_pairs(2, 21, qry=s, triangle=False, hll_bias=bias)
    assert np.array_equal(row, flat_r[keep]) and np.array_equal(col, flat_c[keep]) and np.array_equal(dist, flat_d[keep])
    s.free()
    ctx.close()
