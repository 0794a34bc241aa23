"""Simulated HLL++ bias tables (lash_hll_bias_simulate, lash_amd/csrc/hll_bias_sim.hip): the GPU's tables against the numpy
restatement bit for bit, determinism and arguments, that the tables remove the small-range bias of independent random sets,
and `lash dist --hll-bias-sim` / `lash hll-bias` end to end on genomes of a few kbp."""
import math
import os
import subprocess

import numpy as np
import pytest

import hllsimref as S
import host_lib as H
import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
SEEDS = (42, 0x9E3779B97F4A7C15)
# (p, points, trials): every cardinality 0..80 and the fewest points at p = 4; one workgroup per trial up to p = 14 with checkpoint
# intervals that are no multiple of the workgroup; p = 17 / 18 take the bucket-slice path (4 and 8 workgroups per trial)
CASES = [(4, 81, 16), (4, 6, 5), (7, 24, 8), (10, 24, 8), (14, 24, 8), (17, 12, 3), (18, 12, 3)]


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def default_tables(ctx):
    """{p: (n, raw, bias)} with the default points, trials and seed — simulated once for the tests below"""
    return {p: ctx.hll_bias_simulate(p) for p in (10, 12, 14)}


@pytest.fixture(scope="module")
def restated():
    return {(c, seed): S.simulate(c[0], c[1], c[2], seed) for c in CASES for seed in SEEDS}


@pytest.mark.parametrize("p,points,trials", CASES)
def test_tables_equal_the_restatement_bit_for_bit(ctx, restated, p, points, trials):
    for seed in SEEDS:
        n, raw, bias = ctx.hll_bias_simulate(p, points, trials, seed)
        wn, wraw, wbias = restated[((p, points, trials), seed)]
        assert n.dtype == np.uint64 and np.array_equal(n, wn) and n[0] == 0 and n[-1] == 5 << p
        assert np.array_equal(raw, wraw), (seed, np.flatnonzero(raw != wraw)[:5])
        assert np.array_equal(bias, wbias), (seed, np.flatnonzero(bias != wbias)[:5])


@pytest.mark.parametrize("p,points,trials", CASES)
def test_raw0_is_alpha_m_for_every_trial_count(ctx, p, points, trials):
    """Every trial's estimate at n = 0 is exactly alpha * m (S = m; the multiplications and the division by a power of two are
    exact), and the mean over the trials is the exactly rounded one, so raw[0] is alpha * m for every trial count.  (A sum rounded
    after each addend misses it by one ulp from T = 3 on: 91.55462313776833 against 91.55462313776835 at p = 7, T = 8.)"""
    want = R.hll_alpha(p) * (1 << p)
    for t in (1, 2, 3, 7, trials, 100):
        _, raw, _ = ctx.hll_bias_simulate(p, points, t, 42)
        print("p %d T %d: raw[0] %r, alpha * m %r" % (p, t, float(raw[0]), want))
        assert raw[0] == want, (p, t)


def test_determinism_seeds_defaults_and_arguments(ctx):
    import lash_amd
    from lash_amd import _lib
    a = ctx.hll_bias_simulate(10, 24, 8, 42)
    b = ctx.hll_bias_simulate(10, 24, 8, 42)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = ctx.hll_bias_simulate(10, 24, 8, 43)
    assert np.array_equal(a[0], c[0]) and not np.array_equal(a[1][1:], c[1][1:])
    lib = _lib.load()
    for p, want in ((4, 81), (5, 161), (6, 200), (11, 200), (18, 200), (3, 0), (19, 0)):
        assert lib.lash_hll_bias_default_points(p) == want
    for p in (4, 5, 6):
        n, raw, bias = ctx.hll_bias_simulate(p, trials=4)
        assert len(n) == len(raw) == len(bias) == S.default_points(p)
    for p, points in ((3, 6), (19, 6), (10, 5), (10, 1), (4, 82), (10, 5 * 1024 + 2)):
        with pytest.raises(lash_amd.LashError) as e:
            ctx.hll_bias_simulate(p, points, 2)
        assert e.value.code == _lib.EINVAL, (p, points)
    n = ctx.hll_bias_simulate(10, 5 * 1024 + 1, 1)[0]
    assert np.array_equal(n, np.arange(5 * 1024 + 1, dtype=np.uint64))
    buf = np.zeros(8, np.float64)
    assert lib.lash_hll_bias_simulate(ctx._h, 10, 6, 2, 42, None, None, buf.ctypes.data) == _lib.EINVAL
    assert lib.lash_hll_bias_simulate(ctx._h, 10, 6, 2, 42, None, buf.ctypes.data, None) == _lib.EINVAL
    assert lib.lash_hll_bias_simulate(None, 10, 6, 2, 42, None, buf.ctypes.data, buf.ctypes.data) == _lib.EINVAL
    assert lib.lash_hll_bias_simulate(ctx._h, 10, 6, 2, 42, None, buf.ctypes.data, buf.ctypes.data) == _lib.OK     # out_n may be NULL


@pytest.mark.parametrize("p", [10, 12])
def test_default_tables_remove_the_small_range_bias(default_tables, p):
    """64 independent random sets per cardinality (numpy's generator, not the simulation's hash).  Bound: four standard errors of a
    64-set mean at HyperLogLog's published 1.04 / sqrt(m).  The uncorrected raw estimate has to miss it where the bias is large,
    so a table of zeros cannot pass."""
    import lash_amd
    m = 1 << p
    n, raw, bias = default_tables[p]
    assert len(raw) == 200 and raw[0] == pytest.approx(R.hll_alpha(p) * m, rel=1e-12) and 0.7 * m < raw[0] < 0.73 * m
    assert np.all(np.diff(raw) > 0) and bias[0] == raw[0] and abs(bias[-1]) < 0.05 * m and np.all(bias[:40] > bias[-1])
    tb = lash_amd.HllBias().set(p, raw, bias)
    bound = 4 * 1.04 / math.sqrt(64 * m)
    rng = np.random.default_rng(1000 + p)
    alpha = R.hll_alpha(p)
    for mult in (1.0, 1.5, 2.0, 3.0, 4.7):
        card = int(m * mult)
        err_corr, err_raw = [], []
        for _ in range(64):
            h = rng.integers(0, 1 << 64, size=card, dtype=np.uint64)
            regs = np.zeros(m, np.int64)
            np.maximum.at(regs, (h & np.uint64(m - 1)).astype(np.int64), S.clz64(h >> np.uint64(p)) - p + 1)
            img = np.concatenate([np.zeros(33, np.uint8), regs.astype(np.uint8)])
            err_corr.append(lash_amd.sketch_cardinality("hll", p, img, hll_bias=tb) / card - 1.0)
            err_raw.append(alpha * m * m / float(np.sum(np.ldexp(1.0, -regs))) / card - 1.0)
        mc, mr = float(np.mean(err_corr)), float(np.mean(err_raw))
        print("p %d n = %.1f m: corrected %+.5f raw %+.5f bound %.5f" % (p, mult, mc, mr, bound))
        assert abs(mc) <= bound, (p, mult, mc)
        if mult <= 2.0:
            assert abs(mr) > bound, (p, mult, mr)


# ---- through the command line ----------------------------------------------------------------------------------------------------------

def _run(tmp_path, args, env):
    return subprocess.run([H.CLI] + args, cwd=tmp_path, capture_output=True, text=True, env=env, timeout=600)


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _distinct_canonical(seq, k):
    s = seq.tobytes().decode()
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    n = len(s)
    return len({min(s[i:i + k], rc[n - k - i:n - i]) for i in range(n - k + 1)})


def _rows(text):
    return [ln.split("\t") for ln in text.split("\n")[1:-1]]


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


def _members_text(names, rep):
    return "Representative\tMember\n" + "".join("%s\t%s\n" % (names[rep[i]], names[i]) for i in sorted(range(len(names)), key=lambda i: (rep[i], i)))


def test_cli_small_genomes_end_to_end(tmp_path, ctx, default_tables):
    import lash_amd
    from lash_amd.sketch import dist_rows
    p, k = 14, 21
    m = 1 << p
    lengths = [3_000, 5_000, 8_000, 12_000, 15_000, 18_000, 22_000, 26_000, 30_000, 33_000, 37_000, 40_000]
    genomes = [O.synth_genome(500 + i, n) for i, n in enumerate(lengths)]
    genomes += [_mutated(genomes[i], rate, 70 + i) for i, rate in ((2, 0.02), (4, 0.04), (6, 0.06), (9, 0.08), (11, 0.10))]
    paths = []
    for i, g in enumerate(genomes):
        f = tmp_path / ("v%02d.fa" % i)
        f.write_bytes(b">v\n" + g.tobytes() + b"\n")
        paths.append(str(f))
    (tmp_path / "l.txt").write_text("\n".join(paths) + "\n")
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    r = _run(tmp_path, ["sketch", "-f", "l.txt", "-o", "sm", "-a", "hll", "-p", str(p), "-k", str(k)], env)
    assert r.returncode == 0, r.stderr
    # without the flag: refused, as before
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "no.tsv"], env)
    assert r.returncode != 0 and "bias tables" in r.stderr
    # with it: a row for every pair, and the provenance on stderr; a broken $LASH_HLL_BIAS is not even opened
    env_bad = dict(env, LASH_HLL_BIAS=str(tmp_path / "missing.txt"))
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "sim.tsv", "--hll-bias-sim"], env_bad)
    assert r.returncode == 0, r.stderr
    prov = [ln for ln in r.stderr.split("\n") if "--hll-bias-sim" in ln]
    assert len(prov) == 1 and "simulated" in prov[0] and "not streaming_algorithms" in prov[0]
    assert "p 14: 200 points, 2048 trials, seed 42" in prov[0]
    text = (tmp_path / "sim.tsv").read_text()
    rows = _rows(text)
    n = len(genomes)
    assert len(rows) == n * (n + 1) // 2 and {frozenset((a, b)) for a, b, _ in rows} == {frozenset((x, y)) for x in paths for y in paths}
    # the rows against pyref with the tables HllBias.simulated makes (the same bits as the fixture's)
    _, raw, bias = default_tables[p]
    tables = {p: (raw.tolist(), bias.tolist())}
    imgs = O.sketch_genomes(O.HLL, k, p, 42, *lash_amd.records_to_arrays([[g.tobytes()] for g in genomes]))
    regs = [im[33:].tobytes() for im in imgs]
    length = [R.hll_len_from_regs(p, rg, tables) for rg in regs]
    assert sum(R.hll_len_from_regs(p, rg) is None for rg in regs) >= 8              # most sketches ARE in the refused regime
    for a, b, d in rows:
        i, j = paths.index(a), paths.index(b)
        u = R.hll_len_from_regs(p, bytes(max(x, y) for x, y in zip(regs[i], regs[j])), tables)
        want = R.mash_distance(max((length[i] + length[j] - u) / u, 0.0), k, 1, i == j)
        assert abs(float(d) - want) <= 1.1e-6, (i, j)
    # every cardinality against the exact count: four standard errors of one sketch
    tb = lash_amd.HllBias.simulated(ctx, p)
    for i, g in enumerate(genomes):
        exact = _distinct_canonical(g, k)
        got = lash_amd.sketch_cardinality("hll", p, imgs[i], hll_bias=tb)
        assert got == pytest.approx(length[i], rel=1e-12)
        assert abs(got / exact - 1.0) <= 4 * 1.04 / math.sqrt(m), (i, exact, got)
    # the same bytes through a file written by `lash hll-bias`
    r = _run(tmp_path, ["hll-bias", "-o", "F.txt", "-p", "14"], env)
    assert r.returncode == 0, r.stderr
    ftext = (tmp_path / "F.txt").read_text()
    assert ftext.startswith("#") and "simulated" in ftext and "not streaming_algorithms" in ftext
    assert "# p 14: 200 points, 2048 trials, seed 42\np 14 200\n" in ftext
    loaded = np.array([[float(x) for x in ln.split()] for ln in ftext.split("\n") if ln and ln[0] not in "#p"])
    assert np.array_equal(loaded[:, 0], raw) and np.array_equal(loaded[:, 1], bias)
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "file.tsv", "--hll-bias", "F.txt"], env)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "file.tsv").read_bytes() == (tmp_path / "sim.tsv").read_bytes()
    # the filtered routes agree with what the plain rows imply (full-precision distances from the ABI with the same tables)
    s = ctx.sketch_set("hll", p, imgs)
    card = s.cardinalities(hll_bias=tb)
    s.prepare()
    dense = dist_rows("hll", p, k, 1, card, card, hll_bias=tb, **s.pair_block(0, n))
    s.free()
    d = np.array([0.0 if a == b else dense[paths.index(a), paths.index(b)] for a, b, _ in rows])
    assert np.all(np.abs(d - np.array([float(x) for _, _, x in rows])) <= 5.1e-7)
    assert 3 <= int(np.sum(d <= 0.1)) - n < len(rows) - n                            # the mutated copies are within 0.1, most pairs are not
    lines = text.split("\n")
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "cut.tsv", "--hll-bias-sim", "--max-dist", "0.1"], env)
    assert r.returncode == 0, r.stderr
    cut = (tmp_path / "cut.tsv").read_text()
    assert cut == "\n".join([lines[0]] + [ln for ln, x in zip(lines[1:-1], d) if x <= 0.1]) + "\n"
    keep, seen = np.zeros(len(d), bool), {}
    for i in np.lexsort((np.arange(len(d)), d)):
        for name in set(rows[i][:2]):
            if seen.get(name, 0) < 3:
                keep[i] = True
            seen[name] = seen.get(name, 0) + 1
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "top.tsv", "--hll-bias-sim", "--top", "3"], env)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "top.tsv").read_text() == "\n".join([lines[0]] + [ln for ln, x in zip(lines[1:-1], keep) if x]) + "\n"
    names = []
    for a, _, _ in rows:
        if a not in names:
            names.append(a)
    pos = {a: i for i, a in enumerate(names)}
    edges = [(pos[a], pos[b]) for a, b, _ in _rows(cut) if a != b]
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "cl.tsv", "--hll-bias-sim", "--cluster", "0.1"], env)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "cl.tsv").read_text() == _members_text(names, _components(n, edges))
    near = [set() for _ in names]
    for a, b in edges:
        near[max(a, b)].add(min(a, b))
    rep = []
    for i in range(n):
        rep.append(next((j for j in sorted(near[i]) if rep[j] == j), i))
    r = _run(tmp_path, ["dist", "-q", "sm", "-r", "sm", "-o", "dr.tsv", "--hll-bias-sim", "--derep", "0.1"], env)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "dr.tsv").read_text() == _members_text(names, rep)
    assert len(set(rep)) < n
    # hmh sketches: the flag changes nothing and says nothing
    r = _run(tmp_path, ["sketch", "-f", "l.txt", "-o", "hm", "-k", "16"], env)
    assert r.returncode == 0, r.stderr
    plain = _run(tmp_path, ["dist", "-q", "hm", "-r", "hm", "-o", "hm_plain.tsv"], env)
    sim = _run(tmp_path, ["dist", "-q", "hm", "-r", "hm", "-o", "hm_sim.tsv", "--hll-bias-sim"], env)
    assert plain.returncode == 0 and sim.returncode == 0, sim.stderr
    assert (tmp_path / "hm_plain.tsv").read_bytes() == (tmp_path / "hm_sim.tsv").read_bytes()
    assert "hll-bias-sim" not in sim.stderr and "simulated" not in sim.stderr
