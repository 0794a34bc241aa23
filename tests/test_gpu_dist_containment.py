"""`lash dist --containment query|reference`: the Mash distance of the containment fraction
    frac_c = s/(1+s) * (a_r + a_q) / den,   den = a_q (query) or a_r (reference),   s <= 0 -> d = 1,   frac_c >= 1 -> d = +0
(lash_amd/csrc/dist_pair.h) instead of the Jaccard-derived 2s/(1+s), on every rectangular route: all pairs, --max-dist, --top.
Expected values: tests/pyref.py's similarities and cardinalities through the restatement of the rule below (_restated), to the
tolerance tests/test_gpu_dist.py uses for the Jaccard distance; the filtered routes against the unfiltered run's bytes."""
import glob
import json
import math
import os
import subprocess

import numpy as np
import pytest

import host_lib as H
import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
TOL, TOL_FP32 = 1.1e-6, 2e-6                       # tests/test_gpu_dist.py: the 6-decimal print; the same in f32
DIRECTIONS = ("query", "reference")
CONFIGS = {                                        # sketch arguments, k, p, dist flags
    "hmh": (["-k", "16"], 16, 0, []),
    "hll": (["-k", "21", "-a", "hll", "-p", "10"], 21, 10, []),
    "ull-fgra": (["-k", "16", "-a", "ull", "-p", "12"], 16, 12, ["-e", "fgra"]),
    "ull-ml": (["-k", "16", "-a", "ull", "-p", "12"], 16, 12, ["-e", "ml"]),
}


def _restated(sim, a_r, a_q, k, model, direction, ull=False):
    """the rule: the similarity's clamp (hmh / hll drop a NaN to 0, ull keeps it), s <= 0 -> 1 before any ratio, the fraction in the
    association (s / (1 + s)) * ((a_r + a_q) / den), frac_c >= 1 -> +0, else the model's distance"""
    if ull:
        sim = 0.0 if sim < 0.0 else sim
    elif not sim >= 0.0:
        sim = 0.0
    if sim <= 0.0:
        return 1.0
    den = a_q if direction == "query" else a_r
    frac = float(np.float64(sim) / (1.0 + np.float64(sim)) * ((np.float64(a_r) + np.float64(a_q)) / np.float64(den)))
    if frac >= 1.0:
        return 0.0
    if frac != frac:
        return 1.0 if model == 1 else frac
    return min(-math.log(frac) / k, 1.0) if model == 1 else 1.0 - frac ** (1.0 / k)


def _mutated(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    idx = rng.random(len(seq)) < rate
    out[idx] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(idx.sum()))
    return out


def _run(cwd, args, env=None):
    return subprocess.run([H.CLI] + args, cwd=cwd, capture_output=True, text=True, env=env or dict(os.environ), timeout=600)


def _ok(cwd, args, env=None):
    r = _run(cwd, args, env)
    assert r.returncode == 0, (args, r.stderr)
    return r


def _write(cwd, name, genome):
    path = cwd / name
    path.write_bytes(b">s\n" + genome.tobytes() + b"\n")
    return str(path)


def _sketch(cwd, prefix, paths, sk_args, env=None):
    (cwd / (prefix + ".txt")).write_text("\n".join(paths) + "\n")
    _ok(cwd, ["sketch", "-f", prefix + ".txt", "-o", prefix] + sk_args, env)


def _dist(cwd, q, r, out, flags, env=None):
    _ok(cwd, ["dist", "-q", q, "-r", r, "-o", out] + flags, env)
    text = (cwd / out).read_text()
    assert text.startswith("Reference\tQuery\tDistance\n") and "\t-" not in text          # no negative zero, no negative distance
    return text


def _rows(text):
    return [tuple(ln.split("\t")) for ln in text.split("\n")[1:-1]]


def _image(algo, k, p, genome):
    return O.sketch_genomes({"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}[algo], k, p, 42, genome, np.array([0, len(genome)], np.uint64),
                            np.array([0, 1], np.uint64))[0].tobytes()


class _Reference:
    """cardinalities and similarities of sketch images from tests/pyref.py, each computed once"""

    def __init__(self, config, tables=None):
        self.algo = config.split("-")[0]
        self.est = R.ull_ml if config == "ull-ml" else R.ull_fgra
        _, self.k, self.p, _ = CONFIGS.get(config, (None, 21, 14, None))
        self.tables = tables
        self.ull = self.algo == "ull"
        self._card, self._sim = {}, {}

    def card(self, img):
        if img not in self._card:
            self._card[img] = (R.hmh_cardinality(img) if self.algo == "hmh" else R.hll_len_from_regs(self.p, img[33:], self.tables) if self.algo == "hll"
                               else self.est(list(img[8:]), self.p))
        return self._card[img]

    def sim(self, ref, qry):
        if (ref, qry) not in self._sim:
            if self.algo == "hmh":
                s = R.hmh_similarity(qry, ref)
            elif self.algo == "hll":
                s = R.hll_similarity(self.p, ref, qry, self.tables)
            else:
                u = self.est(list(R.ull_merge(ref[8:], qry[8:])), self.p)
                s = (self.card(ref) + self.card(qry) - u) / u if u else float("nan")
            self._sim[(ref, qry)] = s
        return self._sim[(ref, qry)]

    def frac(self, ref, qry, direction):
        s = self.sim(ref, qry)
        return s / (1.0 + s) * ((self.card(ref) + self.card(qry)) / (self.card(qry) if direction == "query" else self.card(ref))) if s > 0 else 0.0

    def distance(self, ref, qry, model, direction):
        return _restated(self.sim(ref, qry), self.card(ref), self.card(qry), self.k, model, direction, self.ull)


# ---- the nested genomes: A (40 kbp), B = A + 120 kbp, C unrelated, E shorter than k, S: one name, two sequences --------------------------

@pytest.fixture(scope="module")
def nested(tmp_path_factory):
    cwd = tmp_path_factory.mktemp("nested")
    a = O.synth_genome(501, 40_000)
    genomes = {"a.fa": a, "b.fa": np.concatenate([a, O.synth_genome(502, 120_000)]), "c.fa": O.synth_genome(503, 60_000),
               "e.fa": np.frombuffer(b"ACGTACG", np.uint8).copy(), "s.fa": _mutated(a, 0.03, 7)}
    s_again = _mutated(a, 0.10, 8)                                      # s.fa as the queries see it
    xnames, ynames = ["a.fa", "b.fa", "c.fa", "e.fa", "s.fa"], ["a.fa", "b.fa", "s.fa"]
    paths = {n: _write(cwd, n, g) for n, g in genomes.items()}
    for config, (sk, _, _, _) in CONFIGS.items():
        if config != "ull-ml":
            _sketch(cwd, "X" + config[:3], [paths[n] for n in xnames], sk)
    _write(cwd, "s.fa", s_again)
    for config, (sk, _, _, _) in CONFIGS.items():
        if config != "ull-ml":
            _sketch(cwd, "Y" + config[:3], [paths[n] for n in ynames], sk)
    refs, imgs = {}, {}

    def world(config):
        """(reference, {path: image} of the X side, {path: image} of the Y side)"""
        if config not in refs:
            _, k, p, _ = CONFIGS[config]
            algo = config.split("-")[0]
            refs[config] = _Reference(config)
            if algo not in imgs:
                x = {paths[n]: _image(algo, k, p, genomes[n]) for n in xnames}
                y = {paths[n]: (_image(algo, k, p, s_again) if n == "s.fa" else x[paths[n]]) for n in ynames}
                imgs[algo] = (x, y)
        return (refs[config],) + imgs[config.split("-")[0]]

    return cwd, paths, world


def _check_values(text, ref, rimg, qimg, model, direction, tol):
    rows = _rows(text)
    assert len(rows) == len(rimg) * len(qimg)
    for a, b, d in rows:
        want = 0.0 if a == b else ref.distance(rimg[a], qimg[b], model, direction)
        assert abs(float(d) - want) <= tol, (a, b, d, want)
        if a == b or want == 0.0:
            assert d == "0.000000", (a, b, d)
    return {(a, b): d for a, b, d in rows}


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("model", [1, 0])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_values(nested, config, model, fp32):
    cwd, paths, world = nested
    ref, ximg, yimg = world(config)
    pre = config[:3]
    flags = CONFIGS[config][3] + ["-m", str(model)] + (["--fp32"] if fp32 else [])
    plain = _rows(_dist(cwd, "Y" + pre, "X" + pre, "plain.tsv", flags))
    for direction in DIRECTIONS:
        text = _dist(cwd, "Y" + pre, "X" + pre, "c.tsv", flags + ["--containment", direction])
        got = _check_values(text, ref, ximg, yimg, model, direction, TOL_FP32 if fp32 else TOL)
        assert [r[:2] for r in _rows(text)] == [r[:2] for r in plain]                       # the rectangular run's rows and columns
        a, b, c, e, s = (paths[n] for n in ("a.fa", "b.fa", "c.fa", "e.fa", "s.fa"))
        assert got[(s, s)] == "0.000000" and got[(a, a)] == "0.000000"                    # same name, whatever the sketches are
        assert got[(e, a)] == got[(e, b)] == "1.000000"                                   # a sketch of nothing shares nothing
        # C is unrelated: 1 wherever the estimators see no shared k-mer.  (Where the union estimate falls short of a_r + a_q by chance,
        # 3 % standard error at hll p = 10, the pair prints the distance of that excess, which _check_values has compared.)
        for pair in ((c, a), (c, b)):
            if ref.distance(ximg[pair[0]], yimg[pair[1]], model, direction) == 1.0:
                assert got[pair] == "1.000000"
        # A in B: frac_c is 1 up to the estimator's noise; where it reaches 1 the distance is 0, and it is far below the Jaccard one
        inside = (b, a) if direction == "query" else (a, b)
        if ref.frac(ximg[inside[0]], yimg[inside[1]], direction) >= 1.0:
            assert got[inside] == "0.000000"
        jac = float(dict((r[:2], r[2]) for r in plain)[inside])
        assert float(got[inside]) < 0.01 and jac > 0.03
        assert float(got[inside[::-1]]) > jac                                                # B in A: a quarter of it


def test_same_files_print_the_full_square(nested):
    cwd, paths, world = nested
    ref, ximg, _ = world("hll")
    order = R.hashbrown_name_order(list(ximg))
    names = list(ximg)
    for direction in DIRECTIONS:
        text = _dist(cwd, "Xhll", "Xhll", "sq.tsv", ["--containment", direction])
        _check_values(text, ref, ximg, ximg, 1, direction, TOL)
        assert [r[:2] for r in _rows(text)] == [(names[i], names[j]) for i in order for j in order]
        fo = _dist(cwd, "Xhll", "Xhll", "sqfo.tsv", ["--containment", direction, "--file-order", "--block-rows", "2", "-t", "3"])
        assert [r[:2] for r in _rows(fo)] == [(x, y) for x in names for y in names] and sorted(_rows(fo)) == sorted(_rows(text))
    tri = _dist(cwd, "Xhll", "Xhll", "tri.tsv", [])
    assert len(_rows(tri)) == 15                                                          # the default on the same files is still the triangle


@pytest.mark.parametrize("config,flags", [("hmh", []), ("hll", ["-m", "0"]), ("ull-fgra", ["--fp32"]), ("ull-ml", ["-m", "0", "--fp32", "--file-order"])])
def test_direction_symmetry_is_exact(nested, config, flags):
    cwd, _, _ = nested
    pre = config[:3]
    flags = CONFIGS[config][3] + flags
    for d1, d2 in (DIRECTIONS, DIRECTIONS[::-1]):
        one = _rows(_dist(cwd, "X" + pre, "Y" + pre, "s1.tsv", flags + ["--containment", d1]))
        two = _rows(_dist(cwd, "Y" + pre, "X" + pre, "s2.tsv", flags + ["--containment", d2]))
        assert len(one) == 15 and {"\t".join(r) for r in one} == {"\t".join((b, a, d)) for a, b, d in two}


@pytest.mark.parametrize("config,more", [("hmh", []), ("hll", ["-m", "0"]), ("ull-fgra", ["--fp32"]), ("ull-ml", ["-m", "0", "--fp32"])])
def test_copies_of_one_image_print_what_the_default_prints(tmp_path, config, more):
    """equal cardinalities: (a + a) / a is 2 exactly, so frac_c is the default's 2s/(1+s) bit for bit"""
    sk, _, _, flags = CONFIGS[config]
    g = O.synth_genome(601, 50_000)
    paths = [_write(tmp_path, "z%d.fa" % i, g) for i in range(4)]
    _sketch(tmp_path, "Z", paths, sk)
    _sketch(tmp_path, "W", paths, sk)                                   # the same names from other files: the default runs the rectangle
    want = _dist(tmp_path, "W", "Z", "want.tsv", flags + more)
    assert len(_rows(want)) == 16
    tri = {frozenset(r[:2]): r[2] for r in _rows(_dist(tmp_path, "Z", "Z", "tri.tsv", flags + more))}
    assert len(tri) == 10 and all(tri[frozenset(r[:2])] == r[2] for r in _rows(want))
    for direction in DIRECTIONS:
        assert _dist(tmp_path, "W", "Z", "got.tsv", flags + more + ["--containment", direction]) == want
    assert _dist(tmp_path, "Z", "Z", "got.tsv", flags + more + ["--containment", "query"]) == want


# ---- the HLL++ bias-table regime: unchanged ------------------------------------------------------------------------------------------------

def test_hll_table_regime_with_simulated_tables_and_refused_without(tmp_path):
    import lash_amd
    p, k = 14, 21
    env = dict(os.environ)
    env.pop("LASH_HLL_BIAS", None)
    base = O.synth_genome(701, 30_000)
    genomes = [base, np.concatenate([base, O.synth_genome(702, 30_000)]), O.synth_genome(703, 35_000)]
    paths = [_write(tmp_path, "t%d.fa" % i, g) for i, g in enumerate(genomes)]
    _sketch(tmp_path, "T", paths, ["-k", str(k), "-a", "hll", "-p", str(p)], env)
    ctx = lash_amd.Context(0)
    _, raw, bias = ctx.hll_bias_simulate(p)
    ctx.close()
    ref = _Reference("hll", tables={p: (raw.tolist(), bias.tolist())})
    ref.p = p
    imgs = {paths[i]: _image("hll", k, p, g) for i, g in enumerate(genomes)}
    assert all(R.hll_len_from_regs(p, im[33:]) is None for im in imgs.values())             # every sketch needs the tables
    for direction in DIRECTIONS:
        got = _check_values(_dist(tmp_path, "T", "T", "sim.tsv", ["--hll-bias-sim", "--containment", direction], env), ref, imgs, imgs, 1, direction, TOL)
        inside = (paths[1], paths[0]) if direction == "query" else (paths[0], paths[1])
        assert float(got[inside]) < 0.01 < float(got[inside[::-1]])
    # without tables: the run is refused as the default rectangle is, sketch or union
    r = _run(tmp_path, ["dist", "-q", "T", "-r", "T", "-o", "no.tsv", "--containment", "query"], env)
    assert r.returncode == 1 and "bias tables" in r.stderr
    small = [_write(tmp_path, "n%d.fa" % i, O.synth_genome(55 + i, 9_000 - 1_000 * i)) for i in range(2)]  # each in linear counting, their union not
    _sketch(tmp_path, "N", small[:1], ["-k", str(k), "-a", "hll", "-p", str(p)], env)
    _sketch(tmp_path, "M", small[1:], ["-k", str(k), "-a", "hll", "-p", str(p)], env)
    want = _run(tmp_path, ["dist", "-q", "M", "-r", "N", "-o", "no.tsv"], env)
    assert want.returncode == 1 and "union of" in want.stderr and "bias tables" in want.stderr
    for extra in ([], ["--max-dist", "0.2"], ["--top", "1"]):
        r = _run(tmp_path, ["dist", "-q", "M", "-r", "N", "-o", "no.tsv", "--containment", "reference"] + extra, env)
        assert (r.returncode, r.stderr) == (want.returncode, want.stderr), extra


# ---- the filters: 3 reference rows in blocks of 2, 1 030 query columns (one 1 024-column tile and a partial 64-lane word) ---------------

RATES = (0.0, 0.001, 0.002, 0.005, 0.01, 0.02)
N_QUERIES = 1030
D_CUT = 0.03                                       # above the containment distance of the nested family, below its Jaccard distance


def _sketch_files(cwd, prefix):
    import lash_amd
    files = {os.path.basename(f) for f in glob.glob(str(cwd / (prefix + "*")))}
    names = json.loads((cwd / next(f for f in files if f.endswith("files.json"))).read_text())
    raw = H.zstd_read(str(cwd / next(f for f in files if f.endswith(".bin"))))
    ib = lash_amd.image_bytes("hmh", 0)
    return names, np.frombuffer(raw[: len(names) * ib], np.uint8).reshape(len(names), ib)


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """references: r0 = the base of family 0 inside 8 kbp (the nested family), r1 = the base of family 1, r2 = a mutated base of family
    2; queries: four families of near-identical 2 kbp genomes (family 3 has no reference) and r1.fa again with another sequence"""
    import lash_amd
    cwd = tmp_path_factory.mktemp("families")
    bases = [O.synth_genome(800 + f, 2_000) for f in range(4)]
    rpaths = [_write(cwd, "r0.fa", np.concatenate([O.synth_genome(810, 3_000), bases[0], O.synth_genome(811, 3_000)])),
              _write(cwd, "r1.fa", bases[1]), _write(cwd, "r2.fa", _mutated(bases[2], 0.01, 812))]
    _sketch(cwd, "R", rpaths, ["-k", "16"])
    qpaths, fam = [], []
    for i in range(N_QUERIES - 1):
        f, rate = i % 4, RATES[(i // 4) % len(RATES)]
        qpaths.append(_write(cwd, "q%04d.fa" % i, bases[f] if rate == 0 else _mutated(bases[f], rate, 9000 + i)))
        fam.append(f)
    qpaths.insert(517, _write(cwd, "r1.fa", _mutated(bases[3], 0.002, 813)))
    fam.insert(517, 3)
    _sketch(cwd, "Q", qpaths, ["-k", "16"])
    rn, rimg = _sketch_files(cwd, "R")
    qn, qimg = _sketch_files(cwd, "Q")
    assert rn == rpaths and qn == qpaths
    ctx = lash_amd.Context(0)
    rs, qs = ctx.sketch_set("hmh", 0, rimg), ctx.sketch_set("hmh", 0, qimg)
    rc, qc = rs.cardinalities(), qs.cardinalities()
    rs.prepare(qs)
    st = rs.pair_block(0, rs.n, qry=qs)
    st["hmh_ec"] = rs.hmh_expected_collisions(0, rs.n, qry=qs)
    assert st["hmh_ec"] is not None
    cache = {}

    def unfiltered(flags):
        """(the unfiltered containment text, {(reference, query): d at full precision, same names 0}, the Jaccard text)"""
        from lash_amd.sketch import dist_rows
        key = tuple(flags)
        if key not in cache:
            model, fp32 = 0 if "0" in flags else 1, "--fp32" in flags
            d = dist_rows("hmh", 0, 16, model, rc, qc, fp32=fp32, containment="query", **st)
            full = {(a, b): (0.0 if a == b else float(d[i, j])) for i, a in enumerate(rn) for j, b in enumerate(qn)}
            cache[key] = (_dist(cwd, "Q", "R", "full_%d.tsv" % len(cache), flags + ["--containment", "query", "--block-rows", "2"]), full,
                          _dist(cwd, "Q", "R", "jac_%d.tsv" % len(cache), flags))
        return cache[key]

    yield cwd, rpaths, qpaths, fam, unfiltered, (rs, qs, rc, qc, st)
    rs.free()
    qs.free()
    ctx.close()


def _select(rows, full, K, D):
    """the rows in some query's K nearest: rank (printed d, position), per query; NaN never ranked; then d <= D"""
    d = np.array([full[r[:2]] for r in rows])
    keep, seen = np.zeros(len(rows), bool), {}
    for i in np.lexsort((np.arange(len(rows)), d)):
        if d[i] != d[i]:
            continue
        if seen.get(rows[i][1], 0) < K:
            keep[i] = D is None or d[i] <= D
        seen[rows[i][1]] = seen.get(rows[i][1], 0) + 1
    return keep


@pytest.mark.parametrize("devices", [[], ["--devices", "0,0"]])
@pytest.mark.parametrize("flags", [[], ["-m", "0", "--fp32"]])
def test_filters_print_the_unfiltered_bytes(families, flags, devices):
    cwd, rpaths, qpaths, fam, unfiltered, _ = families
    text, full, jac_text = unfiltered(flags)
    lines, rows = text.split("\n"), _rows(text)
    assert len(rows) == 3 * N_QUERIES
    # D separates the two measures on the nested family: the Jaccard predicate would drop every pair of r0 that containment keeps
    jac = {r[:2]: float(r[2]) for r in _rows(jac_text)}
    nested_pairs = [(rpaths[0], q) for q, f in zip(qpaths, fam) if f == 0]
    assert max(full[pr] for pr in nested_pairs) < D_CUT < min(jac[pr] for pr in nested_pairs) and len(nested_pairs) > 250
    assert all(abs(full[r[:2]] - float(r[2])) <= (TOL_FP32 if "--fp32" in flags else TOL) for r in rows)
    assert not any(abs(v - D_CUT) <= 1.5e-6 for v in full.values())                       # no row is ambiguous at 6 decimals
    common = flags + devices + ["--containment", "query", "--block-rows", "2"]
    got = _dist(cwd, "Q", "R", "cut.tsv", common + ["--max-dist", repr(D_CUT)])
    want = [ln for ln, r in zip(lines[1:-1], rows) if full[r[:2]] <= D_CUT]
    assert got == "\n".join(lines[:1] + want) + "\n"
    assert sum(1 for ln in want if ln.startswith(rpaths[0] + "\t")) == len(nested_pairs)
    assert (rpaths[1] + "\t" + rpaths[1] + "\t0.000000") in want                          # the same name: 0, kept
    for K, D in ((3, None), (3, D_CUT), (1, None), (2, D_CUT)):
        got = _dist(cwd, "Q", "R", "top.tsv", common + ["--top", str(K)] + ([] if D is None else ["--max-dist", repr(D)]))
        keep = _select(rows, full, K, D)
        assert got == "\n".join(lines[:1] + [ln for ln, k in zip(lines[1:-1], keep) if k]) + "\n", (K, D)
        if K == 3 and D is None:
            assert got == text


def _restated_block(st, rc, qc, k, model, direction):
    """the block's distances from its pair statistics: hyperminhash's similarity (c - ec) / n, then _restated"""
    c, n, ec = st["c_or_zero"].astype(np.float64), st["n_counts"].astype(np.float64), st["hmh_ec"]
    d = np.empty(c.shape)
    for i in range(c.shape[0]):
        for j in range(c.shape[1]):
            sim = 0.0 if c[i, j] == 0 or c[i, j] < ec[i, j] else (c[i, j] - ec[i, j]) / n[i, j]
            d[i, j] = _restated(sim, rc[i], qc[j], k, model, direction)
    return d


@pytest.mark.parametrize("model,fp32", [(1, False), (0, True)])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_abi_candidates_are_within_the_margin(families, direction, model, fp32):
    from lash_amd.sketch import dist_rows
    _, _, _, _, _, (rs, qs, rc, qc, st) = families
    d = dist_rows("hmh", 0, 16, model, rc, qc, fp32=fp32, containment=direction, **st)
    rest = _restated_block(st, rc, qc, 16, model, direction)
    assert np.all(np.abs(d - rest) <= (2e-7 if fp32 else 1e-14))                            # (f32 arithmetic of a d <= 1: a few 2^-24)
    jac = dist_rows("hmh", 0, 16, model, rc, qc, fp32=fp32, **st)
    margin = 2.0 ** -16 if fp32 else 2.0 ** -40
    for D in (0.0, 0.01, D_CUT, 0.2, 1.0):
        for r0, r1 in ((0, 3), (1, 3)):
            stats = {}
            row, col, dist = rs.pair_block_within(r0, r1, D, 16, qry=qs, model=model, fp32=fp32, stats=stats, containment=direction)
            wr, wc = np.nonzero(d[r0:r1] <= D)
            assert np.array_equal(row, wr.astype(np.uint32) + np.uint32(r0)) and np.array_equal(col, wc.astype(np.uint32))
            assert np.array_equal(dist.view(np.uint64), d[r0:r1][wr, wc].view(np.uint64))
            # hmh: the device places every pair, so the candidates are at most the pairs within twice the margin of D
            assert stats["n_kept"] == len(wr) <= stats["n_candidates"] <= int(np.count_nonzero(rest[r0:r1] <= D + 2 * margin))
    if direction == "query":
        assert np.count_nonzero(d <= D_CUT) > np.count_nonzero(jac <= D_CUT) + 250         # the nested family: another predicate
    # --top through the ABI: every pair of each column's K nearest comes back, with the same distances
    K = 2
    row, col, dist = rs.pair_block_top(0, 3, K, 16, qry=qs, model=model, fp32=fp32, containment=direction)
    got = {(int(r), int(c)): v for r, c, v in zip(row, col, dist)}
    for j in range(qs.n):
        for i in sorted(range(3), key=lambda i: (d[i, j], i))[:K]:
            assert got[(i, j)] == d[i, j]


def test_abi_refuses_a_triangle(families):
    import lash_amd
    from lash_amd import _lib
    _, _, _, _, _, (rs, qs, rc, qc, st) = families
    for direction in DIRECTIONS:
        for call in (lambda **kw: rs.pair_block_within(0, 3, 0.1, 16, **kw), lambda **kw: rs.pair_block_top(0, 3, 2, 16, **kw)):
            with pytest.raises(lash_amd.LashError) as e:
                call(n_cols=3, triangle=True, containment=direction)
            assert e.value.code == _lib.EINVAL
            with pytest.raises(lash_amd.LashError) as e:
                call(qry=qs, triangle=True, containment=direction)
            assert e.value.code == _lib.EINVAL
            call(n_cols=3, triangle=True)                                                   # the default measure takes the triangle as before
            call(qry=qs, containment=direction)
