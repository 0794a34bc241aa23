"""GPU tests of the k-mer abundance filter (`lash sketch --min-count`) past one tile and one slice: kmer_count_kernel / kmer_keep_kernel
(kmer_filter.hip) and the KEEP form of sketch_kernel on files of several work items and tiles, whole wave tiles kept and dropped, single-record
FASTA, the last k-mer start on lane / tile / slice edges, non-default layouts, tables of different sizes in one filter, a keep buffer reused
after a larger call, more files than one grid row and a file longer than one trip of the filter kernels' grid stride.

The reference is tests/min_count_model.py (keys, cells and the kept set in numpy; the expected image is the oracle's sketch of one k-base record
per kept key).  Every comparison is exact: cells byte for byte, images byte for byte.  The k-mer census of a filtered call
(Context.timing()["kmers"]) counts the kept occurrences only, and case A holds it to the model.

test_gpu_min_count.py checks the same route on three 20 kb files; its cases are not repeated here.

Not reachable, so not tested: the filter kernels' `multi_rec == false` branch.  The filter takes raw files only, whose format field is never 0, so a
single-record FASTA walks its (all-zero) record-start bitmap like any other file; test_single_record_fasta holds that path to the model."""
import functools

import numpy as np
import pytest

import lash_amd
import min_count_model as MC
import oracle_lib as O

gpu = pytest.mark.gpu
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
SEED = 42
TYPES = [("hmh", 16, 0), ("hll", 21, 10), ("ull", 32, 12)]
# (codes=ACTG is the one whose complement is NOT the bitwise NOT of a code: A ^ T = 2, where every other spec here has 3)
LAYOUT_SPECS = ["kmer=lsb", "codes=TGCA,kmer=lsb", "hmh_x=low,hmh_reg=be,hmh_hdr=l", "hll_bucket=high,hll_hdr=pzsal", "codes=ACTG",
                "codes=GATC,ull_hdr=,hmh_hdr=Q,hll_bucket=high,kmer=lsb"]
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.zeros(256, np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def bases(rng, n):
    return _ACGT[rng.integers(0, 4, n)]


def revcomp(seq):
    return _COMP[seq[::-1]]


def wrapped(seq, width=70):
    """the lines of one record"""
    full = len(seq) // width
    body = np.empty((full, width + 1), np.uint8)
    body[:, :width] = seq[:full * width].reshape(full, width)
    body[:, width] = 10
    rest = seq[full * width:]
    return body.tobytes() + (rest.tobytes() + b"\n" if len(rest) else b"")


def fasta(records, width=70):
    return b"".join(b">r%d\n" % i + wrapped(r, width) for i, r in enumerate(records))


@functools.lru_cache(maxsize=None)
def genome():
    return bases(np.random.default_rng(1), 300_000)


@functools.lru_cache(maxsize=None)
def records_a():
    """case A: G, and G with every other 20 000-base block replaced by fresh sequence"""
    g = genome()
    h = g.copy()
    rng = np.random.default_rng(2)
    for b in range(20_000, len(g), 40_000):
        h[b:b + 20_000] = bases(rng, 20_000)
    return g, h


@functools.lru_cache(maxsize=None)
def file_a():
    return fasta(records_a())


@functools.lru_cache(maxsize=None)
def file_both_strands():
    return fasta([genome(), revcomp(genome())])


@functools.lru_cache(maxsize=None)
def reads():
    return tuple(MC.read_files())


@functools.lru_cache(maxsize=None)
def keys_of(data, k, spec=None):
    return MC.file_keys(data, k, O.parse_layout(spec) if spec else None)


@functools.lru_cache(maxsize=None)
def expected(data, algo, k, p, L, M, spec=None):
    lay = O.parse_layout(spec) if spec else None
    return MC.expected_image(ALGO[algo], k, p, SEED, MC.kept_keys(keys_of(data, k, spec), L, M), layout=lay)


# ---- calls --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = lash_amd.Context(0)
    yield c
    c.set_layout(None)
    c.close()


def filtered(ctx, algo, k, p, files, Ls, M, cells=False):
    """count, then sketch with the keep rule -> (images, timing of the sketch call, cells per file or None)"""
    flt = ctx.kmer_filter(Ls)
    try:
        flt.count(k, files)
        got_cells = [flt.counts(g) for g in range(len(files))] if cells else None
        ctx.enable_timing(True)
        try:
            img = ctx.sketch_files_raw_filtered(algo, k, p, SEED, files, flt, M)
            tm = ctx.timing()
        finally:
            ctx.enable_timing(False)
        return img, tm, got_cells
    finally:
        flt.free()


def plan_slices(file_bytes, tile_words=2048):
    """(work items, words per item) of ONE file alone in a call, as plan_items cuts it: the file's 16-byte words rounded up to 4, slices of at
    most 8 tiles (the planner's minimum slice: a single file is far below the share of the chip that would ask for longer ones), and
    `per` = the words per slice rounded up to 4.  tile_words: 512 threads x 4 words, what a file above 100 kB gets."""
    nw = ((file_bytes + 15) // 16 + 3) & ~3
    ns = -(-nw // (8 * tile_words))
    per = (-(-nw // ns) + 3) & ~3
    return -(-nw // per), per


# ---- the model, without a GPU -------------------------------------------------------------------------------------------------------
def _slow_keys(rec, k, lay):
    """one k-mer at a time with Python integers"""
    code = {c: int(lay.base_code[i]) for i, c in enumerate("ACGT")}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    s = "".join(c for c in rec.decode() if c in code)
    out = []
    for i in range(len(s) - k + 1):
        km = s[i:i + k]
        rc = "".join(comp[c] for c in reversed(km))
        vals = []
        for t in (km, rc):
            v = 0
            for j, c in enumerate(t):
                v |= code[c] << (2 * j if lay.kmer_lsb_first else 2 * (k - 1 - j))
            vals.append(v)
        out.append(min(vals))
    return np.array(out, np.uint64)


def test_model_matches_the_oracle():
    """default layout: the keys are the oracle's record_kmers; every layout: the keys are those of a k-mer-at-a-time restatement, and the oracle's
    sketch of a file is its sketch of one k-base record per distinct key (M = 1 keeps everything)"""
    recs = MC.fastx_records(reads()[0])
    for k in (14, 16, 21, 32):
        for rec in recs[:40]:
            want = O.record_kmers(rec, k)
            assert np.array_equal(MC.record_keys(rec, k), want)
            assert np.array_equal(MC.record_keys(rec, k, O.default_layout()), want)
    for spec in LAYOUT_SPECS:
        lay = O.parse_layout(spec)
        for k in (14, 16, 21, 32):
            assert np.array_equal(MC.record_keys(recs[3], k, lay), _slow_keys(recs[3], k, lay)), (spec, k)
        for algo, k, p in TYPES:
            keys = MC.file_keys(reads()[1], k, lay)
            assert np.array_equal(MC.expected_image(ALGO[algo], k, p, SEED, np.unique(keys), layout=lay),
                                  O.sketch_files(ALGO[algo], k, p, SEED, [reads()[1]], layout=lay)[0]), (spec, algo)
    keys = MC.file_keys(reads()[2], 16)
    for L, M in ((10, 2), (14, 2), (24, 3)):
        c1, c2 = MC.occurrence_cells(keys, L)
        assert MC.kept_occurrences(keys, L, M) == sum(1 for a, b in zip(c1.tolist(), c2.tolist()) if min(a, b) >= M)
        assert MC.kept_occurrences(keys, L, M) == int(np.isin(keys, MC.kept_keys(keys, L, M)).sum())
    assert MC.keys_fasta(np.array([0x1B, 0xE4], np.uint64), 4) == b">k\nACGT\n>k\nTGCA\n"


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("algo,k,p", TYPES + [("hll", 14, 10), ("hmh", 11, 0), ("ull", 11, 12)])   # (every algorithm at k < 16 too)
def test_two_slices_long_kept_and_dropped_runs(ctx, algo, k, p):
    """A: a 608 kB FASTA of two records (G, and G with alternate 20 000-base blocks replaced) is cut into several work items of several tiles;
    with M = 2 the shared blocks are kept whole (more than 3 x 4 096 positions: some wave tile is all kept, the all_valid branch under KEEP)
    and the replaced blocks are dropped but for collisions (L = 22).  Cells, image, and the census = the kept occurrences."""
    L, M = 22, 2
    f = file_a()
    keys = keys_of(f, k)
    kept_n = MC.kept_occurrences(keys, L, M)
    true_n = int(np.isin(keys, MC.true_keys(keys, M)).sum())
    assert 300_000 < true_n < kept_n < len(keys) - 200_000                 # long kept runs, long dropped runs, and collisions
    img, tm, cells = filtered(ctx, algo, k, p, [f], [L], M, cells=True)
    assert np.array_equal(cells[0], MC.cells_dense(keys, L))
    assert np.array_equal(img[0], expected(f, algo, k, p, L, M))
    assert tm["sketch_workgroups"] > 1, tm
    assert tm["kmers"] == kept_n, (tm["kmers"], kept_n, len(keys))


# ---- B ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("algo,k,p", TYPES)
def test_both_strands_are_one_key(ctx, algo, k, p):
    """B (i): G and its reverse complement as two records: every key occurs twice, M = 2 keeps everything whatever collides"""
    f = file_both_strands()
    img, tm, _ = filtered(ctx, algo, k, p, [f], [24], 2)
    want = ctx.sketch_files_raw(algo, k, p, SEED, [f])
    assert np.array_equal(want[0], O.sketch_files(ALGO[algo], k, p, SEED, [f])[0])
    assert np.array_equal(img, want)
    assert tm["sketch_workgroups"] > 1 and tm["kmers"] == 2 * (300_000 - k + 1), tm


@gpu
@pytest.mark.parametrize("algo,k,p", TYPES)
def test_single_record_fasta(ctx, algo, k, p):
    """B (ii): G followed by G in ONE record (the filter kernels' multi_rec == false branch): the k - 1 k-mers across the joint occur once"""
    f = fasta([np.concatenate([genome(), genome()])])
    keys = keys_of(f, k)
    img, tm, cells = filtered(ctx, algo, k, p, [f], [24], 2, cells=True)
    assert np.array_equal(cells[0], MC.cells_dense(keys, 24))
    assert np.array_equal(img[0], expected(f, algo, k, p, 24, 2))
    assert tm["sketch_workgroups"] > 1 and tm["kmers"] == MC.kept_occurrences(keys, 24, 2), tm
    assert len(keys) - (k - 1) <= tm["kmers"] <= len(keys)                 # all but the joint (a joint k-mer may collide its way in)


# ---- C ------------------------------------------------------------------------------------------------------------------------------
SLICED_FILE_BYTES = 300_000


def edge_file(form, n_bases, file_bytes=None):
    """n_bases surviving bases as one record G|G, or as two records G1|G1 and G2|G2 (the last one cut to fit); file_bytes: the file padded to
    exactly that size with lines of N behind the last base (deleted bytes: the planner cuts by the file's size, the kernels walk the bases)"""
    rng = np.random.default_rng(n_bases)

    def doubled(n):
        g = bases(rng, (n + 1) // 2)
        return np.concatenate([g, g])[:n]
    recs = [doubled(n_bases)] if form == "single" else [doubled(40_022), doubled(n_bases - 40_022)]
    f = fasta(recs)
    if file_bytes is not None:
        pad = file_bytes - len(f)
        assert pad > 100
        if pad % 71 == 1:                                                  # (the last line would be a lone line end)
            f += b"N" * 35 + b"\n"
            pad -= 36
        lines, rest = divmod(pad, 71)
        f += (b"N" * 70 + b"\n") * lines + (b"N" * (rest - 1) + b"\n" if rest else b"")
        assert len(f) == file_bytes
    return f


@gpu
@pytest.mark.parametrize("algo,k,p", [("hmh", 16, 0), ("ull", 32, 12)])
@pytest.mark.parametrize("edge", ["lane", "tile", "slice"])
@pytest.mark.parametrize("form", ["single", "two"])
def test_last_kmer_on_an_edge(ctx, form, edge, algo, k, p):
    """C: the last k-mer start (surviving bases - k) one before, on and one after a multiple of 64 (a lane's positions), of 32 768 (a
    workgroup tile) and the first slice boundary.  The boundary is derived from the planner's rule (plan_slices) for a file of
    SLICED_FILE_BYTES, and the call's sketch_workgroups must confirm the number of slices that rule gives.  k = 16 and k = 32: one and two
    look-ahead words.  Records are G|G, M = 2 keeps all but the joints; the expectation is the model's."""
    n_items, per = (1, 0)
    file_bytes = None
    if edge == "lane":
        at = 64 * 1031
    elif edge == "tile":
        at = 4 * 32768
    else:
        file_bytes = SLICED_FILE_BYTES
        n_items, per = plan_slices(file_bytes)
        assert n_items == 2
        at = per * 16
    for d in (-1, 0, 1):
        f = edge_file(form, at + d + k, file_bytes)
        assert plan_slices(len(f))[0] == n_items
        keys = keys_of(f, k)
        assert len(keys) == at + d + 1 - (0 if form == "single" else k - 1)
        img, tm, cells = filtered(ctx, algo, k, p, [f], [24], 2, cells=True)
        assert tm["sketch_workgroups"] == n_items, (tm, n_items)
        assert np.array_equal(cells[0], MC.cells_dense(keys, 24)), (form, edge, d)
        assert np.array_equal(img[0], expected(f, algo, k, p, 24, 2)), (form, edge, d)
        assert tm["kmers"] == MC.kept_occurrences(keys, 24, 2), (form, edge, d, tm)


# ---- D ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("spec", LAYOUT_SPECS)
def test_layouts_on_reads(ctx, spec):
    """D: the key is the canonical k-mer under the context's layout (its base codes, kmer=lsb): cells and images of the read files at
    L = 14, M = 2 against the layout-aware model.  Under kmer=lsb and under the combined spec the cells must differ from the default
    layout's, so a model (or a kernel) that ignored the layout could not pass; codes=ACTG is the spec whose complement mask differs."""
    files = list(reads())
    ctx.set_layout(spec)
    try:
        for algo, k, p in TYPES:
            img, _, cells = filtered(ctx, algo, k, p, files, [14] * 3, 2, cells=True)
            for g, f in enumerate(files):
                model = MC.cells_dense(keys_of(f, k, spec), 14)
                assert np.array_equal(cells[g], model), (spec, k, g)
                if spec in ("kmer=lsb", "codes=ACTG", LAYOUT_SPECS[-1]):
                    assert not np.array_equal(model, MC.cells_dense(keys_of(f, k), 14))
                elif spec == "codes=TGCA,kmer=lsb":                        # (lsb-first under the complemented codes IS the default key)
                    assert np.array_equal(model, MC.cells_dense(keys_of(f, k), 14))
                assert np.array_equal(img[g], expected(f, algo, k, p, 14, 2, spec)), (spec, algo, g)
    finally:
        ctx.set_layout(None)


@gpu
@pytest.mark.parametrize("spec", LAYOUT_SPECS)
def test_layouts_on_a_sliced_file(ctx, spec):
    """D: case A's file under each layout, images only: the x = low / bucket = high variants of the filtered launch on several work items —
    each variant at k < 16, k = 16 and k > 16 under the specs that select it"""
    cases = [("hmh", 16, 0), ("hll", 21, 10)]
    if "hmh_x=low" in spec:
        cases += [("hmh", 11, 0), ("hmh", 21, 0)]
    if "hll_bucket=high" in spec:
        cases += [("hll", 11, 10), ("hll", 16, 10)]
    ctx.set_layout(spec)
    try:
        for algo, k, p in cases:
            img, tm, _ = filtered(ctx, algo, k, p, [file_a()], [22], 2)
            assert tm["sketch_workgroups"] > 1
            assert np.array_equal(img[0], expected(file_a(), algo, k, p, 22, 2, spec)), (spec, algo)
    finally:
        ctx.set_layout(None)


# ---- E ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Ls", [(10, 24, 14), (24, 10, 10)])
def test_tables_of_different_sizes(ctx, Ls):
    """E: one filter, a table size per file: every file's cells sit at its own offset and nothing lands outside the cells the model fills"""
    files = list(reads())
    for algo, k, p in TYPES:
        img, _, cells = filtered(ctx, algo, k, p, files, list(Ls), 2, cells=True)
        for g, f in enumerate(files):
            model = MC.cells_dense(keys_of(f, k), Ls[g])
            assert len(cells[g]) == 1 << Ls[g] and not cells[g][model == 0].any(), (Ls, k, g)
            assert np.array_equal(cells[g], model), (Ls, k, g)
            assert np.array_equal(img[g], expected(f, algo, k, p, Ls[g], 2)), (Ls, algo, g)


# ---- F ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_keep_bits_of_an_earlier_call_are_not_seen():
    """F: the context's keep buffer is reused and never cleared.  After a call that set every keep bit of a 600 kb file (M = 1), the read files at
    M = 3 and a single 40-base read at M = 2 (nothing kept: the empty image) must give what a fresh context gives, and what the model says."""
    files = list(reads())
    one = b">one\n" + bases(np.random.default_rng(3), 40).tobytes() + b"\n"
    with lash_amd.Context(0) as used, lash_amd.Context(0) as fresh:
        for algo, k, p in TYPES:
            big, _, _ = filtered(used, algo, k, p, [file_both_strands()], [24], 1)
            assert np.array_equal(big, used.sketch_files_raw(algo, k, p, SEED, [file_both_strands()]))
            assert len(MC.kept_keys(keys_of(one, k), 24, 2)) == 0          # (2^24 cells: the read does not collide with itself)
            for fs, L, M in ((files, 24, 3), ([one], 24, 2)):
                got = filtered(used, algo, k, p, fs, [L] * len(fs), M)[0]
                assert np.array_equal(got, filtered(fresh, algo, k, p, fs, [L] * len(fs), M)[0]), (algo, M)
                for g, f in enumerate(fs):
                    assert np.array_equal(got[g], expected(f, algo, k, p, L, M)), (algo, M, g)
            assert np.array_equal(got[0], O.sketch_files(ALGO[algo], k, p, SEED, [b">empty\n"])[0])


# ---- G ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_more_files_than_one_grid_row(ctx):
    """G: 65 600 files (the filter kernels' grid has at most 65 535 rows and strides over the rest) of one 40-base read, 20 reads cycled; an
    odd-numbered file holds its read twice (two records: all kept at M = 2), an even-numbered one once (nothing kept, but for a read that
    collides with itself in 1 024 cells: the 40 distinct expectations come from the model).  hll k = 16 p = 4, L = 10.
    Measured on an MI355X: under 0.1 s for the whole test."""
    algo, k, p, L, M, n = "hll", 16, 4, 10, 2, 65_600
    rng = np.random.default_rng(4)
    rd = [bases(rng, 40).tobytes() for _ in range(20)]
    kinds = [b">a\n" + rd[i // 2] + b"\n" + (b">b\n" + rd[i // 2] + b"\n" if i % 2 else b"") for i in range(40)]
    want = np.stack([expected(f, algo, k, p, L, M) for f in kinds])
    empty = O.sketch_files(ALGO[algo], k, p, SEED, [b">empty\n"])[0]
    unfiltered = O.sketch_files(ALGO[algo], k, p, SEED, kinds)
    assert all(np.array_equal(want[i], unfiltered[i]) for i in range(1, 40, 2))
    assert sum(np.array_equal(want[i], empty) for i in range(0, 40, 2)) >= 15
    files = [kinds[i % 40] for i in range(n)]
    img, tm, _ = filtered(ctx, algo, k, p, files, [L] * n, M)
    assert np.array_equal(img, want[np.arange(n) % 40])
    assert tm["kmers"] == sum(MC.kept_occurrences(keys_of(files[i], k), L, M) for i in range(40)) * (n // 40)


# ---- H ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_file_past_one_trip_of_the_filter_grid(ctx):
    """H: a 17.5 Mbp genome and its reverse complement as two records, 35.5 MB: more k-mer starts than the 2 048 x 16 384 one trip of the filter
    kernels' grid covers, so the second trip of their stride counts and writes keep bits.  M = 2 keeps everything by construction (L = 28):
    the filtered image is the unfiltered one (hmh, hll) and the oracle's (hll).  The all-cells comparison is deliberately left out at this
    size (256 MiB of cells, a 35 M-key numpy model); instead the two cells of the first 4 096 keys of record 1 must each be >= 2.
    Measured on an MI355X: 0.6 s for the whole test (the oracle's 35 Mbp HyperLogLog sketch is most of it)."""
    n, L, M = 17_500_000, 28, 2
    assert 2 * n > 2048 * 16384 + 32768
    g = bases(np.random.default_rng(5), n)
    f = fasta([g, revcomp(g)])
    for algo, k, p in (("hll", 21, 12), ("hmh", 16, 0)):
        flt = ctx.kmer_filter([L])
        try:
            flt.count(k, [f])
            ctx.enable_timing(True)
            try:
                img = ctx.sketch_files_raw_filtered(algo, k, p, SEED, [f], flt, M)
                tm = ctx.timing()
            finally:
                ctx.enable_timing(False)
            cells = flt.counts(0)
        finally:
            flt.free()
        assert tm["kmers"] == 2 * (n - k + 1), tm
        assert np.array_equal(img, ctx.sketch_files_raw(algo, k, p, SEED, [f])), algo
        if algo == "hll":
            assert np.array_equal(img, O.sketch_files(ALGO[algo], k, p, SEED, [f]))
        i1, i2 = MC.cell_addresses(MC.record_keys(g[:4096 + k - 1].tobytes(), k), L)
        assert cells[i1.astype(np.int64)].min() >= 2 and cells[i2.astype(np.int64)].min() >= 2
        del cells


# ---- I ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_accumulate_across_a_sliced_file(ctx):
    """I: case A's file in two chunks cut between its records, both counted into one filter, sketched one after the other with F_ACCUMULATE:
    the image of case A's single call"""
    L, M = 22, 2
    f = file_a()
    cut = f.index(b">r1\n")
    chunks = [f[:cut], f[cut:]]
    for algo, k, p in (("hmh", 16, 0), ("hll", 21, 10)):
        flt = ctx.kmer_filter([L])
        try:
            for c in chunks:
                flt.count(k, [c])
            assert np.array_equal(flt.counts(0), MC.cells_dense(keys_of(f, k), L))
            img = ctx.sketch_files_raw_filtered(algo, k, p, SEED, [chunks[0]], flt, M)
            img = ctx.sketch_files_raw_filtered(algo, k, p, SEED, [chunks[1]], flt, M, flags=lash_amd.F_ACCUMULATE, out=img)
        finally:
            flt.free()
        assert np.array_equal(img[0], expected(f, algo, k, p, L, M)), algo
