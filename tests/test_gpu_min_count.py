"""GPU tests of the k-mer abundance filter (`lash sketch --min-count`; lash_kmer_filter_*, lash_sketch_files_raw_filtered; kmer_filter.hip
and the KEEP form of sketch_kernel).  The reference is tests/min_count_model.py: keys, cells and the kept set in numpy, the expected image from the
oracle's sketch of one k-base record per kept key.  Every comparison is exact: cells byte for byte, images byte for byte."""
import functools

import numpy as np
import pytest

import lash_amd
import min_count_model as MC
import oracle_lib as O

pytestmark = pytest.mark.gpu
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
SEED = 42
CASES = [("hmh", 16, 0), ("hll", 21, 10), ("ull", 32, 12), ("hll", 14, 10)]


@pytest.fixture(scope="module")
def ctx():
    c = lash_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reads():
    return tuple(MC.read_files())


@functools.lru_cache(maxsize=None)
def keys_of(k):
    return tuple(MC.file_keys(f, k) for f in reads())


@functools.lru_cache(maxsize=None)
def expected(algo, k, p, L, M):
    return np.stack([MC.expected_image(ALGO[algo], k, p, SEED, MC.kept_keys(keys, L, M)) for keys in keys_of(k)])


def filtered(ctx, algo, k, p, files, L, M, flags=0):
    flt = ctx.kmer_filter([L] * len(files))
    try:
        flt.count(k, files)
        return ctx.sketch_files_raw_filtered(algo, k, p, SEED, files, flt, M, flags=flags)
    finally:
        flt.free()


def test_model_keys_match_the_oracle():
    for k in (14, 16, 21, 32):
        for rec in MC.fastx_records(reads()[0])[:40]:
            assert np.array_equal(MC.record_keys(rec, k), O.record_kmers(rec, k))


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("algo,k,p", CASES)
def test_exact_without_collisions(ctx, algo, k, p, M):
    """shape 1: L = 24, no dropped key has both cells >= M, so the sketch holds exactly the keys with a true count >= M"""
    for keys in keys_of(k):
        assert np.array_equal(MC.kept_keys(keys, 24, M), MC.true_keys(keys, M))
        assert 0 < len(MC.true_keys(keys, M)) < len(np.unique(keys))
    got = filtered(ctx, algo, k, p, list(reads()), 24, M)
    assert np.array_equal(got, expected(algo, k, p, 24, M))


@pytest.mark.parametrize("L", [10, 14])
@pytest.mark.parametrize("algo,k,p,M", [("hmh", 16, 0, 2), ("hll", 21, 10, 3), ("ull", 32, 12, 2)])
def test_collisions_on_purpose(ctx, algo, k, p, M, L):
    """shape 2: L = 10 — thousands of k-mers in 1 024 cells, collisions let every k-mer through; L = 14 — some of the rare ones"""
    files = list(reads())
    flt = ctx.kmer_filter([L] * len(files))
    try:
        flt.count(k, files)
        for g, keys in enumerate(keys_of(k)):
            assert np.array_equal(flt.counts(g), MC.cells_dense(keys, L))
            kept, true = MC.kept_keys(keys, L, M), MC.true_keys(keys, M)
            assert np.all(np.isin(true, kept)) and len(kept) > len(true)
            assert L == 10 or len(kept) < len(np.unique(keys))
        got = ctx.sketch_files_raw_filtered(algo, k, p, SEED, files, flt, M)
    finally:
        flt.free()
    assert np.array_equal(got, expected(algo, k, p, L, M))


def test_saturation(ctx):
    """shape 3: a 2 000-base poly-A record: its cells stop at 255 exactly, nothing carries into the neighbouring cells"""
    k, L = 16, 16
    f = reads()[0] + b"@polyA\n" + b"A" * 2000 + b"\n+\n" + b"I" * 2000 + b"\n" + reads()[1]
    keys = MC.file_keys(f, k)
    a1, a2 = MC.cell_addresses(np.zeros(1, np.uint64), L)           # poly-A (and poly-T) is key 0
    assert a1[0] == a2[0] == 0
    model = MC.cells_dense(keys, L)
    assert model[0] == 255 and int(np.sum(keys == 0)) == 1985
    flt = ctx.kmer_filter([L])
    try:
        flt.count(k, [f])
        cells = flt.counts(0)
        assert cells[0] == 255 and np.array_equal(cells[1:4], model[1:4])
        assert np.array_equal(cells, model)
        got = ctx.sketch_files_raw_filtered("hmh", k, 0, SEED, [f], flt, 255)
    finally:
        flt.free()
    assert np.array_equal(MC.kept_keys(keys, L, 255), np.zeros(1, np.uint64))
    assert np.array_equal(got[0], MC.expected_image(O.HMH, k, 0, SEED, np.zeros(1, np.uint64)))


@pytest.mark.parametrize("algo,k,p", [("hmh", 16, 0), ("hll", 21, 10), ("ull", 32, 12)])
def test_files_are_counted_separately(ctx, algo, k, p):
    """shape 4: the same read once in each of two files, M = 2: nothing is kept in either"""
    rd = MC.fastx_records(reads()[0])[0]
    f = b"@r\n" + rd + b"\n+\n" + b"I" * len(rd) + b"\n"
    got = filtered(ctx, algo, k, p, [f, f], 20, 2)
    empty = O.sketch_files(ALGO[algo], k, p, SEED, [b">empty\n"])[0]
    assert np.array_equal(got[0], empty) and np.array_equal(got[1], empty)


@pytest.mark.parametrize("algo,k,p", CASES)
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_boundaries(ctx, algo, k, p, fmt):
    """shape 5: record lengths that put k-mer starts on word and 64-position edges, every record twice: M = 2 keeps everything"""
    import random
    rng = random.Random(5)
    recs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (16, 17, 63, 64, 65, 129)] * 2
    if fmt == "fasta":          # multi-line
        f = "".join(">s%d\n%s\n" % (i, "\n".join(r[j:j + 50] for j in range(0, len(r), 50))) for i, r in enumerate(recs)).encode()
    else:                       # CRLF
        f = "".join("@s%d\r\n%s\r\n+\r\n%s\r\n" % (i, r, "I" * len(r)) for i, r in enumerate(recs)).encode()
    want = ctx.sketch_files_raw(algo, k, p, SEED, [f])
    assert np.array_equal(want[0], O.sketch_files(ALGO[algo], k, p, SEED, [f])[0])
    assert np.array_equal(filtered(ctx, algo, k, p, [f], 24, 2), want)


@pytest.mark.parametrize("algo,k,p", CASES)
def test_min_count_one_is_the_unfiltered_sketch(ctx, algo, k, p):
    """shape 6"""
    files = list(reads())
    assert np.array_equal(filtered(ctx, algo, k, p, files, 16, 1), ctx.sketch_files_raw(algo, k, p, SEED, files))


def test_chunks_equal_the_whole(ctx):
    """shape 7: counting and sketching a file in two pieces cut between records gives the cells and the image of one call"""
    k, L, M = 21, 12, 2
    files = list(reads())
    halves = []
    for f in files:
        lines = f.split(b"\n")
        cut = 4 * (len(lines) // 8)
        halves.append((b"\n".join(lines[:cut]) + b"\n", b"\n".join(lines[cut:])))
    whole, parts = ctx.kmer_filter([L] * 3), ctx.kmer_filter([L] * 3)
    try:
        whole.count(k, files)
        parts.count(k, [h[0] for h in halves])
        parts.count(k, [h[1] for h in halves])
        for g in range(3):
            assert np.array_equal(parts.counts(g), whole.counts(g))
        for algo, p in (("hll", 10), ("hmh", 0)):
            one = ctx.sketch_files_raw_filtered(algo, k, p, SEED, files, whole, M)
            two = ctx.sketch_files_raw_filtered(algo, k, p, SEED, [h[0] for h in halves], parts, M)
            two = ctx.sketch_files_raw_filtered(algo, k, p, SEED, [h[1] for h in halves], parts, M, flags=lash_amd.F_ACCUMULATE, out=two)
            assert np.array_equal(one, two)
    finally:
        whole.free()
        parts.free()


def test_refusals(ctx):
    """shape 8"""
    files = list(reads())[:2]
    flt = ctx.kmer_filter([16, 16])
    try:
        flt.count(16, files)

        def refused(algo="hmh", k=16, p=0, fs=files, M=2, flags=0):
            with pytest.raises(lash_amd.LashError) as e:
                ctx.sketch_files_raw_filtered(algo, k, p, SEED, fs, flt, M, flags=flags)
            assert e.value.code == lash_amd.EINVAL
        refused(k=8, flags=lash_amd.F_AMINO)
        refused(fs=files[:1])
        refused(M=0)
        refused(M=256)
        refused(algo="hll", p=16)
        refused(algo="ull", p=15)
        refused(algo="ull", p=20)
        with pytest.raises(lash_amd.LashError) as e:
            flt.count(16, files[:1])
        assert e.value.code == lash_amd.EINVAL
        for bad in ([9], [37]):
            with pytest.raises(lash_amd.LashError) as e:
                ctx.kmer_filter(bad)
            assert e.value.code == lash_amd.EINVAL
        # the largest supported precisions are served
        assert ctx.sketch_files_raw_filtered("hll", 16, 15, SEED, files, flt, 2).shape == (2, 33 + (1 << 15))
        assert ctx.sketch_files_raw_filtered("ull", 16, 14, SEED, files, flt, 2).shape == (2, 8 + (1 << 14))
    finally:
        flt.free()
