"""`lash sketch --translate`: six-frame protein sketches of nucleotide FASTA.  The translated buffer, seg_off and rec_seg made on the GPU
(lash_fasta_translate[_device]) against the pure-Python model of the rule (tests/translate_model.py); the images of lash_sketch_translated
against the oracle's amino-acid image of the model's segments and against lash_sketch_batch with LASH_F_AMINO on the same arrays; proteins
encoded in a genome found in its sketch; and the command line against `lash sketch --aa` of the model's segments written one per record."""
import gzip
import json
import os
import random
import subprocess

import numpy as np
import pytest

import host_lib as H
import lash_amd
import oracle_lib as O
import translate_model as M

pytestmark = pytest.mark.gpu
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
CONFIGS = [("hmh", 0), ("hll", 12), ("ull", 10), ("ull", 18)]                    # (ull 18: a binned table)
KS = [1, 5, 7, 12]
TILE = 4096


def dna(seed, n):
    return O.synth_genome(seed, n).tobytes()


def lines(s, width, eol=b"\n"):
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width))


def offsets(files):
    return np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)


def small_records(n, seed=5):
    rng = random.Random(seed)
    g = dna(13, 400_000)
    return b"".join(b">r%d\n%s\n" % (i, g[s:s + rng.randint(30, 300)]) for i, s in ((i, rng.randrange(0, len(g) - 300)) for i in range(n)))


def edge_files(n_small=2_000, big=True):
    g = dna(17, 120_000)
    # output tiles (this file comes first, so its records' places in the translated buffer are known): a record of 2L + 2 = 4096 bytes, then
    # records whose frame 0 (n_0 residues and its terminator) ends exactly at a tile boundary, one byte before it and one byte after it, each
    # starting at a tile boundary thanks to the record before it
    out_tiles = b"".join(b">o%d L=%d\n" % (i, n) + lines(g[1000 * i:1000 * i + n], 60) for i, n in enumerate((2047, 12285, 2049, 12282, 4, 12288)))
    tiny = b"".join(b">L%d\n%s\n" % (n, g[100:100 + n]) for n in range(9))                       # L = 0..8: empty frames, every partial codon
    odd = b">header_only\n>\n" + g[200:290] + b"\n>header_only_again desc\n>last_has_no_newline\n" + g[300:400]   # ... and another file follows
    widths = b"".join(b">w%d\n" % w + lines(g[500 * w:500 * w + 200 + w], w) for w in (1, 2, 3, 4, 60, 61))   # codons span line ends in every phase
    crlf = b">crlf\r\n" + lines(g[2000:2400], 70, b"\r\n") + b">lone_cr\r\n" + g[2400:2450] + b"\r" + g[2450:2500] + b"\r\n\r\n" + g[2500:2531] + b"\r\n"
    case = b">lower\n" + lines(g[3000:3300].lower(), 60) + b">mixed\n" + g[3300:3350] + g[3350:3400].lower() + b"\n" + g[3400:3433].lower() + g[3433:3460] + b"\n"
    n_runs = b">n_runs\n" + g[4000:4050] + b"N" + g[4050:4101] + b"NN" + g[4101:4150] + b"NNN" + g[4150:4200] + b"\n" + lines(b"N" * 257, 60) + g[4200:4260] + b"\n"
    other = b">u_and_gt\n" + g[5000:5030] + b"U" + g[5030:5061] + b">" + g[5061:5090] + b"u\n" + g[5090:5100] + b"\n"
    stops = b">stops\n" + lines(b"TAATAGTGA" * 40, 60)
    poly_a = b">poly_a\n" + lines(b"A" * 20_000, 60)
    files = [out_tiles, tiny, odd, b"", widths, crlf, case, n_runs, other, stops, poly_a]
    # input tiles: a sequence that starts at the first byte of a 4 KiB tile and crosses two tile boundaries, one that starts at the first byte
    # of a 16-byte lane
    at = sum(len(f) for f in files)
    hdr = b">seq_at_tile_start\n"
    fill = b">fill\n" + g[6000:6000 + (-(at + 7 + len(hdr))) % TILE] + b"\n"
    assert (at + len(fill) + len(hdr)) % TILE == 0
    t = fill + hdr + lines(g[10_000:19_000], 80)
    hdr2 = b">seq_at_lane_start\n"
    extra = next(x for x in range(1, 40) if (at + len(t) + x + 1 + len(hdr2)) % 16 == 0 and (at + len(t) + x + 1 + len(hdr2)) % TILE)
    t += g[20_000:20_000 + extra] + b"\n" + hdr2 + g[21_000:21_100] + b"\n"
    assert (at + t.index(hdr2) + len(hdr2)) % 16 == 0
    files.append(t)
    if big:
        files.append(b">big one above 384 KiB\n" + lines(dna(11, 450_000), 80))
    files.append(small_records(n_small))
    return files


@pytest.fixture(scope="module")
def ctx():
    c = lash_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge():
    files = edge_files()
    return files, M.Model(files)


@pytest.fixture(scope="module")
def image_case():
    """the edge collection with fewer small records and without the long one: the per-record images of a binned sketch stay small"""
    files = edge_files(n_small=150, big=False) + [b">big\n" + lines(dna(11, 150_000), 80)]
    return files, M.Model(files)


# ---- 1. the stage against the model --------------------------------------------------------------------------------------------------
class _DeviceBytes:
    """n bytes of device memory at ptr, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def check_stage(ctx, files, model):
    import torch
    raw = np.frombuffer(b"".join(files), np.uint8)
    off = offsets(files)
    index = ctx.fasta_index(raw, off, keep=True)
    try:
        assert index.n_records == len(model.lengths)
        d_raw = torch.from_numpy(raw.copy()).cuda()
        for name, src, device in (("host bytes of the index", raw, False), ("other host bytes", raw.copy(), False), ("device bytes", d_raw, True)):
            ti = ctx.fasta_translate(src, off, index, device=device, keep=True)
            try:
                assert ti.nbytes == len(model.buffer) and ti.n_segments == len(model.seg_off) - 1, name
                seg_off, rec_seg = ti.arrays()
                if ti.nbytes:
                    ctx.synchronize()
                    host = torch.as_tensor(_DeviceBytes(ti.device_ptr, ti.nbytes), device="cuda").cpu().numpy()
                    bad = np.nonzero(host != np.frombuffer(model.buffer, np.uint8))[0]
                    assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (name, bad.size, bad[0])
                assert seg_off.dtype == model.seg_off.dtype and np.array_equal(seg_off, model.seg_off), name
                assert np.array_equal(rec_seg, model.rec_seg), name
            finally:
                ti.free()
    finally:
        index.free()


def test_edge_collection_holds_what_it_should(edge):
    files, m = edge
    assert set(range(9)) <= set(m.lengths) and 450_000 in m.lengths and 20_000 in m.lengths and len(m.lengths) > 2_000
    assert b"" in m.ids and b"header_only" in m.ids and m.lengths[m.ids.index(b"header_only")] == 0
    # where the frames of the first file's records end in the buffer: exactly at an output-tile boundary, one byte before, one byte after
    ends = set()
    at = 0
    for r in range(6):
        for f in M.record_frames(M.sequence_bytes(M.records_of(files[0])[r])):
            at += len(f) + 1
            ends.add(at % TILE)
    assert {0, TILE - 1, 1} <= ends and at == int(m.seg_off[m.rec_seg[6]])
    poly = m.rec_segments[m.ids.index(b"poly_a")]
    assert [len(s) for s in poly] == [6667, 6667, 6667, 6667, 6667, 6667] and poly[0][:2] == b"KK" and poly[3][:2] == b"FF"
    assert set(b"".join(m.rec_segments[m.ids.index(b"stops")][:40])) == {ord("*")}
    assert any(len(s) == 1 for r in m.rec_segments for s in r) and b"X" in m.buffer


def test_stage_equals_the_model(ctx, edge):
    check_stage(ctx, *edge)


def test_stage_on_single_files_and_nothing(ctx):
    for f in edge_files(n_small=40, big=False):
        check_stage(ctx, [f], M.Model([f]))
    check_stage(ctx, [b"", b""], M.Model([b"", b""]))                # no record at all


def test_stage_past_1024_input_tiles_and_2048_output_tiles(ctx):
    """one file of more than 1024 input tiles, more than 1024 records and more than 2048 output tiles: the single-workgroup scans of the tile
    counts, of the record sizes and of the output tiles' break counts give a thread two elements, two and three"""
    rng = random.Random(31)
    g = dna(23, 400_000)
    recs = []
    for i in range(1480):
        n = rng.randint(1000, 4900)
        s = rng.randrange(0, len(g) - n)
        recs.append(b">q%d\n" % i + lines(g[s:s + n], 97))
    raw = b"".join(recs)
    assert 1024 < -(-len(raw) // TILE) <= 1100 and len(recs) > 1024
    m = M.Model([raw])
    assert -(-len(m.buffer) // TILE) > 2048 and len(set(m.lengths)) > 500                             # lengths that are multiples of nothing
    check_stage(ctx, [raw], m)


def test_refusals(ctx):
    fa = b">a\nACGTACGTACGTACGTACGTAAATTTGGGCCC\n>b\nACGT\n"
    raw, off = np.frombuffer(fa, np.uint8), offsets([fa])
    index = ctx.fasta_index(raw, off, keep=True)
    other = lash_amd.Context(0)
    try:
        with pytest.raises(lash_amd.LashError) as e:                 # not the buffer the index was made from
            ctx.fasta_translate(np.frombuffer(fa + b"A", np.uint8), offsets([fa + b"A"]), index)
        assert e.value.code == lash_amd.EINVAL
        ti = ctx.fasta_translate(raw, off, index, keep=True)
        assert ti.n_records == 2
        for k in (0, 13, 16):
            with pytest.raises(lash_amd.LashError) as e:
                ctx.sketch_translated("hmh", k, 0, 42, ti)
            assert e.value.code == lash_amd.EINVAL
        for goff in ([1, 0], [0, 3], [2, 1, 2]):
            with pytest.raises(lash_amd.LashError) as e:
                ctx.sketch_translated("hmh", 5, 0, 42, ti, goff)
            assert e.value.code == lash_amd.EINVAL
        assert ctx.sketch_translated("hmh", 5, 0, 42, ti, [0, 1, 2]).shape[0] == 2
        assert ctx.sketch_translated("hmh", 5, 0, 42, ti, [1]).shape[0] == 0
        ti.free()
    finally:
        index.free()
        other.close()


# ---- 2. images against the oracle ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translated(ctx, image_case):
    files, m = image_case
    raw = np.frombuffer(b"".join(files), np.uint8)
    index = ctx.fasta_index(raw, offsets(files), keep=True)
    ti = ctx.fasta_translate(raw, offsets(files), index, keep=True)
    yield ti
    ti.free()
    index.free()


def check_groups(ctx, ti, m, algo, k, p, goff, layout=None):
    seq, rec_off, gseg = m.group_arrays(goff)
    got = ctx.sketch_translated(algo, k, p, 42, ti, goff)
    want = O.sketch_genomes(ALGO[algo], k, p, 42, seq, rec_off, gseg, threads=16, amino=True, layout=layout)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s p=%d k=%d: group %d of %d differs from the oracle's amino-acid image of its segments" % (algo, p, k, bad[0], len(goff) - 1)
    batch = ctx.sketch_batch(algo, k, p, 42, seq, rec_off, gseg, flags=lash_amd.F_AMINO)
    assert np.array_equal(got, batch), "differs from lash_sketch_batch with LASH_F_AMINO on the same arrays"
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("algo,p", CONFIGS)
def test_images_per_file_and_per_record(ctx, image_case, translated, algo, p, k):
    files, m = image_case
    assert translated.n_segments == len(m.seg_off) - 1
    check_groups(ctx, translated, m, algo, k, p, m.file_rec_off())
    check_groups(ctx, translated, m, algo, k, p, np.arange(len(m.lengths) + 1, dtype=np.uint64))


@pytest.mark.parametrize("algo,p", CONFIGS[:3])
def test_other_code_table_skipped_records_and_accumulation(ctx, image_case, translated, algo, p):
    files, m = image_case
    n = len(m.lengths)
    ctx.set_layout("aa_codes=zero")
    try:
        check_groups(ctx, translated, m, algo, 5, p, m.file_rec_off(), layout=O.make_layout(aa_codes="zero"))
    finally:
        ctx.set_layout(None)
    check_groups(ctx, translated, m, algo, 7, p, [3, 10, 10, 40, n - 5])           # groups that skip records, one of them empty
    whole = ctx.sketch_translated(algo, 7, p, 42, translated)
    two = ctx.sketch_translated(algo, 7, p, 42, translated, [0, n // 2])
    two = ctx.sketch_translated(algo, 7, p, 42, translated, [n // 2, n], flags=lash_amd.F_ACCUMULATE, out=two)
    assert np.array_equal(whole, two)
    assert np.array_equal(whole, check_groups(ctx, translated, m, algo, 7, p, [0, n]))


# ---- 3. encoded proteins are already there -------------------------------------------------------------------------------------------
RESIDUES = "ACDEFGHIKLMNPQRSTVWY"
SYNONYMS = {r: [c.decode() for c, a in M.CODON.items() if a == r.encode()] for r in RESIDUES}
PROTEIN_SEED = 72                         # (71: the stranger happens to leave the 1 024 UltraLogLog registers as they are)


def encoded_case(seed):
    rng = random.Random(seed)
    proteins = ["".join(rng.choice(RESIDUES) for _ in range(rng.randint(30, 200))) for _ in range(40)]
    parts = []
    for prot in proteins:
        parts.append("".join(rng.choice("ACGT") for _ in range(rng.randint(50, 400))))       # any frame
        coding = "".join(rng.choice(SYNONYMS[r]) for r in prot)
        parts.append(coding if rng.random() < 0.5 else coding.encode().translate(M.COMPLEMENT)[::-1].decode())
    parts.append("".join(rng.choice("ACGT") for _ in range(100)))
    genome = b">genome with 40 genes\n" + lines("".join(parts).encode(), 70)
    stranger = "".join(rng.choice(RESIDUES) for _ in range(120))
    return genome, [p.encode() for p in proteins], stranger.encode()


@pytest.mark.parametrize("algo,p", CONFIGS[:3])
def test_encoded_proteins_are_in_the_translated_sketch(ctx, algo, p):
    k = 7
    genome, proteins, stranger = encoded_case(PROTEIN_SEED)
    m = M.Model([genome])
    # the oracle on the CPU: the proteins add nothing to the genome's segments, the stranger does (this is what fixes the seed)
    segs = m.group_segments(0, 1)
    with_p = lash_amd.records_to_arrays([segs + proteins])
    with_s = lash_amd.records_to_arrays([segs + [stranger]])
    alone = lash_amd.records_to_arrays([segs])
    o_alone, o_p, o_s = (O.sketch_genomes(ALGO[algo], k, p, 42, *a, threads=8, amino=True) for a in (alone, with_p, with_s))
    assert np.array_equal(o_alone, o_p) and not np.array_equal(o_alone, o_s)
    raw = np.frombuffer(genome, np.uint8)
    index = ctx.fasta_index(raw, offsets([genome]), keep=True)
    ti = ctx.fasta_translate(raw, offsets([genome]), index, keep=True)
    try:
        image = ctx.sketch_translated(algo, k, p, 42, ti)
        assert np.array_equal(image, o_alone)
        seq, rec_off, goff = lash_amd.records_to_arrays([proteins])
        plus = ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff, flags=lash_amd.F_AMINO | lash_amd.F_ACCUMULATE, out=image.copy())
        assert np.array_equal(plus, image), "a protein the genome encodes changed its translated sketch"
        seq, rec_off, goff = lash_amd.records_to_arrays([[stranger]])
        plus = ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff, flags=lash_amd.F_AMINO | lash_amd.F_ACCUMULATE, out=image.copy())
        assert not np.array_equal(plus, image)
    finally:
        ti.free()
        index.free()


# ---- 4. command line -----------------------------------------------------------------------------------------------------------------
def run(*args, cwd=None):
    return subprocess.run([H.CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=900)


def segments_fasta(segments):
    return b"".join(b">s\n" + s + b"\n" for s in segments)


CLI_CONFIGS = (("hmh", 7, 10), ("ull", 5, 12))


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """three multi-record files, the third gzipped, above 1 MiB together; the model's segments of every file, and of every record, written as
    protein FASTA and sketched with --aa"""
    d = tmp_path_factory.mktemp("translate_cli")
    e = edge_files(n_small=60, big=False)
    datas = {"one.fa": b"".join(b">chr%d of one\n" % i + lines(dna(30 + i, 40_000), 80) for i in range(16)),
             "two.fa": b">big two\n" + lines(dna(11, 450_000), 80) + e[-1],
             "three.fa": b"".join(f for f in e[:-1] if f)}
    assert sum(len(x) for x in datas.values()) > (1 << 20)
    paths, file_prot, rec_prot = [], [], []
    prot = d / "prot"
    prot.mkdir()
    for name, data in datas.items():
        gz = name == "three.fa"
        (d / (name + (".gz" if gz else ""))).write_bytes(gzip.compress(data, 1) if gz else data)
        paths.append(str(d / (name + (".gz" if gz else ""))))
        m = M.Model([data])
        file_prot.append(str(prot / (name + ".faa")))
        (prot / (name + ".faa")).write_bytes(segments_fasta(m.group_segments(0, len(m.lengths))))
        for r in range(len(m.lengths)):
            rec_prot.append(str(prot / ("%s.%05d.faa" % (name, r))))
            (prot / ("%s.%05d.faa" % (name, r))).write_bytes(segments_fasta(m.rec_segments[r]))
    (d / "genomes.txt").write_text("\n".join(paths) + "\n")
    (d / "file_prot.txt").write_text("\n".join(file_prot) + "\n")
    (d / "rec_prot.txt").write_text("\n".join(rec_prot) + "\n")
    ref = {}
    for algo, k, p in CLI_CONFIGS:
        for what in ("file", "rec"):
            prefix = str(d / ("aa_%s_%s" % (what, algo)))
            r = run("sketch", "-f", d / (what + "_prot.txt"), "-o", prefix, "--aa", "-a", algo, "-k", k, "-p", p, "-t", 4)
            assert r.returncode == 0, r.stderr
            ref[what, algo] = (H.zstd_read(prefix + "_sketches.bin"), open(prefix + "_parameters.json", "rb").read())
    # the names: what the runs without the flag write
    names = {}
    for what, extra in (("file", []), ("rec", ["--per-record"])):
        prefix = str(d / ("plain_" + what))
        r = run("sketch", "-f", d / "genomes.txt", "-o", prefix, "-k", 7, "-t", 4, *extra)
        assert r.returncode == 0, r.stderr
        names[what] = json.load(open(prefix + "_files.json"))
    assert names["file"] == paths and len(names["rec"]) == len(rec_prot)
    return d, ref, names


@pytest.mark.parametrize("case,what,extra", [("plain", "file", []), ("batch1", "file", ["--batch-mb", "1"]), ("workers2", "file", ["--devices", "0,0"]),
                                             ("per_record", "rec", ["--per-record"]),
                                             ("per_record_batch1_workers2", "rec", ["--per-record", "--batch-mb", "1", "--devices", "0,0"])])
def test_cli_translate_equals_aa_of_the_segments(cli_case, tmp_path, case, what, extra):
    d, ref, names = cli_case
    for algo, k, p in CLI_CONFIGS if case in ("plain", "per_record") else CLI_CONFIGS[:1]:
        out = str(tmp_path / ("tr_" + algo))
        r = run("sketch", "-f", d / "genomes.txt", "-o", out, "--translate", "-a", algo, "-k", k, "-p", p, "-t", 4, *extra)
        assert r.returncode == 0, r.stderr
        assert H.zstd_read(out + "_sketches.bin") == ref[what, algo][0], (case, algo)
        assert open(out + "_parameters.json", "rb").read() == ref[what, algo][1]
        assert json.load(open(out + "_parameters.json"))["molecule"] == "amino_acid"
        assert json.load(open(out + "_files.json")) == names[what]


def test_cli_streamed_file_equals_the_unstreamed_run(tmp_path):
    data = b"".join(b">rec%d of thirty\n" % i + lines(dna(60 + i, 100_000), 80) for i in range(30))
    assert len(data) > 3_000_000
    (tmp_path / "thirty.fa").write_bytes(data)
    (tmp_path / "l.txt").write_text("%s\n" % (tmp_path / "thirty.fa"))
    blobs = []
    for name, extra in (("whole", []), ("streamed", ["--stream-mb", "1"]), ("streamed_records", ["--stream-mb", "1", "--per-record"]), ("records", ["--per-record"])):
        out = str(tmp_path / name)
        r = run("sketch", "-f", tmp_path / "l.txt", "-o", out, "--translate", "-k", 7, "-t", 4, *extra)
        assert r.returncode == 0, r.stderr
        blobs.append(H.zstd_read(out + "_sketches.bin"))
    assert blobs[0] == blobs[1] and blobs[2] == blobs[3] and len(blobs[2]) == 30 * len(blobs[0])


def test_cli_refusals_name_the_record_and_the_file(tmp_path):
    def nothing_left(prefix):
        return not any(os.path.exists(prefix + s) for s in ("_files.json", "_parameters.json"))
    big = tmp_path / "big.fa"
    big.write_bytes(b">small\nACGTACGT\n>the_big_one desc\n" + b"\n".join([dna(3, 80)] * 30_000) + b"\n>after\nACGT\n")
    lst = tmp_path / "l.txt"
    lst.write_text("%s\n" % big)
    for extra in ([], ["--per-record"]):
        out = str(tmp_path / ("o1" + "".join(extra)))
        r = run("sketch", "-f", lst, "-o", out, "--translate", "-k", 7, "--stream-mb", 1, *extra)
        assert r.returncode == 1 and str(big) in r.stderr and "the_big_one" in r.stderr and "--stream-mb" in r.stderr and "--translate" in r.stderr, r.stderr
        assert nothing_left(out)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    fa = tmp_path / "ok.fa"
    fa.write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    lst.write_text("%s\n%s\n" % (fa, fq))
    for extra in ([], ["--per-record"]):
        out = str(tmp_path / ("o2" + "".join(extra)))
        r = run("sketch", "-f", lst, "-o", out, "--translate", "-k", 7, *extra)
        assert r.returncode != 0 and str(fq) in r.stderr and "--translate" in r.stderr and "FASTA" in r.stderr, r.stderr
        assert nothing_left(out)


def test_library_refuses_k_13(ctx, translated):
    with pytest.raises(lash_amd.LashError):
        ctx.sketch_translated("ull", 13, 10, 42, translated)
