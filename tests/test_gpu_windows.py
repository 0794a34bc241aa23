"""`lash sketch --window W`: one sketch per W-base window of every FASTA record.  The window table made on the GPU (lash_fasta_windows[_device])
against a pure-Python model written from the rule — the sequence bytes of a record are the bytes after its header line that are neither LF nor
CR, window j holds coordinates [jW, min(L, (j + 1)W)) — the images of lash_sketch_windows_raw against the oracle's image of every window's
bytes sketched alone and against lash_sketch_batch with one genome per window; the command line against the plain `lash sketch` of the same
windows written one per file; and `lash dist --containment` finding an insert's windows in its host."""
import gzip
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import host_lib as H
import lash_amd
import oracle_lib as O

pytestmark = pytest.mark.gpu
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
CONFIGS = [("hmh", 16, 0), ("hll", 21, 14), ("ull", 16, 12)]
WINDOWS = [1, 7, 16, 100, 4096, 10 ** 6]


# ---- the rule, in Python -------------------------------------------------------------------------------------------------------------
def records_of(data):
    """the records of one file: a record starts at the file's first byte and at every '>' whose preceding byte is a newline"""
    assert data[:1] == b">"
    starts = [m.start() for m in re.finditer(rb"(?<![^\n])>", data)] + [len(data)]
    return [data[a:b] for a, b in zip(starts[:-1], starts[1:])]


def record_id(rec):
    return re.compile(rb"[^ \t\r\n]*").match(rec, 1).group()


def sequence_bytes(rec):
    """the bytes after the header line's LF that are neither LF nor CR; everything else counts"""
    nl = rec.find(b"\n")
    return b"" if nl < 0 else rec[nl + 1:].replace(b"\n", b"").replace(b"\r", b"")


def model(files, w):
    """-> (record[n], begin[n], length[n], [bytes of every window], [id of every window's record]) in file, record, window order"""
    rec, beg, ln, data, ids = [], [], [], [], []
    r = 0
    for f in files:
        for record in (records_of(f) if f else []):
            s = sequence_bytes(record)
            for b in range(0, len(s), w):
                rec.append(r)
                beg.append(b)
                ln.append(min(w, len(s) - b))
                data.append(s[b:b + w])
                ids.append(record_id(record))
            r += 1
    return np.array(rec, np.uint64), np.array(beg, np.uint64), np.array(ln, np.uint64), data, ids


def offsets(files):
    return np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)


def dna(seed, n):
    return O.synth_genome(seed, n).tobytes()


def lines(s, width, eol=b"\n"):
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width))


def edge_files():
    g = dna(17, 70_000)
    a = (b">r1 first record\n" + g[:200] + b"\n" + g[200:333] + b"\n"
         b">r2>with>gt inside\tand a TAB\n" + g[400:470] + b">" + g[470:540] + b"\n"          # '>' inside a header and a sequence line
         b"\n\n>blank_lines_before\n\n" + g[600:700] + b"\n\n" + g[700:800] + b"\n"
         b">header_only\n"
         b">\n" + g[900:1000] + b"\n"                                                         # an empty id
         b">header_only_again desc\n"
         b">last_has_no_newline\n" + g[1100:1200])                                            # ... and another file follows in the buffer
    first_is_header_only = b">h0 nothing here\n>h1\n" + g[1300:1400] + b"\n>h2_header_only_last\n"
    crlf = (b">c1 crlf\r\n" + lines(g[2000:2400], 100, b"\r\n") +                            # W = 100: every boundary falls inside a CR LF pair
            b">c2\r\n" + g[2400:2500] + b"\r\n>c3_header_only\r\n>c4\r\n\r\n" + g[2500:2550] + b"\r" + g[2550:2600] + b"\r\n")
    long_hdr = b">long" + (b"x>ACGT>" * 1500)[:10_000] + b" tail\n" + g[3000:3500] + b"\n>after_long\n" + g[3500:3600] + b"\n"
    # lengths around the window lengths: L = W - 1, W, W + 1 for W = 7, 16, 100 (lines of 100: a boundary at a line end), 4096
    exact = b"".join(b">len%d\n" % n + lines(g[5000 + n:5000 + 2 * n], 100) for n in (6, 7, 8, 15, 16, 17, 99, 100, 101, 200, 4095, 4096, 4097))
    # '>' as the first byte of a 4 KiB tile, of a 16-byte lane, and of a file; a record whose sequence crosses two tile boundaries
    t = b">t0\n"
    t += g[20000:20000 + 4096 - len(t) - 1] + b"\n"
    assert len(t) == 4096
    t += b">t1 at a tile start\n" + g[29000:29100] + b"\n"
    pad = 2 * 4096 + 16 - len(t) - 1
    t += g[30000:30000 + pad] + b"\n"
    t += b">t2 at a lane start\n" + g[32000:32100] + b"\n"
    t += g[33000:33000 + 3 * 4096 - len(t)]                                                  # ends at a tile boundary, no final newline
    assert len(t) == 3 * 4096
    u = b">u0 a file at a tile start\n" + g[40000:40100] + b"\n>u1\n" + g[40100:40130]
    dirty = (b">lower\n" + g[50000:50300].lower() + b"\n>mixed\n" + g[50300:50400] + b"N" * 257 + g[50400:50500] + b"\n" + g[50500:50600].lower() +
             b"\n>all_n\n" + lines(b"N" * 300, 60) + b">short\nACGTAC\n>single\nA\n")
    pre = a + first_is_header_only + crlf + long_hdr + exact
    fill = b">fill\n" + g[60000:60000 + (-(len(pre) + 7) % 4096)] + b"\n"                     # so that `t` starts at a tile start
    assert (len(pre) + len(fill)) % 4096 == 0
    return [a, first_is_header_only, b"", crlf, long_hdr, exact, fill, t, u, b"", dirty, b">only_a_header", b""]


def one_long_record():
    return [b">big one above 384 KiB\n" + lines(dna(11, 450_000), 80)]


def many_windows():
    rng = random.Random(5)
    g = dna(13, 3_000_000)
    small = b"".join(b">r%d\n%s\n" % (i, g[s:s + rng.randint(30, 300)]) for i, s in ((i, rng.randrange(0, len(g) - 300)) for i in range(2_000)))
    return {30: [b">three_mbp\n" + lines(g, 70)], 64: [small]}


@pytest.fixture(scope="module")
def ctx():
    c = lash_amd.Context(0)
    yield c
    c.close()


# ---- 1. the window table -------------------------------------------------------------------------------------------------------------
class _DeviceBytes:
    """n bytes of device memory at ptr, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def check_table(ctx, files, w):
    import torch
    raw = np.frombuffer(b"".join(files), np.uint8)
    off = offsets(files)
    want = model(files, w)
    index = ctx.fasta_index(raw, off, keep=True)
    try:
        got = ctx.fasta_windows(raw, off, index, w)
        moved = raw.copy()                                           # other host bytes than the index was made from: sent again
        got_moved = ctx.fasta_windows(moved, off, index, w)
        d_raw = torch.from_numpy(raw.copy()).cuda()
        got_dev = ctx.fasta_windows(d_raw, off, index, w, device=True)
        wi = ctx.fasta_windows(raw, off, index, w, keep=True)
        try:
            assert wi.n_windows == len(want[3]) and wi.nbytes == sum(len(d) for d in want[3]) + 3 * len(want[3])
            o = wi.offsets()
            assert np.array_equal(o, np.cumsum([0] + [len(d) + 3 for d in want[3]]).astype(np.uint64))
            if wi.nbytes:                                            # the rewritten buffer: one well-formed one-record FASTA file per window
                ctx.synchronize()
                host = torch.as_tensor(_DeviceBytes(wi.device_ptr, wi.nbytes), device="cuda").cpu().numpy()
                assert host.tobytes() == b"".join(b">\n" + d + b"\n" for d in want[3])
        finally:
            wi.free()
    finally:
        index.free()
    for name, x, g, gm, gd in zip(("record", "begin", "length"), want, got, got_moved, got_dev):
        assert x.dtype == g.dtype and np.array_equal(x, g), "%s, W = %d" % (name, w)
        assert np.array_equal(g, gm) and np.array_equal(g, gd), "%s, W = %d (other host bytes / device bytes)" % (name, w)
    return want


@pytest.mark.parametrize("w", WINDOWS)
def test_window_table_equals_the_model(ctx, w):
    files = edge_files()
    rec, beg, ln, data, ids = check_table(ctx, files, w)
    lens = [len(sequence_bytes(r)) for f in files if f for r in records_of(f)]
    assert 0 in lens and lens[len(records_of(files[0]))] == 0 and lens[-1] == 0                      # header-only: among others, a file's first and last
    assert len(data) == sum(-(-n // w) for n in lens)
    if w == 10 ** 6:
        assert len(data) == sum(1 for n in lens if n) and all(int(b) == 0 for b in beg)
    else:
        assert any(n and n % w == 0 for n in lens)                                                    # no empty tail
        if w > 1:
            assert any(n < w for n in lens if n)                                                      # L < W
            assert w - 1 in lens and w + 1 in lens and any(0 < int(x) < w for x in ln)               # L = W -+ 1; short last windows kept
    assert b"" in ids and b"r2>with>gt" in ids and b">" in b"".join(data)


def test_window_boundaries_fall_where_the_issue_asks(ctx):
    """the boundary cases the edge files were built for, located in the input bytes by the model's own coordinates"""
    files = edge_files()
    buf = b"".join(files)
    # position in the buffer of every sequence byte of every record, by the rule
    pos = []
    at = 0
    for f in files:
        for record in (records_of(f) if f else []):
            nl = record.find(b"\n")
            pos.append([at + i for i in range(nl + 1, len(record)) if record[i] not in b"\r\n"] if nl >= 0 else [])
            at += len(record)
    seen = set()
    for w in (7, 100, 4096):
        for p in pos:
            for b in range(w, len(p), w):                            # window boundary between coordinates b - 1 and b
                between = buf[p[b - 1] + 1:p[b]]
                seen.add({b"": "mid-line", b"\n": "line end", b"\r\n": "crlf"}.get(between, "other"))
            for b in range(0, len(p), w):
                if p[b] // 4096 != p[min(len(p), b + w) - 1] // 4096:
                    seen.add("tile")
    assert {"mid-line", "line end", "crlf", "tile"} <= seen


def test_single_files_and_refusals(ctx):
    for f in edge_files():
        for w in (7, 4096):
            check_table(ctx, [f], w)
    check_table(ctx, [b"", b""], 16)                                 # no record at all
    fa = b">a\nACGTACGTACGTACGTACGT\n>b\nACGT\n"
    raw, off = np.frombuffer(fa, np.uint8), offsets([fa])
    index = ctx.fasta_index(raw, off, keep=True)
    other = lash_amd.Context(0)
    try:
        with pytest.raises(lash_amd.LashError) as e:
            ctx.fasta_windows(raw, off, index, 0)
        assert e.value.code == lash_amd.EINVAL
        with pytest.raises(lash_amd.LashError) as e:                 # not the buffer the index was made from
            ctx.fasta_windows(np.frombuffer(fa + b"A", np.uint8), offsets([fa + b"A"]), index, 8)
        assert e.value.code == lash_amd.EINVAL
        wi = ctx.fasta_windows(raw, off, index, 8, keep=True)
        assert wi.n_windows == 4
        for w0, w1 in ((3, 2), (0, 5), (5, 5)):
            with pytest.raises(lash_amd.LashError) as e:
                ctx.sketch_windows("hmh", 8, 0, 42, wi, w0, w1)
            assert e.value.code == lash_amd.EINVAL
        with pytest.raises(lash_amd.LashError) as e:
            ctx.sketch_windows("hmh", 8, 0, 42, wi, flags=lash_amd.F_AMINO)
        assert e.value.code == lash_amd.EINVAL
        assert ctx.sketch_windows("hmh", 8, 0, 42, wi).shape[0] == 4
        wi.free()
    finally:
        index.free()
        other.close()


def test_window_table_past_1024_tiles_and_1024_records(ctx):
    """one file of more than 1024 input tiles and more than 1024 records: the single-workgroup scans of the tile counts and of the records'
    window counts each give a thread more than one element"""
    rng = random.Random(29)
    g = dna(19, 400_000)
    recs = []
    for i in range(1480):
        n = rng.randint(1000, 4900)
        s = rng.randrange(0, len(g) - n)
        recs.append(b">q%d\n" % i + lines(g[s:s + n], 97))
    raw = b"".join(recs)
    assert 1024 < -(-len(raw) // 4096) <= 1100 and len(recs) > 1024
    rec, beg, ln, data, ids = check_table(ctx, [raw], 997)
    assert len(data) > 4096 and int(rec[-1]) == len(recs) - 1 and len({int(x) for x in ln}) > 500      # lengths that are multiples of nothing


# ---- 2. - 4. images ------------------------------------------------------------------------------------------------------------------
def check_images(ctx, files, w, algo, k, p, step=1 << 30, oracle_every=1, cuts=()):
    raw = np.frombuffer(b"".join(files), np.uint8)
    off = offsets(files)
    data = model(files, w)[3]
    n = len(data)
    index = ctx.fasta_index(raw, off, keep=True)
    try:
        wi = ctx.fasta_windows(raw, off, index, w, keep=True)
        try:
            assert wi.n_windows == n
            whole = []
            for w0 in range(0, n, step):
                w1 = min(n, w0 + step)
                seq, rec_off, goff = lash_amd.records_to_arrays([[d] for d in data[w0:w1]])
                got = ctx.sketch_windows(algo, k, p, 42, wi, w0, w1)
                batch = ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff)
                assert got.shape == batch.shape and np.array_equal(got, batch), "differs from lash_sketch_batch with one genome per window"
                pick = list(range(0, w1 - w0, oracle_every))
                seq, rec_off, goff = lash_amd.records_to_arrays([[data[w0 + i]] for i in pick])
                want = O.sketch_genomes(ALGO[algo], k, p, 42, seq, rec_off, goff, threads=16)
                for i in np.nonzero((got[pick] != want).any(axis=1))[0]:
                    raise AssertionError("%s k=%d W=%d: window %d differs from the oracle's image of its bytes alone" % (algo, k, w, w0 + pick[i]))
                if cuts:
                    whole.append(got)
            if cuts:
                whole = np.concatenate(whole)
                for a, b in cuts:
                    assert np.array_equal(ctx.sketch_windows(algo, k, p, 42, wi, a, b), whole[a:b]), (a, b)
        finally:
            wi.free()
    finally:
        index.free()
    return data


@pytest.mark.parametrize("algo,k,p", CONFIGS)
@pytest.mark.parametrize("w", [16, 100, 4096])
def test_window_images_equal_the_oracle_and_the_batch_entry(ctx, w, algo, k, p):
    files = edge_files()
    n = len(model(files, w)[3])
    data = check_images(ctx, files, w, algo, k, p, cuts=[(0, 0), (0, 1), (1, 2), (2, 9), (n // 2, n - 1), (n - 1, n), (n, n), (5, 5)])
    assert any(len(d) < k for d in data) and any(set(d) == {ord("N")} for d in data)


@pytest.mark.parametrize("algo,k,p", CONFIGS)
@pytest.mark.parametrize("w,n_windows", [(3_000, 150), (400_000, 2)])
def test_both_kernel_families(ctx, w, n_windows, algo, k, p):
    """W = 3 000: 150 windows for the persistent small-genome kernel; W = 400 000: a first window above LASH_SOLE_MAX, for the long-genome one"""
    data = check_images(ctx, one_long_record(), w, algo, k, p)
    assert len(data) == n_windows and len(data[0]) == w


@pytest.mark.parametrize("algo,k,p", CONFIGS)
@pytest.mark.parametrize("w", [30, 64])
def test_many_windows(ctx, w, algo, k, p):
    data = check_images(ctx, many_windows()[w], w, algo, k, p, step=12_500, oracle_every=97)
    assert len(data) == 100_000 if w == 30 else len(data) > 3_000


# ---- 5. command line -----------------------------------------------------------------------------------------------------------------
CLI_W = 1000


def run(*args, cwd=None):
    return subprocess.run([H.CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=900)


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """three multi-record files (the third above 1 MiB, its records below) and the plain sketch of their windows written one per file"""
    d = tmp_path_factory.mktemp("windows_cli")
    e = [f for f in edge_files() if f]
    three = b"".join(b">chr%d of three\n" % i + lines(dna(20 + i, 450_000), 80) for i in range(3))
    datas = {"one.fa": b"".join(e[:4]), "two.fa": one_long_record()[0] + b"".join(e[4:]), "three.fa": three}
    assert len(three) > (1 << 20)
    names, windows = [], []
    for name, data in datas.items():
        (d / name).write_bytes(data)
        (d / (name + ".gz")).write_bytes(gzip.compress(data, 1))
        _, beg, ln, wdata, ids = model([data], CLI_W)
        names += ["%s:%d-%d" % (i.decode(), int(b) + 1, int(b) + int(n)) for i, b, n in zip(ids, beg, ln)]
        windows += wdata
    (d / "plain.txt").write_text("".join("%s\n" % (d / name) for name in datas))
    (d / "gz.txt").write_text("".join("%s.gz\n" % (d / name) for name in datas))
    split = d / "split"
    split.mkdir()
    paths = []
    for i, wd in enumerate(windows):
        (split / ("%06d.fa" % i)).write_bytes(b">\n" + wd + b"\n")
        paths.append(str(split / ("%06d.fa" % i)))
    (d / "split.txt").write_text("\n".join(paths) + "\n")
    ref = {}
    for algo, k, p in (("hmh", 16, 10), ("ull", 16, 12)):
        prefix = str(d / ("files_" + algo))
        r = run("sketch", "-f", d / "split.txt", "-o", prefix, "-a", algo, "-k", k, "-p", p, "-t", 4)
        assert r.returncode == 0, r.stderr
        ref[algo] = (H.zstd_read(prefix + "_sketches.bin"), open(prefix + "_parameters.json", "rb").read())
    return d, names, ref


@pytest.mark.parametrize("case,lst,extra", [("plain", "plain.txt", []), ("gz", "gz.txt", []), ("batch1", "plain.txt", ["--batch-mb", "1"]),
                                            ("workers2", "plain.txt", ["--devices", "0,0"]), ("stream", "plain.txt", ["--stream-mb", "1"]),
                                            ("per_record_too", "gz.txt", ["--per-record", "--stream-mb", "1", "--devices", "0,0"])])
def test_cli_window_equals_one_file_per_window(cli_case, tmp_path, case, lst, extra):
    d, names, ref = cli_case
    assert ":1-100" in names and "r1:1-333" in names and "len4097:4001-4097" in names and names[-1] == "chr2:449001-450000"
    for algo, k, p in (("hmh", 16, 10), ("ull", 16, 12)) if case in ("plain", "gz") else (("hmh", 16, 10),):
        out = str(tmp_path / ("win_" + algo))
        r = run("sketch", "-f", d / lst, "-o", out, "--window", CLI_W, "-a", algo, "-k", k, "-p", p, "-t", 4, *extra)
        assert r.returncode == 0, r.stderr
        assert "%d windows" % len(names) in r.stderr
        assert H.zstd_read(out + "_sketches.bin") == ref[algo][0]
        assert json.load(open(out + "_files.json")) == names
        assert open(out + "_parameters.json", "rb").read() == ref[algo][1]


def test_cli_refusals_name_the_file_and_leave_nothing(tmp_path):
    def nothing_left(prefix):
        return not any(os.path.exists(prefix + s) for s in ("_sketches.bin", "_files.json", "_parameters.json"))
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    fa = tmp_path / "ok.fa"
    fa.write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    lst = tmp_path / "l.txt"
    lst.write_text("%s\n%s\n" % (fa, fq))
    out = str(tmp_path / "o1")
    r = run("sketch", "-f", lst, "-o", out, "--window", 16)
    assert r.returncode == 2 and str(fq) in r.stderr and "--window" in r.stderr and "FASTA" in r.stderr, r.stderr
    assert nothing_left(out)
    # a record larger than the chunk: an error that names it, not a silent merge
    big = tmp_path / "big.fa"
    big.write_bytes(b">small\nACGTACGT\n>the_big_one desc\n" + b"\n".join([dna(3, 80)] * 30_000) + b"\n>after\nACGT\n")
    lst.write_text("%s\n" % big)
    out = str(tmp_path / "o2")
    r = run("sketch", "-f", lst, "-o", out, "--window", 1000, "--stream-mb", 1)
    assert r.returncode == 1 and str(big) in r.stderr and "the_big_one" in r.stderr and "--stream-mb" in r.stderr and "--window" in r.stderr, r.stderr
    assert nothing_left(out)
    # header-only input: no window, an empty set — what --per-record writes for a file list without records is the model
    hdr = tmp_path / "hdr.fa"
    hdr.write_bytes(b">h1\n>h2 nothing\n")
    lst.write_text("%s\n" % hdr)
    out = str(tmp_path / "o3")
    r = run("sketch", "-f", lst, "-o", out, "--window", 1000)
    assert r.returncode == 0 and "0 windows" in r.stderr, r.stderr
    assert json.load(open(out + "_files.json")) == [] and H.zstd_read(out + "_sketches.bin") == b""


# ---- 6. end to end with dist ---------------------------------------------------------------------------------------------------------
def test_dist_containment_finds_the_insert(tmp_path):
    h, insert = dna(101, 180_000), dna(202, 20_000)
    host = h[:100_000] + insert + h[100_000:]                         # the insert is bases 100 001 - 120 000 of the 200 kbp host
    assert len(host) == 200_000
    (tmp_path / "host.fa").write_bytes(b">host chromosome\n" + lines(host, 60))
    (tmp_path / "insert.fa").write_bytes(b">insert\n" + lines(insert, 60))
    (tmp_path / "host.txt").write_text("%s\n" % (tmp_path / "host.fa"))
    (tmp_path / "insert.txt").write_text("%s\n" % (tmp_path / "insert.fa"))
    r = run("sketch", "-f", "host.txt", "-o", "windows", "--window", 10000, "-t", 4, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = run("sketch", "-f", "insert.txt", "-o", "insert", "-t", 4, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    names = json.load(open(tmp_path / "windows_files.json"))
    assert names == ["host:%d-%d" % (b + 1, b + 10_000) for b in range(0, 200_000, 10_000)]
    r = run("dist", "-q", "windows", "-r", "insert", "-o", "dist.txt", "--containment", "query", "--file-order", "-t", 4, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "dist.txt").read_text()
    assert text.startswith("Reference\tQuery\tDistance\n")
    rows = [ln.split("\t") for ln in text.split("\n")[1:] if ln]
    assert len(rows) >= 3
    rows.sort(key=lambda row: float(row[2]))
    assert {rows[0][1], rows[1][1]} == {"host:100001-110000", "host:110001-120000"}
    assert float(rows[1][2]) < float(rows[2][2])
