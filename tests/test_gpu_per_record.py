"""`lash sketch --per-record`: one sketch per FASTA record.  The record index made on the GPU (lash_fasta_index[_device]) against a
pure-Python splitter written from the rules; the images of lash_sketch_records_raw against the oracle's image of every record sketched
alone and against lash_sketch_batch with one record per genome; the command line against the plain `lash sketch` of the same records
written one per file.  Every generated record is compared."""
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


# ---- the rules, in Python ------------------------------------------------------------------------------------------------------------
def split(files):
    """(start[n + 1], id_len[n], file[n]) of the files laid back to back: a record starts at a file's first byte and at every '>' whose
    preceding byte in the same file is a newline; the id runs from after the '>' to the first space / TAB / CR / LF / end of file."""
    start, id_len, fidx, base = [], [], [], 0
    for f, data in enumerate(files):
        assert data[:1] == b">"
        for m in re.finditer(rb"(?<![^\n])>", data):
            start.append(base + m.start())
            id_len.append(len(re.compile(rb"[^ \t\r\n]*").match(data, m.start() + 1).group()))
            fidx.append(f)
        base += len(data)
    return np.array(start + [base], np.uint64), np.array(id_len, np.uint32), np.array(fidx, np.uint32)


def record_seq(rec):
    """what needletail's seq() yields for one record: the lines after the header line, line ends (LF, CRLF) stripped"""
    nl = rec.find(b"\n")
    if nl < 0:
        return b""
    return b"".join(line[:-1] if line.endswith(b"\r") else line for line in rec[nl + 1:].split(b"\n"))


def offsets(files):
    return np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)


def dna(seed, n):
    return O.synth_genome(seed, n).tobytes()


def edge_files():
    g = dna(7, 60_000)
    a = (b">r1 first record\n" + g[:200] + b"\n" + g[200:333] + b"\n"
         b">r2>with>gt inside\tand a TAB\n" + g[400:470] + b">" + g[470:540] + b"\n"          # '>' inside a header and a sequence line
         b"\n\n>blank_lines_before\n\n" + g[600:700] + b"\n\n" + g[700:800] + b"\n"
         b">header_only\n"
         b">\n" + g[900:1000] + b"\n"                                                         # an empty id
         b">header_only_again desc\n"
         b">ends_at_space more words\n" + g[1000:1100] + b"\n"
         b">ends_at_tab\tthe TAB ends the id\n" + g[1200:1300] + b"\n"
         b">tab_then_nothing\t\n" + g[1300:1400] + b"\n"
         b">last_has_no_newline\n" + g[1100:1200])                                            # ... and another file follows in the buffer
    crlf = (b">c1 crlf\r\n" + g[2000:2100] + b"\r\n" + g[2100:2150] + b"\r\n"
            b">c2\r\n" + g[2200:2300] + b"\r\n>c3_header_only\r\n>c4\r\n\r\n" + g[2300:2400] + b"\r\n"
            b">c5_tab\tcrlf and a TAB\r\n" + g[2400:2500] + b"\r\n>c6 space\r\n" + g[2500:2600] + b"\r\n")
    long_hdr = b">long" + (b"x>ACGT>" * 1500)[:10_000] + b" tail\n" + g[3000:3500] + b"\n>after_long\n" + g[3500:3600] + b"\n"
    # '>' as the first byte of a 4 KiB tile (the '\n' before it the last byte of the previous tile), of a 16-byte lane, and of a file
    t = b">t0\n"
    t += g[4000:4000 + 4096 - len(t) - 1] + b"\n"
    assert len(t) == 4096
    t += b">t1 at a tile start\n" + g[9000:9100] + b"\n"
    pad = 2 * 4096 + 16 - len(t) - 1
    t += g[10000:10000 + pad] + b"\n"
    t += b">t2 at a lane start\n" + g[12000:12100] + b"\n"
    t += g[13000:13000 + 3 * 4096 - len(t)]                                                  # ends at a tile boundary, no final newline
    assert len(t) == 3 * 4096
    assert len(a + crlf + long_hdr) % 16 != 0
    u = b">u0 a file at a tile start\n" + g[20000:20100] + b"\n>u1\n" + g[20100:20130]
    dirty = (b">lower\n" + g[30000:30300].lower() + b"\n>mixed\n" + g[30300:30400] + b"N" * 57 + g[30400:30500] + b"\n" + g[30500:30600].lower() +
             b"\n>all_n\n" + b"N" * 100 + b"\n>short\nACGTAC\n>k_minus_1\n" + g[31000:31015] + b"\n>single\nA\n")
    pre = a + crlf + long_hdr
    fill = b">fill\n" + g[40000:40000 + (-(len(pre) + 7) % 4096)] + b"\n"                     # so that `t` starts at a tile start
    assert (len(pre) + len(fill)) % 4096 == 0
    return [a, crlf, long_hdr, fill, t, u, dirty]


def big_among_small():
    g = dna(11, 500_000)
    small = [b">s%d\n" % i + b"\n".join(g[j:j + 60] for j in range(1000 * i, 1000 * i + 700, 60)) + b"\n" for i in range(20)]
    big = b">big one above 384 KiB\n" + b"\n".join(g[j:j + 80] for j in range(0, 450_000, 80)) + b"\n"
    return [b"".join(small[:10]) + big + b"".join(small[10:])]


def many_records(n=100_000):
    rng = random.Random(5)
    g = dna(13, 2_000_000)
    out = []
    for i in range(n):
        s, ln = rng.randrange(0, len(g) - 300), rng.randint(30, 300)
        out.append(b">r%d\n%s\n" % (i, g[s:s + ln]))
    return [b"".join(out)]


@pytest.fixture(scope="module")
def ctx():
    c = lash_amd.Context(0)
    yield c
    c.close()


# ---- index ---------------------------------------------------------------------------------------------------------------------------
def check_index(ctx, files):
    import torch
    raw = np.frombuffer(b"".join(files), np.uint8)
    off = offsets(files)
    want = split(files)
    got = ctx.fasta_index(raw, off)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    got_dev = ctx.fasta_index(d_raw, off, device=True)
    for name, w, g, gd in zip(("start", "id_len", "file"), want, got, got_dev):
        assert w.dtype == g.dtype and np.array_equal(w, g), name
        assert np.array_equal(g, gd), name + " (device bytes)"
    return want


@pytest.mark.parametrize("which", ["edges", "edges_one_by_one", "big_among_small", "many"])
def test_index_equals_the_python_splitter(ctx, which):
    if which == "edges":
        start, id_len, fidx = check_index(ctx, edge_files())
        ids = [b"".join(edge_files())[int(s) + 1:int(s) + 1 + int(n)] for s, n in zip(start, id_len)]
        assert b"" in ids and b"r2>with>gt" in ids and b"last_has_no_newline" in ids and b"c1" in ids and len(ids[ids.index(b"c1") + 2]) == 14
        assert any(n == 10_004 for n in id_len)
        for want_id in (b"ends_at_tab", b"tab_then_nothing", b"c5_tab", b"c6", b"ends_at_space", b"c3_header_only", b"r1"):   # TAB, space, CR, LF
            assert want_id in ids, want_id
        assert {int(s) % 4096 for s in start} >= {0, 16}
    elif which == "edges_one_by_one":
        for f in edge_files():
            check_index(ctx, [f])
    elif which == "big_among_small":
        assert len(check_index(ctx, big_among_small())[1]) == 21
    else:
        assert len(check_index(ctx, many_records())[1]) == 100_000


def test_index_refuses_what_is_not_fasta(ctx):
    fq = b"@r\nACGT\n+\nIIII\n"
    fa = b">a\nACGT\n"
    for files in ([fq], [fa, fq], [fa, b"ACGT\n"]):
        with pytest.raises(lash_amd.LashError) as e:
            ctx.fasta_index(np.frombuffer(b"".join(files), np.uint8), offsets(files))
        assert e.value.code == lash_amd.EINVAL
    with pytest.raises(lash_amd.LashError) as e:
        ctx.sketch_records_raw("hmh", 12, 0, 42, np.frombuffer(fa, np.uint8), offsets([fa]), flags=lash_amd.F_AMINO)
    assert e.value.code == lash_amd.EINVAL
    start, id_len, fidx = ctx.fasta_index(np.frombuffer(fa, np.uint8), offsets([b"", fa, b""]))          # empty files hold no record
    assert list(start) == [0, len(fa)] and list(id_len) == [1] and list(fidx) == [1]


# ---- images --------------------------------------------------------------------------------------------------------------------------
def check_images(ctx, files, algo, k, p, step):
    raw = np.frombuffer(b"".join(files), np.uint8)
    buf = raw.tobytes()
    off = offsets(files)
    start = split(files)[0]
    n = len(start) - 1
    index = ctx.fasta_index(raw, off, keep=True)
    try:
        _check_images(ctx, index, raw, buf, off, start, n, algo, k, p, step)
    finally:
        index.free()


def _check_images(ctx, index, raw, buf, off, start, n, algo, k, p, step):
    assert index.n_records == n
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        seqs = [[record_seq(buf[int(start[r]):int(start[r + 1])])] for r in range(r0, r1)]
        seq, rec_off, goff = lash_amd.records_to_arrays(seqs)
        got = ctx.sketch_records_raw(algo, k, p, 42, raw, off, index=index, r0=r0, r1=r1)
        want = O.sketch_genomes(ALGO[algo], k, p, 42, seq, rec_off, goff, threads=16)
        assert got.shape == want.shape
        for i in np.nonzero((got != want).any(axis=1))[0]:
            raise AssertionError("%s k=%d: record %d differs from the oracle's image of that record alone" % (algo, k, r0 + i))
        batch = ctx.sketch_batch(algo, k, p, 42, seq, rec_off, goff)
        assert np.array_equal(got, batch), "differs from lash_sketch_batch with one record per genome"


@pytest.mark.parametrize("algo,k,p", CONFIGS)
@pytest.mark.parametrize("which", ["edges", "big_among_small", "many"])
def test_record_images_equal_the_oracle_and_the_batch_entry(ctx, which, algo, k, p):
    files = {"edges": edge_files, "big_among_small": big_among_small, "many": many_records}[which]()
    check_images(ctx, files, algo, k, p, 12_500 if which == "many" else 1 << 30)


@pytest.mark.parametrize("algo,k,p", CONFIGS)
def test_split_calls_give_the_same_bytes(ctx, algo, k, p):
    files = edge_files() + big_among_small()
    raw, off = np.frombuffer(b"".join(files), np.uint8), offsets(files)
    index = ctx.fasta_index(raw, off, keep=True)
    try:
        n = index.n_records
        whole = ctx.sketch_records_raw(algo, k, p, 42, raw, off)
        assert whole.shape[0] == n == len(split(files)[1])
        cuts = [0, 1, 2, 7, 8, n // 2, n - 1, n, n]
        parts = [ctx.sketch_records_raw(algo, k, p, 42, raw, off, index=index, r0=a, r1=b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole)
        # the same bytes at another host address: the index's device copy does not stand for them, they are sent again
        moved = raw.copy()
        assert np.array_equal(ctx.sketch_records_raw(algo, k, p, 42, moved, off, index=index, r0=1, r1=n - 1), whole[1:n - 1])
    finally:
        index.free()


# ---- command line --------------------------------------------------------------------------------------------------------------------
def run(*args, cwd=None):
    return subprocess.run([H.CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=900)


def cli_inputs(tmp_path, case):
    """-> (list of input paths, the records in output order)"""
    files = edge_files()
    if case == "two_files":
        datas = {"one.fa": b"".join(files[:3]), "two.fa": b"".join(files[3:]) + big_among_small()[0]}
    elif case == "gz":
        datas = {"multi.fa.gz": gzip.compress(b"".join(files) + big_among_small()[0], 1)}
    else:                                                   # larger than --stream-mb 1: ~ 2 MiB, many records
        datas = {"large.fa": many_records(8_000)[0] + big_among_small()[0]}
    paths, records = [], []
    for name, data in datas.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
        plain = gzip.decompress(data) if name.endswith(".gz") else data
        start = split([plain])[0]
        records += [plain[int(a):int(b)] for a, b in zip(start[:-1], start[1:])]
    return paths, records


@pytest.mark.parametrize("extra", [["--batch-mb", "1"], ["--devices", "0,0,0"]], ids=["batch1", "workers3"])
@pytest.mark.parametrize("case", ["two_files", "gz", "stream"])
def test_cli_per_record_equals_one_file_per_record(tmp_path, case, extra):
    paths, records = cli_inputs(tmp_path, case)
    lst = tmp_path / "multi.txt"
    lst.write_text("\n".join(paths) + "\n")
    ids = [re.compile(rb"[^ \t\r\n]*").match(r, 1).group().decode() for r in records]
    split_dir = tmp_path / "split"
    split_dir.mkdir()
    split_paths = []
    for i, r in enumerate(records):
        (split_dir / ("%06d.fa" % i)).write_bytes(r)
        split_paths.append(str(split_dir / ("%06d.fa" % i)))
    (tmp_path / "split.txt").write_text("\n".join(split_paths) + "\n")
    stream = ["--stream-mb", "1"] if case == "stream" else []
    for algo, k, p in (("hmh", 16, 10), ("ull", 16, 12)) if case != "stream" else (("hmh", 16, 10),):
        common = ["-a", algo, "-k", k, "-p", p, "-t", 4]
        a, b = str(tmp_path / ("rec_" + algo)), str(tmp_path / ("files_" + algo))
        r = run("sketch", "-f", lst, "-o", a, "--per-record", *common, *stream, *extra)
        assert r.returncode == 0, r.stderr
        assert "%d records" % len(records) in r.stderr
        r = run("sketch", "-f", tmp_path / "split.txt", "-o", b, *common)
        assert r.returncode == 0, r.stderr
        assert H.zstd_read(a + "_sketches.bin") == H.zstd_read(b + "_sketches.bin")
        assert json.load(open(a + "_files.json")) == ids
        assert open(a + "_parameters.json", "rb").read() == open(b + "_parameters.json", "rb").read()
        if algo == "hmh":
            rows = []
            for prefix in (a, b):
                out = prefix + "_dist.txt"                   # (dist looks its prefixes up in the working directory)
                name = os.path.basename(prefix)
                r = run("dist", "-q", name, "-r", name, "-o", out, "--max-dist", "0.2", "--file-order", "-t", 4, cwd=tmp_path)
                assert r.returncode == 0, r.stderr
                rows.append(open(out).read())
            name_of = dict(zip(split_paths, ids))
            assert len(set(ids)) == len(ids), "the generated ids are unique, so the mapping is one to one"
            mapped = "\n".join("\t".join(name_of.get(c, c) for c in line.split("\t")) for line in rows[1].split("\n"))
            assert rows[0] == mapped and rows[0].count("\n") > 0


def test_cli_refusals_name_the_file_and_leave_nothing(tmp_path):
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    fa = tmp_path / "ok.fa"
    fa.write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    lst = tmp_path / "l.txt"
    lst.write_text("%s\n%s\n" % (fa, fq))
    out = str(tmp_path / "o1")
    r = run("sketch", "-f", lst, "-o", out, "--per-record")
    assert r.returncode == 1 and str(fq) in r.stderr and "--per-record" in r.stderr and "FASTA" in r.stderr
    assert not os.path.exists(out + "_sketches.bin") and not os.path.exists(out + "_files.json") and not os.path.exists(out + "_parameters.json")
    # a record larger than the chunk: an error, not a silent merge
    big = tmp_path / "big.fa"
    big.write_bytes(b">small\nACGTACGT\n>the_big_one desc\n" + b"\n".join([dna(3, 80)] * 30_000) + b"\n>after\nACGT\n")
    lst.write_text("%s\n" % big)
    out = str(tmp_path / "o2")
    r = run("sketch", "-f", lst, "-o", out, "--per-record", "--stream-mb", "1")
    assert r.returncode == 1 and str(big) in r.stderr and "the_big_one" in r.stderr and "--stream-mb" in r.stderr
    assert not os.path.exists(out + "_sketches.bin") and not os.path.exists(out + "_files.json") and not os.path.exists(out + "_parameters.json")
