"""GPU tests of `lash sketch --min-count` (host/sketch_files.cpp): batches, .gz input, files streamed in chunks (read twice) and several
workers must all write the bytes lash_sketch_files_raw_filtered gives for the same files."""
import gzip
import json
import subprocess

import numpy as np
import pytest

import host_lib as H
import lash_amd
import min_count_model as MC
import oracle_lib as O

pytestmark = pytest.mark.gpu
ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}


def default_log2(n_bytes):
    l2 = 16
    while l2 < 36 and (1 << l2) < 8 * n_bytes:
        l2 += 1
    return l2


def abi_images(files, algo, k, p, M):
    ctx = lash_amd.Context(0)
    flt = ctx.kmer_filter([default_log2(len(f)) for f in files])
    try:
        flt.count(k, files)
        return ctx.sketch_files_raw_filtered(algo, k, p, 42, files, flt, M)
    finally:
        flt.free()
        ctx.close()


def run_cli(tmp_path, paths, tag, algo, k, p, extra):
    lst = tmp_path / (tag + ".txt")
    lst.write_text("\n".join(paths) + "\n")
    out = str(tmp_path / tag)
    r = subprocess.run([H.CLI, "sketch", "-f", str(lst), "-o", out, "-a", algo, "-k", str(k), "-p", str(p), "-s", "42", "-t", "4"] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.load(open(out + "_files.json")) == paths
    return H.zstd_read(out + "_sketches.bin"), r.stderr


@pytest.mark.parametrize("algo,k,p", [("hmh", 16, 10), ("hll", 21, 10), ("ull", 32, 12)])
def test_cli_equals_the_abi(tmp_path, algo, k, p):
    files = MC.read_files()
    want = abi_images(files, algo, k, p, 2)
    assert np.array_equal(want[0], MC.expected_image(ALGO[algo], k, p, 42, MC.kept_keys(MC.file_keys(files[0], k), default_log2(len(files[0])), 2)))
    plain, packed = [], []
    for i, f in enumerate(files):
        (tmp_path / ("r%d.fastq" % i)).write_bytes(f)
        (tmp_path / ("r%d.fastq.gz" % i)).write_bytes(gzip.compress(f))
        plain.append(str(tmp_path / ("r%d.fastq" % i)))
        packed.append(str(tmp_path / ("r%d.fastq.gz" % i)))
    blob, err = run_cli(tmp_path, plain, "plain", algo, k, p, ["--min-count", "2"])
    assert blob == want.tobytes()
    assert "count tables of 2^%d cells" % default_log2(len(files[0])) in err
    assert run_cli(tmp_path, packed, "gz", algo, k, p, ["--min-count", "2"])[0] == want.tobytes()
    assert run_cli(tmp_path, plain + packed, "two", algo, k, p, ["--min-count", "2", "--devices", "0,0", "--batch-mb", "1"])[0] == want.tobytes() * 2


def test_cli_streamed_file_is_read_twice(tmp_path):
    """a ~3 MB read file with --stream-mb 1: every chunk counted, then every chunk sketched, the same bytes as the file in one piece"""
    f = MC.read_files(seed=9, n_files=1, genome=20000, n_reads=9000)[0]
    assert len(f) > 5 * (1 << 19)
    algo, k, p, M = "hll", 21, 12, 3
    want = abi_images([f], algo, k, p, M)
    path, gz = tmp_path / "big.fastq", tmp_path / "big.fastq.gz"
    path.write_bytes(f)
    gz.write_bytes(gzip.compress(f, 1))
    whole, _ = run_cli(tmp_path, [str(path)], "whole", algo, k, p, ["--min-count", str(M)])
    assert whole == want.tobytes()
    assert run_cli(tmp_path, [str(path)], "chunks", algo, k, p, ["--min-count", str(M), "--stream-mb", "1"])[0] == whole
    assert run_cli(tmp_path, [str(gz)], "gzchunks", algo, k, p, ["--min-count", str(M), "--stream-mb", "1"])[0] == whole
