"""CPU model of `lash sketch --min-count` (include/lash_gfx950.h, "K-mer abundance filter"), numpy only.
Part 1: the keys of a file's records, their two cells in a table of 2^L saturating byte counters, the kept set.
Part 2: the expected sketch of a kept set is the ORACLE's sketch of a FASTA with one record of exactly k bases per kept key
(a k-base record yields exactly that one k-mer, and a canonical key is its own canonical k-mer).
Every function that forms or decodes a key takes an oracle_lib layout (None = the default): the base codes are layout.base_code, the
complement of a base is the code of the complementary letter, and under kmer=lsb a k-mer's first base sits in its least significant bits."""
import random

import numpy as np

import oracle_lib as O

MUL1, MUL2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)


def _codes(layout):
    """(byte -> 2-bit code table with 255 outside ACGT, code -> complement's code, code -> letter, lsb_first)"""
    base_code = [0, 1, 2, 3] if layout is None else [int(c) for c in layout.base_code]
    tab = np.full(256, 255, np.uint8)
    comp = np.zeros(4, np.uint64)
    letter = np.zeros(4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        tab[c] = base_code[i]
        comp[base_code[i]] = base_code[3 - i]                        # A <-> T, C <-> G
        letter[base_code[i]] = c
    return tab, comp, letter, bool(layout is not None and layout.kmer_lsb_first)


def fastx_records(data: bytes):
    """sequences of a well-formed FASTA (multi-line) / FASTQ file, line ends (LF or CRLF) stripped"""
    lines = [ln.rstrip(b"\r") for ln in data.split(b"\n")]
    if lines and lines[-1] == b"":
        lines.pop()
    if data[:1] == b"@":
        return [lines[i + 1] for i in range(0, len(lines), 4)]
    recs = []
    for ln in lines:
        if ln[:1] == b">":
            recs.append([])
        else:
            recs[-1].append(ln)
    return [b"".join(r) for r in recs]


def _window_keys(codes: np.ndarray, k: int, comp: np.ndarray, lsb: bool) -> np.ndarray:
    """min(k-mer, reverse complement) of every window of k consecutive codes"""
    codes = codes.astype(np.uint64)
    ccodes = comp[codes.astype(np.int64)]
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        first_high, first_low = np.uint64(2 * (k - 1 - j)), np.uint64(2 * j)
        fwd |= codes[j:j + n] << (first_low if lsb else first_high)
        rc |= ccodes[j:j + n] << (first_high if lsb else first_low)   # base j of the k-mer is base k-1-j of its reverse complement
    return np.minimum(fwd, rc)


def record_keys(rec: bytes, k: int, layout=None) -> np.ndarray:
    """masked canonical k-mer values of one record, as u64, one per occurrence: bytes outside ACGT deleted first (utils.rs:33-41),
    the k-mer's value under the layout's codes (first base in the most significant bits, or the least under kmer=lsb),
    min(k-mer, reverse complement)"""
    tab, comp, _, lsb = _codes(layout)
    codes = tab[np.frombuffer(rec, np.uint8)]
    return _window_keys(codes[codes < 4], k, comp, lsb)


def file_keys(data: bytes, k: int, layout=None) -> np.ndarray:
    """the keys of every record, in file order: the windows of the records' surviving bases laid end to end, without those that span two records"""
    recs = fastx_records(data)
    if not recs:
        return np.zeros(0, np.uint64)
    tab, comp, _, lsb = _codes(layout)
    codes = tab[np.frombuffer(b"".join(recs), np.uint8)]
    rec_of = np.repeat(np.arange(len(recs)), [len(r) for r in recs])[codes < 4]
    keys = _window_keys(codes[codes < 4], k, comp, lsb)
    return keys[rec_of[:len(keys)] == rec_of[k - 1:]]


def cell_addresses(keys: np.ndarray, L: int):
    with np.errstate(over="ignore"):
        i1 = (keys * MUL1) >> np.uint64(64 - L)
        i2 = ((keys ^ (keys >> np.uint64(32))) * MUL2) >> np.uint64(64 - L)
    return i1, i2


def occurrence_cells(keys: np.ndarray, L: int):
    """(c1, c2): the saturated value of each occurrence's two cells after the whole file has been counted"""
    i1, i2 = cell_addresses(keys, L)
    hits = np.concatenate([i1, i2[i2 != i1]])                    # i1 == i2: that cell once
    u, cnt = np.unique(hits, return_counts=True)
    cnt = np.minimum(cnt, 255)
    return cnt[np.searchsorted(u, i1)], cnt[np.searchsorted(u, i2)]


def cells_dense(keys: np.ndarray, L: int) -> np.ndarray:
    i1, i2 = cell_addresses(keys, L)
    hits = np.concatenate([i1, i2[i2 != i1]]).astype(np.int64)
    return np.minimum(np.bincount(hits, minlength=1 << L), 255).astype(np.uint8)


def kept_keys(keys: np.ndarray, L: int, M: int) -> np.ndarray:
    """sorted distinct keys of the occurrences the keep rule lets through"""
    if not len(keys):
        return keys
    c1, c2 = occurrence_cells(keys, L)
    return np.unique(keys[np.minimum(c1, c2) >= M])


def kept_occurrences(keys: np.ndarray, L: int, M: int) -> int:
    """how many OCCURRENCES the keep rule lets through (what the k-mer census of a filtered call counts)"""
    if not len(keys):
        return 0
    c1, c2 = occurrence_cells(keys, L)
    return int(np.count_nonzero(np.minimum(c1, c2) >= M))


def true_keys(keys: np.ndarray, M: int) -> np.ndarray:
    u, cnt = np.unique(keys, return_counts=True)
    return u[cnt >= M]


def keys_fasta(keys: np.ndarray, k: int, layout=None) -> bytes:
    """one record of exactly k bases per key, the key decoded under the layout: rows of ">k\n" + k letters + "\n" """
    if not len(keys):
        return b">none\n"
    _, _, letter, lsb = _codes(layout)
    keys = np.asarray(keys, np.uint64)
    rows = np.empty((len(keys), k + 4), np.uint8)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, k + 3] = ord(">"), ord("k"), ord("\n"), ord("\n")
    for j in range(k):
        sh = np.uint64(2 * j if lsb else 2 * (k - 1 - j))
        rows[:, 3 + j] = letter[((keys >> sh) & np.uint64(3)).astype(np.int64)]
    return rows.tobytes()


def expected_image(algo, k, p, seed, kept: np.ndarray, layout=None) -> np.ndarray:
    fa = keys_fasta(kept, k, layout)
    assert np.array_equal(np.unique(file_keys(fa, k, layout)), kept)   # part 1 agrees that this input's keys ARE the kept set
    return O.sketch_files(algo, k, p, seed, [fa], layout=layout)[0]


def read_files(seed=7, n_files=3, genome=4000, n_reads=134, read_len=150, fmt="fastq"):
    """per file: reads drawn from a random genome (~5x) with 1 % substitutions, an N in some reads, two reads shorter than any k"""
    rng = random.Random(seed)
    files = []
    for f in range(n_files):
        g = [rng.choice("ACGT") for _ in range(genome)]
        reads = []
        for r in range(n_reads):
            s = rng.randrange(genome - read_len + 1)
            rd = g[s:s + read_len]
            if rng.random() < 0.5:
                rd = ["TGCA"["ACGT".index(c)] for c in reversed(rd)]
            rd = [rng.choice("ACGT".replace(c, "")) if rng.random() < 0.01 else c for c in rd]
            if rng.random() < 0.06:
                rd[rng.randrange(read_len)] = "N"
            reads.append("".join(rd))
        reads.insert(n_reads // 3, "ACGTA")
        reads.insert(2 * n_reads // 3, "GATTACAGATTAC")
        if fmt == "fastq":
            files.append("".join("@r%d/%d\n%s\n+\n%s\n" % (f, i, rd, "I" * len(rd)) for i, rd in enumerate(reads)).encode())
        else:
            files.append("".join(">r%d/%d\n%s\n" % (f, i, rd) for i, rd in enumerate(reads)).encode())
    return files
