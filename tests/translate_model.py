"""`lash sketch --translate`: the six-frame translation rule, in Python, written from its text (include/lash_gfx950.h, lash_fasta_translate).

  sequence bytes  of a record: the bytes after the header line's LF up to the next record that are neither LF nor CR, in order: S[0..L)
  bases           ACGTacgt, case ignored; every other byte (N, U, '>' ...) is no base
  frames          f = 0, 1, 2 read S from offset f; f = 3, 4, 5 read the reverse complement R[t] = comp(S[L - 1 - t]) from offset f - 3 (a
                  no-base stays a no-base); frame f has max(0, (L - offset) // 3) codons, a trailing partial codon is dropped
  codons          three bases: NCBI table 1, a stop gives '*'; any no-base: 'X'.  '*' and 'X' are break bytes
  buffer          records in order, frames 0..5 in order, each frame its residues and one '*'
  segments        a segment ends after every break byte; seg_off[0] = 0; rec_seg[r] = the first segment of record r
"""
import re

import numpy as np

CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"      # base order T, C, A, G
CODON = {(a + b + c).encode(): CODE[16 * i + 4 * j + k].encode() for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
BREAKS = b"*X"


def records_of(data):
    """the records of one file: a record starts at the file's first byte and at every '>' whose preceding byte is a newline"""
    if not data:
        return []
    assert data[:1] == b">"
    starts = [m.start() for m in re.finditer(rb"(?<![^\n])>", data)] + [len(data)]
    return [data[a:b] for a, b in zip(starts[:-1], starts[1:])]


def record_id(rec):
    return re.compile(rb"[^ \t\r\n]*").match(rec, 1).group()


def sequence_bytes(rec):
    nl = rec.find(b"\n")
    return b"" if nl < 0 else rec[nl + 1:].replace(b"\n", b"").replace(b"\r", b"")


BASE_CODE = np.full(256, 4, np.uint8)                                           # T C A G -> 0..3, every other byte 4
BASE_CODE[np.frombuffer(b"TCAG", np.uint8)] = np.arange(4, dtype=np.uint8)
RESIDUE = np.frombuffer(CODE.encode(), np.uint8)


def translate_frame(s):
    """residues of the codons of s read from its first byte (s: upper case): CODON[s[i:i + 3]], 'X' where that is no codon of three bases;
    the same table looked up for all codons at once"""
    n = len(s) // 3
    c = BASE_CODE[np.frombuffer(s, np.uint8, 3 * n)].reshape(n, 3).astype(np.intp)
    return np.where((c > 3).any(axis=1), ord("X"), RESIDUE[(16 * c[:, 0] + 4 * c[:, 1] + c[:, 2]) & 63]).astype(np.uint8).tobytes()


def record_frames(s):
    """the six frames of a record's sequence bytes, unterminated"""
    fwd = s.upper()
    rev = s.translate(COMPLEMENT)[::-1].upper()
    return [translate_frame(x[o:]) for x in (fwd, rev) for o in (0, 1, 2)]


def record_buffer(s):
    out = b"".join(f + b"*" for f in record_frames(s))
    assert len(out) == 6 + 2 * max(0, len(s) - 2)
    return out


def segments_of(buf):
    """the segments of a buffer that ends with a break byte, each with its trailing break byte"""
    return [m.group() for m in re.finditer(rb"[^*X]*[*X]", buf)]


class Model:
    """files: list of file contents -> .buffer, .seg_off[n_seg + 1], .rec_seg[n_rec + 1], .rec_file[n_rec], .ids, .rec_segments (per record)"""

    def __init__(self, files):
        bufs, self.rec_file, self.ids, self.lengths = [], [], [], []
        for fi, f in enumerate(files):
            for rec in records_of(f):
                s = sequence_bytes(rec)
                bufs.append(record_buffer(s))
                self.rec_file.append(fi)
                self.ids.append(record_id(rec))
                self.lengths.append(len(s))
        self.n_files = len(files)
        self.buffer = b"".join(bufs)
        self.rec_segments = [segments_of(b) for b in bufs]
        brk = np.frombuffer(self.buffer, np.uint8)
        ends = np.nonzero((brk == ord("*")) | (brk == ord("X")))[0].astype(np.uint64) + np.uint64(1)
        self.seg_off = np.concatenate([np.zeros(1, np.uint64), ends])
        self.rec_seg = np.cumsum([0] + [len(x) for x in self.rec_segments]).astype(np.uint64)
        assert int(self.rec_seg[-1]) == len(self.seg_off) - 1 and int(self.seg_off[-1]) == len(self.buffer)

    def file_rec_off(self):
        """records of file g: [off[g], off[g + 1])"""
        return np.searchsorted(np.array(self.rec_file, np.int64), np.arange(self.n_files + 1)).astype(np.uint64)

    def group_arrays(self, group_rec_off):
        """(seq, rec_off, genome_rec_off) as lash_sketch_batch takes them: the records are the segments, genome g = the segments of records
        [group_rec_off[g], group_rec_off[g + 1])"""
        seq = np.frombuffer(self.buffer, np.uint8)
        return seq, self.seg_off, np.array([int(self.rec_seg[int(r)]) for r in group_rec_off], np.uint64)

    def group_segments(self, r0, r1):
        return [s for r in range(r0, r1) for s in self.rec_segments[r]]
