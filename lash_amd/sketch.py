"""Python face of the C ABI (include/lash_gfx950.h).  Mirrors the reference's sketch interface for the hot path:
`sketch_files::<S>(precision, files, k, out, threads, seed, aa)` (utils.rs:439-447) becomes
`Context.sketch_batch(algo, k, p, seed, records...)` returning the bytes `S::save` would write (utils.rs:571-573).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Layout, Params, Timing

ALGOS = {"hmh": _lib.HMH, "hll": _lib.HLL, "ull": _lib.ULL}
ULL_ESTIMATORS = {"fgra": 0, "ml": 1}


class HllBias:
    """HLL++ empirical bias tables (include/lash_gfx950.h: lash_hll_bias).  They are not part of this repository: load the
    text file tools/ref_probe/extract_hll_bias.py or `lash hll-bias` writes, build from arrays, or simulate them on the GPU
    (HllBias.simulated: regenerated numbers, not the crate's).  Without them the estimate <= 5 * 2^p regime of
    streaming_algorithms' len() is refused with ERANGE."""

    def __init__(self, path=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if path is not None:
            rc = self._lib.lash_hll_bias_load(str(path).encode(), C.byref(self._h))
            if rc != _lib.OK:
                raise LashError(rc, "%s: %s" % (path, self._lib.lash_strerror(rc).decode()))

    def set(self, p, raw, bias):
        r = np.ascontiguousarray(raw, dtype=np.float64)
        b = np.ascontiguousarray(bias, dtype=np.float64)
        assert r.shape == b.shape and r.ndim == 1
        rc = self._lib.lash_hll_bias_from_arrays(C.byref(self._h), int(p), r.ctypes.data, b.ctypes.data, len(r))
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())
        return self

    def has(self, p):
        return bool(self._lib.lash_hll_bias_has(self._h, int(p)))

    @classmethod
    def simulated(cls, ctx, ps, points=None, trials=None, seed=42):
        """Tables for the precisions `ps` (an int or an iterable) from Context.hll_bias_simulate"""
        tb = cls()
        for p in ([ps] if isinstance(ps, int) else ps):
            _, raw, bias = ctx.hll_bias_simulate(p, points, trials, seed)
            tb.set(p, raw, bias)
        return tb

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.lash_hll_bias_free(self._h)
            self._h = C.c_void_p()


def _bias_handle(hll_bias):
    return None if hll_bias is None else hll_bias._h


def sketch_cardinality(algo, p, image, layout=None, estimator="fgra", hll_bias=None):
    """Distinct-count estimate of ONE serialized sketch, as `lash dist` computes it per sketch (utils.rs:101-103, 213-217, 314-315):
    hmh LogLog-beta, hll `len()` (LashError(ERANGE) in the bias-table regime unless `hll_bias` covers p), ull FGRA / ML.  Host only."""
    lib = _lib.load()
    a = _algo(algo)
    lay = parse_layout(layout)
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    regs = img[header_bytes(a, lay):]
    if a == _lib.HMH:
        return float(lib.lash_hmh_cardinality(regs.ctypes.data, int(lay.hmh_reg_be)))
    if a == _lib.ULL:
        return float(lib.lash_ull_estimate(regs.ctypes.data, int(p), ULL_ESTIMATORS[estimator]))
    out = C.c_double()
    rc = lib.lash_hll_cardinality(regs.ctypes.data, int(p), _bias_handle(hll_bias), C.byref(out))
    if rc != _lib.OK:
        raise LashError(rc, lib.lash_strerror(rc).decode())
    return out.value


MEASURES = {None: _lib.MEASURE_JACCARD, "jaccard": _lib.MEASURE_JACCARD, "query": _lib.MEASURE_CONTAIN_QUERY,
            "reference": _lib.MEASURE_CONTAIN_REFERENCE}


def dist_rows(algo, p, k, model, ref_card, qry_card, c_or_zero=None, n_counts=None, sum_or_union=None, fp32=False, hll_bias=None,
              hmh_ec=None, containment=None):
    """The distances the reference prints for an [n_ref, n_qry] block, from the GPU's pair statistics and the per-sketch
    cardinalities (lash_dist_rows; utils.rs:164-167, 272-278, 355-365 + main.rs:415-423).  numpy in, float64 [n_ref, n_qry] out.
    containment: None (the Jaccard-derived distance), "query" or "reference": `lash dist --containment` (lash_dist_rows_measure)."""
    lib = _lib.load()
    rc_ = np.ascontiguousarray(ref_card, dtype=np.float64)
    qc_ = np.ascontiguousarray(qry_card, dtype=np.float64)
    nr, nq = len(rc_), len(qc_)
    a = None if c_or_zero is None else np.ascontiguousarray(c_or_zero, dtype=np.uint32)
    b = None if n_counts is None else np.ascontiguousarray(n_counts, dtype=np.uint32)
    d = None if sum_or_union is None else np.ascontiguousarray(sum_or_union, dtype=np.float64)
    out = np.zeros((nr, nq), dtype=np.float64)
    bad = C.c_uint64()
    ec = None if hmh_ec is None else np.ascontiguousarray(hmh_ec, dtype=np.float64)       # (kept alive across the call)
    assert ec is None or ec.size == nr * nq
    rc = lib.lash_dist_rows_measure(_algo(algo), int(p or 0), int(k), int(model), 1 if fp32 else 0, nr, nq, rc_.ctypes.data, qc_.ctypes.data,
                                    None if a is None else a.ctypes.data, None if b is None else b.ctypes.data,
                                    None if d is None else d.ctypes.data, _bias_handle(hll_bias),
                                    None if ec is None else ec.ctypes.data, MEASURES[containment], out.ctypes.data, C.byref(bad))
    if rc != _lib.OK:
        raise LashError(rc, lib.lash_strerror(rc).decode() + (" (pair %d)" % bad.value if rc == _lib.ERANGE else ""))
    return out


class PinnedArray:
    """numpy view of page-locked host memory from lash_host_alloc_pinned (freed with the object)"""

    def __init__(self, nbytes, dtype=np.uint8):
        self._lib = _lib.load()
        self._p = self._lib.lash_host_alloc_pinned(int(max(nbytes, 1)))
        if not self._p:
            raise MemoryError("lash_host_alloc_pinned(%d)" % nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * int(max(nbytes, 1))).from_address(self._p)).view(dtype)

    def __del__(self):
        try:
            if self._p:
                self._lib.lash_host_free_pinned(self._p)
                self._p = None
        except Exception:
            pass


def ull_estimate(registers, p, estimator="fgra"):
    """FGRA / ML distinct-count estimate of ONE UltraLogLog sketch from its 2^p register bytes (host only; utils.rs:213-217)."""
    regs = np.ascontiguousarray(registers, dtype=np.uint8)
    assert regs.size == 1 << int(p)
    return float(_lib.load().lash_ull_estimate(regs.ctypes.data, int(p), ULL_ESTIMATORS[estimator]))


class LashError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lash error %d: %s" % (code, msg))
        self.code = code


def _algo(a):
    if isinstance(a, str):
        if a not in ALGOS:
            # main.rs:245 panics with this text
            raise LashError(_lib.EINVAL, "Algorithm must be either hmh, ull, or hll")
        return ALGOS[a]
    return int(a)


def parse_layout(spec):
    """"key=value,..." (see lash_layout_parse in include/lash_gfx950.h) -> Layout; None / "" = the default."""
    if isinstance(spec, Layout):
        return spec
    lay = Layout()
    rc = _lib.load().lash_layout_parse((spec or "").encode(), C.byref(lay))
    if rc != _lib.OK:
        raise LashError(rc, "bad layout spec %r" % (spec,))
    return lay


def image_bytes(algo, p=0, layout=None):
    if layout is None:
        return int(_lib.load().lash_sketch_image_bytes(_algo(algo), int(p)))
    return int(_lib.load().lash_layout_image_bytes(C.byref(parse_layout(layout)), _algo(algo), int(p)))


def header_bytes(algo, layout=None):
    lay = parse_layout(layout)
    return int(_lib.load().lash_layout_header_bytes(C.byref(lay), _algo(algo)))


def params_check(algo, k, p=0):
    prm = Params(_algo(algo), int(k), int(p), 0, 0)
    return int(_lib.load().lash_params_check(C.byref(prm)))


def records_to_arrays(genomes):
    """genomes: list of lists of record byte strings -> (seq u8, rec_off u64, genome_rec_off u64)."""
    recs = [r for g in genomes for r in g]
    seq = np.frombuffer(b"".join(recs), dtype=np.uint8).copy() if recs else np.zeros(0, np.uint8)
    rec_off = np.zeros(len(recs) + 1, dtype=np.uint64)
    if recs:
        rec_off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    goff = np.zeros(len(genomes) + 1, dtype=np.uint64)
    if genomes:
        goff[1:] = np.cumsum([len(g) for g in genomes], dtype=np.uint64)
    return seq, rec_off, goff


def _ptr(x):
    """device pointer of a torch tensor / raw int, or host pointer of a numpy array"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


class Packed:
    """Device-resident 2-bit genomes (lash_packed*)."""

    def __init__(self, ctx, handle, n_genomes):
        self._ctx, self._h, self.n_genomes = ctx, handle, n_genomes

    @property
    def device_bytes(self):
        return int(_lib.load().lash_packed_bytes(self._h))

    def free(self):
        if self._h:
            _lib.load().lash_packed_free(self._ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceIndex:
    """what the device-resident results of the fasta_* stages share: the context, the C handle, how a table is copied out and how it all is freed"""
    _FREE = None                                                     # name of the C function that frees the handle

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle

    def _copy(self, fn, n, dtype):
        out = np.zeros(n, dtype)
        self._ctx._check(getattr(_lib.load(), fn)(self._ctx._h, self._h, out.ctypes.data))
        return out

    def free(self):
        if self._h:
            getattr(_lib.load(), self._FREE)(self._ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WindowIndex(_DeviceIndex):
    """Device-resident windows of the records of a RecordIndex, rewritten as one-record FASTA files (lash_win_index*)."""
    _FREE = "lash_win_index_free"

    def __init__(self, ctx, handle):
        super().__init__(ctx, handle)
        self.n_windows = int(_lib.load().lash_win_index_n_windows(handle))
        self.nbytes = int(_lib.load().lash_win_index_bytes(handle))

    def arrays(self):
        """(record[n], begin[n], length[n]) u64, each one copy to the host"""
        return tuple(self._copy("lash_win_index_" + t, self.n_windows, np.uint64) for t in ("record", "begin", "length"))

    def offsets(self):
        """offset[n + 1] u64: where every window's file starts in the device buffer"""
        return self._copy("lash_win_index_offset", self.n_windows + 1, np.uint64)

    @property
    def device_ptr(self):
        return _lib.load().lash_win_index_buffer_device(self._h) or 0


class TranslatedIndex(_DeviceIndex):
    """Device-resident six-frame translation of the records of a RecordIndex, cut into segments at stops and ambiguous codons
    (lash_tr_index*)."""
    _FREE = "lash_tr_index_free"

    def __init__(self, ctx, handle, n_records):
        super().__init__(ctx, handle)
        self.n_records = int(n_records)
        self.n_segments = int(_lib.load().lash_tr_index_n_segments(handle))
        self.nbytes = int(_lib.load().lash_tr_index_bytes(handle))

    def arrays(self):
        """(seg_off[n_segments + 1], rec_seg[n_records + 1]) u64, each one copy to the host"""
        return self._copy("lash_tr_index_seg_off", self.n_segments + 1, np.uint64), self._copy("lash_tr_index_rec_seg", self.n_records + 1, np.uint64)

    @property
    def device_ptr(self):
        return _lib.load().lash_tr_index_buffer_device(self._h) or 0


class RecordIndex(_DeviceIndex):
    """Device-resident record index of raw multi-FASTA bytes (lash_rec_index*)."""
    _FREE = "lash_rec_index_free"

    def __init__(self, ctx, handle):
        super().__init__(ctx, handle)
        self.n_records = int(_lib.load().lash_rec_index_n_records(handle))

    def arrays(self):
        """(start[n + 1] u64, id_len[n] u32, file[n] u32), each one copy to the host"""
        n = self.n_records
        return (self._copy("lash_rec_index_start", n + 1, np.uint64), self._copy("lash_rec_index_id_len", n, np.uint32),
                self._copy("lash_rec_index_file", n, np.uint32))


class KmerFilter:
    """lash_kmer_filter: per-file k-mer count tables (Context.kmer_filter) — count() adds files or chunks of them, counts() reads
    a file's cells, Context.sketch_files_raw_filtered applies the keep rule."""

    def __init__(self, ctx, handle, log2_cells):
        self._ctx, self._h = ctx, handle
        self.log2_cells = [int(x) for x in log2_cells]

    def count(self, k, files_bytes):
        """adds every valid k-mer occurrence of files_bytes (one entry per file of the filter; b"" adds nothing) to the tables"""
        prm = Context._params("hmh", k, 0, 0, 0)
        raw, off, fmt = _raw_files(files_bytes, empty_ok=True)
        self._ctx._check_einval(self._ctx._lib.lash_kmer_filter_count_raw(self._ctx._h, C.byref(prm), raw.ctypes.data if raw.size else None,
                                                                          off.ctypes.data, fmt.ctypes.data if fmt.size else None, len(files_bytes), self._h))

    def counts(self, file):
        out = np.zeros(1 << self.log2_cells[file], dtype=np.uint8)
        self._ctx._check(self._ctx._lib.lash_kmer_filter_counts(self._ctx._h, self._h, int(file), out.ctypes.data))
        return out

    def free(self):
        if self._h is not None and getattr(self._ctx, "_h", None):
            self._ctx._lib.lash_kmer_filter_free(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _raw_files(files_bytes, empty_ok=False):
    """file contents -> (raw bytes back to back, offsets, formats) as lash_sketch_files_raw takes them; empty_ok: b"" stands for a file
    that has nothing in this call (a chunk of a batch streamed in pieces)"""
    raw = np.frombuffer(b"".join(files_bytes), dtype=np.uint8) if files_bytes else np.zeros(0, np.uint8)
    off = np.zeros(len(files_bytes) + 1, dtype=np.uint64)
    if files_bytes:
        off[1:] = np.cumsum([len(f) for f in files_bytes], dtype=np.uint64)
    for f in files_bytes:                                   # parse_fastx_file(..).expect("Invalid input file"), utils.rs:453
        if f[:1] not in (b">", b"@") and not (empty_ok and not f):
            raise LashError(_lib.EINVAL, "Invalid input file: the first byte must be '>' (FASTA) or '@' (FASTQ)")
    fmt = np.array([_lib.FMT_FASTQ if f[:1] == b"@" else _lib.FMT_FASTA for f in files_bytes], dtype=np.uint8)
    return raw, off, fmt


class Context:
    """One lash_ctx: a GPU, a stream and the HBM workspace.  Not thread-safe (like the C object)."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.lash_ctx_create(C.byref(h), int(device))
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())
        self._h = h
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    # -- plumbing ---------------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _lib.OK:
            detail = self._lib.lash_ctx_last_error(self._h).decode() if rc in (_lib.EHIP, _lib.ENOMEM) else ""
            raise LashError(rc, self._lib.lash_strerror(rc).decode() + (": " + detail if detail else ""))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lash_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream):
        """stream: a raw hipStream_t as int, or an object with .cuda_stream (torch.cuda.Stream); None = own stream"""
        ptr = None if stream is None else int(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.lash_ctx_set_stream(self._h, ptr))

    def synchronize(self):
        self._check(self._lib.lash_ctx_synchronize(self._h))

    def set_layout(self, layout=None):
        """layout: None (default), a spec string, or a Layout.  Every later call reads / writes images in that layout."""
        self._layout = None if layout is None else parse_layout(layout)
        self._check(self._lib.lash_ctx_set_layout(self._h, None if self._layout is None else C.byref(self._layout)))

    def image_bytes(self, algo, p=0):
        return image_bytes(algo, p, getattr(self, "_layout", None))

    def enable_timing(self, on=True):
        self._check(self._lib.lash_ctx_enable_timing(self._h, 1 if on else 0))

    def timing(self):
        t = Timing()
        self._check(self._lib.lash_ctx_get_timing(self._h, C.byref(t)))
        return {f[0]: getattr(t, f[0]) for f in Timing._fields_ if f[0] != "reserved"}

    @staticmethod
    def _params(algo, k, p, seed, flags):
        return Params(_algo(algo), int(k), int(p or 0), int(flags), int(seed) & (2**64 - 1))

    # -- hot path ---------------------------------------------------------------------------------------------
    def sketch_batch(self, algo, k, p, seed, seq, rec_off, genome_rec_off, flags=0, out=None):
        """Host buffers in, images[n_genomes, image_bytes] (numpy uint8) out."""
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_params_check(C.byref(prm)))
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        n_g, n_rec = len(goff) - 1, len(rec_off) - 1
        ib = self.image_bytes(prm.algo, prm.p)
        if out is None:
            out = np.zeros((n_g, ib), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size == n_g * ib and out.flags.c_contiguous
        seq_p = seq.ctypes.data if seq.size else None
        self._check(self._lib.lash_sketch_batch(self._h, C.byref(prm), seq_p, rec_off.ctypes.data, n_rec,
                                                goff.ctypes.data, n_g, out.ctypes.data if out.size else None))
        return out

    def sketch_batch_async(self, algo, k, p, seed, seq, rec_off, genome_rec_off, out, flags=0):
        """lash_sketch_batch_async: queue one batch (host buffers in, images into `out`) and return; synchronize() before
        reading `out` or touching seq / rec_off.  Pass page-locked arrays (pinned_array) for the copies to overlap."""
        prm = self._params(algo, k, p, seed, flags)
        assert seq.dtype == np.uint8 and rec_off.dtype == np.uint64 and out.dtype == np.uint8
        assert seq.flags.c_contiguous and rec_off.flags.c_contiguous and out.flags.c_contiguous
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        self._keep_async = getattr(self, "_keep_async", [])[-4:] + [(seq, rec_off, out)]
        self._check(self._lib.lash_sketch_batch_async(self._h, C.byref(prm), seq.ctypes.data if seq.size else None, rec_off.ctypes.data,
                                                      len(rec_off) - 1, goff.ctypes.data, len(goff) - 1, out.ctypes.data if out.size else None))

    def sketch_files_raw(self, algo, k, p, seed, files_bytes, flags=0):
        """files_bytes: list of uncompressed FASTA / FASTQ file contents (bytes).  The parse runs on the GPU.
        Returns images[n_files, image_bytes]."""
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_params_check(C.byref(prm)))
        raw, off, fmt = _raw_files(files_bytes)
        ib = self.image_bytes(prm.algo, prm.p)
        out = np.zeros((len(files_bytes), ib), dtype=np.uint8)
        self._check(self._lib.lash_sketch_files_raw(self._h, C.byref(prm), raw.ctypes.data if raw.size else None,
                                                    off.ctypes.data, fmt.ctypes.data if fmt.size else None,
                                                    len(files_bytes), out.ctypes.data if out.size else None))
        return out

    def _check_einval(self, rc):
        if rc == _lib.EINVAL:
            raise LashError(rc, self._lib.lash_ctx_last_error(self._h).decode() or self._lib.lash_strerror(rc).decode())
        self._check(rc)

    def kmer_filter(self, log2_cells):
        """lash_kmer_filter_create: one count table of 2^L cells per file (`lash sketch --min-count`)"""
        l2 = np.ascontiguousarray(log2_cells, dtype=np.uint8)
        h = C.c_void_p()
        self._check(self._lib.lash_kmer_filter_create(self._h, len(l2), l2.ctypes.data if l2.size else None, C.byref(h)))
        return KmerFilter(self, h, l2)

    def sketch_files_raw_filtered(self, algo, k, p, seed, files_bytes, kmer_filter, min_count, flags=0, out=None):
        """lash_sketch_files_raw_filtered: sketch_files_raw with the k-mers whose two cells in `kmer_filter` are not both >= min_count
        left out.  out: images to union into (with F_ACCUMULATE).  Returns images[n_files, image_bytes]."""
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_params_check(C.byref(prm)))
        raw, off, fmt = _raw_files(files_bytes, empty_ok=True)
        if out is None:
            out = np.zeros((len(files_bytes), self.image_bytes(prm.algo, prm.p)), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        self._check_einval(self._lib.lash_sketch_files_raw_filtered(self._h, C.byref(prm), raw.ctypes.data if raw.size else None, off.ctypes.data,
                                                                    fmt.ctypes.data if fmt.size else None, len(files_bytes), kmer_filter._h,
                                                                    int(min_count), out.ctypes.data if out.size else None))
        return out

    def _fasta_stage(self, name, raw, file_off, device, *args):
        """what the fasta_* methods share: lash_<name>[_device](ctx, raw, file_off, n_files, *args, &handle) -> handle.  raw: uint8 array (or
        bytes) of the files back to back — device=True: a device pointer / torch tensor; file_off: n_files + 1 byte offsets."""
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        if not device:
            raw = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
            assert raw.size >= int(off[-1])
        h = C.c_void_p()
        fn = getattr(self._lib, name + ("_device" if device else ""))
        self._check_einval(fn(self._h, _ptr(raw) if int(off[-1]) else None, off.ctypes.data, len(off) - 1, *args, C.byref(h)))
        return h

    @staticmethod
    def _kept_or_arrays(index, keep):
        if keep:
            return index
        try:
            return index.arrays()
        finally:
            index.free()

    def fasta_index(self, raw, file_off, device=False, keep=False):
        """lash_fasta_index: the records of raw multi-FASTA bytes, found on the GPU.  raw: uint8 array (or bytes) of the files back to
        back — device=True: a device pointer / torch tensor; file_off: n_files + 1 byte offsets.  Returns (start[n + 1] u64,
        id_len[n] u32, file[n] u32); keep=True returns a RecordIndex (for sketch_records_raw) instead."""
        return self._kept_or_arrays(RecordIndex(self, self._fasta_stage("lash_fasta_index", raw, file_off, device)), keep)

    def fasta_windows(self, raw, file_off, index, window, device=False, keep=False):
        """lash_fasta_windows: the records of `index` (a RecordIndex made from the same raw / file_off) cut into windows of `window` bases
        on the GPU.  raw as for fasta_index.  Returns (record[n], begin[n], length[n]) u64; keep=True returns a WindowIndex (for
        sketch_windows) instead."""
        return self._kept_or_arrays(WindowIndex(self, self._fasta_stage("lash_fasta_windows", raw, file_off, device, index._h, int(window))), keep)

    def sketch_windows(self, algo, k, p, seed, windows, w0=0, w1=None, flags=0):
        """lash_sketch_windows_raw: one image per window, windows [w0, w1) of a WindowIndex.  Returns images[w1 - w0, image_bytes]."""
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_params_check(C.byref(prm)))
        if w1 is None:
            w1 = windows.n_windows
        out = np.zeros((max(int(w1) - int(w0), 0), self.image_bytes(prm.algo, prm.p)), dtype=np.uint8)
        self._check_einval(self._lib.lash_sketch_windows_raw(self._h, C.byref(prm), windows._h, int(w0), int(w1),
                                                             out.ctypes.data if out.size else None))
        return out

    def fasta_translate(self, raw, file_off, index, device=False, keep=False):
        """lash_fasta_translate: the six reading frames of the records of `index` (a RecordIndex made from the same raw / file_off),
        translated on the GPU and cut into segments at stops and ambiguous codons.  raw as for fasta_index.  Returns
        (seg_off[n_segments + 1], rec_seg[n_records + 1]) u64; keep=True returns a TranslatedIndex (for sketch_translated) instead."""
        h = self._fasta_stage("lash_fasta_translate", raw, file_off, device, index._h)
        return self._kept_or_arrays(TranslatedIndex(self, h, index.n_records), keep)

    def sketch_translated(self, algo, k, p, seed, translated, group_rec_off=None, flags=0, out=None):
        """lash_sketch_translated: one amino-acid image per group of records of a TranslatedIndex; group g = records
        [group_rec_off[g], group_rec_off[g + 1]) (None: one group of all records).  out: images to union into (with F_ACCUMULATE).
        Returns images[n_groups, image_bytes]."""
        prm = self._params(algo, k, p, seed, flags)
        goff = np.ascontiguousarray([0, translated.n_records] if group_rec_off is None else group_rec_off, dtype=np.uint64)
        if out is None:
            out = np.zeros((max(len(goff) - 1, 0), self.image_bytes(prm.algo, prm.p)), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        self._check_einval(self._lib.lash_sketch_translated(self._h, C.byref(prm), translated._h, goff.ctypes.data, max(len(goff) - 1, 0),
                                                            out.ctypes.data if out.size else None))
        return out

    def sketch_records_raw(self, algo, k, p, seed, raw, file_off, index=None, r0=0, r1=None, flags=0):
        """lash_sketch_records_raw: one image per FASTA record of raw (host bytes), records [r0, r1) of `index` (a RecordIndex made
        from the same raw / file_off; None: made here).  Returns images[r1 - r0, image_bytes]."""
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_params_check(C.byref(prm)))
        raw = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        own = index is None
        if own:
            index = self.fasta_index(raw, off, keep=True)
        try:
            if r1 is None:
                r1 = index.n_records
            out = np.zeros((max(int(r1) - int(r0), 0), self.image_bytes(prm.algo, prm.p)), dtype=np.uint8)
            self._check(self._lib.lash_sketch_records_raw(self._h, C.byref(prm), raw.ctypes.data if raw.size else None, off.ctypes.data,
                                                          len(off) - 1, index._h, int(r0), int(r1), out.ctypes.data if out.size else None))
        finally:
            if own:
                index.free()
        return out

    def format_errors(self):
        """indices of the files of the last raw call whose FASTQ structure broke (lash_ctx_format_errors)"""
        n = int(self._lib.lash_ctx_format_errors(self._h, None, 0))
        idx = (C.c_uint32 * max(n, 1))()
        self._lib.lash_ctx_format_errors(self._h, idx, n)
        return [int(idx[i]) for i in range(n)]

    def hll_inexact_sums(self):
        """genomes of the last HyperLogLog sketch call with a register above 53 - p (include/lash_gfx950.h:
        lash_ctx_hll_inexact_sums); synchronizes the stream"""
        n = int(self._lib.lash_ctx_hll_inexact_sums(self._h, None, 0))
        idx = (C.c_uint32 * max(n, 1))()
        self._lib.lash_ctx_hll_inexact_sums(self._h, idx, n)
        return [int(idx[i]) for i in range(n)]

    def hll_replay_sums_device(self, k, p, seed, d_seq, d_rec_off, n_rec, genome_rec_off, d_images, flags=0):
        """After sketch_batch_device("hll", ...) with the same arguments: the genomes hll_inexact_sums() lists get the `sum` the
        reference's incremental rule leaves (include/lash_gfx950.h: lash_hll_replay_sums_device); synchronizes."""
        prm = self._params("hll", k, p, seed, flags)
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        self._check(self._lib.lash_hll_replay_sums_device(self._h, C.byref(prm), _ptr(d_seq), _ptr(d_rec_off), int(n_rec),
                                                          goff.ctypes.data_as(C.c_void_p), len(goff) - 1, _ptr(d_images)))

    def sketch_batch_device(self, algo, k, p, seed, d_seq, d_rec_off, n_rec, genome_rec_off, genome_byte_off, d_out,
                            flags=0):
        """Device-resident records in, device images out; asynchronous on the context's stream."""
        prm = self._params(algo, k, p, seed, flags)
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        gbo = np.ascontiguousarray(genome_byte_off, dtype=np.uint64)
        assert len(goff) == len(gbo)
        self._keep = (goff, gbo)
        self._check(self._lib.lash_sketch_batch_device(self._h, C.byref(prm), _ptr(d_seq), _ptr(d_rec_off), int(n_rec),
                                                       goff.ctypes.data, gbo.ctypes.data, len(goff) - 1, _ptr(d_out)))

    def pack_device(self, d_seq, d_rec_off, n_rec, genome_rec_off, genome_byte_off):
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        gbo = np.ascontiguousarray(genome_byte_off, dtype=np.uint64)
        h = C.c_void_p()
        self._check(self._lib.lash_pack_device(self._h, _ptr(d_seq), _ptr(d_rec_off), int(n_rec), goff.ctypes.data,
                                               gbo.ctypes.data, len(goff) - 1, C.byref(h)))
        return Packed(self, h, len(goff) - 1)

    def sketch_packed_device(self, algo, k, p, seed, packed, d_out, flags=0):
        prm = self._params(algo, k, p, seed, flags)
        self._check(self._lib.lash_sketch_packed_device(self._h, C.byref(prm), packed._h, _ptr(d_out)))

    def merge_images_device(self, algo, p, d_dst, d_src, n_images):
        self._check(self._lib.lash_merge_images_device(self._h, _algo(algo), int(p or 0), _ptr(d_dst), _ptr(d_src),
                                                       int(n_images)))

    def merge_images(self, algo, p, dst, src):
        """dst[i] = dst[i] U src[i] on the GPU; numpy uint8 arrays [n, image_bytes]; returns dst."""
        assert dst.dtype == np.uint8 and src.dtype == np.uint8 and dst.shape == src.shape
        assert dst.flags.c_contiguous and src.flags.c_contiguous
        n = dst.shape[0] if dst.ndim == 2 else 1
        self._check(self._lib.lash_merge_images(self._h, _algo(algo), int(p or 0), dst.ctypes.data, src.ctypes.data, n))
        return dst

    def hmh_pair_expected_collisions(self, ref_card, qry_card):
        """hyperminhash's expected_collisions(n, m) for every pair, float64 [n_ref, n_qry]; the 65 536-cell regime (both
        cardinalities <= 2^19) runs on the GPU (include/lash_gfx950.h)"""
        r = np.ascontiguousarray(ref_card, dtype=np.float64)
        q = np.ascontiguousarray(qry_card, dtype=np.float64)
        out = np.zeros((len(r), len(q)), dtype=np.float64)
        self._check(self._lib.lash_hmh_pair_expected_collisions(self._h, r.ctypes.data, len(r), q.ctypes.data, len(q), out.ctypes.data))
        return out

    def hmh_pair_counts(self, ref_images, qry_images):
        """HyperMinHash pair statistics (C, N) of serialized sketches: numpy uint8 [n, 32768] in, two uint32
        [n_ref, n_qry] arrays out (hyperminhash Sketch::similarity's register scan, utils.rs:164)."""
        ref = np.ascontiguousarray(ref_images, dtype=np.uint8)
        qry = np.ascontiguousarray(qry_images, dtype=np.uint8)
        ib = self.image_bytes("hmh")
        assert ref.ndim == 2 and qry.ndim == 2 and ref.shape[1] == ib and qry.shape[1] == ib
        c = np.zeros((ref.shape[0], qry.shape[0]), dtype=np.uint32)
        n = np.zeros_like(c)
        self._check(self._lib.lash_hmh_pair_counts(self._h, ref.ctypes.data, ref.shape[0], qry.ctypes.data, qry.shape[0],
                                                   c.ctypes.data, n.ctypes.data))
        return c, n

    def hll_pair_union_stats(self, p, ref_images, qry_images):
        """HyperLogLog union statistics of serialized sketches: numpy uint8 [n, 33 + 2^p] in; (zero uint32, sum float64)
        [n_ref, n_qry] out — what `len()` reads after `union` (utils.rs:355-363)."""
        ref = np.ascontiguousarray(ref_images, dtype=np.uint8)
        qry = np.ascontiguousarray(qry_images, dtype=np.uint8)
        ib = self.image_bytes("hll", p)
        assert ref.ndim == 2 and qry.ndim == 2 and ref.shape[1] == ib and qry.shape[1] == ib
        zero = np.zeros((ref.shape[0], qry.shape[0]), dtype=np.uint32)
        usum = np.zeros((ref.shape[0], qry.shape[0]), dtype=np.float64)
        self._check(self._lib.lash_hll_pair_union_stats(self._h, int(p), ref.ctypes.data, ref.shape[0], qry.ctypes.data,
                                                        qry.shape[0], zero.ctypes.data, usum.ctypes.data))
        return zero, usum

    # device-resident forms (asynchronous on the context's stream): image blocks and outputs are device pointers / torch tensors
    def hmh_pair_counts_device(self, d_ref, n_ref, d_qry, n_qry, d_c, d_n):
        self._check(self._lib.lash_hmh_pair_counts_device(self._h, _ptr(d_ref), int(n_ref), _ptr(d_qry), int(n_qry), _ptr(d_c), _ptr(d_n)))

    def hll_pair_union_stats_device(self, p, d_ref, n_ref, d_qry, n_qry, d_zero, d_sum):
        self._check(self._lib.lash_hll_pair_union_stats_device(self._h, int(p), _ptr(d_ref), int(n_ref), _ptr(d_qry), int(n_qry),
                                                               _ptr(d_zero), _ptr(d_sum)))

    def ull_pair_union_estimates_device(self, p, estimator, d_ref, n_ref, d_qry, n_qry, d_est):
        self._check(self._lib.lash_ull_pair_union_estimates_device(self._h, int(p), ULL_ESTIMATORS[estimator], _ptr(d_ref), int(n_ref),
                                                                   _ptr(d_qry), int(n_qry), _ptr(d_est)))

    def ull_pair_union_estimates(self, p, ref_images, qry_images, estimator="fgra"):
        """UltraLogLog: estimated distinct count of merge(ref_i, qry_j) for every pair (utils.rs:260-270): numpy uint8
        [n, header + 2^p] in, float64 [n_ref, n_qry] out."""
        ref = np.ascontiguousarray(ref_images, dtype=np.uint8)
        qry = np.ascontiguousarray(qry_images, dtype=np.uint8)
        ib = self.image_bytes("ull", p)
        assert ref.ndim == 2 and qry.ndim == 2 and ref.shape[1] == ib and qry.shape[1] == ib
        est = np.zeros((ref.shape[0], qry.shape[0]), dtype=np.float64)
        self._check(self._lib.lash_ull_pair_union_estimates(self._h, int(p), ULL_ESTIMATORS[estimator], ref.ctypes.data, ref.shape[0],
                                                            qry.ctypes.data, qry.shape[0], est.ctypes.data))
        return est

    def hll_bias_simulate(self, p, points=None, trials=None, seed=42):
        """One precision's HLL++ bias table by Monte-Carlo on the GPU (lash_hll_bias_simulate): (n uint64, raw, bias float64), one
        entry per checkpoint cardinality n_j = j * 5 * 2^p / (points - 1).  None = the defaults (min(200, 5 * 2^p + 1) points,
        2048 trials).  Deterministic in (p, points, trials, seed)."""
        n_pts = int(points) if points else int(self._lib.lash_hll_bias_default_points(int(p)))
        if not 0 <= n_pts < 2**32 or not 0 <= int(trials or 0) < 2**32:
            raise LashError(_lib.EINVAL, self._lib.lash_strerror(_lib.EINVAL).decode())
        n = np.zeros(max(n_pts, 1), dtype=np.uint64)
        raw = np.zeros(max(n_pts, 1), dtype=np.float64)
        bias = np.zeros(max(n_pts, 1), dtype=np.float64)
        self._check(self._lib.lash_hll_bias_simulate(self._h, int(p), n_pts, int(trials or 0), int(seed) & (2**64 - 1), n.ctypes.data,
                                                     raw.ctypes.data, bias.ctypes.data))
        return n, raw, bias

    # -- dist side, resident form (include/lash_gfx950.h: lash_sketch_set_*) ---------------------------------------------
    def sketch_set(self, algo, p, images, order=None):
        """N serialized sketches resident on the context's GPU: numpy uint8 [n, image_bytes] (uploaded once; `order` = member
        indices into images) or a CUDA torch tensor (adopted, not copied: keep it alive)."""
        return SketchSet(self, algo, p, images, order)

    def synth_genomes_device(self, first_genome, n_genomes, n_bases, d_out):
        self._check(self._lib.lash_synth_genomes_device(self._h, int(first_genome), int(n_genomes), int(n_bases),
                                                        _ptr(d_out)))


class SketchSet:
    """lash_sketch_set: the sketches of a `dist` run kept in HBM (reference: the two hash maps of utils.rs:107-127), with
    per-member cardinalities from GPU register histograms and pair statistics by row block, lower triangle aware."""

    def __init__(self, ctx, algo, p, images, order=None):
        self._ctx, self._lib = ctx, ctx._lib
        self.algo, self.p = _algo(algo), int(p or 0)
        h = C.c_void_p()
        ib = ctx.image_bytes(self.algo, self.p)
        if isinstance(images, np.ndarray):
            img = np.ascontiguousarray(images, dtype=np.uint8)
            assert img.ndim == 2 and img.shape[1] == ib
            o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
            n = img.shape[0] if o is None else len(o)
            ctx._check(self._lib.lash_sketch_set_create(ctx._h, self.algo, self.p, img.ctypes.data if img.size else None, img.shape[0],
                                                        None if o is None else o.ctypes.data, n, C.byref(h)))
        else:
            assert order is None and images.is_cuda and images.is_contiguous() and images.numel() % ib == 0
            self._keep = images
            n = images.numel() // ib
            ctx._check(self._lib.lash_sketch_set_create_device(ctx._h, self.algo, self.p, images.data_ptr() if n else None, n, C.byref(h)))
        self._h, self.n = h, n

    def free(self):
        if getattr(self, "_h", None) and self._ctx._h:
            self._lib.lash_sketch_set_free(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def cardinalities(self, estimator="fgra", hll_bias=None):
        out = np.zeros(self.n, dtype=np.float64)
        bad = C.c_uint32()
        rc = self._lib.lash_sketch_set_cardinalities(self._ctx._h, self._h, ULL_ESTIMATORS[estimator], _bias_handle(hll_bias),
                                                     out.ctypes.data, C.byref(bad))
        if rc == _lib.ERANGE:
            raise LashError(rc, self._lib.lash_strerror(rc).decode() + " (sketch %d)" % bad.value)
        self._ctx._check(rc)
        return out

    def prepare(self, qry=None):
        self._ctx._check(self._lib.lash_sketch_set_prepare(self._ctx._h, self._h, (qry or self)._h))

    def prefix_union_cardinalities(self, orders, estimator="fgra", hll_bias=None, slices=0, hist_budget_bytes=0):
        """`lash growth`: orders = uint32 [n_orders, len] member indices; float64 [n_orders, len] out, entry (o, t) the distinct-count
        estimate of members orders[o][0..t] united — the bits cardinalities() gives for the image of that union
        (lash_sketch_set_prefix_union_cardinalities).  slices / hist_budget_bytes: how the work is cut (0 = the library chooses); the
        numbers do not depend on them.  LASH_ERANGE / LASH_EINVAL raise a LashError whose .index is the refused position o * len + t."""
        o = np.ascontiguousarray(orders, dtype=np.uint32)
        assert o.ndim == 2
        out = np.zeros(o.shape, dtype=np.float64)
        opts = _lib.PrefixUnionOpts(int(slices), int(hist_budget_bytes))
        bad = C.c_uint64(2**64 - 1)
        rc = self._lib.lash_sketch_set_prefix_union_cardinalities(self._ctx._h, self._h, o.ctypes.data if o.size else None, o.shape[0], o.shape[1],
                                                                  ULL_ESTIMATORS[estimator], _bias_handle(hll_bias), C.byref(opts),
                                                                  out.ctypes.data if out.size else None, C.byref(bad))
        if rc != _lib.OK:
            msg = self._lib.lash_strerror(rc).decode() + (" (order %d, step %d)" % divmod(bad.value, o.shape[1]) if rc == _lib.ERANGE else "")
            last = self._lib.lash_ctx_last_error(self._ctx._h)
            e = LashError(rc, msg + (" " + last.decode() if rc == _lib.EINVAL and last else ""))
            e.index = bad.value
            raise e
        return out

    def _groups_csr(self, groups):
        if isinstance(groups, np.ndarray) and groups.ndim == 2:              # equal-sized groups as a matrix
            return np.arange(groups.shape[0] + 1, dtype=np.uint64) * np.uint64(groups.shape[1]), np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        off = np.zeros(len(groups) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64)
        mem = np.ascontiguousarray([m for g in groups for m in g], dtype=np.uint32)
        return off, mem

    def group_union(self, groups, segment=None, slices=None, scratch_budget=None, device_out=None):
        """`lash merge`: groups = a list of lists of member indices (overlaps, repeats and empty groups are fine); one image per group, the
        union of its members — byte for byte the fold of merge_images over them from the empty sketch (lash_sketch_set_group_union).
        Returns uint8 [n_groups, image_bytes]; with device_out (a CUDA uint8 tensor of that many bytes) the images are written there,
        asynchronously on the context's stream, and device_out is returned.  segment / slices / scratch_budget: how the work is cut
        (None = the library chooses); the bytes do not depend on them.  LASH_EINVAL for a bad member raises a LashError whose .index
        is its position in the flattened list."""
        off, mem = self._groups_csr(groups)
        opts = _lib.GroupUnionOpts(int(segment or 0), int(slices or 0), int(scratch_budget or 0))
        bad = C.c_uint64(2**64 - 1)
        ib = self._ctx.image_bytes(self.algo, self.p)
        mp = mem.ctypes.data if mem.size else None
        if device_out is None:
            out = np.zeros((len(groups), ib), dtype=np.uint8)
            rc = self._lib.lash_sketch_set_group_union(self._ctx._h, self._h, off.ctypes.data, mp, len(groups), C.byref(opts),
                                                       out.ctypes.data if out.size else None, C.byref(bad))
        else:
            assert device_out.is_cuda and device_out.is_contiguous() and device_out.numel() * device_out.element_size() >= len(groups) * ib
            out = device_out
            rc = self._lib.lash_sketch_set_group_union_device(self._ctx._h, self._h, off.ctypes.data, mp, len(groups), C.byref(opts),
                                                              device_out.data_ptr() if len(groups) else None, C.byref(bad))
        if rc != _lib.OK:
            last = self._lib.lash_ctx_last_error(self._ctx._h)
            e = LashError(rc, self._lib.lash_strerror(rc).decode() + (" " + last.decode() if last else ""))
            e.index = bad.value
            raise e
        return out

    def group_union_plan(self, groups, segment=None, slices=None, scratch_budget=None):
        """(segment, slices, scratch bytes) a group_union call with these arguments runs with (lash_sketch_set_group_union_plan)"""
        off, _ = self._groups_csr(groups)
        opts = _lib.GroupUnionOpts(int(segment or 0), int(slices or 0), int(scratch_budget or 0))
        plan = _lib.GroupUnionOpts()
        self._ctx._check(self._lib.lash_sketch_set_group_union_plan(self._ctx._h, self._h, off.ctypes.data, len(groups), C.byref(opts), C.byref(plan)))
        return int(plan.segment), int(plan.slices), int(plan.scratch_budget_bytes)

    def group_spectrum(self, groups, segment=None, slices=None, scratch_budget=None, union_images=False, device_out=None):
        """`lash spectrum` (HyperMinHash sets): groups as for group_union; per group a uint32 array of len(group) + 1 bins, bin c the
        buckets whose union register is held by exactly c members (bin 0: the empty buckets; the bins sum to 16 384): a uniform sample
        of the group's k-mer multiplicity spectrum (lash_sketch_set_group_spectrum).  union_images=True also returns group_union's
        images: (bins, uint8 [n_groups, image_bytes]).  segment / slices / scratch_budget: how the work is cut; the bins do not
        depend on them.  device_out = (a CUDA int32 / uint32 tensor of sum(len(g) + 1) words, a CUDA uint8 tensor of the images or
        None): both are written there, asynchronously on the context's stream, and device_out is returned.  LASH_EINVAL raises a
        LashError (an hll / ull set; a bad member, whose position in the flattened list is .index)."""
        off, mem = self._groups_csr(groups)
        opts = _lib.GroupUnionOpts(int(segment or 0), int(slices or 0), int(scratch_budget or 0))
        bad = C.c_uint64(2**64 - 1)
        ib = self._ctx.image_bytes(self.algo, self.p)
        mp = mem.ctypes.data if mem.size else None
        n_bins = int(off[-1]) + len(groups)
        if device_out is None:
            hist = np.zeros(n_bins, dtype=np.uint32)
            img = np.zeros((len(groups), ib), dtype=np.uint8) if union_images else None
            rc = self._lib.lash_sketch_set_group_spectrum(self._ctx._h, self._h, off.ctypes.data, mp, len(groups), C.byref(opts),
                                                          hist.ctypes.data if hist.size else None,
                                                          img.ctypes.data if img is not None and img.size else None, C.byref(bad))
        else:
            d_hist, d_img = device_out
            assert d_hist.is_cuda and d_hist.is_contiguous() and d_hist.element_size() == 4 and d_hist.numel() >= n_bins
            assert d_img is None or (d_img.is_cuda and d_img.is_contiguous() and d_img.numel() * d_img.element_size() >= len(groups) * ib)
            rc = self._lib.lash_sketch_set_group_spectrum_device(self._ctx._h, self._h, off.ctypes.data, mp, len(groups), C.byref(opts),
                                                                 d_hist.data_ptr() if len(groups) else None,
                                                                 d_img.data_ptr() if d_img is not None and len(groups) else None, C.byref(bad))
        if rc != _lib.OK:
            last = self._lib.lash_ctx_last_error(self._ctx._h)
            e = LashError(rc, self._lib.lash_strerror(rc).decode() + (" " + last.decode() if last else ""))
            e.index = bad.value
            raise e
        if device_out is not None:
            return device_out
        bins = [hist[int(off[g]) + g:int(off[g + 1]) + g + 1] for g in range(len(groups))]
        return (bins, img) if union_images else bins

    def screen_wta(self, qry, candidates, segment=None, slices=None, scratch_budget=None, device_out=None):
        """`lash screen` (HyperMinHash sets; called on the reference set): candidates = one list per row of `qry` of rows of this set, best
        first.  Reference i holds bucket b of a query iff the query's register there is not 0 and i's equals it; a bucket goes to the first
        candidate of the list that holds it.  Returns (shared, won), each a list of uint32 arrays, one per query: shared[j][t] the buckets
        position t of query j's list holds (the C of hmh_pair_counts), won[j][t] those it won (lash_sketch_set_screen_wta).  segment /
        slices / scratch_budget: how the work is cut; the counts do not depend on them.  device_out = (two CUDA int32 / uint32 tensors of
        sum(len(l)) words): both are written there, asynchronously on the context's stream, and device_out is returned.  LASH_EINVAL
        raises a LashError (an hll / ull set; a bad row, whose position in the flattened lists is .index)."""
        assert len(candidates) == qry.n
        off, mem = self._groups_csr(candidates)
        opts = _lib.GroupUnionOpts(int(segment or 0), int(slices or 0), int(scratch_budget or 0))
        bad = C.c_uint64(2**64 - 1)
        mp = mem.ctypes.data if mem.size else None
        n = int(off[-1])
        if device_out is None:
            shared, won = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            rc = self._lib.lash_sketch_set_screen_wta(self._ctx._h, self._h, qry._h, off.ctypes.data, mp, C.byref(opts),
                                                      shared.ctypes.data if n else None, won.ctypes.data if n else None, C.byref(bad))
        else:
            d_shared, d_won = device_out
            for d in device_out:
                assert d.is_cuda and d.is_contiguous() and d.element_size() == 4 and d.numel() >= n
            rc = self._lib.lash_sketch_set_screen_wta_device(self._ctx._h, self._h, qry._h, off.ctypes.data, mp, C.byref(opts),
                                                             d_shared.data_ptr() if n else None, d_won.data_ptr() if n else None, C.byref(bad))
        if rc != _lib.OK:
            last = self._lib.lash_ctx_last_error(self._ctx._h)
            e = LashError(rc, self._lib.lash_strerror(rc).decode() + (" " + last.decode() if last else ""))
            e.index = bad.value
            raise e
        if device_out is not None:
            return device_out
        cut = [(int(off[j]), int(off[j + 1])) for j in range(len(candidates))]
        return [shared[a:b] for a, b in cut], [won[a:b] for a, b in cut]

    def hmh_expected_collisions(self, r0, r1, qry=None, n_cols=None):
        """hyperminhash's expected collisions of the block's SMALL pairs (both sketches <= 2^19 distinct k-mers) as a float64
        [r1 - r0, n_cols] array for lash_dist_rows' hmh_ec (other entries are not read), or None when the block has none.
        cardinalities() must have run on both sets."""
        q = qry or self
        nc = q.n if n_cols is None else int(n_cols)
        out = np.empty((int(r1) - int(r0), nc), dtype=np.float64)
        cnt = C.c_uint64()
        self._ctx._check(self._lib.lash_sketch_set_hmh_expected_collisions(self._ctx._h, self._h, int(r0), int(r1), q._h, nc, out.ctypes.data, C.byref(cnt)))
        return out if cnt.value else None

    def _check_pair(self, rc, bad):
        """rc of a filtered-block entry: LASH_ERANGE raises a LashError whose .pair is the refused pair, (row - r0) * n_cols + col."""
        if rc == _lib.ERANGE:
            e = LashError(rc, self._lib.lash_strerror(rc).decode() + " (pair %d)" % bad.value)
            e.pair = bad.value
            raise e
        self._ctx._check(rc)

    def _kept_rows(self, cap, stats, call):
        """call((out_row, out_col, out_dist, cap, &n_kept, &bad_pair, &n_candidates)) -> rc until the buffers hold every kept row (cap: once)."""
        size = (1 << 12) if cap is None else int(cap)
        while True:
            row, col = np.empty(size, np.uint32), np.empty(size, np.uint32)
            dist = np.empty(size, np.float64)
            kept, bad, cand = C.c_uint64(), C.c_uint64(), C.c_uint64()
            self._check_pair(call((row.ctypes.data, col.ctypes.data, dist.ctypes.data, size, C.byref(kept), C.byref(bad), C.byref(cand))), bad)
            if cap is not None or kept.value <= size:
                break
            size = kept.value
        if stats is not None:
            stats.update(n_kept=kept.value, n_candidates=cand.value)
        n = min(kept.value, size)
        return row[:n], col[:n], dist[:n]

    def pair_block_within(self, r0, r1, max_dist, k, qry=None, n_cols=None, triangle=False, model=1, fp32=False, estimator="fgra",
                          hll_bias=None, cap=None, stats=None, containment=None):
        """`lash dist --max-dist`: the pairs of rows [r0, r1) x columns [0, n_cols) whose distance d (lash_dist_rows' number, before the
        "same name -> 0" rule) passes d <= max_dist, as numpy arrays (row, col, dist) in (row, col) order — filtered on the GPU, each
        survivor evaluated exactly on the host (lash_sketch_set_pair_block_within).  cap: at most that many (default: all, growing the
        buffers as needed).  stats: optional dict, gets n_kept (the full count) and n_candidates (the pairs the filter kernel let through).
        cardinalities() must have run on both sets.  containment: None, "query" or "reference" as dist_rows (rectangles only: with
        triangle the library answers LASH_EINVAL)."""
        q = qry or self
        nc = q.n if n_cols is None else int(n_cols)
        return self._kept_rows(cap, stats, lambda out: self._lib.lash_sketch_set_pair_block_within_measure(
            self._ctx._h, self._h, int(r0), int(r1), q._h, nc, 1 if triangle else 0, int(k), int(model), 1 if fp32 else 0,
            ULL_ESTIMATORS[estimator], _bias_handle(hll_bias), MEASURES[containment], float(max_dist), *out))

    def pair_block_top(self, r0, r1, top, k, qry=None, n_cols=None, triangle=False, max_dist=None, same_col=None, col_bound=None,
                       row_bound=None, model=1, fp32=False, estimator="fgra", hll_bias=None, cap=None, stats=None, containment=None):
        """`lash dist --top`: the pairs of rows [r0, r1) x columns [0, n_cols) that can still be among some name's `top` nearest, as numpy
        arrays (row, col, dist) in (row, col) order, each evaluated exactly on the host (lash_sketch_set_pair_block_top): a superset of
        the block's part of every name's N_K given the bounds.  same_col: per block row the column with the row's name (its pair is 0),
        0xFFFFFFFF for none; col_bound / row_bound: TOP_KEY arrays (TopK.bounds), or None.  max_dist: also d <= max_dist.  cap / stats /
        LashError.pair / containment as pair_block_within."""
        q = qry or self
        nc = q.n if n_cols is None else int(n_cols)
        sc = None if same_col is None else np.ascontiguousarray(same_col, dtype=np.uint32)
        cb = None if col_bound is None else np.ascontiguousarray(col_bound, dtype=TOP_KEY)
        rb = None if row_bound is None else np.ascontiguousarray(row_bound, dtype=TOP_KEY)
        assert sc is None or len(sc) >= int(r1) - int(r0)
        assert cb is None or len(cb) >= nc
        assert rb is None or len(rb) >= int(r1) - int(r0)
        return self._kept_rows(cap, stats, lambda out: self._lib.lash_sketch_set_pair_block_top_measure(
            self._ctx._h, self._h, int(r0), int(r1), q._h, nc, 1 if triangle else 0, int(k), int(model), 1 if fp32 else 0,
            ULL_ESTIMATORS[estimator], _bias_handle(hll_bias), MEASURES[containment], int(top), float("nan") if max_dist is None else float(max_dist),
            None if sc is None else sc.ctypes.data, None if cb is None else cb.ctypes.data, None if rb is None else rb.ctypes.data, *out))

    def top_pairs(self, top, k, qry=None, triangle=None, max_dist=None, same_col=None, block_rows=None, **kw):
        """`lash dist --top` over the whole set: walks row blocks of `block_rows` (default: all rows in one block) through
        pair_block_top and a TopK, and returns the kept pairs (row, col, dist) in (row, col) order.  triangle (default: qry is None or
        this set) prints the lower triangle, rows and columns being the same names; same_col: per row, as pair_block_top.  The other
        keywords go to pair_block_top."""
        q = qry or self
        tri = (q is self) if triangle is None else bool(triangle)
        acc = TopK(self.n if tri else q.n, top, tri, self._lib)
        step = self.n if not block_rows else int(block_rows)
        for r0 in range(0, self.n, max(step, 1)):
            r1 = min(self.n, r0 + step)
            nc = min(r1, q.n) if tri else q.n
            cb, rb = acc.bounds(r0, r1, nc)
            sc = None if same_col is None else np.asarray(same_col, np.uint32)[r0:r1]
            row, col, dist = self.pair_block_top(r0, r1, top, k, qry=q, n_cols=nc, triangle=tri, max_dist=max_dist, same_col=sc, col_bound=cb,
                                                 row_bound=rb if tri else None, **kw)
            acc.add(row, col, dist)
        out = acc.result()
        acc.free()
        return out

    def pair_block_cluster(self, r0, r1, max_dist, k, clusters, n_cols=None, model=1, fp32=False, estimator="fgra", hll_bias=None, stats=None):
        """`lash dist --cluster`: rows [r0, r1) x columns [0, n_cols) (default r1) of this set's lower triangle joined into `clusters` (a
        Clusters of this set's size): two members are linked iff pair_block_within(..., triangle=True) returns their pair
        (lash_sketch_set_pair_block_cluster).  Blocks may run in any order and over several Clusters objects (merge).  stats: optional
        dict, gets pairs, pruned, joined_on_device, sent_to_host, clusters.  LashError.pair as pair_block_within.  cardinalities() must
        have run."""
        nc = min(int(r1), self.n) if n_cols is None else int(n_cols)
        st, bad = _lib.ClusterStats(), C.c_uint64()
        self._check_pair(self._lib.lash_sketch_set_pair_block_cluster(self._ctx._h, self._h, int(r0), int(r1), self._h, nc, int(k), int(model),
                                                                      1 if fp32 else 0, ULL_ESTIMATORS[estimator], _bias_handle(hll_bias),
                                                                      float(max_dist), clusters._h, C.byref(st), C.byref(bad)), bad)
        if stats is not None:
            stats.update({f: getattr(st, f) for f, _ in st._fields_})

    def clusters(self, max_dist, k, block_rows=None, **kw):
        """`lash dist --cluster` over the whole set: walks the triangle in row blocks of `block_rows` (default: one block) and returns,
        as a numpy uint32 array, for every member the smallest index of its single-linkage cluster.  The other keywords go to
        pair_block_cluster."""
        acc = Clusters(self._ctx, self.n)
        step = self.n if not block_rows else int(block_rows)
        for r0 in range(0, self.n, max(step, 1)):
            self.pair_block_cluster(r0, min(self.n, r0 + step), max_dist, k, acc, **kw)
        out = acc.labels()
        acc.free()
        return out

    def pair_block_derep(self, r0, r1, max_dist, k, acc, n_cols=None, model=1, fp32=False, estimator="fgra", hll_bias=None, stats=None):
        """`lash dist --derep`: rows [r0, r1) x columns [0, n_cols) (default r1) of this set's lower triangle decided in `acc` (a Derep of
        this set's size): a row is a representative iff no representative before it is within max_dist (pair_block_within(...,
        triangle=True) returns their pair), else a member of the first such one (lash_sketch_set_pair_block_derep).  Blocks must come in
        row order, contiguous from 0 (LashError EINVAL otherwise).  stats: optional dict, gets pairs, pruned_not_rep, pruned_after_hit,
        sent_to_host, evaluated, representatives.  LashError.pair as pair_block_within.  cardinalities() must have run."""
        nc = min(int(r1), self.n) if n_cols is None else int(n_cols)
        st, bad = _lib.DerepStats(), C.c_uint64()
        self._check_pair(self._lib.lash_sketch_set_pair_block_derep(self._ctx._h, self._h, int(r0), int(r1), self._h, nc, int(k), int(model),
                                                                    1 if fp32 else 0, ULL_ESTIMATORS[estimator], _bias_handle(hll_bias),
                                                                    float(max_dist), acc._h, C.byref(st), C.byref(bad)), bad)
        if stats is not None:
            stats.update({f: getattr(st, f) for f, _ in st._fields_})

    def derep(self, max_dist, k, block_rows=None, **kw):
        """`lash dist --derep` over the whole set: walks the triangle in row blocks of `block_rows` (default: one block), in row order,
        and returns the numpy uint32 array rep: rep[i] == i for a representative, else the representative i is a member of.  The other
        keywords go to pair_block_derep."""
        acc = Derep(self._ctx, self.n)
        step = self.n if not block_rows else int(block_rows)
        for r0 in range(0, self.n, max(step, 1)):
            self.pair_block_derep(r0, min(self.n, r0 + step), max_dist, k, acc, **kw)
        out = acc.result()
        acc.free()
        return out

    def pair_block(self, r0, r1, qry=None, n_cols=None, triangle=False, estimator="fgra", out=None):
        """statistics of rows [r0, r1) against columns [0, n_cols) of `qry` (default: this set) as the dict lash_dist_rows takes.
        `out`: optional dict of preallocated (e.g. pinned) flat arrays 'c', 'n' (uint32), 'u' (float64) of >= (r1-r0)*n_cols."""
        q = qry or self
        nc = q.n if n_cols is None else int(n_cols)
        nr = int(r1) - int(r0)
        np_ = nr * nc

        def buf(key, dt):
            if out is not None and key in out:
                return out[key][:np_].reshape(nr, nc)
            return np.empty((nr, nc), dtype=dt)
        c = buf("c", np.uint32) if self.algo != _lib.ULL else None
        n = buf("n", np.uint32) if self.algo == _lib.HMH else None
        u = buf("u", np.float64) if self.algo != _lib.HMH else None
        self._ctx._check(self._lib.lash_sketch_set_pair_block(self._ctx._h, self._h, int(r0), int(r1), q._h, nc, 1 if triangle else 0,
                                                              ULL_ESTIMATORS[estimator], None if c is None else c.ctypes.data,
                                                              None if n is None else n.ctypes.data, None if u is None else u.ctypes.data))
        st = {}
        if c is not None:
            st["c_or_zero"] = c
        if n is not None:
            st["n_counts"] = n
        if u is not None:
            st["sum_or_union"] = u
        return st


# lash_top_key: a name's K-th (d, row, col) rank key, d = +inf for none
TOP_KEY = np.dtype([("d", np.float64), ("row", np.uint32), ("col", np.uint32)])


class TopK:
    """lash_top: per name the `top` smallest (d, row, col) keys of the pairs added so far — the host half of `lash dist --top`, shared
    with the command line.  n_names: the columns (rectangular) or the set (triangle: a pair counts for its row and its column)."""

    def __init__(self, n_names, top, triangle=False, lib=None):
        self._lib = lib or _lib.load()
        self.n_names, self.top, self.triangle = int(n_names), int(top), bool(triangle)
        h = C.c_void_p()
        rc = self._lib.lash_top_create(self.n_names, self.top, 1 if triangle else 0, C.byref(h))
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())
        self._h = h

    def _check(self, rc):
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())

    def add(self, row, col, dist):
        row = np.ascontiguousarray(row, np.uint32)
        col = np.ascontiguousarray(col, np.uint32)
        dist = np.ascontiguousarray(dist, np.float64)
        assert len(row) == len(col) == len(dist)
        self._check(self._lib.lash_top_add(self._h, row.ctypes.data, col.ctypes.data, dist.ctypes.data, len(row)))

    def bounds(self, r0, r1, n_cols):
        """(col_bound [n_cols], row_bound [r1 - r0]) TOP_KEY arrays for pair_block_top"""
        cb = np.zeros(int(n_cols), TOP_KEY)
        rb = np.zeros(int(r1) - int(r0), TOP_KEY)
        self._check(self._lib.lash_top_bounds(self._h, int(r0), int(r1), int(n_cols), cb.ctypes.data, rb.ctypes.data))
        return cb, rb

    def merge(self, other):
        self._check(self._lib.lash_top_merge(self._h, other._h))

    def result(self):
        """the kept pairs (row, col, dist) in (row, col) order"""
        n = C.c_uint64()
        self._check(self._lib.lash_top_result(self._h, None, None, None, 0, C.byref(n)))
        row, col = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32)
        dist = np.empty(n.value, np.float64)
        if n.value:
            self._check(self._lib.lash_top_result(self._h, row.ctypes.data, col.ctypes.data, dist.ctypes.data, n.value, C.byref(n)))
        return row, col, dist

    def free(self):
        if getattr(self, "_h", None):
            self._lib.lash_top_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Clusters:
    """lash_cluster: the single-linkage clusters of n names joined so far — a label array on the context's GPU, where pair_block_cluster
    joins both the links the device is sure of and the ones only the host could confirm; shared with the command line."""

    def __init__(self, ctx, n):
        self._ctx, self._lib, self.n = ctx, ctx._lib, int(n)
        h = C.c_void_p()
        ctx._check(self._lib.lash_cluster_create(ctx._h, self.n, C.byref(h)))
        self._h = h

    def _check(self, rc):
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())

    def merge(self, other):
        """folds another accumulator's clusters in (one per worker / device); `other` is unchanged"""
        self._check(self._lib.lash_cluster_merge(self._h, other._h))

    def labels(self):
        """numpy uint32 [n]: for every name the smallest index of its cluster"""
        out = np.empty(self.n, np.uint32)
        self._check(self._lib.lash_cluster_labels(self._h, out.ctypes.data))
        return out

    def free(self):
        if getattr(self, "_h", None):
            self._lib.lash_cluster_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Derep:
    """lash_derep: the greedy representatives of n names decided so far, in row order — rep[] on the context's GPU (where
    pair_block_derep prunes the columns that are not representatives) with a mirror on the host; shared with the command line."""

    def __init__(self, ctx, n):
        self._ctx, self._lib, self.n = ctx, ctx._lib, int(n)
        h = C.c_void_p()
        ctx._check(self._lib.lash_derep_create(ctx._h, self.n, C.byref(h)))
        self._h = h

    def _check(self, rc):
        if rc != _lib.OK:
            raise LashError(rc, self._lib.lash_strerror(rc).decode())

    def result(self):
        """numpy uint32 [n]: rep[i] == i for a representative, else the representative of i; LashError EINVAL before all are decided"""
        out = np.empty(self.n, np.uint32)
        self._check(self._lib.lash_derep_result(self._h, out.ctypes.data))
        return out

    def free(self):
        if getattr(self, "_h", None):
            self._lib.lash_derep_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
