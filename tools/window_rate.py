#!/usr/bin/env python3
"""tools/window_rate.py — what `lash sketch --window W` costs on the device (GPU box; run by hand, writes profiles/r08/windows.txt).
G genomes of 5 Mbp as 80-column FASTA, one record each, resident on the device; hmh k = 16; W = 3 000 and W = 100 000.  HIP-event times of
  the window stage alone (lash_fasta_windows_device: every pass, the two-word read-back and the allocations of the result included),
  the sketch of the rewritten buffer (lash_sketch_files_raw_device over the window index's buffer),
  and, as the baseline — what a user had to do before — the sketch of the same windows pre-cut as records (here on the device with torch, the
  cutting itself not timed) through the record index and the raw-file route.
Usage: window_rate.py [G=1000] [repeats=5]"""
import ctypes
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lash_amd

G = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
L, COLS, k = 5_000_000, 80, 16
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(dev)
ctx = lash_amd.Context(0, stream=stream)
out_lines = []


def say(s):
    print(s, flush=True)
    out_lines.append(s)


def timed(fn):
    """median HIP-event milliseconds of REP runs after one warm-up, on the context's stream"""
    ms = []
    for i in range(REP + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        r = fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if i < REP and hasattr(r, "free"):
            r.free()
    return float(np.median(ms[1:])), r


def fasta_on_device(seq, n_rec, rec_len, COLS=COLS):
    """n_rec records of rec_len bases (a multiple of COLS) as '>rNNNNNNNNN\\n' + lines of COLS bases; -> (bytes, record length in bytes)"""
    rows = rec_len // COLS
    hdr = 12
    fa = torch.empty((n_rec, hdr + rows * (COLS + 1)), dtype=torch.uint8, device=dev)
    names = np.frombuffer(b"".join(b">r%09d\n" % i for i in range(n_rec)), np.uint8).reshape(n_rec, hdr)
    fa[:, :hdr] = torch.from_numpy(names.copy()).to(dev)
    body = fa[:, hdr:].view(n_rec, rows, COLS + 1)
    body[:, :, :COLS] = seq.view(n_rec, rows, COLS)
    body[:, :, COLS] = 10
    return fa.view(-1), fa.shape[1]


def raw_device(d_ptr, file_off, fmt, d_img):
    """lash_sketch_files_raw_device: asynchronous on the context's stream"""
    prm = ctx._params("hmh", k, 0, 42, 0)
    ctx._check(ctx._lib.lash_sketch_files_raw_device(ctx._h, ctypes.byref(prm), d_ptr, file_off.ctypes.data, fmt.ctypes.data, len(fmt), d_img.data_ptr()))


def hbm_copy_rate():
    try:
        text = open(os.path.join(ROOT, "profiles", "r02", "hbm_calibration.txt")).read()
        ns = float(re.search(r"cal_FETCH\s+copy_kernel\s+dispatches=\d+ avg_ns=(\d+)\s+FETCH_SIZE\s+avg/dispatch = ([0-9.e+]+)", text).group(1))
        rd = float(re.search(r"cal_FETCH\s+copy_kernel.*?avg/dispatch = ([0-9.e+]+)", text, re.S).group(1))
        wr = float(re.search(r"cal_WRITE\s+copy_kernel.*?avg/dispatch = ([0-9.e+]+)", text, re.S).group(1))
        return (rd + wr) * 1024 / (ns * 1e-9)
    except Exception:
        return None


d_seq = torch.empty(G * L, dtype=torch.uint8, device=dev)
ctx.synth_genomes_device(0, G, L, d_seq)
ctx.synchronize()
d_fa, rec_bytes = fasta_on_device(d_seq, G, L)
torch.cuda.synchronize()
off = np.array([0, d_fa.numel()], np.uint64)
copy_rate = hbm_copy_rate()
say("window_rate: %d x %d bp, %d-column FASTA (%.3f GB resident), hmh k=%d, median of %d HIP-event times" % (G, L, COLS, d_fa.numel() / 1e9, k, REP))
say("HBM copy rate of profiles/r02/hbm_calibration.txt (read + written): %s" % ("%.3g B/s" % copy_rate if copy_rate else "not found"))
ib = lash_amd.image_bytes("hmh")
index = ctx.fasta_index(d_fa, off, device=True, keep=True)
for W in (3_000, 100_000):
    ms_stage, wi = timed(lambda: ctx.fasta_windows(d_fa, off, index, W, device=True, keep=True))
    n = wi.n_windows
    woff = wi.offsets()
    fmt = np.ones(n, np.uint8)                                        # LASH_FMT_FASTA
    d_img = torch.zeros(n * ib, dtype=torch.uint8, device=dev)
    ms_sketch, _ = timed(lambda: raw_device(wi.device_ptr, woff, fmt, d_img))
    moved = 2 * d_fa.numel() + 2 * (d_fa.numel() // 4) + wi.nbytes     # input read twice, lane words written and read, output written
    say("W = %-7d %d windows: window stage %.3f ms (%.3g B/s read + written%s); sketch of the rewritten buffer %.3f ms; stage share %.1f %%"
        % (W, n, ms_stage, moved / (ms_stage * 1e-3), ", %.2f of the copy rate" % (moved / (ms_stage * 1e-3) / copy_rate) if copy_rate else "",
           ms_sketch, 100 * ms_stage / (ms_stage + ms_sketch)))
    wi.free()
    # baseline: the same windows as records of one pre-cut FASTA (L is a multiple of both W), indexed and sketched as records
    d_cut, _ = fasta_on_device(d_seq, G * (L // W), W, COLS if W % COLS == 0 else 60)      # W = 3 000 is no multiple of 80: lines of 60
    torch.cuda.synchronize()
    coff = np.array([0, d_cut.numel()], np.uint64)
    ms_index, cix = timed(lambda: ctx.fasta_index(d_cut, coff, device=True, keep=True))
    start = cix.arrays()[0]
    ms_base, _ = timed(lambda: raw_device(d_cut.data_ptr(), start, fmt, d_img))
    say("            baseline, pre-cut records: record index %.3f ms, sketch %.3f ms (the host-side cutting is not in these numbers)" % (ms_index, ms_base))
    cix.free()
    del d_cut, d_img
index.free()
os.makedirs(os.path.join(ROOT, "profiles", "r08"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "r08", "windows.txt"), "w").write("\n".join(out_lines) + "\n")
