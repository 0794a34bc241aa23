#!/usr/bin/env python3
"""tools/translate_rate.py — what `lash sketch --translate` costs on the device (GPU box; run by hand, writes profiles/translate_rate.txt).
G genomes of 5 Mbp of random DNA as 80-column FASTA, one record each, resident on the device; hmh k = 7 and ull p = 12 k = 10.  Times of
  the translate stage alone (lash_fasta_translate_device: every pass, the read-backs of the totals and the allocations of the result
  included), in input GB/s,
  the amino-acid sketch of the translated buffer (lash_sketch_translated, one sketch per genome; its copy of the images to the host
  included), in k-mers/s,
  and, next to them, the same kernel on proteins of 300 residues, 1 000 to a sketch (the shape of tools/aa_rate.py), resident on the device.
Translated random DNA has segments of about 21 residues (3 of 64 codons are stops): one record fetch of aa_sketch_kernel per ~21 bytes.
Usage: translate_rate.py [G=200] [repeats=5]"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lash_amd

G = int(sys.argv[1]) if len(sys.argv) > 1 else 200
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
L, COLS = 5_000_000, 80
CONFIGS = (("hmh", 7, 0), ("ull", 10, 12))
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(dev)
ctx = lash_amd.Context(0, stream=stream)
out_lines = []


def say(s):
    print(s, flush=True)
    out_lines.append(s)


def timed(fn, free=True):
    """median wall milliseconds of REP runs after one warm-up; every call here ends with the context's stream drained"""
    ms = []
    for i in range(REP + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if free and i < REP and hasattr(r, "free"):
            r.free()
    return float(np.median(ms[1:])), r


def fasta_on_device(seq, n_rec, rec_len):
    """n_rec records of rec_len bases (a multiple of COLS) as '>rNNNNNNNNN\\n' + lines of COLS bases"""
    rows = rec_len // COLS
    hdr = 12
    fa = torch.empty((n_rec, hdr + rows * (COLS + 1)), dtype=torch.uint8, device=dev)
    names = np.frombuffer(b"".join(b">r%09d\n" % i for i in range(n_rec)), np.uint8).reshape(n_rec, hdr)
    fa[:, :hdr] = torch.from_numpy(names.copy()).to(dev)
    body = fa[:, hdr:].view(n_rec, rows, COLS + 1)
    body[:, :, :COLS] = seq.view(n_rec, rows, COLS)
    body[:, :, COLS] = 10
    return fa.view(-1)


def kmers_of(fn):
    ctx.enable_timing(True)
    fn()
    n = ctx.timing()["kmers"]
    ctx.enable_timing(False)
    return n


d_seq = torch.empty(G * L, dtype=torch.uint8, device=dev)
ctx.synth_genomes_device(0, G, L, d_seq)
ctx.synchronize()
d_fa = fasta_on_device(d_seq, G, L)
del d_seq
torch.cuda.synchronize()
off = np.array([0, d_fa.numel()], np.uint64)
say("translate_rate: %d x %d bp of random DNA, %d-column FASTA (%.3f GB resident), median of %d wall times" % (G, L, COLS, d_fa.numel() / 1e9, REP))
index = ctx.fasta_index(d_fa, off, device=True, keep=True)
ms_stage, ti = timed(lambda: ctx.fasta_translate(d_fa, off, index, device=True, keep=True))
say("translate stage: %.3f ms, %.3g input B/s; %.3f GB of residues, %d segments (%.1f bytes each), %.3f GB of seg_off"
    % (ms_stage, d_fa.numel() / (ms_stage * 1e-3), ti.nbytes / 1e9, ti.n_segments, ti.nbytes / max(ti.n_segments, 1), 8 * ti.n_segments / 1e9))
goff = np.arange(G + 1, dtype=np.uint64)
rates = {}
for algo, k, p in CONFIGS:
    n_kmers = kmers_of(lambda: ctx.sketch_translated(algo, k, p, 42, ti, goff))
    ms, _ = timed(lambda: ctx.sketch_translated(algo, k, p, 42, ti, goff))
    rates[algo] = n_kmers / (ms * 1e-3)
    say("%s k=%d%s: sketch of the translated buffer %.3f ms, %.3g k-mers/s, %.3g residues/s; translate stage share %.1f %%"
        % (algo, k, "" if algo == "hmh" else " p=%d" % p, ms, rates[algo], ti.nbytes / (ms * 1e-3), 100 * ms_stage / (ms_stage + ms)))
ti.free()
index.free()
del d_fa

# the same kernel on proteins: N x 300 residues, 1 000 proteins to a sketch
N, PLEN, PER = 2_000_000, 300, 1000
letters = torch.from_numpy(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8).copy()).to(dev)
d_prot = letters[torch.randint(0, 20, (N * PLEN,), device=dev)]
d_rec = (torch.arange(N + 1, dtype=torch.int64, device=dev) * PLEN)
pgoff = np.arange(0, N + 1, PER, dtype=np.uint64)
pgbo = pgoff * np.uint64(PLEN)
torch.cuda.synchronize()
say("proteins: %d x %d residues (%.3f GB resident), %d sketches of %d proteins" % (N, PLEN, N * PLEN / 1e9, len(pgoff) - 1, PER))
for algo, k, p in CONFIGS:
    d_img = torch.zeros((len(pgoff) - 1) * lash_amd.image_bytes(algo, p), dtype=torch.uint8, device=dev)
    call = lambda: ctx.sketch_batch_device(algo, k, p, 42, d_prot, d_rec, N, pgoff, pgbo, d_img, flags=lash_amd.F_AMINO)
    n_kmers = kmers_of(call)
    assert n_kmers == N * (PLEN - k + 1)
    ms, _ = timed(call, free=False)
    rate = n_kmers / (ms * 1e-3)
    say("%s k=%d%s: %.3f ms, %.3g k-mers/s, %.3g residues/s; the translated shape runs at %.2f of this rate"
        % (algo, k, "" if algo == "hmh" else " p=%d" % p, ms, rate, N * PLEN / (ms * 1e-3), rates[algo] / rate))
    del d_img
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "translate_rate.txt"), "w").write("\n".join(out_lines) + "\n")
