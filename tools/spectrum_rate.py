#!/usr/bin/env python3
"""tools/spectrum_rate.py [N] [RUNS] [L] — what lash_sketch_set_group_spectrum costs next to lash_sketch_set_group_union.

N (default 100 000) hmh sketches of L-base synthetic genomes (default 20 000) are made on the device and kept there as one
lash_sketch_set.  The three shapes of merge_rate.py over them:
  (i)   N / 2 groups of 2          (ii)  N / 100 groups of 100          (iii) 1 group of N
Per shape, after one warm-up call of each entry on the whole shape, RUNS (default 7) rounds of [group_union_device, group_spectrum_device]
alternate on one stream, each call between two device events; the medians and their ratio are printed.  group_union is the yardstick:
the traffic model (every member read twice, one union image per task) puts the ratio at about 2, the bar is 3.
The bins of a few groups of every shape are compared with the numpy definition (max, equality, bincount) before anything is timed."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lash_amd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
L = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
k = 16

import torch  # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
ctx = lash_amd.Context(0, stream=stream)
ok = True
ib = lash_amd.image_bytes("hmh", 0)

img = torch.zeros((N, ib), dtype=torch.uint8, device=dev)
chunk = min(max(1, 1_000_000_000 // L), N)
base = torch.empty(chunk * L, dtype=torch.uint8, device=dev)
for g0 in range(0, N, chunk):
    n = min(chunk, N - g0)
    ctx.synth_genomes_device(g0, n, L, base)
    ctx.synchronize()
    rec_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    d_rec = torch.from_numpy(rec_off.astype(np.int64)).to(dev)
    ctx.sketch_batch_device("hmh", k, 0, 42, base, d_rec, n, np.arange(n + 1, dtype=np.uint64), rec_off, img[g0:g0 + n].reshape(-1))
    ctx.synchronize()
del base
print("sketched %d genomes of %d bases, %d-byte images" % (N, L, ib), flush=True)
s = ctx.sketch_set("hmh", 0, img)


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    call()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3


def model_bins(members):
    """max, equality, bincount with torch, 1024 members at a time"""
    idx = torch.from_numpy(members.astype(np.int64)).to(dev)
    regs = lambda i: img[idx[i:i + 1024]].view(torch.int16).to(torch.int32) & 0xFFFF   # noqa: E731
    top = torch.zeros(16384, dtype=torch.int32, device=dev)
    for i in range(0, len(members), 1024):
        top = torch.maximum(top, regs(i).max(dim=0).values)
    holders = torch.zeros(16384, dtype=torch.int64, device=dev)
    for i in range(0, len(members), 1024):
        holders += ((regs(i) == top) & (top != 0)).sum(dim=0)
    return torch.bincount(holders, minlength=len(members) + 1).cpu().numpy()


ids = np.arange(N, dtype=np.uint32)
for tag, groups in (("(i)", ids[:N - N % 2].reshape(-1, 2)), ("(ii)", ids[:N - N % 100].reshape(-1, 100)), ("(iii)", ids.reshape(1, -1))):
    G, M = groups.shape
    out = torch.empty((G, ib), dtype=torch.uint8, device=dev)
    hist = torch.empty(G * (M + 1), dtype=torch.int32, device=dev)
    s.group_union(groups, device_out=out)                                 # warm-up: code objects, the first allocations
    s.group_spectrum(groups, device_out=(hist, out))
    ctx.synchronize()
    got = hist.cpu().numpy().view(np.uint32).reshape(G, M + 1)
    same = all(np.array_equal(got[g], model_bins(groups[g])) for g in sorted({0, G // 2, G - 1})) and bool((got.sum(axis=1) == 16384).all())
    ok = ok and same
    union, spectrum = [], []
    for run in range(RUNS):
        union.append(timed(lambda: s.group_union(groups, device_out=out)))
        spectrum.append(timed(lambda: s.group_spectrum(groups, device_out=(hist, out))))
    mu, ms = statistics.median(union), statistics.median(spectrum)
    seg, sl, scratch = s.group_union_plan(groups)
    read = G * M * ib
    print("%s %d groups of %d: segment %d, slices %d; bins %s" % (tag, G, M, seg, sl, "equal to the model" if same else "DIFFER"), flush=True)
    print("%s group_union    median %.3f ms (%s), %.1f GB/s of members" % (tag, mu * 1e3, " ".join("%.3f" % (t * 1e3) for t in union), read / 1e9 / mu))
    print("%s group_spectrum median %.3f ms (%s), %.1f GB/s of members read twice" %
          (tag, ms * 1e3, " ".join("%.3f" % (t * 1e3) for t in spectrum), 2 * read / 1e9 / ms))
    print("%s ratio %.2f (model 2, bar 3)%s" % (tag, ms / mu, "" if ms / mu <= 3.0 else "  ABOVE THE BAR"), flush=True)
    del out, hist
s.free()
ctx.close()
sys.exit(0 if ok else 1)
