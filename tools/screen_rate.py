#!/usr/bin/env python3
"""tools/screen_rate.py [N] [RUNS] [L] — what lash_sketch_set_screen_wta costs next to lash_sketch_set_pair_block.

N (default 100 000) hmh sketches of L-base synthetic genomes (default 20 000) are made on the device and kept there as the reference
set; the 4 queries are the unions of 100 references each (lash_sketch_set_group_union), so that buckets are held and contested.  Cases:
  (i)  every reference a candidate of every query, in row order: N x 4 entries
  (ii) the first 1 000 references the candidates of every query: 1 000 x 4 entries
Per case, after one warm-up call of each entry, RUNS (default 7) rounds of [pair_block, screen_wta_device] alternate on one stream, each
call between two device events; the medians and their ratio are printed.  pair_block of the same rectangle reads the same images once:
the yardstick.  The traffic model (every candidate read twice) puts the ratio at about 2; no rate is fixed in advance.
The counts are compared with the definition (equality, first position, counting in torch) before anything is timed."""
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
NQ = 4
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
ref = ctx.sketch_set("hmh", 0, img)
qimg = torch.zeros((NQ, ib), dtype=torch.uint8, device=dev)
ref.group_union([list(range(j * (N // NQ), j * (N // NQ) + min(100, N // NQ))) for j in range(NQ)], device_out=qimg)
ctx.synchronize()
qry = ctx.sketch_set("hmh", 0, qimg)
ref.cardinalities()
qry.cardinalities()
ref.prepare(qry)


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    call()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3


def model(j, n_cand):
    """(shared, won) of query j against candidates 0 .. n_cand - 1 in row order, 1024 candidates at a time"""
    q = qimg[j].view(torch.int16).to(torch.int32) & 0xFFFF
    winner = torch.full((16384,), n_cand, dtype=torch.int64, device=dev)
    shared = torch.zeros(n_cand, dtype=torch.int64, device=dev)
    for i in range(0, n_cand, 1024):
        regs = img[i:min(i + 1024, n_cand)].view(torch.int16).to(torch.int32) & 0xFFFF
        holds = (regs == q) & (q != 0)
        shared[i:i + holds.shape[0]] = holds.sum(dim=1)
        pos = torch.arange(i, i + holds.shape[0], dtype=torch.int64, device=dev)[:, None]
        winner = torch.minimum(winner, torch.where(holds, pos, n_cand).min(dim=0).values)
    won = torch.bincount(winner, minlength=n_cand + 1)[:n_cand]
    return shared.cpu().numpy(), won.cpu().numpy()


for tag, n_cand in (("(i)", N), ("(ii)", min(1000, N))):
    lists = np.tile(np.arange(n_cand, dtype=np.uint32), (NQ, 1))
    d_shared = torch.empty(NQ * n_cand, dtype=torch.int32, device=dev)
    d_won = torch.empty(NQ * n_cand, dtype=torch.int32, device=dev)
    ref.pair_block(0, n_cand, qry=qry)                                      # warm-up: code objects, the first allocations
    ref.screen_wta(qry, lists, device_out=(d_shared, d_won))
    ctx.synchronize()
    gs, gw = d_shared.cpu().numpy().reshape(NQ, n_cand), d_won.cpu().numpy().reshape(NQ, n_cand)
    same = True
    for j in (0, NQ - 1):
        ms, mw = model(j, n_cand)
        same = same and np.array_equal(gs[j], ms) and np.array_equal(gw[j], mw)
    ok = ok and same
    pair, screen = [], []
    for run in range(RUNS):
        pair.append(timed(lambda: ref.pair_block(0, n_cand, qry=qry)))
        screen.append(timed(lambda: ref.screen_wta(qry, lists, device_out=(d_shared, d_won))))
    mp, msc = statistics.median(pair), statistics.median(screen)
    seg, sl, _ = ref.group_union_plan(lists)
    read = NQ * n_cand * ib
    print("%s %d candidates x %d queries: segment %d, slices %d; counts %s; won %s of the occupied buckets" %
          (tag, n_cand, NQ, seg, sl, "equal to the model" if same else "DIFFER", gw.sum(axis=1).tolist()), flush=True)
    print("%s pair_block  median %.3f ms (%s)" % (tag, mp * 1e3, " ".join("%.3f" % (t * 1e3) for t in pair)))
    print("%s screen_wta  median %.3f ms (%s), %.1f GB/s of candidate images read twice" %
          (tag, msc * 1e3, " ".join("%.3f" % (t * 1e3) for t in screen), 2 * read / 1e9 / msc))
    print("%s ratio %.2f (model 2)" % (tag, msc / mp), flush=True)
    del d_shared, d_won
qry.free()
ref.free()
ctx.close()
sys.exit(0 if ok else 1)
