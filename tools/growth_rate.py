#!/usr/bin/env python3
"""tools/growth_rate.py [N] [ORDERS] [RUNS] [L] [BASELINE_SECONDS] — what the growth curve costs on the new entry and on the route it replaces.

N (default 10 000) hmh k=16 sketches of L-base synthetic genomes (default 100 000) are made on the device and kept there as one
lash_sketch_set; ORDERS (default 64) orderings as `lash growth` draws them (seed 42).

(a) lash_sketch_set_prefix_union_cardinalities on all orders: one warm-up call on two orders, then RUNS (default 3) timed calls.  Prints every
    wall time, the median and the spread, and the bytes the kernel reads (orders x N x 32 KiB of images) per second of the whole call against
    the 8 TB/s HBM figure of DESIGN.md §5.  The call's wall time includes the histogram copy and the host finish: it is an end-to-end rate of the
    entry, not the kernel's share of peak.
(b) the step-by-step composition of what the library offered before: lash_merge_images_device of the running image with the next member,
    then lash_sketch_set_cardinalities on a one-image set of it, for as many steps as fit BASELINE_SECONDS (default 30) after 200 warm-up
    steps; extrapolated to ORDERS x N steps.  The numbers of the steps it ran are compared with (a)'s, bit for bit."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lash_amd  # noqa: E402
import growth_model as G  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
ORDERS = int(sys.argv[2]) if len(sys.argv) > 2 else 64
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
L = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
BASELINE_S = float(sys.argv[5]) if len(sys.argv) > 5 else 30.0
k = 16

import torch  # noqa: E402

ctx = lash_amd.Context(0)
dev = torch.device("cuda", 0)
ib = lash_amd.image_bytes("hmh")
img = torch.zeros((N, ib), dtype=torch.uint8, device=dev)
chunk = min(max(1, 2_000_000_000 // L), N)
base = torch.empty(chunk * L, dtype=torch.uint8, device=dev)
t0 = time.perf_counter()
for g0 in range(0, N, chunk):
    n = min(chunk, N - g0)
    ctx.synth_genomes_device(g0, n, L, base)
    ctx.synchronize()
    rec_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    d_rec = torch.from_numpy(rec_off.astype(np.int64)).to(dev)
    ctx.sketch_batch_device("hmh", k, 0, 42, base, d_rec, n, np.arange(n + 1, dtype=np.uint64), rec_off, img[g0:g0 + n].reshape(-1))
    ctx.synchronize()
print("sketched %d genomes of %d bases in %.2f s" % (N, L, time.perf_counter() - t0), flush=True)
del base

orders = G.orders(N, ORDERS, 42)
s = ctx.sketch_set("hmh", 0, img)
s.prefix_union_cardinalities(orders[:2])                              # warm-up: code objects, the first allocations
walls, got = [], None
for run in range(RUNS):
    t0 = time.perf_counter()
    got = s.prefix_union_cardinalities(orders)
    walls.append(time.perf_counter() - t0)
med = statistics.median(walls)
read = ORDERS * N * ib
print("(a) prefix_union_cardinalities, %d orders x %d steps: walls %s, median %.3f s, spread %.3f s" %
      (ORDERS, N, " ".join("%.3f" % w for w in walls), med, max(walls) - min(walls)), flush=True)
print("(a) %.3f us per step; %.2f GB of images read per call, %.1f GB/s over the whole call = %.2f %% of 8 TB/s" %
      (med / (ORDERS * N) * 1e6, read / 1e9, read / 1e9 / med, read / med / 8e12 * 100), flush=True)

acc = torch.empty((1, ib), dtype=torch.uint8, device=dev)
one = ctx.sketch_set("hmh", 0, acc)                                   # adopts acc: its cardinality is that of the running union
steps, t_used, same = 0, 0.0, True
WARM = min(200, ORDERS * N // 2)
t_start = time.perf_counter()
for o in range(ORDERS):
    acc.copy_(img[int(orders[o, 0])].reshape(1, ib))
    torch.cuda.synchronize(dev)
    for t in range(N):
        if steps == WARM:
            t_start = time.perf_counter()
        if t:
            ctx.merge_images_device("hmh", 0, acc, img[int(orders[o, t])], 1)
        c = one.cardinalities()[0]
        same = same and c == got[o, t]
        steps += 1
        if steps > WARM:
            t_used = time.perf_counter() - t_start
            if t_used >= BASELINE_S:
                break
    if t_used >= BASELINE_S:
        break
timed = steps - WARM
per = t_used / timed
print("(b) merge_images_device + one-image cardinalities: %d steps in %.2f s, %.1f us per step, %.1f s extrapolated to %d steps" %
      (timed, t_used, per * 1e6, per * ORDERS * N, ORDERS * N), flush=True)
print("(b) its %d numbers %s (a)'s bit for bit; (b) / (a) = %.1f" % (steps, "equal" if same else "DIFFER FROM", per * ORDERS * N / med), flush=True)
one.free()
s.free()
ctx.close()
sys.exit(0 if same else 1)
