#!/usr/bin/env python3
"""tools/merge_rate.py [N] [RUNS] [L] [BASELINE_SECONDS] — what unions of groups cost on lash_sketch_set_group_union and on the route it replaces.

N (default 100 000) sketches of L-base synthetic genomes (default 20 000) are made on the device and kept there as one lash_sketch_set,
once as hmh images (32 KiB) and once as hll p = 14 images (16 KiB + header).  Three shapes of the group list over them:
  (i)   N / 2 groups of 2          (ii)  N / 100 groups of 100          (iii) 1 group of N

(a) lash_sketch_set_group_union_device into a device buffer: one warm-up call, then RUNS (default 3) timed calls, each ended by a
    synchronize.  Prints the walls, the median, the plan, and the member bytes read per second of the whole call as a fraction of the copy
    rate measured in profiles/r02/hbm_calibration.txt (copy_kernel: 1 GiB read and 1 GiB written in 0.918 ms = 2.34 TB/s moved, 1.17 TB/s
    read) and of its read-only rate (read64_kernel: 1 GiB in 0.336 ms = 3.20 TB/s).
(b) the composition the library offered before: per group, lash_merge_images_device of a running image with one member at a time, for
    as many groups as fit BASELINE_SECONDS (default 5) per shape after a warm-up, extrapolated to all members.  The images of the
    groups it finished are compared with (a)'s, byte for byte."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lash_amd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
L = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
BASELINE_S = float(sys.argv[4]) if len(sys.argv) > 4 else 5.0
k = 16
COPY_MOVED, COPY_READ, READ_ONLY = 2 * 2**30 / 0.918366e-3, 2**30 / 0.918366e-3, 2**30 / 0.335822e-3

import torch  # noqa: E402

ctx = lash_amd.Context(0)
dev = torch.device("cuda", 0)
ok = True


def sketch_all(algo, p):
    ib = lash_amd.image_bytes(algo, p)
    img = torch.zeros((N + 1, ib), dtype=torch.uint8, device=dev)          # image N: an input shorter than k, the empty sketch
    chunk = min(max(1, 1_000_000_000 // L), N)
    base = torch.empty(chunk * L, dtype=torch.uint8, device=dev)
    for g0 in range(0, N, chunk):
        n = min(chunk, N - g0)
        ctx.synth_genomes_device(g0, n, L, base)
        ctx.synchronize()
        rec_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        d_rec = torch.from_numpy(rec_off.astype(np.int64)).to(dev)
        ctx.sketch_batch_device(algo, k, p, 42, base, d_rec, n, np.arange(n + 1, dtype=np.uint64), rec_off, img[g0:g0 + n].reshape(-1))
        ctx.synchronize()
    rec_off = np.array([0, 4], dtype=np.uint64)
    d_rec = torch.from_numpy(rec_off.astype(np.int64)).to(dev)
    ctx.sketch_batch_device(algo, k, p, 42, base, d_rec, 1, np.arange(2, dtype=np.uint64), rec_off, img[N:].reshape(-1))
    ctx.synchronize()
    return img, ib


def shapes():
    ids = np.arange(N, dtype=np.uint32)
    yield "(i)", ids[:N - N % 2].reshape(-1, 2)
    yield "(ii)", ids[:N - N % 100].reshape(-1, 100)
    yield "(iii)", ids.reshape(1, -1)


for algo, p in (("hmh", 0), ("hll", 14)):
    t0 = time.perf_counter()
    img, ib = sketch_all(algo, p)
    print("%s p %d: sketched %d genomes of %d bases in %.2f s, %d-byte images" % (algo, p, N, L, time.perf_counter() - t0, ib), flush=True)
    s = ctx.sketch_set(algo, p, img)
    for tag, groups in shapes():
        G, M = groups.shape
        out = torch.empty((G, ib), dtype=torch.uint8, device=dev)
        s.group_union(groups[:max(1, G // 50)], device_out=out)                # warm-up: code objects, the first allocations
        ctx.synchronize()
        walls = []
        for run in range(RUNS):
            t0 = time.perf_counter()
            s.group_union(groups, device_out=out)
            ctx.synchronize()
            walls.append(time.perf_counter() - t0)
        med = statistics.median(walls)
        read = G * M * ib
        seg, sl, scratch = s.group_union_plan(groups)
        print("%s %s %d groups of %d (a): walls %s, median %.4f s; segment %d, slices %d, scratch %.1f MB" %
              (algo, tag, G, M, " ".join("%.4f" % w for w in walls), med, seg, sl, scratch / 1e6), flush=True)
        print("%s %s (a): %.2f GB of members read, %.1f GB/s = %.1f %% of the copy rate (2.34 TB/s moved; %.1f %% of its 1.17 TB/s read), "
              "%.1f %% of the read-only rate (3.20 TB/s)" % (algo, tag, read / 1e9, read / 1e9 / med, read / med / COPY_MOVED * 100,
                                                             read / med / COPY_READ * 100, read / med / READ_ONLY * 100), flush=True)
        # (b): a running image per group, one member at a time
        acc = torch.empty((1, ib), dtype=torch.uint8, device=dev)
        done, steps, same = 0, 0, True
        warm = 1 if G > 1 else 0
        t_start = time.perf_counter()
        for g in range(G):
            if g == warm:
                ctx.synchronize()
                t_start, steps = time.perf_counter(), 0
            acc.copy_(img[N].reshape(1, ib))
            torch.cuda.synchronize(dev)
            for m in groups[g]:
                ctx.merge_images_device(algo, p, acc, img[int(m)], 1)
                steps += 1
                if G == 1 and steps % 256 == 0 and time.perf_counter() - t_start >= BASELINE_S:
                    break
            ctx.synchronize()
            if G > 1:
                same = same and bool(torch.equal(acc[0], out[g]))
                done += 1
            if time.perf_counter() - t_start >= BASELINE_S:
                break
        ctx.synchronize()
        used = time.perf_counter() - t_start
        per = used / max(steps, 1)
        ok = ok and same
        print("%s %s (b) merge_images_device per member: %d steps in %.2f s, %.1f us per step, %.2f s extrapolated to %d members; (b) / (a) = %.1f; "
              "%d groups compared: %s" % (algo, tag, steps, used, per * 1e6, per * G * M, G * M, per * G * M / med, done,
                                          "equal" if same else "DIFFER"), flush=True)
        del out
    s.free()
    del img
ctx.close()
sys.exit(0 if ok else 1)
