#!/usr/bin/env python3
"""tools/tree_rate.py [--nj] [N[,N...]] [RUNS] [CLI_N] [L] — what `lash dist --tree` costs, and what the route it replaces costs.

Part 1, per N (default 4096,16384): lash_tree_build (average linkage) on a random uniform N x N matrix through the ABI: one warm-up build,
then RUNS (default 3) timed ones, each on a freshly uploaded matrix (a build consumes it).  Prints every wall time, the median, the
spread (max - min) and the rescanned rows the build reports.

Part 2, for CLI_N (default: the largest N; 0 = skip): CLI_N hmh k=16 sketches of L-base genomes (default 1 000 000: above 2^19 distinct
k-mers, so no expected-collision matrix product on either route) made on the device as families of 64, written as a sketch-file set
under /dev/shm; then, after one warm-up run of each, RUNS times each, with -t 16 and --file-order: `lash dist --dm` (the matrix as text, the route to an external
clustering tool) and `lash dist --tree` (with its LASH_CLI_TIMING line).  Prints every wall time, medians and spreads.

--nj: part 1 also times lash_tree_build_nj the same way, after the average-linkage lines of the same N, and prints beside its median the
traffic model of the scan (8 bytes x the sum over r = N .. 3 of r x N / 2 cells, about 2 N^3 bytes: retired columns are still fetched) and
the GB/s that implies; part 2 also runs `lash dist --tree --nj`."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lash_amd  # noqa: E402
import host_lib as H  # noqa: E402
import tree_model as T  # noqa: E402
import nj_model as NJ  # noqa: E402

WITH_NJ = "--nj" in sys.argv
sys.argv = [a for a in sys.argv if a != "--nj"]
NS = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "4096,16384").split(",")]
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
CLI_N = int(sys.argv[3]) if len(sys.argv) > 3 else max(NS)
L = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
FAM, k = 64, 16


def summary(what, walls):
    print("%s: walls %s, median %.3f s, spread %.3f s" % (what, " ".join("%.3f" % w for w in walls), statistics.median(walls), max(walls) - min(walls)),
          flush=True)


ctx = lash_amd.Context(0)
for n in NS:
    d = np.random.default_rng(n).random((n, n))                # set_rows reads the triangle: the device's matrix is symmetric
    walls, rescanned = [], []
    for run in range(RUNS + 1):
        t = T.Tree(ctx, n)
        t0 = time.perf_counter()
        t.set_rows(0, n, d)
        t1 = time.perf_counter()
        mg, st = t.build(T.AVERAGE)
        t2 = time.perf_counter()
        t.free()
        print("N %d %s: set_rows %.3f s, lash_tree_build %.3f s, %d steps, %d rescanned rows, %d matrix bytes"
              % (n, "warm-up" if run == 0 else "run %d" % run, t1 - t0, t2 - t1, st["steps"], st["rescanned_rows"], st["bytes"]), flush=True)
        if run:
            walls.append(t2 - t1)
            rescanned.append(st["rescanned_rows"])
    summary("N %d lash_tree_build average (rescanned rows %s)" % (n, sorted(set(rescanned))), walls)
    walls = []
    for run in range(RUNS + 1 if WITH_NJ else 0):
        t = T.Tree(ctx, n)
        t0 = time.perf_counter()
        t.set_rows(0, n, d)
        t1 = time.perf_counter()
        jn, st = NJ.njbuild(t)
        t2 = time.perf_counter()
        t.free()
        print("N %d %s: set_rows %.3f s, lash_tree_build_nj %.3f s, %d steps, %d matrix bytes"
              % (n, "warm-up" if run == 0 else "run %d" % run, t1 - t0, t2 - t1, st["steps"], st["bytes"]), flush=True)
        if run:
            walls.append(t2 - t1)
    if WITH_NJ:
        summary("N %d lash_tree_build_nj" % n, walls)
        scan_bytes = 8 * sum(r * n // 2 for r in range(3, n + 1))
        print("N %d lash_tree_build_nj: scan traffic model %.3f TB (2 N^3 = %.3f TB), %.0f GB/s at the median"
              % (n, scan_bytes / 1e12, 2 * n ** 3 / 1e12, scan_bytes / 1e9 / statistics.median(walls)), flush=True)
    del d

if CLI_N:
    import torch
    assert CLI_N % FAM == 0
    work = tempfile.mkdtemp(prefix="tree_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    dev = torch.device("cuda", 0)
    ib = lash_amd.image_bytes("hmh")
    img = torch.zeros((CLI_N, ib), dtype=torch.uint8, device=dev)
    n_fam = CLI_N // FAM
    rates = np.geomspace(0.001, 0.05, FAM - 1)
    chunk = min(max(1, 4_000_000_000 // L), n_fam)
    base = torch.empty(chunk * L, dtype=torch.uint8, device=dev)
    member = torch.empty_like(base)
    out = torch.empty((chunk, ib), dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    t0 = time.perf_counter()
    for f0 in range(0, n_fam, chunk):
        n = min(chunk, n_fam - f0)
        ctx.synth_genomes_device(f0, n, L, base)
        ctx.synchronize()
        rec_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        d_rec = torch.from_numpy(rec_off.astype(np.int64)).to(dev)
        for m in range(FAM):
            member[: n * L].copy_(base[: n * L])
            if m:
                n_sub = int(rates[m - 1] * n * L)
                at = torch.randint(0, n * L, (n_sub,), device=dev, generator=gen)
                member[at] = acgt[torch.randint(0, 4, (n_sub,), device=dev, generator=gen)]
            torch.cuda.synchronize(dev)
            ctx.sketch_batch_device("hmh", k, 0, 42, member, d_rec, n, np.arange(n + 1, dtype=np.uint64), rec_off, out[:n].reshape(-1))
            ctx.synchronize()
            img[torch.arange(f0, f0 + n, device=dev) * FAM + m] = out[:n]
    torch.cuda.synchronize(dev)
    print("sketched %d genomes of %d bases (%d families of %d) in %.2f s" % (CLI_N, L, n_fam, FAM, time.perf_counter() - t0), flush=True)
    del base, member, out
    H.zstd_write(os.path.join(work, "w_sketches.bin"), img.cpu().numpy().tobytes(), 3, 16)
    open(os.path.join(work, "w_files.json"), "w").write(H.json_array(["g%06d.fa" % i for i in range(CLI_N)]))
    H.write_parameters(os.path.join(work, "w"), "hmh", k, 0, 42)
    del img
    torch.cuda.empty_cache()
    ctx.close()
    env = dict(os.environ, LASH_CLI_TIMING="1")
    walls = {"--dm": [], "--tree": []}
    if WITH_NJ:
        walls["--tree --nj"] = []
    try:
        for run in range(RUNS + 1):                           # run 0 warms up: not counted
            for key in walls:
                path = os.path.join(work, "out" + key.replace("--", "_").replace(" ", ""))
                t0 = time.perf_counter()
                r = subprocess.run([H.CLI, "dist", "-q", "w", "-r", "w", "-o", path, "-t", "16", "--file-order"] + key.split(), cwd=work, capture_output=True,
                                   text=True, env=env)
                wall = time.perf_counter() - t0
                print("run %d: N %d %s: rc %d, %.2f s wall, %d output bytes" % (run, CLI_N, key, r.returncode, wall, os.path.getsize(path)), flush=True)
                if r.returncode:
                    print(r.stderr[-1800:], flush=True)
                    sys.exit(1)
                if run:
                    walls[key].append(wall)
                if key != "--dm":
                    print("".join(ln + "\n" for ln in r.stderr.split("\n") if key + ":" in ln or (run == 0 and "[lash dist]" in ln)), end="", flush=True)
                os.remove(path)
        for key, w in walls.items():
            summary("N %d lash dist %s" % (CLI_N, key), w)
    finally:
        for f in os.listdir(work):
            os.remove(os.path.join(work, f))
        os.rmdir(work)
else:
    ctx.close()
