#!/usr/bin/env python3
"""tools/dist_derep_rate.py [N] [FAM] [MAX_RATE] [L] [WORKDIR] [RUNS] — `lash dist --derep 0.05` against the other reduced outputs on one
set where dereplication matters.

N (default 20 000) hmh k=16 sketches of L-base genomes (default 1 000 000) made on the device as families of FAM (default 100: a
synthetic base genome and FAM - 1 copies with substitution rates spread geometrically from 0.1 % to MAX_RATE, default 0.01), in family
order, written as the sketch-file set WORKDIR/w (default: a fresh directory under /dev/shm, removed at the end).  Then RUNS times
(default 3), with LASH_CLI_TIMING=1 and -t 16, in turn:
    lash dist -q w -r w --max-dist 0.05 | --top 5 | --cluster 0.05     with this build and, when LASH_PARENT_CLI names another build's
                                                                        `lash` binary, with that one too
    lash dist -q w -r w --derep 0.05                                    (the --derep timing line)
and prints every wall time, and per case the median and the spread (max - min).  The --derep file is checked against the greedy walk
over the --max-dist rows when those are at most 2 * 10^7."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lash_amd  # noqa: E402
import host_lib as H  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
FAM = int(sys.argv[2]) if len(sys.argv) > 2 else 100
MAX_RATE = float(sys.argv[3]) if len(sys.argv) > 3 else 0.01
L = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
keep_dir = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
RUNS = int(sys.argv[6]) if len(sys.argv) > 6 else 3
k, D = 16, "0.05"
RATES = np.geomspace(0.001, MAX_RATE, FAM - 1)             # member m > 0: substitution rate RATES[m - 1]
assert N % FAM == 0
work = keep_dir or tempfile.mkdtemp(prefix="derep_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
os.makedirs(work, exist_ok=True)

if not os.path.exists(os.path.join(work, "w_sketches.bin")):
    ctx = lash_amd.Context(0)
    dev = torch.device("cuda", 0)
    ib = lash_amd.image_bytes("hmh")
    img = torch.zeros((N, ib), dtype=torch.uint8, device=dev)
    n_fam = N // FAM
    chunk = min(max(1, 6_000_000_000 // L), n_fam)         # base genomes held at a time
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
                n_sub = int(RATES[m - 1] * n * L)
                at = torch.randint(0, n * L, (n_sub,), device=dev, generator=gen)
                member[at] = acgt[torch.randint(0, 4, (n_sub,), device=dev, generator=gen)]
            torch.cuda.synchronize(dev)
            ctx.sketch_batch_device("hmh", k, 0, 42, member, d_rec, n, np.arange(n + 1, dtype=np.uint64), rec_off, out[:n].reshape(-1))
            ctx.synchronize()
            img[torch.arange(f0, f0 + n, device=dev) * FAM + m] = out[:n]
    torch.cuda.synchronize(dev)
    print("sketched %d genomes of %d bases (%d families of %d, rates up to %g) in %.2f s" % (N, L, n_fam, FAM, MAX_RATE, time.perf_counter() - t0),
          flush=True)
    del base, member, out
    names = ["g%06d.fa" % i for i in range(N)]
    H.zstd_write(os.path.join(work, "w_sketches.bin"), img.cpu().numpy().tobytes(), 3, 16)
    open(os.path.join(work, "w_files.json"), "w").write(H.json_array(names))
    H.write_parameters(os.path.join(work, "w"), "hmh", k, 0, 42)
    ctx.close()
    del img
    torch.cuda.empty_cache()

env = dict(os.environ, LASH_CLI_TIMING="1")
parent = os.environ.get("LASH_PARENT_CLI")
cases = []
for extra in (["--max-dist", D], ["--top", "5"], ["--cluster", D]):
    if parent:
        cases.append(("parent " + extra[0], extra, parent))
    cases.append(("this " + extra[0], extra, H.CLI))
cases.append(("this --derep", ["--derep", D], H.CLI))
walls = {c[0]: [] for c in cases}
for run in range(RUNS):
    for key, extra, cli in cases:
        out = os.path.join(work, key.replace(" ", "_").replace("--", "") + ".tsv")
        t0 = time.perf_counter()
        r = subprocess.run([cli, "dist", "-q", "w", "-r", "w", "-o", out, "-t", "16", "--file-order"] + extra, cwd=work, capture_output=True, text=True,
                           env=env)
        wall = time.perf_counter() - t0
        walls[key].append(wall)
        print("run %d: %s: rc %d, %.2f s wall, %d output bytes" % (run, key, r.returncode, wall, os.path.getsize(out)), flush=True)
        if r.returncode:
            print(r.stderr[-1800:], flush=True)
            sys.exit(1)
        if key == "this --derep":
            print("".join(ln + "\n" for ln in r.stderr.split("\n") if "--derep:" in ln or (run == 0 and "[lash dist]" in ln)), end="", flush=True)
for key, w in walls.items():
    print("%s: walls %s, median %.2f s, spread %.2f s" % (key, " ".join("%.2f" % x for x in w), statistics.median(w), max(w) - min(w)), flush=True)

# the --derep file against the greedy walk over the --max-dist rows (list order: the names sort as their indices)
kept = os.path.join(work, "this_max-dist.tsv")
with open(kept, "rb") as f:
    rows = sum(c.count(b"\n") for c in iter(lambda: f.read(1 << 24), b"")) - 1
print("rows kept at --max-dist %s: %d (%.2f per sketch)" % (D, rows, rows / N))
got = [ln.split("\t") for ln in open(os.path.join(work, "this_derep.tsv")).read().split("\n")[1:-1]]
print("representatives: %d over %d names" % (len({g[0] for g in got}), len(got)))
if rows <= 20_000_000:
    near = [[] for _ in range(N)]
    with open(kept) as f:
        next(f)
        for ln in f:
            a, b, _ = ln.split("\t")
            a, b = int(a[1:7]), int(b[1:7])
            if a != b:
                near[max(a, b)].append(min(a, b))
    rep = []
    for i in range(N):
        rep.append(next((j for j in sorted(near[i]) if rep[j] == j), i))
    order = sorted(range(N), key=lambda i: (rep[i], i))
    same = got == [["g%06d.fa" % rep[i], "g%06d.fa" % i] for i in order]
    print("equal to the greedy walk over the --max-dist rows: %s" % same, flush=True)
    if not same:
        sys.exit(1)
if keep_dir is None:
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)
