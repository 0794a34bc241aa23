#!/usr/bin/env python3
"""tools/dist_cluster_rate.py [N] [FAM] [MAX_RATE] [WORKDIR] [RUNS] — `lash dist --cluster 0.05` against `--max-dist 0.05` on one set.

N (default 100 000) hmh k=16 sketches of 5 Mbp genomes made on the device as families of FAM (default 10: a synthetic base genome and
FAM - 1 copies with substitution rates spread geometrically from 0.1 % to MAX_RATE, default 0.1), written as the sketch-file set
WORKDIR/w (default: a fresh directory under /dev/shm, removed at the end).  The two shapes of DESIGN.md §4.6:
    sparse   100000 10 0.1        (the set of tools/dist_within_rate.py: few links per name)
    dense    20000 1000 0.01      (20 families of 1 000: ~10^7 links)
Then RUNS times (default 3), with LASH_CLI_TIMING=1 and -t 16:
    lash dist -q w -r w -o WORKDIR/kept.tsv --max-dist 0.05     (rows and bytes counted)
    lash dist -q w -r w -o WORKDIR/clusters.tsv --cluster 0.05  (the --cluster timing line; bytes counted)
and prints the wall times, their median and spread.  When the kept rows are at most 2 * 10^7 it also checks that the cluster file is
the connected components of the --max-dist rows.  With a WORKDIR given the files stay, so that a separate
`rocprofv3 --kernel-trace --stats -- lash dist ... --cluster 0.05` can read them.  To compare with another build's --max-dist, point
LASH_MAXDIST_CLI at its `lash` binary."""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
FAM = int(sys.argv[2]) if len(sys.argv) > 2 else 10
MAX_RATE = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
keep_dir = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else None
RUNS = int(sys.argv[5]) if len(sys.argv) > 5 else 3
L, k, D = 5_000_000, 16, "0.05"
RATES = np.geomspace(0.001, MAX_RATE, FAM - 1)             # member m > 0: substitution rate RATES[m - 1]
assert N % FAM == 0
work = keep_dir or tempfile.mkdtemp(prefix="cluster_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
os.makedirs(work, exist_ok=True)

if not os.path.exists(os.path.join(work, "w_sketches.bin")):
    ctx = lash_amd.Context(0)
    dev = torch.device("cuda", 0)
    ib = lash_amd.image_bytes("hmh")
    img = torch.zeros((N, ib), dtype=torch.uint8, device=dev)
    n_fam = N // FAM
    chunk = min(1250, n_fam)                               # base genomes held at a time
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
    print("sketched %d genomes (%d families of %d, rates up to %g) in %.2f s" % (N, n_fam, FAM, MAX_RATE, time.perf_counter() - t0), flush=True)
    del base, member, out
    names = ["g%06d.fa" % i for i in range(N)]
    H.zstd_write(os.path.join(work, "w_sketches.bin"), img.cpu().numpy().tobytes(), 3, 16)
    open(os.path.join(work, "w_files.json"), "w").write(H.json_array(names))
    H.write_parameters(os.path.join(work, "w"), "hmh", k, 0, 42)
    ctx.close()
    del img
    torch.cuda.empty_cache()

env = dict(os.environ, LASH_CLI_TIMING="1")
kept, clu = os.path.join(work, "kept.tsv"), os.path.join(work, "clusters.tsv")
cases = ((["--max-dist", D], kept, os.environ.get("LASH_MAXDIST_CLI") or H.CLI), (["--cluster", D], clu, H.CLI))
walls = {c[0][0]: [] for c in cases}
for run in range(RUNS):
    for extra, out, cli in cases:
        t0 = time.perf_counter()
        r = subprocess.run([cli, "dist", "-q", "w", "-r", "w", "-o", out, "-t", "16"] + extra, cwd=work, capture_output=True, text=True, env=env)
        wall = time.perf_counter() - t0
        walls[extra[0]].append(wall)
        print("run %d: lash dist %s: rc %d, %.2f s wall, %d output bytes" % (run, " ".join(extra), r.returncode, wall, os.path.getsize(out)))
        if run == 0 or r.returncode:
            print(r.stderr[-1800:], flush=True)
        else:
            print("".join(ln + "\n" for ln in r.stderr.split("\n") if "--cluster:" in ln and "pairs" in ln), end="", flush=True)
        if r.returncode:
            sys.exit(1)
for key, w in walls.items():
    print("%s %s: walls %s, median %.2f s, spread %.2f s" % (key, D, " ".join("%.2f" % x for x in w), statistics.median(w), max(w) - min(w)))
spread = max(walls["--max-dist"]) - min(walls["--max-dist"])
m_c, m_w = statistics.median(walls["--cluster"]), statistics.median(walls["--max-dist"])
print("--cluster / --max-dist median wall: %.3f (not slower within max(10 %%, spread %.2f s): %s)"
      % (m_c / m_w, spread, m_c <= m_w + max(0.1 * m_w, spread)), flush=True)

# the cluster file against the connected components of the --max-dist rows
with open(kept, "rb") as f:
    rows = sum(c.count(b"\n") for c in iter(lambda: f.read(1 << 24), b"")) - 1
print("rows kept at --max-dist %s: %d (%.2f per sketch)" % (D, rows, rows / N))
got = [ln.split("\t") for ln in open(clu).read().split("\n")[1:-1]]
n_clusters = len({g[0] for g in got})
print("clusters: %d over %d names" % (n_clusters, len(got)))
if rows <= 20_000_000:
    order = {g[1]: i for i, g in enumerate(got)}                      # any fixed numbering of the names
    parent = np.arange(len(got))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    with open(kept) as f:
        next(f)
        for ln in f:
            a, b, _ = ln.split("\t")
            a, b = find(order[a]), find(order[b])
            if a != b:
                parent[max(a, b)] = min(a, b)
    comp = {}
    for name, i in order.items():
        comp.setdefault(find(i), set()).add(name)
    mine = {}
    for rep, member in got:
        mine.setdefault(rep, set()).add(member)
    same = sorted(map(sorted, comp.values())) == sorted(map(sorted, mine.values()))
    print("components of the --max-dist rows: %d; equal to the cluster file: %s" % (len(comp), same), flush=True)
    if not same:
        sys.exit(1)
if keep_dir is None:
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)
