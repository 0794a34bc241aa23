#!/usr/bin/env python3
"""tools/per_record_rate.py [genomes] [runs] [dir] — `lash sketch --per-record` on ONE multi-FASTA against plain `lash sketch` on the
same records written one per file (what a user had to do before the flag): N small genomes of unequal size (the viral_rate.py
distribution: 3..300 kbp, log-uniform), hmh k=16, -t 16 (GPU box; put `dir` on tmpfs).  Checks that the two decompressed _sketches.bin are
equal, prints the wall time of every run and the medians."""
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import host_lib as H

G = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
base = sys.argv[3] if len(sys.argv) > 3 else ("/dev/shm" if os.path.isdir("/dev/shm") else None)
work = tempfile.mkdtemp(prefix="per_record_rate_", dir=base)
try:
    rng = np.random.default_rng(13)
    lens = np.exp(rng.uniform(np.log(3e3), np.log(3e5), size=G)).astype(np.int64)
    pool = rng.integers(0, 4, size=int(lens.max()) + (1 << 22), dtype=np.uint8)
    pool = np.frombuffer(b"ACGT", np.uint8)[pool]                     # every genome: a window of one random sequence, 80 per line
    os.mkdir(os.path.join(work, "split"))
    paths = []
    t0 = time.perf_counter()
    with open(os.path.join(work, "multi.fa"), "wb") as multi:
        for g in range(G):
            L = int(lens[g])
            s = int(rng.integers(0, 1 << 22))
            body = pool[s:s + L]
            full = (L // 80) * 80
            lines = np.empty((L // 80, 81), np.uint8)
            lines[:, :80] = body[:full].reshape(-1, 80)
            lines[:, 80] = 10
            rec = b">g%d len=%d\n" % (g, L) + lines.tobytes() + (body[full:].tobytes() + b"\n" if L > full else b"")
            multi.write(rec)
            d = os.path.join(work, "split", "%03d" % (g // 1000))
            if g % 1000 == 0:
                os.mkdir(d)
            paths.append(os.path.join(d, "g%d.fa" % g))
            with open(paths[-1], "wb") as f:
                f.write(rec)
    with open(os.path.join(work, "multi.txt"), "w") as f:
        f.write(os.path.join(work, "multi.fa") + "\n")
    with open(os.path.join(work, "split.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    print("%d genomes, %.2f GB of FASTA text, written twice in %.1f s" % (G, os.path.getsize(os.path.join(work, "multi.fa")) / 1e9,
                                                                        time.perf_counter() - t0), flush=True)

    def run(form):
        out = os.path.join(work, "out_" + form)
        cmd = [H.CLI, "sketch", "-f", os.path.join(work, form + ".txt"), "-o", out, "-a", "hmh", "-k", "16", "-t", "16"]
        if form == "multi":
            cmd.append("--per-record")
        t = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        dt = time.perf_counter() - t
        if r.returncode != 0:
            sys.exit("%s failed: %s" % (" ".join(cmd), r.stderr))
        print("  %-5s %.2f s   %s" % (form, dt, r.stderr.strip().split("\n")[-1]), flush=True)
        return dt

    times = {"split": [], "multi": []}
    for i in range(RUNS):                                            # interleaved, so that both forms see the same machine
        for form in ("split", "multi"):
            times[form].append(run(form))
    a = H.zstd_read(os.path.join(work, "out_multi_sketches.bin"))
    b = H.zstd_read(os.path.join(work, "out_split_sketches.bin"))
    print("decompressed _sketches.bin equal: %s (%d bytes)" % (a == b, len(a)))
    ms, mm = statistics.median(times["split"]), statistics.median(times["multi"])
    spread = max(times["split"]) - min(times["split"])
    print("split files: median %.2f s (spread %.2f s); one multi-FASTA --per-record: median %.2f s (%+.1f %%); margin: the larger of 10 %% and the spread -> %s"
          % (ms, spread, mm, 100 * (mm - ms) / ms, "inside" if mm <= ms + max(0.1 * ms, spread) else "OUTSIDE"))
    if a != b:
        sys.exit(1)
finally:
    shutil.rmtree(work, ignore_errors=True)
