#!/usr/bin/env python3
"""tools/dist_within_rate.py [--containment] [N] [WORKDIR] — `lash dist --max-dist` against the unfiltered run on the BASELINE configs[3] shape.

N (default 100 000) hmh k=16 sketches of 5 Mbp genomes made on the device as families of 10 (a synthetic base genome and 9 copies with
0.1-10 % substitutions), written as the sketch-file set WORKDIR/w (default: a fresh directory under /dev/shm, removed at the end).
Then, with LASH_CLI_TIMING=1:
    lash dist -q w -r w -o WORKDIR/kept.tsv --max-dist 0.05        (rows kept: counted)
    lash dist -q w -r w -o /dev/null                               (the unfiltered run)
and prints the wall times and stage marks.  With a WORKDIR given the files stay, so that a separate
`rocprofv3 --kernel-trace --stats -- lash dist ... --max-dist 0.05` can read them.
--containment: the cost of `lash dist --containment query` in the filter.  A containment run is always the rectangle, so the set is
also written under a second prefix v (the same sketches and names from other files: the default measure then runs the rectangle too), and
    lash dist -q v -r w -o /dev/null --max-dist 0.05                          three times
    lash dist -q v -r w -o /dev/null --max-dist 0.05 --containment query      three times
are timed instead of the two runs above."""
import os
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

containment = "--containment" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--containment"]
N = int(argv[0]) if len(argv) > 0 else 100_000
keep_dir = argv[1] if len(argv) > 1 else None
L, k, FAM = 5_000_000, 16, 10
RATES = np.geomspace(0.001, 0.1, FAM - 1)                  # member m > 0: substitution rate RATES[m - 1]
assert N % FAM == 0
work = keep_dir or tempfile.mkdtemp(prefix="within_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
os.makedirs(work, exist_ok=True)

if not os.path.exists(os.path.join(work, "w_sketches.bin")):
    ctx = lash_amd.Context(0)
    dev = torch.device("cuda", 0)
    ib = lash_amd.image_bytes("hmh")
    img = torch.zeros((N, ib), dtype=torch.uint8, device=dev)
    n_fam, chunk = N // FAM, 1250
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
    print("sketched %d genomes (%d families of %d) in %.2f s" % (N, n_fam, FAM, time.perf_counter() - t0), flush=True)
    del base, member, out
    names = ["g%06d.fa" % i for i in range(N)]
    H.zstd_write(os.path.join(work, "w_sketches.bin"), img.cpu().numpy().tobytes(), 3, 16)
    open(os.path.join(work, "w_files.json"), "w").write(H.json_array(names))
    H.write_parameters(os.path.join(work, "w"), "hmh", k, 0, 42)
    ctx.close()
    del img
    torch.cuda.empty_cache()

env = dict(os.environ, LASH_CLI_TIMING="1")
if containment:
    if not os.path.exists(os.path.join(work, "v_sketches.bin")):
        os.symlink("w_sketches.bin", os.path.join(work, "v_sketches.bin"))
        open(os.path.join(work, "v_files.json"), "w").write(open(os.path.join(work, "w_files.json")).read())
        H.write_parameters(os.path.join(work, "v"), "hmh", k, 0, 42)
    for extra in ([], ["--containment", "query"]):
        for rep in range(3):
            t0 = time.perf_counter()
            r = subprocess.run([H.CLI, "dist", "-q", "v", "-r", "w", "-o", "/dev/null", "-t", "16", "--max-dist", "0.05"] + extra, cwd=work,
                               capture_output=True, text=True, env=env)
            print("lash dist -q v -r w --max-dist 0.05 %s: run %d, rc %d, %.2f s wall" % (" ".join(extra) or "(default measure)", rep, r.returncode,
                                                                                          time.perf_counter() - t0))
            print(r.stderr[-1500:], flush=True)
            if r.returncode:
                sys.exit(1)
for extra, out in () if containment else ((["--max-dist", "0.05"], os.path.join(work, "kept.tsv")), ([], "/dev/null")):
    t0 = time.perf_counter()
    r = subprocess.run([H.CLI, "dist", "-q", "w", "-r", "w", "-o", out, "-t", "16"] + extra, cwd=work, capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t0
    print("lash dist %s: rc %d, %.2f s wall" % (" ".join(extra) or "(unfiltered, /dev/null)", r.returncode, wall))
    print(r.stderr[-1500:], flush=True)
    if r.returncode:
        sys.exit(1)
    if extra:
        with open(out, "rb") as f:
            rows = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b"")) - 1
        print("rows kept at --max-dist 0.05: %d (%.2f per sketch)" % (rows, rows / N), flush=True)
if keep_dir is None:
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)
