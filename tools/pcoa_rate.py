#!/usr/bin/env python3
"""What lash_tree_build_pcoa costs on a synthetic matrix (not a test): python tools/pcoa_rate.py [--n 16384]

For K = 3 and K = 10 it prints the iterations of a full solve and its wall time; the time of one iteration (one B Q product plus its
panel work and two host round trips), taken as the difference of two runs cut off at 12 and at 4 iterations, so an upper bound for the
product kernel; that time as a fraction of a plain device-to-device copy of 8 n^2 bytes timed in the same run (the copy reads AND
writes 8 n^2 bytes; the product only reads them); and the wall time of torch.linalg.eigvalsh of the same matrix on the same device,
the full solve a user has today."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=24)
    a = ap.parse_args()
    import torch
    import lash_amd
    from lash_amd import _lib
    n = a.n
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, a.dim)) * (0.7 ** np.arange(a.dim))
    g = x @ x.T
    sq = np.diag(g)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * g, 0.0))
    d = d * (1.0 + 0.05 * np.sin(np.add.outer(np.arange(n), np.arange(n)) * 0.37))      # not Euclidean: B gets negative eigenvalues
    d = np.tril(d, -1)
    d = d + d.T
    ctx = lash_amd.Context(0)
    lib = ctx._lib

    def build(k, max_iter):
        h = C.c_void_p()
        assert lib.lash_tree_create(ctx._h, n, C.byref(h)) == 0
        assert lib.lash_tree_set_rows(ctx._h, h, 0, n, d.ctypes.data) == 0
        eig, coords, st = np.zeros(k), np.zeros((n, k)), _lib.PcoaStats()
        t0 = time.perf_counter()
        rc = lib.lash_tree_build_pcoa(ctx._h, h, k, 0.0, max_iter, eig.ctypes.data, coords.ctypes.data, C.byref(st))
        ms = (time.perf_counter() - t0) * 1e3
        lib.lash_tree_free(ctx._h, h)
        return rc, ms, st, eig

    td = torch.from_numpy(d).cuda()
    out = torch.empty_like(td)
    for _ in range(3):
        out.copy_(td)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        out.copy_(td)
    torch.cuda.synchronize()
    copy_ms = (time.perf_counter() - t0) * 1e2
    print("n = %d: a device-to-device copy of %.3f GB takes %.3f ms (%.2f TB/s read + written)" % (n, 8e-9 * n * n, copy_ms, 16e-9 * n * n / copy_ms))
    del out
    build(3, 2)                                                                          # warm-up: module load
    for k in (3, 10):
        rc, ms, st, eig = build(k, 0)
        _, ms4, _, _ = build(k, 4)
        _, ms12, _, _ = build(k, 12)
        it_ms = (ms12 - ms4) / 8.0
        print("K = %d: rc %d, %d iterations, %d products, full solve %.1f ms, worst residual %.3g, shift %.4g, eigenvalues %s" %
              (k, rc, st.iterations, st.products, ms, st.worst_residual, st.shift, " ".join("%.6g" % v for v in eig[:3])))
        print("K = %d: %.3f ms per iteration (one B Q product and its panel work): %.2f TB/s of matrix read, copy time / iteration time = %.2f" %
              (k, it_ms, 8e-9 * n * n / it_ms, copy_ms / it_ms))
    a_ = -0.5 * td * td
    r = a_.mean(1)
    b = a_ - r[:, None] - r[None, :] + r.mean()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = torch.linalg.eigvalsh(b)
    torch.cuda.synchronize()
    print("torch.linalg.eigvalsh of the same B on the same device: %.1f ms; its top three: %s" %
          ((time.perf_counter() - t0) * 1e3, " ".join("%.6g" % v for v in w[-3:].flip(0).tolist())))
    ctx.close()


if __name__ == "__main__":
    main()
