"""The model of `lash spectrum` (tests/spectrum_model.py) against what it claims, and the command line's arithmetic against the model.

The claim: a bucket's union register belongs to one k-mer of the union, drawn uniformly from the bucket's distinct
k-mers, and the members whose register equals it are the holders of that k-mer — so the bins over the occupied buckets are a uniform
sample of the multiplicity spectrum.  It is checked on sets built in numpy with a known spectrum: 24 sets, 30 000 k-mers in all of them,
20 000 in the first 10, 2 000 private to each (and the same at a tenth of the size), registers (lz << 10) | 10 random bits.  Every
fraction the truth has must lie within 5 binomial standard errors sqrt(f (1 - f) / occupied) of it; the mass at counts the truth does
not have (two distinct k-mers tying at a bucket's top register) must stay below 1e-3.  Seen with these seeds: at most 1.21 standard
errors and 1.22e-4 (-s prints every figure)."""
import ctypes as C
import math

import numpy as np
import pytest

import spectrum_model as S

N_SETS, N_SHELL = 24, 10


def _table(rng, n_kmers):
    """the register table of n_kmers random k-mers: bucket uniform, lz geometric from 1, ten random bits"""
    bucket = rng.integers(0, S.M, n_kmers)
    lz = np.minimum(rng.geometric(0.5, n_kmers), 63)
    reg = ((lz << 10) | rng.integers(0, 1024, n_kmers)).astype(np.uint32)
    tab = np.zeros(S.M, dtype=np.uint32)
    np.maximum.at(tab, bucket, reg)
    return tab


def _sets(seed, core, shell, private):
    rng = np.random.default_rng(seed)
    in_all, in_some = _table(rng, core), _table(rng, shell)
    regs = np.zeros((N_SETS, S.M), dtype=np.uint32)
    for j in range(N_SETS):
        regs[j] = np.maximum(in_all, _table(rng, private))
        if j < N_SHELL:
            regs[j] = np.maximum(regs[j], in_some)
    total = core + shell + N_SETS * private
    return regs, {N_SETS: core / total, N_SHELL: shell / total, 1: N_SETS * private / total}


@pytest.mark.parametrize("seed,core,shell,private", [(1, 30_000, 20_000, 2_000), (2, 30_000, 20_000, 2_000), (3, 30_000, 20_000, 2_000),
                                                      (4, 3_000, 2_000, 200)], ids=["seed1", "seed2", "seed3", "tenth"])
def test_the_bins_sample_the_multiplicity_spectrum(seed, core, shell, private):
    regs, truth = _sets(seed, core, shell, private)
    h = S.hist(regs, range(N_SETS))
    assert h.dtype == np.uint32 and len(h) == N_SETS + 1 and int(h.sum()) == S.M
    occ = S.occupied(h)
    assert occ == int((regs.max(axis=0) != 0).sum()) and occ > S.M // 3
    worst = 0.0
    for c, f in truth.items():
        se = math.sqrt(f * (1.0 - f) / occ)
        z = abs(int(h[c]) / occ - f) / se
        worst = max(worst, z)
        print("seed %d count %d: fraction %.5f, truth %.5f, %.2f standard errors" % (seed, c, int(h[c]) / occ, f, z))
        assert z <= 5.0, (c, int(h[c]) / occ, f, z)
    stray = sum(int(h[c]) for c in range(1, N_SETS + 1) if c not in truth) / occ
    print("seed %d: occupied %d, worst %.2f standard errors, stray mass %.2e" % (seed, occ, worst, stray))
    assert stray <= 1e-3


def test_the_invariants_of_the_bins():
    regs, _ = _sets(7, 3_000, 2_000, 200)
    filled = int((regs[3] != 0).sum())
    assert 0 < filled < S.M
    assert S.hist(regs, []).tolist() == [S.M]
    assert S.hist(regs, [3]).tolist() == [S.M - filled, filled]                              # a single member holds all it has
    assert S.hist(regs, [3, 3]).tolist() == [S.M - filled, 0, filled]                        # a member with itself: listed twice, counted twice
    for members in ([0, 1], [5, 5, 6], list(range(N_SETS)), [23, 0, 11, 0]):
        h = S.hist(regs, members)
        assert len(h) == len(members) + 1 and int(h.sum()) == S.M
        assert S.occupied(h) == int((regs[members].max(axis=0) != 0).sum())
    # the pair case is dist's (C, N): registers equal and not 0; registers not both 0
    a, b = regs[2], regs[15]
    h = S.hist(regs, [2, 15])
    assert int(h[2]) == int(((a == b) & (a != 0)).sum()) and S.occupied(h) == int(((a != 0) | (b != 0)).sum())


def test_registers_follow_the_layout():
    rng = np.random.default_rng(5)
    regs = rng.integers(0, 65536, (2, S.M)).astype(np.uint32)
    le = np.concatenate([np.zeros((2, 8), np.uint8), regs.astype("<u2").view(np.uint8).reshape(2, -1)], axis=1)
    be = regs.astype(">u2").view(np.uint8).reshape(2, -1)
    assert np.array_equal(S.registers(le, 8), regs) and np.array_equal(S.registers(be, 0, big_endian=True), regs)


def _spectra():
    regs, _ = _sets(11, 3_000, 2_000, 200)
    yield S.hist(regs, range(N_SETS)), 9_876.543
    yield S.hist(regs, [0, 1, 2]), 3_400.25
    yield S.hist(regs, [4]), 1.0e9
    yield np.array([S.M, 0, 0], dtype=np.uint32), 0.0                                        # nothing occupied


def test_the_curves_end_where_they_must():
    for h, U in _spectra():
        n = len(h) - 1
        pan, core = S.curves(h, U)
        assert len(pan) == len(core) == n
        if S.occupied(h) == 0:
            assert pan == [0.0] * n and core == [0.0] * n and S.classes(h, U) == (0.0, 0.0, 0.0)
            continue
        assert abs(pan[-1] - U) <= 1e-12 * U and abs(core[-1] - S.kmers(h, n, U)) <= 1e-12 * max(S.kmers(h, n, U), 1e-300)
        assert all(pan[m] >= pan[m - 1] * (1 - 1e-12) and core[m] <= core[m - 1] * (1 + 1e-12) for m in range(1, n))
        # one genome: pan(1) = core(1) = the mean size of a member, sum_c c K(c) / n
        mean = sum(c * S.kmers(h, c, U) for c in range(1, n + 1)) / n
        assert abs(pan[0] - mean) <= 1e-12 * mean and abs(core[0] - mean) <= 1e-12 * mean
        assert abs(sum(S.classes(h, U)) - U) <= 1e-12 * U


def test_the_command_line_computes_the_models_numbers():
    """csrc/host/spectrum.cpp through its test hook: the class sums are the model's doubles, the curves within 1e-9 relative"""
    import host_lib as H
    fn = H.lib.lash_host_spectrum_numbers
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    for h, U in _spectra():
        n = len(h) - 1
        h = np.ascontiguousarray(h, dtype=np.uint32)
        for core, cloud in ((0.95, 0.15), (1.0, 1.0), (0.5, 0.05)):
            k, pan, in_all = np.zeros(3), np.zeros(n), np.zeros(n)
            fn(h.ctypes.data, n, U, core, cloud, k.ctypes.data, pan.ctypes.data, in_all.ctypes.data)
            assert tuple(k.tolist()) == S.classes(h, U, core, cloud)
            want_pan, want_core = S.curves(h, U)
            assert np.allclose(pan, want_pan, rtol=1e-9, atol=0.0) and np.allclose(in_all, want_core, rtol=1e-9, atol=0.0)
