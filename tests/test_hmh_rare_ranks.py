"""tests/golden/hmh_rare_ranks.json holds 32-bit HyperMinHash inputs whose rank random genomes never reach (found by hashing all 2^32 inputs:
tests/golden/make_hmh_rare_ranks.py).  The GPU tests (tests/test_gpu_rare_hashes.py) trust it; this module checks it without a GPU: every row
hashed by two independent restatements of xxh3_128 (the oracle's C, tests/pyref.py's Python) gives the same bucket, rank and signature, the
rank is what the row's group promises, a genome spelling such an input sets exactly that one register, and the groups the GPU tests build
their genomes from are there."""
import numpy as np
import pytest

import oracle_lib as O
import pyref as R


@pytest.fixture(scope="module")
def groups():
    return O.hmh_rare_ranks()


def _pyref_rank(w, seed, x_is_low):
    lo, hi = R.xxh3_128_4b(w, seed)
    x, y = (lo, hi) if x_is_low else (hi, lo)
    return x >> 50, R.clz64(((x << 14) & R.M64) ^ 0x3FFF), y & 0x3FF


def test_every_row_has_the_rank_its_group_promises_under_both_hash_restatements(groups):
    n = 0
    for g in groups:
        low = g["x"] == "low"
        assert g["x"] in ("high", "low") and g["kind"] in ("floor", "single", "pair") and g["w"], g
        ranks = []
        for w in g["w"]:
            assert 0 <= w < 2**32
            r = O.hmh_rank(w, g["seed"], low)
            assert r == _pyref_rank(w, g["seed"], low), (g["seed"], g["x"], hex(w))
            ranks.append(r)
            if g["kind"] == "floor":
                assert r[1] >= g["min_lzm1"], (g["seed"], g["x"], hex(w), r)
            else:
                assert r[1] == g["lzm1"], (g["seed"], g["x"], hex(w), r)
        if g["kind"] == "floor":
            assert g["w"] == sorted(set(g["w"]))
        if g["kind"] == "pair":
            assert len(ranks) % 2 == 0
            for a, b in zip(ranks[::2], ranks[1::2]):
                assert a[0] == b[0] and a[1] == b[1] and a[2] != b[2], (g, a, b)       # same bucket, same rank, another signature
        n += len(ranks)
    assert n > 8000


def _spell(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)).encode()


def test_a_genome_spelling_a_row_sets_exactly_that_register(groups):
    """a sample: every row of rank >= 28 and every 40th of the others, as a 16-mer where that is its own canonical form, else as a 32-mer
    (leading As: only the low 32 bits are hashed)"""
    done = 0
    for g in groups:
        low = g["x"] == "low"
        for i, w in enumerate(g["w"]):
            bucket, lzm1, sig = O.hmh_rank(w, g["seed"], low)
            if lzm1 < 28 and i % 40:
                continue
            km, k = _spell(w, 16), 16
            if int(O.record_kmers(km, 16)[0]) != w:
                km, k = b"A" * 16 + km, 32
                if int(O.record_kmers(km, 32)[0]) & 0xFFFFFFFF != w:
                    continue
            seq = np.frombuffer(km, np.uint8)
            img = O.sketch_genomes(O.HMH, k, 0, g["seed"], seq, np.array([0, k], np.uint64), np.array([0, 1], np.uint64), hmh_x_is_low=int(low))
            regs = img[0].view("<u2")
            assert np.flatnonzero(regs).tolist() == [bucket] and int(regs[bucket]) == ((lzm1 + 1) << 10) | sig, (g["seed"], g["x"], hex(w))
            done += 1
    assert done > 250


def test_the_groups_the_gpu_tests_rely_on_exist(groups):
    for x in ("high", "low"):
        cap = 16 if x == "high" else 14
        rows = {}                                              # (seed, bucket) -> [(lzm1, sig)]
        levels = set()
        for g in groups:
            if g["x"] != x:
                continue
            for w in g["w"]:
                b, z, s = O.hmh_rank(w, g["seed"], x == "low")
                rows.setdefault((g["seed"], b), set()).add((z, s))
                if g["seed"] == 42:
                    levels.add(z)
        assert any(z >= 32 for v in rows.values() for z, _ in v), x                                  # a register >= 0x8000 with room to spare
        beyond = [sorted(r for r in v if r[0] > cap) for v in rows.values()]
        assert any(len({z for z, _ in v}) >= 2 for v in beyond), x                                    # one bucket, two ranks beyond the cap
        assert any(a[0] == b[0] and a[1] != b[1] for v in beyond for a, b in zip(v, v[1:])), x       # one bucket, one rank, two signatures
        assert levels >= set(range(13, 20)), (x, sorted(levels))
