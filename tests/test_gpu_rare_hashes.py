"""k-mers whose hash has 32 and more leading zeros above / below the bucket bits: one in 2^32 and rarer, i.e. never met by random test data,
yet each kernel family has code for exactly them —
  * the word loops take the rank from ONE 32-bit `v_ffbh` and re-run a word whose rank bits were all zero with the exact 64-bit form
    (sketch_rules.h `z_redo`);
  * UltraLogLog tables in LDS keep a 64-bit nlz bitmap per register as two words: nlz >= 32 lands in the second;
  * round 6: `bins_apply_kernel` (UltraLogLog p = 18 .. 22) keeps only the bitmap's LOW word in LDS; an entry with nlz >= 32 goes to the genome's
    fallback table in global memory and the registers are read out of both;
  * HyperLogLog ranks above 32 (and, above 53 - p, the `sum` corner with its replay: tests/test_gpu_hll_corner.py pins four found k-mers).
  * HyperMinHash (xxh3_128 of 4 bytes: not invertible, but all 2^32 inputs can be hashed — tests/golden/hmh_rare_ranks.json holds the rare ones, made
    by tests/golden/make_hmh_rare_ranks.py and checked without a GPU by tests/test_hmh_rare_ranks.py): threshold words beyond their cap of 16 / 14
    leading zeros (sketch_rules.h LdsThrRegsT: the rank moves into the low half), the fast forms' re-runs (REDO_BELOW, `z_redo`), the exact form's
    64-bit count with a zero top word, the x = low filter, and registers >= 0x8000 (lz >= 32) in every packed-u16 step after them.  The second half
    of this module builds genomes from those inputs; the deepest rank found in 14 seeds is 38 (lz = 39), 39 .. 50 stay uncovered.
xxh3_64 of 8 bytes is a bijection (tests/pyref.py `xxh3_64_8b_inverse`), so the test BUILDS such k-mers: choose the hash, invert it, keep the
value if it is a canonical k-mer (k = 32: every 64-bit value is a 32-mer; k = 31 / 28: the top bits must be zero too), spell it in ACGT.
Bit-exact against the oracle on every route, like every other parity test."""
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu

ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
SEED = 42


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.close()


def _spell(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)).encode()


def _kmer_with_hash(make_hash, k, rng, tries=20000):
    """A canonical k-mer (as ASCII) whose xxh3_64 is make_hash(rng): the free bits of the hash are redrawn until the preimage fits 2k bits and is
    its own canonical form."""
    for _ in range(tries):
        h = make_hash(rng)
        v = R.xxh3_64_8b_inverse(h, SEED)
        if k < 32 and v >> (2 * k):
            continue
        km = _spell(v, k)
        if O.record_kmers(km, k)[0] == v:
            assert O.xxh3_64_8b(v, SEED) == h
            return km, h
    raise AssertionError("no canonical preimage found")


# fewer free bits in the hash than this: the register is drawn too (a preimage is a canonical k-mer once in 2 / 2^3 / 2^9 draws)
FREE_BITS = {32: 5, 31: 8, 28: 14}


def _ull_hash(p, idx, nlz, k):
    """hash4j's split: idx = h >> (64 - p), nlz = leading zeros of the 64 - p bits below it."""
    q = 64 - p
    def make(rng):
        if nlz >= q:
            return rng.getrandbits(p) << q
        below = q - 1 - nlz                                    # bits under the leading one
        i = idx if below >= FREE_BITS[k] else rng.getrandbits(p)
        return (i << q) | (1 << below) | rng.getrandbits(below)
    return make


def _hll_hash(p, bucket, rho, k):
    """streaming_algorithms' split: bucket = h & (2^p - 1), rho = (64 - p) - bitlen(h >> p) + 1."""
    bl = 64 - p - rho + 1                                      # bit length of h >> p
    def make(rng):
        if bl == 0:
            return rng.getrandbits(p)
        b = bucket if bl - 1 >= FREE_BITS[k] else rng.getrandbits(p)
        return ((1 << (bl - 1)) | rng.getrandbits(bl - 1)) << p | b
    return make


def _genomes(kms, rng):
    """The built k-mers as records of their own between random records (no neighbours), inline in one long record (neighbouring k-mers overlap
    them), and in a genome of several work items."""
    rnd = O.synth_genome(rng.randrange(1 << 20), 2_600_000).tobytes()
    a, at = [], 0
    for km in kms:
        a += [rnd[at:at + 3000], km]; at += 3000
    inline = b"".join(rnd[100_000 + 5000 * i:100_000 + 5000 * (i + 1)] + km for i, km in enumerate(kms))
    big = rnd[200_000:1_400_000] + kms[0] + b"N" + kms[-1] + rnd[1_400_000:2_600_000]
    return [a, [inline], [big], [kms[len(kms) // 2]]]


@pytest.mark.parametrize("k", [32, 31, 28])
@pytest.mark.parametrize("p", [10, 12, 14, 16, 17, 18, 20, 22, 23, 24])
def test_ultraloglog_kmers_with_32_and_more_leading_zeros(ctx, p, k):
    import lash_amd
    rng = random.Random(zlib.crc32(repr(("ull", p, k)).encode()))
    q = 64 - p
    top = (1 << p) - 1
    # (register, nlz): alone in their registers; 31 + 32 and 32 + 33 + 34 sharing one (the two bits below the top come from both words of the
    # bitmap); the first and the last register of the table and of a bin; the largest nlz there is.  (Where the hash has too few free bits
    # left the register is drawn, not chosen: _ull_hash.)
    plan = [(5, 32), (6, 33), (7, min(40, q - 1)), (top, q), (0, 35), (1 << (p - 1), q - 1), (top, 33),
            (9, 31), (9, 32), (11, 32), (11, 33), (11, 34), ((1 << 14) - 1 if p > 14 else 3, 36), (1 << 14 if p > 14 else 4, 32)]
    kms, held = [], {}
    for idx, nlz in plan:
        km, h = _kmer_with_hash(_ull_hash(p, idx & top, min(nlz, q), k), k, rng)
        kms.append(km)
        held.setdefault(h >> q, set()).add(min(nlz, q))
    gs = _genomes(kms, rng)
    seq, off, goff = lash_amd.records_to_arrays(gs)
    want = oracle_images(ALGO["ull"], k, p, seq, off, goff)
    hdr = want.shape[1] - (1 << p)
    # the oracle agrees on what these registers hold: 4 * (nlz + p - 1) of the rarest k-mer, and the bits of the two ranks below it
    for idx, zs in held.items():
        z = max(zs)
        assert int(want[0, hdr + idx]) == ((z + p - 1) << 2) | (2 if z - 1 in zs else 0) | (1 if z - 2 in zs else 0), (idx, zs)
    assert len(held) >= 8 and (k != 32 or any(len(zs) == 3 for zs in held.values()))
    got = ctx.sketch_batch("ull", k, p, SEED, seq, off, goff)
    assert np.array_equal(got, want), "ull p=%d k=%d: %d bytes differ" % (p, k, int((got != want).sum()))
    got = ctx.sketch_batch("ull", k, p, SEED, seq, off, goff, flags=lash_amd.F_NO_DIRECT)
    assert np.array_equal(got, want), "ull p=%d k=%d pack-first: %d bytes differ" % (p, k, int((got != want).sum()))


@pytest.mark.parametrize("p", [18, 20, 22, 23])
def test_more_rare_entries_in_one_bin_than_its_short_list_holds(ctx, p):
    """bins_apply_kernel keeps the entries with nlz >= 32 of one (genome, bin) in a list of 62 beside its table; the 63rd and later go to the
    genome's fallback table in global memory (and the workgroup then pays an agent-scope fence).  Hashed input never gets there; 150 built k-mers
    in one quarter of the table's first 2^16 registers (one bin, whichever size bins have) do — some sharing a register with each other and with the list's entries."""
    import lash_amd
    k = 32
    rng = random.Random(p)
    q = 64 - p
    kms, held = [], {}
    for i in range(150):
        idx = (3 << 14) | rng.choice((rng.randrange(1 << 14), 7, 8, (1 << 14) - 1))       # bin 3 of 2^14 registers = the upper half of bin 1 of 2^15
        nlz = rng.choice((31, 32, 33, 34, 35))
        km, h = _kmer_with_hash(_ull_hash(p, idx, nlz, k), k, rng)
        assert h >> q == idx
        kms.append(km)
        held.setdefault(idx, set()).add(nlz)
    rnd = O.synth_genome(4242 + p, 900_000).tobytes()
    gs = [[rnd[:400_000]] + kms + [rnd[400_000:]], [b"".join(kms)], [rnd[:50_000]]]
    seq, off, goff = lash_amd.records_to_arrays(gs)
    want = oracle_images(ALGO["ull"], k, p, seq, off, goff)
    hdr = want.shape[1] - (1 << p)
    for idx, zs in held.items():
        z = max(zs)
        assert int(want[0, hdr + idx]) == ((z + p - 1) << 2) | (2 if z - 1 in zs else 0) | (1 if z - 2 in zs else 0), (idx, zs)
    for flags in (0, lash_amd.F_NO_DIRECT):
        got = ctx.sketch_batch("ull", k, p, SEED, seq, off, goff, flags=flags)
        assert np.array_equal(got, want), "ull p=%d flags=%d: %d bytes differ" % (p, flags, int((got != want).sum()))
    # ... and the fallback table was left empty: the next call on the same context (same buffers) sees none of it
    seq2, off2, goff2 = lash_amd.records_to_arrays([[rnd[:300_000]], [rnd[300_000:700_000]]])
    assert np.array_equal(ctx.sketch_batch("ull", k, p, SEED, seq2, off2, goff2), oracle_images(ALGO["ull"], k, p, seq2, off2, goff2))


@pytest.mark.parametrize("k", [32, 28])
@pytest.mark.parametrize("p", [10, 14, 16])
def test_hyperloglog_ranks_above_32(ctx, p, k):
    import lash_amd
    rng = random.Random(zlib.crc32(repr(("hll", p, k)).encode()))
    top = (1 << p) - 1
    exact = 53 - p                                             # up to here `sum` is order-free (above: the corner and its replay)
    plan = [(5, 32), (6, 33), (7, 34), (0, min(37, exact)), (top, exact), (9, 31), (9, 33), (12, exact + 1), (13, 65 - p)]
    kms, held = [], {}
    for b, rho in plan:
        km, h = _kmer_with_hash(_hll_hash(p, b, rho, k), k, rng)
        kms.append(km)
        held[h & top] = max(held.get(h & top, 0), rho)
    gs = _genomes(kms, rng)
    seq, off, goff = lash_amd.records_to_arrays(gs)
    want = oracle_images(ALGO["hll"], k, p, seq, off, goff)
    hdr = want.shape[1] - (1 << p)
    for b, rho in held.items():
        assert int(want[0, hdr + b]) == rho, (b, rho)
    assert len(held) >= 7 and max(held.values()) == 65 - p
    got = ctx.sketch_batch("hll", k, p, SEED, seq, off, goff)                     # (the host entry replays `sum` where a rank exceeds 53 - p)
    assert np.array_equal(got, want), "hll p=%d k=%d: %d bytes differ" % (p, k, int((got != want).sum()))
    got = ctx.sketch_batch("hll", k, p, SEED, seq, off, goff, flags=lash_amd.F_NO_DIRECT)
    assert np.array_equal(got, want), "hll p=%d k=%d pack-first: %d bytes differ" % (p, k, int((got != want).sum()))


def oracle_images(algo, k, p, seq, off, goff):
    return O.sketch_genomes(algo, k, p, SEED, seq, off, goff, threads=8)


# ------------------------------------------------------------------------------------------------------------
# HyperMinHash: ranks beyond the threshold words' cap, and registers with bit 15 set.  The inputs come from tests/golden/hmh_rare_ranks.json
# (seed 42: every input of rank lz - 1 >= 20, a ladder of single inputs and of same-bucket, same-rank pairs at 12 .. 19; seeds 0, 1, 11:
# every input of rank >= 24, up to 38).  Ranks 39 .. 50 were found in none of 14 seeds and are not covered.
# ------------------------------------------------------------------------------------------------------------
class Row:
    """one fixture input as a k-mer: w, its bucket / lz - 1 / signature under (seed, variant), the register it sets, its spelling"""
    def __init__(self, w, seed, low, km):
        self.w, self.km = w, km
        self.bucket, self.lzm1, self.sig = O.hmh_rank(w, seed, low)
        self.reg = ((self.lzm1 + 1) << 10) | self.sig


_LSB = R.Lay(kmer="lsb")


def _hmh_kmer(w, k, lsb=False):
    """w spelled as a k-mer (k < 16: only w < 4^k; k > 16: As in the bits above the hashed 32), or None if the iterator's first (canonical,
    masked) k-mer of that record is not w — checked with the oracle, under kmer=lsb with the Python restatement (the oracle's entry takes no layout)"""
    if k < 16 and w >> (2 * k):
        return None
    n = min(k, 16)
    if lsb:
        km = "".join("ACGT"[(w >> (2 * i)) & 3] for i in range(n)) + "A" * (k - n)
        first = R.canonical_kmers(km, k, _LSB)[0]
    else:
        km = "A" * (k - n) + _spell(w, n).decode()
        first = int(O.record_kmers(km.encode(), k)[0])
    return km.encode() if first & 0xFFFFFFFF == w else None


_GROUPS = []


def _hmh_pick(seed, low, k, lsb):
    """What a test's genomes are built from: `ladder` up to two k-mers per rank 12 .. 19 (both caps, both REDO_BELOW values, the 18-bit fast
    form's last rank and the first beyond it), `deep` the eight deepest, `diff` same-bucket pairs of two different ranks beyond the cap (deeper
    first), `eq` same-bucket pairs of one rank and two signatures (larger signature first) on the ladder and beyond the cap."""
    if not _GROUPS:
        _GROUPS.extend(O.hmh_rare_ranks())
    cap = 14 if low else 16
    rows, eq = {}, []
    for g in _GROUPS:
        if g["seed"] != seed or (g["x"] == "low") != low:
            continue
        for w in g["w"]:
            km = _hmh_kmer(w, k, lsb)
            if km is not None:
                rows[w] = Row(w, seed, low, km)
        if g["kind"] == "pair":
            for a, b in zip(g["w"][::2], g["w"][1::2]):
                if a in rows and b in rows and sum(1 for e in eq if e[0].lzm1 == g["lzm1"]) < 1:
                    eq.append(tuple(sorted((rows[a], rows[b]), key=lambda r: -r.sig)))
    rows = sorted(rows.values(), key=lambda r: r.w)
    ladder = [r for z in range(12, 20) for r in [r for r in rows if r.lzm1 == z][:2]]
    deep = sorted(rows, key=lambda r: (-r.lzm1, r.w))[:8]
    by_bucket = {}
    for r in rows:
        if r.lzm1 > cap:
            by_bucket.setdefault(r.bucket, []).append(r)
    diff, eq_beyond = [], []
    for b in sorted(by_bucket):
        v = sorted(by_bucket[b], key=lambda r: (-r.reg, r.w))
        for x, y in zip(v, v[1:]):
            if x.lzm1 != y.lzm1 and len(diff) < 3:
                diff.append((x, y))
            if x.lzm1 == y.lzm1 and x.sig != y.sig and len(eq_beyond) < 2:
                eq_beyond.append((x, y))
    return dict(ladder=ladder, deep=deep, diff=diff, eq=eq + eq_beyond, cap=cap)


def _hmh_genomes(pick, k, rng):
    """-> [(records, [Row, ...])]: the shapes of _genomes above, and the orders inside one record that the deferring launches' filter could
    tell apart (it reads the bucket's word back before the k-mer's own update: what came first decides who passes)."""
    rnd = O.synth_genome(rng.randrange(1 << 20), 1_500_000).tobytes()
    ladder, deep, diff, eq = pick["ladder"], pick["deep"], pick["diff"], pick["eq"]
    singles = ladder + deep
    gs = []
    gs.append(([x for i, r in enumerate(singles) for x in (rnd[3000 * i:3000 * (i + 1)], r.km)], singles))
    inl = ladder[1::2] + deep[:4] + [r for pr in diff + eq for r in pr]
    gs.append(([b"".join(rnd[100_000 + 5000 * i:100_000 + 5000 * (i + 1)] + r.km for i, r in enumerate(inl))], inl))
    head, mid, tail = deep[:3] + ladder[::3], [deep[0], ladder[-1] if ladder else deep[-1]], deep[1]
    big = (b"".join(r.km for r in head) + rnd[200_000:850_000] + mid[0].km + b"N" + mid[1].km + rnd[850_000:1_500_000 - 300]
           + tail.km + rnd[7:27])                                    # ~1.3 Mbp: work items past the deferring threshold, several slices
    gs.append(([big], head + mid + [tail]))
    gs.append(([deep[0].km], [deep[0]]))
    some = [deep[0], deep[-1]] + ladder[5::2]                                                        # (ranks 14 .. 19)
    for i, r in enumerate(some):
        gs.append(([r.km + rnd[300_000 + 20_000 * i:320_000 + 20_000 * i]], [r]))                    # (a) the rare k-mer first
        gs.append(([rnd[320_000 + 20_000 * i:340_000 + 20_000 * i] + r.km], [r]))                    # (b) ... and last
    for i, (x, y) in enumerate(diff + eq):                                                           # (c), (d): both orders, near and far
        gap = rnd[500_000 + 10_000 * i:500_000 + 10_000 * i + (40, 9000)[i & 1]]
        gs.append(([x.km + gap + y.km + rnd[600_000:602_000]], [x, y]))
        gs.append(([y.km + gap + x.km + rnd[600_000:602_000]], [x, y]))
    for r in (deep[0], (ladder or deep)[-1]):                                                        # (e) the same k-mer twice
        gs.append(([r.km + rnd[700_000:700_100] + r.km], [r]))
    return gs


def _hmh_check_oracle(gs, want, hdr, be=False):
    """the oracle holds what the fixture says (the `held` idiom above): at a built bucket the register of the winning built k-mer — or, for ranks
    below 20 only, a larger one (a random k-mer of the genome may beat those: one in 2^13 and rarer per k-mer of the same bucket)"""
    regs = np.ascontiguousarray(want[:, hdr:]).view(">u2" if be else "<u2")
    for g, (_, built) in enumerate(gs):
        best = {}
        for r in built:
            best[r.bucket] = max(best.get(r.bucket, 0), r.reg)
        for b, reg in best.items():
            have = int(regs[g, b])
            assert have == reg or (have > reg and reg < (21 << 10)), (g, b, hex(have), hex(reg))
    return regs


def _hmh_routes():
    import lash_amd
    return [("default (small genomes through the persistent kernel)", 0, {}),
            ("sliced direct kernel", lash_amd.F_NO_SOLE, {}),
            ("sliced direct kernel, every HyperMinHash launch deferring", lash_amd.F_NO_SOLE, {"LASH_DEFER_MIN": "0"}),
            ("the same, lane stacks of the smallest depth named explicitly", lash_amd.F_NO_SOLE, {"LASH_DEFER_MIN": "0", "LASH_SIGQ_DEPTH": "7"}),
            ("stream kernel", lash_amd.F_STREAM_ONLY, {}),
            ("stream kernel, deferring", lash_amd.F_STREAM_ONLY, {"LASH_DEFER_MIN": "0"}),
            ("pack first", lash_amd.F_NO_DIRECT | lash_amd.F_NO_SOLE, {}),
            ("pack first, persistent kernel on packed words", lash_amd.F_NO_DIRECT, {})]


# (seed, x, k, layout): x = "low" alone is the flag F_HMH_X_LOW, with a layout it is the layout's hmh_x=low
HMH_CASES = [(42, "high", 16, None), (42, "high", 13, None), (42, "high", 32, None), (42, "high", 21, None),
             (42, "low", 16, None), (42, "low", 13, None), (42, "low", 32, "hmh_x=low"), (42, "low", 21, "hmh_x=low,hmh_reg=be,hmh_hdr=l"),
             (42, "high", 16, "kmer=lsb"), (42, "low", 21, "kmer=lsb,hmh_x=low"),
             (0, "high", 21, None), (0, "low", 32, None), (0, "low", 16, "hmh_x=low"), (1, "high", 32, None), (11, "low", 21, None)]
BIT15 = {(0, "high"), (0, "low"), (1, "high"), (11, "low")}          # where an input of rank >= 32 exists (the census in the fixture's maker)


@pytest.mark.parametrize("seed,x,k,spec", HMH_CASES)
def test_hyperminhash_rare_ranks_through_every_route(ctx, seed, x, k, spec, monkeypatch):
    """Every route the library can take for a genome (the list of tests/test_gpu_layout.py test_rule_alternatives_through_every_route), both
    variants, on genomes built from inputs of rank 12 .. 38.  The lanes' stacks of the deferring launches have depth LASH_SIGQ_DEPTH, whose
    default is also its smallest value (7): one route names it."""
    import lash_amd
    low, lsb = x == "low", bool(spec) and "kmer=lsb" in spec
    lay = O.parse_layout(spec) if spec else None
    rng = random.Random(zlib.crc32(repr(("hmh", seed, x, k, spec)).encode()))
    pick = _hmh_pick(seed, low, k, lsb)
    # what the fixture must provide for this case to test anything: all ranks 13 .. 19 at seed 42 (k = 13 spells one input in 64: both
    # caps' neighbours 14 .. 17 at least), pairs wherever whole 16-mers are spelled, a register >= 0x8000 where the census found one
    levels = {r.lzm1 for r in pick["ladder"]}
    if seed == 42:
        assert levels >= (set(range(14, 18)) if k < 16 else set(range(13, 20))), sorted(levels)
        assert pick["deep"][0].lzm1 >= (24 if k < 16 else 29)
        if k >= 16:
            assert pick["diff"] and any(a.lzm1 > pick["cap"] for a, _ in pick["eq"]) and any(a.lzm1 <= pick["cap"] for a, _ in pick["eq"])
    if seed != 42:
        assert (seed, x) in BIT15 and pick["deep"][0].lzm1 >= 32
    gs = _hmh_genomes(pick, k, rng)
    assert all(len(built) <= 40 for _, built in gs)
    seq, off, goff = lash_amd.records_to_arrays([recs for recs, _ in gs])
    flag = lash_amd.F_HMH_X_LOW if low and not (spec and "hmh_x=low" in spec) else 0
    want = O.sketch_genomes(O.HMH, k, 0, seed, seq, off, goff, threads=8, hmh_x_is_low=int(bool(flag)), layout=lay)
    hdr = want.shape[1] - 32768
    regs = _hmh_check_oracle(gs, want, hdr, be=bool(lay and lay.hmh_reg_be))
    if seed != 42:
        assert int(regs.max()) >= 0x8000
    ctx.set_layout(spec)
    try:
        for name, flags, envs in _hmh_routes():
            with monkeypatch.context() as m:
                for key, v in envs.items():
                    m.setenv(key, v)
                ctx.enable_timing(True)
                got = ctx.sketch_batch("hmh", k, 0, seed, seq, off, goff, flags=flags | flag)
                tm = ctx.timing()
                ctx.enable_timing(False)
            if not np.array_equal(got, want):
                gr = np.ascontiguousarray(got[:, hdr:]).view(regs.dtype)
                bad = [(int(g), int(b), hex(int(gr[g, b])), hex(int(regs[g, b]))) for g, b in zip(*np.nonzero(gr != regs))][:8]
                raise AssertionError("hmh seed=%d x=%s k=%d %s, %s: (genome, bucket, got, want) %s" % (seed, x, k, spec, name, bad))
            if envs.get("LASH_DEFER_MIN") == "0" and not (flags & lash_amd.F_STREAM_ONLY):
                assert tm["defer_launches"] >= 1, (name, tm)
    finally:
        ctx.set_layout(None)


def _numpy_pair_counts(ref, qry):
    """tests/test_gpu_dist.py test_hmh_pair_counts_match_numpy's count"""
    c = ((ref[:, None, :] == qry[None, :, :]) & (ref[:, None, :] != 0)).sum(axis=2)
    n = ((ref[:, None, :] != 0) | (qry[None, :, :] != 0)).sum(axis=2)
    return c, n


@pytest.mark.parametrize("seed,x", [(0, "high"), (11, "low")])
def test_hyperminhash_registers_with_bit_15_set_downstream_of_the_image(ctx, seed, x, tmp_path):
    """lz >= 32 sets bit 15 of the u16 register: everything that merges, compares or counts registers after the sketch kernels — the packed-u16
    maximum of LASH_F_ACCUMULATE and lash_merge_images[_device], bit plane 15 and the u16-pair kernel of the pair counts, the histogram behind a
    resident set's cardinalities — against the oracle's merge, numpy's counts and the Python restatement of hyperminhash's cardinality."""
    import torch
    import lash_amd
    low, k = x == "low", 21
    flag = lash_amd.F_HMH_X_LOW if low else 0
    deep = _hmh_pick(seed, low, k, False)["deep"]
    top = [r for r in deep if r.lzm1 >= 31]
    assert len(top) >= 3
    rnd = O.synth_genome(900 + seed, 400_000).tobytes()
    rare, plain = lash_amd.records_to_arrays([[rnd[:3000]] + [r.km for r in deep]]), lash_amd.records_to_arrays([[rnd[3000:]]])
    X = O.sketch_genomes(O.HMH, k, 0, seed, *rare, hmh_x_is_low=int(low))
    Y = O.sketch_genomes(O.HMH, k, 0, seed, *plain, hmh_x_is_low=int(low))
    xr, yr = X[0].view("<u2"), Y[0].view("<u2")
    for r in top:                                               # X holds the deep registers, Y something shallower in the same buckets
        assert int(xr[r.bucket]) == r.reg >= 0x8000 and 0 < int(yr[r.bucket]) < 0x8000
    XY = O.merge_images(O.HMH, 0, X[0], Y[0])[None]
    assert all(int(XY[0].view("<u2")[r.bucket]) == r.reg for r in top)
    for flags in (0, lash_amd.F_NO_SOLE, lash_amd.F_NO_DIRECT, lash_amd.F_NO_DIRECT | lash_amd.F_NO_SOLE):
        got = ctx.sketch_batch("hmh", k, 0, seed, *plain, flags=flags | flag | lash_amd.F_ACCUMULATE, out=X.copy())
        assert np.array_equal(got, XY), ("a shallower genome into an image that holds the deeper registers", flags, _hmh_diff(got, XY))
        got = ctx.sketch_batch("hmh", k, 0, seed, *rare, flags=flags | flag | lash_amd.F_ACCUMULATE, out=Y.copy())
        assert np.array_equal(got, XY), ("the deeper genome into an image that holds shallower registers", flags, _hmh_diff(got, XY))
    # unions of images: real ones, and made-up ones whose registers differ in bit 15 only / agree in bit 15 and differ below it
    rng = np.random.default_rng(seed)
    A = np.stack([xr, yr, xr, XY[0].view("<u2"), rng.integers(0, 65536, 16384).astype(np.uint16), np.full(16384, 0x8000, np.uint16)])
    B = np.stack([yr, xr, xr ^ np.where(np.arange(16384) % 3 == 0, 0x8000, 0).astype(np.uint16), xr,
                  rng.integers(0, 65536, 16384).astype(np.uint16), np.full(16384, 0x7FFF, np.uint16)])
    A8, B8 = A.view(np.uint8).reshape(len(A), -1), B.view(np.uint8).reshape(len(B), -1)
    want = np.stack([O.merge_images(O.HMH, 0, A8[i], B8[i]) for i in range(len(A))])
    assert np.array_equal(want.view("<u2"), np.maximum(A, B))
    assert np.array_equal(ctx.merge_images("hmh", 0, A8.copy(), B8), want)
    d_a, d_b = torch.from_numpy(A8.copy()).cuda(), torch.from_numpy(B8.copy()).cuda()
    ctx.merge_images_device("hmh", 0, d_a, d_b, len(A))
    ctx.synchronize()
    assert np.array_equal(d_a.cpu().numpy(), want)
    # pair counts: X against itself (identical, bit 15 set), against a copy with bit 15 of ONE register cleared, and the rest
    one = xr.copy()
    one[top[0].bucket] ^= 0x8000
    S = np.stack([xr, one, xr.copy(), yr, XY[0].view("<u2"), B[2]])
    S8 = S.view(np.uint8).reshape(len(S), -1)
    wc, wn = _numpy_pair_counts(S, S)
    filled = int((xr != 0).sum())
    assert wc[0, 2] == filled and wc[0, 1] == filled - 1 and wn[0, 1] == filled
    c, n = ctx.hmh_pair_counts(S8, S8)
    assert np.array_equal(c, wc) and np.array_equal(n, wn)
    c, n = ctx.hmh_pair_counts(S8[:2], S8[1:])                                     # (two different sets: row and column planes built apart)
    assert np.array_equal(c, wc[:2, 1:]) and np.array_equal(n, wn[:2, 1:])
    # ... and through the u16-pair kernel (LASH_HMH_PAIRS_WORDS is read once per process: a child)
    np.save(tmp_path / "s.npy", S8)
    code = ("import numpy as np, lash_amd, sys\n"
            "s = np.load(sys.argv[1])\n"
            "c, n = lash_amd.Context(0).hmh_pair_counts(s, s)\n"
            "sys.stdout.buffer.write(c.tobytes() + n.tobytes())\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "s.npy")], capture_output=True,
                       env=dict(os.environ, PYTHONPATH=root, LASH_HMH_PAIRS_WORDS="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == wc.astype(np.uint32).tobytes() + wn.astype(np.uint32).tobytes()
    # a resident set's cardinalities (register histograms made on the GPU): exactly the restatement's, as tests/test_gpu_sketch_set.py
    # test_set_cardinalities_equal_the_per_image_entries asks of the per-image entries (no lz above 39: every partial sum is exact)
    st = ctx.sketch_set("hmh", 0, S8)
    got = st.cardinalities()
    st.free()
    want = np.array([R.hmh_cardinality(S8[i].tobytes()) for i in range(len(S))])
    assert np.array_equal(got, want), (got, want)


def _hmh_diff(got, want):
    g, w = got.view("<u2"), want.view("<u2")
    return [(int(i), int(b), hex(int(g[i, b])), hex(int(w[i, b]))) for i, b in zip(*np.nonzero(g != w))][:8]
