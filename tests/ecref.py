"""High-precision reference of hyperminhash's expected_collisions(n, m), for tests only (no GPU, no lash_amd, nothing shared with
the kernels of dist_kernels.hip or with pyref's loop).

The published rule (axiomhq/hyperminhash, p = 14, q = 6, r = 10): with n >= m,
  n > 2^74                     u64::MAX
  n > 2^19                     0.1699... * 2^(p-r) * (4 n / m) / ((1 + n) / m)^2 + 0.5
  otherwise                    (x p + 0.5) / p,  x = sum over the 64 x 1024 cells of
                               [(1-b2)^n - (1-b1)^n] [(1-b2)^m - (1-b1)^m],
                               rows i = 1..63: b1 = (1024 + j) / 2^(24+i), b2 = (1025 + j) / 2^(24+i); row 64: b1 = j / 2^87, b2 = (j + 1) / 2^87.
A cell is the interval (b1, b2] of the minimum hash: (1-b2)^n - (1-b1)^n = -P(the minimum of n hashes falls into it).

Here each cell factor is evaluated in numpy.longdouble (64-bit mantissa) without the cancellation of the difference of two powers:
  (1-b2)^n - (1-b1)^n = exp(n log1p(-b1)) * expm1(n (log1p(-b2) - log1p(-b1))),
  log1p(-b2) - log1p(-b1) = log1p(-(b2 - b1) / (1 - b1))           (b2 - b1 = 1 / den exactly)
and the 65 536 products are summed pairwise in long double (numpy's reduction along a contiguous axis); f64 BLAS is of no use
as a reference, its worst-case summation error 65536 * 2^-53 * x is what the tests bound.  tests/test_ec_reference.py checks
the vectors against mpmath at 50 digits.

The pool: made-up HyperMinHash images, prefixes of one master register array (image k = its first K[k] registers, the rest
zero), whose LogLog-beta cardinalities spread over [100, 2^19] at least 2 % apart, and three large images (> 2^19).  Tests give
sketch sets their cardinalities through these images, and whole-matrix entries through the numbers.
"""
import math

import numpy as np

LD = np.longdouble
CELLS = 65536
E_POW = 16                                   # allowance for ocml's f64 pow, in ulp (nobody here has measured it; glibc's is below 1)
T0 = (4 * E_POW + 2) * 2.0 ** -53


def tol(x):
    """T(x): |GPU ec - reference ec| allowed at cell sum x.  Each pow result lies in [0, 1] with absolute error <= E 2^-53, a cell
    value carries <= 2 E 2^-53, both vectors' absolute sums are <= 1: 4 E 2^-53 on x; the MFMA accumulation (16 384 sequential
    4-term steps) <= 2^-39 x; the two roundings of (x 14 + 0.5) / 14: 2 * 2^-53."""
    return T0 + 2.0 ** -39 * np.asarray(x, dtype=np.float64)


def cell_bounds():
    """(b1, b2, 1 / den) of the 65 536 cells in long double, all exact: cell index = (i - 1) * 1024 + (j - 1)"""
    i = np.repeat(np.arange(1, 65), 1024)
    j = np.tile(np.arange(1, 1025), 64).astype(LD)
    last = i == 64
    inv = np.ldexp(LD(1), -np.where(last, 87, 24 + i))
    num = np.where(last, j, j + LD(1024))
    return num * inv, (num + LD(1)) * inv, inv


_B = None


def vector(n):
    """the 65 536 cell factors (1-b2)^n - (1-b1)^n (all <= 0) of cardinality n, long double"""
    global _B
    if _B is None:
        b1, b2, inv = cell_bounds()
        _B = (np.log1p(-b1), np.log1p(-inv / (LD(1) - b1)))
    l1, dl = _B
    n = LD(n)
    return np.exp(n * l1) * np.expm1(n * dl)


def closed_form(n, m):
    """the O(1) regimes in plain f64 (None below them)"""
    if n < m:
        n, m = m, n
    if n > 2.0 ** 74:
        return 1.8446744073709552e19
    if n > 2.0 ** 19:
        t = (1.0 + n) / m
        d = (4.0 * n / m) / (t * t)
        return 0.169919487159739093975315012348 * 16.0 * d + 0.5
    return None


def ec_from_x(x):
    """(x 14 + 0.5) / 14 in long double, rounded once"""
    return np.asarray((np.asarray(x, dtype=LD) * LD(14) + LD(0.5)) / LD(14), dtype=np.float64)


def ec(n, m):
    """expected_collisions(n, m) of two cardinalities, every regime, f64"""
    c = closed_form(float(n), float(m))
    if c is not None:
        return c
    return float(ec_from_x((vector(n) * vector(m)).sum()))


class Table:
    """x(a, b) and ec(a, b) of every pair of a pool of small cardinalities (<= 2^19), symmetric; long double x, f64 ec"""

    def __init__(self, cards):
        self.cards = np.asarray(cards, dtype=np.float64)
        assert self.cards.ndim == 1 and (self.cards <= 2.0 ** 19).all() and (self.cards > 0).all()
        n = len(self.cards)
        self.V = np.stack([vector(c) for c in self.cards])
        self.x = np.zeros((n, n), dtype=LD)
        for a in range(n):                                         # the upper triangle, one row of products at a time
            row = (self.V[a:] * self.V[a]).sum(axis=1)
            self.x[a, a:] = row
            self.x[a:, a] = row
        self.ec = ec_from_x(self.x)
        self.x64 = self.x.astype(np.float64)

    def lookup(self, ri, ci):
        """(ec, x) [len(ri), len(ci)] in f64 for pool indices of rows and columns"""
        ri, ci = np.asarray(ri), np.asarray(ci)
        return self.ec[np.ix_(ri, ci)], self.x64[np.ix_(ri, ci)]


def expected(table, ri, ci, rcard, ccard):
    """The whole [len(rcard), len(ccard)] matrix a GPU entry should return: small x small cells from the table (ri / ci: pool
    index, anything where the member is large), every other cell the closed form of its two cardinalities.
    -> (ec, tolerance): tolerance 0 where the closed form holds (those cells are the host's f64 expression: equality)."""
    rcard, ccard = np.asarray(rcard, np.float64), np.asarray(ccard, np.float64)
    rs, cs = rcard <= 2.0 ** 19, ccard <= 2.0 ** 19
    ec = np.zeros((len(rcard), len(ccard)))
    t = np.zeros_like(ec)
    e, x = table.lookup(np.where(rs, ri, 0), np.where(cs, ci, 0))
    small = rs[:, None] & cs[None, :]
    ec[small] = e[small]
    t[small] = tol(x[small])
    for i in np.flatnonzero(~rs):
        for j in range(len(ccard)):
            ec[i, j] = closed_form(rcard[i], ccard[j])
    for j in np.flatnonzero(~cs):
        for i in np.flatnonzero(rs):
            ec[i, j] = closed_form(rcard[i], ccard[j])
    return ec, t, small


def worst_in_ulp(got, want, t, small):
    """asserts |got - want| <= t on every cell (t = 0: equality) and returns the worst small-cell error in ulp(ec) = 2^-57"""
    err = np.abs(got - want)
    bad = ~(err <= t)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist(), got[bad][:4], want[bad][:4], t[bad][:4])
    return float(err[small].max() / 2.0 ** -57) if small.any() else 0.0


# ---- the pool: made-up images -------------------------------------------------------------------------------------------------
def _mix(i):
    """splitmix64 of the integers i (uint64 arithmetic wraps)"""
    with np.errstate(over="ignore"):
        z = (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def master_registers(lz_base=4, salt=0):
    """16 384 u16 registers (lz << 10 | signature), none zero: lz = lz_base + 1 + (trailing zeros of a hash, at most 12): half of
    them lz_base + 1, a quarter lz_base + 2, ... as a filled sketch has them (lz_base = 4: LogLog-beta says 564 573)"""
    h = _mix(np.arange(16384, dtype=np.uint64) + np.uint64(salt) * np.uint64(1 << 20))
    g = np.zeros(16384, np.int64)
    low = h & np.uint64(0xFFF)
    for t in range(12):
        g += (low & np.uint64((1 << (t + 1)) - 1)) == 0
    sig = ((h >> np.uint64(20)) & np.uint64(1023)).astype(np.int64)
    return (((lz_base + 1 + g) << 10) | sig).astype(np.uint16)


# how many leading registers of the master array each pool image keeps: chosen once so that the cardinalities step by about 9 %
# from 100 up (tests/test_ec_reference.py asserts the range and the 2 % separation)
K = (
     100, 109, 120, 131, 143, 156, 171, 187, 204, 223, 244, 267, 292, 319, 348, 380,
     415, 453, 495, 540, 589, 643, 701, 764, 833, 907, 988, 1075, 1170, 1272, 1382, 1502,
     1630, 1768, 1917, 2076, 2246, 2429, 2623, 2830, 3050, 3284, 3531, 3791, 4065, 4352, 4653, 4966,
     5291, 5628, 5976, 6333, 6699, 7072, 7450, 7834, 8220, 8607, 8994, 9379, 9760, 10137, 10506, 10867,
     11219, 11561, 11892, 12210, 12515, 12807, 13085, 13350, 13601, 13837, 14060, 14269, 14466, 14649, 14820, 14979,
     15128, 15265, 15392, 15509, 15618, 15717, 15809, 15894, 15971, 16042, 16107, 16166, 16220, 16269, 16314, 16354,
)


def pool_images():
    """(images uint8 [len(K) + 3, 32768], number of small ones): the pool, then three large images that match nothing in it"""
    m = master_registers()
    out = np.zeros((len(K) + 3, 16384), np.uint16)
    for a, k in enumerate(K):
        out[a, :k] = m[:k]
    for b in range(3):
        out[len(K) + b] = master_registers(8 + b, salt=1 + b)
    return out.view(np.uint8).reshape(len(out), 32768), len(K)


_POOL = None


def pool():
    """(images, cardinalities f64 [len(K) + 3]) with the cardinalities by pyref's restatement of the crate's LogLog-beta (the
    library's are the same numbers bit for bit: tests/test_gpu_sketch_set.py, and every GPU user of the pool asserts it again)"""
    global _POOL
    if _POOL is None:
        import pyref as R
        imgs, _ = pool_images()
        _POOL = (imgs, np.array([R.hmh_cardinality(im.tobytes()) for im in imgs]))
    return _POOL


_TABLE = None


def pool_table():
    """the Table of the pool's small cardinalities, computed once per process (about 4 s)"""
    global _TABLE
    if _TABLE is None:
        _TABLE = Table(pool()[1][:len(K)])
    return _TABLE


# the fixed rules by which tests spread pool values over rows and columns: neighbours at every structural distance of the GEMM
# (lanes, MFMA blocks, waves, tiles) differ
ALIAS_D = (1, 2, 3, 4, 8, 12, 16, 32, 48, 64, 128, 256)


def row_rule(n, shift=0):
    """pool indices 7..95 by r mod 89 (89 is prime and divides no ALIAS_D)"""
    return (np.arange(n) + shift) % 89 + (len(K) - 89)


def col_rule(n, shift=0):
    """pool indices 0..82 by (5 c + 3) mod 83"""
    return (5 * (np.arange(n) + shift) + 3) % 83


def assert_alias_free(card):
    card = np.asarray(card)
    for d in ALIAS_D:
        if d < len(card):
            assert (card[:-d] != card[d:]).all(), d


# ---- the chunk test's set (tests/test_gpu_hmh_ec_tiles.py), and what its block must give -----------------------------------------
CHUNK_N = 4096 + 344                     # 4437 small members: one full chunk of query vectors and a short one of 341
CHUNK_LARGE = (5, 2000, 4200)
CHUNK_ROWS = (1990, 2020)                # 30 rows, the large member 2000 among them, rbase = 1989
K_MER = 16
# The set draws on every third pool value (32 of them, 29 % apart).  ec(n, m) peaks near n = m, so two different n can give one m
# nearly the same ec; with all 96 values 124 of the pool's pairs have such a neighbour within 100 of the DISTANCE's tolerances
# (f64's own noise in the distance, not T, sets that tolerance).  Among these 32 the nearest is 205 tolerances away.
CHUNK_POOL = tuple(range(1, 96, 3))


def _distance(c, n, ec, k=K_MER):
    """the Mash distance of hyperminhash's similarity, plain numpy f64 (c > ec > 0)"""
    s = (c - ec) / n
    return np.minimum(-np.log(2.0 * s / (1.0 + s)) / k, 1.0)


def _distance_tol(c, n, ec, x, k=K_MER):
    """How far two f64 evaluations of the distance may be apart when their ec differ by T(x):
      a = c - ec         differs by <= T + ulp(a): relative T / a + 2^-52
      s = a / n          one more rounding on each side: + 2^-52
      f = 2 s / (1 + s)  1 + s moves by less than s does, one rounding each for the sum and the quotient: relative 2 T / a + 2^-49 in all
      L = -ln f          moves by f's relative change; glibc's log is within 1 ulp on both sides: + 2 ulp(L)
      d = L / k          + ulp(d)
    The T term is T / (k a (1 + s)) to first order; it is below f64's own noise here, which is why the separation is asserted too."""
    a = c - ec
    s = a / n
    L = np.abs(np.log(2.0 * s / (1.0 + s)))
    return (2.0 * tol(x) / a + 2.0 ** -49 + 2.0 * np.spacing(L)) / k + np.spacing(L / k)


def chunk_members():
    order = np.array(CHUNK_POOL, np.int64)[np.arange(CHUNK_N) % 31]        # (31 is prime and divides no ALIAS_D)
    for b, at in enumerate(CHUNK_LARGE):
        order[at] = len(K) + b
    return order


def chunk_block_reference(table):
    """what the 30 x 4440 block must give, from the reference and the images alone: (ec, T, small, c, n, distance, its tolerance)"""
    order = chunk_members()
    cards = pool()[1][order]
    r0, r1 = CHUNK_ROWS
    want, t, small = expected(table, order[r0:r1], order, cards[r0:r1], cards)
    keep = np.array(list(K) + [0, 0, 0])[order]                  # registers of the master array a member keeps; large ones match nothing
    c = np.where(small, np.minimum(keep[r0:r1, None], keep[None, :]), 0).astype(np.float64)
    filled = np.where(order < len(K), keep, 16384)
    n = np.maximum(filled[r0:r1, None], filled[None, :]).astype(np.float64)
    x = np.where(small, want - 1 / 28, 0.0)
    d = np.ones_like(want)
    dt = np.zeros_like(want)
    d[small] = _distance(c[small], n[small], want[small])
    dt[small] = _distance_tol(c[small], n[small], want[small], x[small])
    return order, want, t, small, c, n, d, dt
