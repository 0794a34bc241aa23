"""UltraLogLog: a plain high-precision reference of the dist side's arithmetic and the makers of its test inputs.  No GPU, no
lash_amd: numpy + mpmath (>= 50 digits) only, so that the product's estimators (ull_estimators.h, on the host and in the
gfx950 pair kernels) are compared with something that shares no code with them.

The model (O. Ertl, "UltraLogLog", VLDB 2024): a register sees update value k >= 1 with probability 1 - exp(-lambda P(k)),
lambda = n / m, P(k) = 2^-k for k < K = 65 - p and P(K) = 2^-(K-1) (the cap: every ideal value >= K lands on K).  Its byte
r = 4 (u + p - 2) + 2 [u-1 seen] + [u-2 seen] holds the largest value u and two bits; values below 1 do not exist, so the
bytes 0, 4p-4, 4p, 4p+2 ("small range") leave bits of the IDEAL register (virtual values 0, -1, ...) unknown, and r >= 252
("saturated", u = K) leaves the ideal largest value K + j unknown.

  fgra_ref   every register contributes E[eta_bits 2^(-tau u') | what was observed] of its ideal register, the expectation
             taken under the Poisson model at the rate z the product estimates from the counts (small_range_z /
             large_range_z, restated here as the same quadratics: their CHOICE is checked by the sampler tests, not here);
             all series summed to convergence.
  ml_ref     the exact likelihood equation  A = sum_e B_e 2^-e / (exp(lambda 2^-e) - 1)  built register by register and
             solved by Newton's method from a bracketed double start, to 40+ digits, then the first-order bias correction.
  merge_ref  pack(unpack(a) | unpack(b)) on arrays.
"""
import functools
import math
import struct

import mpmath as mp
import numpy as np

import pyref as R

DPS = 60
ETA = R.ULL_ETA
TAU = R.ULL_TAU
V = R.ULL_V
ML_BIAS = 0.48147376527720065
INV_SQRT_FISHER = 0.7608621002725182
HDR = 8                                                          # image = u64 register count + 2^p register bytes


def fgra_tol(p):
    """relative: m sequential additions (fast kernel) or <= 256 products, a few ulp per pow, times 1/tau for the final power"""
    return ((1 << p) + 1024) * 2.0 ** -52


def ml_tol(p):
    """relative: twice the solver's stopping step 0.001 * 0.7608 / sqrt(m) (the rule bounds the last step, not the error)"""
    return 2.0 * 0.001 * INV_SQRT_FISHER / math.sqrt(1 << p)


def valid_values(p):
    return [0, 4 * p - 4, 4 * p, 4 * p + 2] + list(range(4 * p + 4, 256))


def _check_hist(hist, p):
    hist = [int(c) for c in hist]
    assert len(hist) == 256 and sum(hist) == 1 << p, "not the histogram of 2^p registers"
    ok = set(valid_values(p))
    bad = [r for r, c in enumerate(hist) if c and r not in ok]
    if bad:
        raise ValueError("register values %r do not occur at p = %d" % (bad, p))
    return hist


def _eta2(qa, qb):
    """E[eta] when bit 1 is clear with probability qa and bit 0 with probability qb"""
    return qa * qb * ETA[0] + qa * (1 - qb) * ETA[1] + (1 - qa) * qb * ETA[2] + (1 - qa) * (1 - qb) * ETA[3]


def _quadratic(alpha, beta, gamma):
    return (mp.sqrt(beta * beta + 4 * alpha * gamma) - beta) / (2 * alpha)


def _empty_term(z, tiny):
    """empty register: the largest virtual value is -j with probability z^(2^j - 1) (1 - z^(2^j)) (given the register is
    empty), weight 2^(tau j); the two bits below belong to -j-1 and -j-2 (rates 2^(j+1) lambda and 2^(j+2) lambda)"""
    s, j = mp.mpf(0), 0
    lz = mp.log(z)
    while True:
        zj = mp.exp(lz * 2 ** j)
        term = mp.mpf(2) ** (TAU * j) * mp.exp(lz * (2 ** j - 1)) * (-mp.expm1(lz * 2 ** j)) * _eta2(zj ** 2, zj ** 4)
        s += term
        if zj < 0.5 and term <= tiny * s:
            return s
        j += 1


def _saturated_term(t, b1, b0, tiny):
    """saturated register (u = K, observed bits b1 = [K-1 seen], b0 = [K-2 seen]) at t = exp(-lambda 2^-K): the ideal largest
    value is K + j with probability proportional to (1 - q_j) q_j, q_j = t^(2^-j) = "K + j not seen"; its bits are the observed
    ones (j = 0), [K seen] unknown and b1 (j = 1), both unknown (j >= 2).  Returns E[eta 2^(-tau j)]; 2^(-tau K) is the caller's."""
    if t == 0:
        return mp.mpf(0)                                         # lambda -> infinity: all the weight runs off to j -> infinity
    lt = mp.log(t)
    q = lambda j: mp.exp(lt * mp.mpf(2) ** -j)
    w = lambda j: -mp.expm1(lt * mp.mpf(2) ** -j) * q(j)
    num = w(0) * ETA[(b1 << 1) | b0] + mp.mpf(2) ** -TAU * w(1) * (t * ETA[b1] + (1 - t) * ETA[2 | b1])
    den = w(0) + w(1)
    j = 2
    while True:
        wj = w(j)
        term = mp.mpf(2) ** (-TAU * j) * wj * _eta2(q(j - 1), q(j - 2))
        num += term
        den += wj
        if term <= tiny * num and wj <= tiny * den:
            return num / den
        j += 1


@functools.lru_cache(maxsize=None)
def _fgra_cached(hist, p):
    with mp.workdps(DPS):
        tiny = mp.mpf(10) ** -(DPS - 5)
        m, K, off = 1 << p, 65 - p, 4 * p + 4
        c0, c4, c8, c10 = hist[0], hist[off - 8], hist[off - 4], hist[off - 2]
        W = hist[252:256]
        total = mp.mpf(0)
        if c0 == m:
            return 0.0                                           # z = 1: an empty register's term is infinite
        if c0 or c4 or c8 or c10:
            x = _quadratic(mp.mpf(m + 3 * (c0 + c4 + c8 + c10)), mp.mpf(m - c0 - c4), mp.mpf(4 * c0 + 2 * c4 + 3 * c8 + c10))
            z = x ** 4                                           # exp(-lambda)
            if c0:
                total += c0 * _empty_term(z, tiny)
            total += c4 * mp.mpf(2) ** -TAU * _eta2(z, z * z)                                  # u = 1: bits = values 0, -1
            total += c8 * mp.mpf(4) ** -TAU * (z * ETA[0] + (1 - z) * ETA[1])                  # u = 2, 1 not seen; bit 0 = value 0
            total += c10 * mp.mpf(4) ** -TAU * (z * ETA[2] + (1 - z) * ETA[3])                 # u = 2, 1 seen
        for r in range(off, 252):
            if hist[r]:
                total += hist[r] * ETA[r & 3] * mp.mpf(2) ** (-TAU * ((r >> 2) - p + 2))
        if any(W):
            y = _quadratic(mp.mpf(m + 3 * sum(W)), mp.mpf(W[0] + W[1] + 2 * (W[2] + W[3])), mp.mpf(m + 2 * W[0] + W[2] - W[3]))
            t = mp.sqrt(y)                                       # y = exp(-lambda 2^-(K-1)), t = exp(-lambda 2^-K)
            for low in range(4):
                if W[low]:
                    total += W[low] * mp.mpf(2) ** (-TAU * K) * _saturated_term(t, low >> 1, low & 1, tiny)
        if total == 0:
            return math.inf
        factor = mp.mpf(m) ** (1 + 1 / mp.mpf(TAU)) / (1 + mp.mpf(V) * (1 + mp.mpf(TAU)) / (2 * m))
        return float(factor * total ** (-1 / mp.mpf(TAU)))


def fgra_ref(hist256, p):
    return _fgra_cached(tuple(_check_hist(hist256, p)), p)


def ml_coefficients(hist, p):
    """(A * 2^64 as an exact integer, {e: B_e}): log L = -lambda A + sum_e B_e log(1 - exp(-lambda 2^-e))"""
    K = 65 - p
    A, B = 0, {}
    for r, c in enumerate(hist):
        if not c:
            continue
        if r == 0:
            A += c << 64                                         # no value at all: total rate 1
            continue
        u, b1, b0 = (r >> 2) - p + 2, (r >> 1) & 1, r & 1
        if u < K:
            A += c << (64 - u)                                   # nothing above u: rates 2^-(u+1) + ... (the cap included) = 2^-u
        for k, seen in ((u, 1), (u - 1, b1), (u - 2, b0)):
            if k < 1:
                continue
            e = min(k, K - 1)                                    # the saturated value has its predecessor's rate
            if seen:
                B[e] = B.get(e, 0) + c
            else:
                A += c << (64 - e)
    return A, B


@functools.lru_cache(maxsize=None)
def _ml_cached(hist, p):
    m = 1 << p
    A64, B = ml_coefficients(hist, p)
    if not B:
        return 0.0
    if A64 == 0:
        return math.inf
    a = A64 / 2.0 ** 64
    items = sorted(B.items())

    def f_double(lam):
        s = -a
        for e, c in items:
            x = math.ldexp(lam, -e)
            s += math.ldexp(c, -e) / math.expm1(x) if x < 700.0 else 0.0
        return s
    lo, hi = -80.0, 80.0                                         # log2(lambda)
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        if f_double(2.0 ** mid) > 0:
            lo = mid
        else:
            hi = mid
    with mp.workdps(DPS):
        A = mp.mpf(A64) / mp.mpf(2) ** 64
        lam = mp.mpf(2.0 ** (0.5 * (lo + hi)))

        def f(lam, deriv):
            s, d = -A, mp.mpf(0)
            for e, c in items:
                rate = mp.mpf(2) ** -e
                em = mp.expm1(lam * rate)
                s += c * rate / em
                if deriv:
                    d -= c * rate * rate * (em + 1) / (em * em)
            return s, d
        for _ in range(12):
            s, d = f(lam, True)
            step = s / d
            lam -= step
            if abs(step) <= lam * mp.mpf(10) ** -45:
                break
        else:
            raise ArithmeticError("Newton did not settle")
        eps = mp.mpf(10) ** -40                                  # f decreases: the root is bracketed to 40 digits
        assert f(lam * (1 - eps), False)[0] > 0 > f(lam * (1 + eps), False)[0]
        return float(m * lam / (1 + mp.mpf(ML_BIAS) / m))


def ml_ref(hist256, p):
    return _ml_cached(tuple(_check_hist(hist256, p)), p)


_UNPACK = np.array([R.ull_unpack(r) if r == 0 or r >= 8 else 0 for r in range(256)], dtype=np.uint64)


def merge_ref(a, b):
    """pack(unpack(a) | unpack(b)) element-wise on uint8 arrays (registers 0 or >= 8)"""
    x = _UNPACK[np.asarray(a, np.uint8)] | _UNPACK[np.asarray(b, np.uint8)]
    out = np.zeros(x.shape, np.uint8)
    nz = x != 0
    xs = x[nz]
    top = np.zeros(xs.shape, np.uint64)
    for s in (32, 16, 8, 4, 2, 1):                               # floor(log2) without going through float
        big = (xs >> (top + np.uint64(s))) != 0
        top[big] += np.uint64(s)
    out[nz] = ((top << np.uint64(2)) | ((xs >> (top - np.uint64(2))) & np.uint64(3))).astype(np.uint8)
    return out


_LUT = None


def merge_hist(a, b):
    """histogram of merge_ref(a, b), through merge_ref's table of all 256 x 256 byte pairs"""
    global _LUT
    if _LUT is None:
        v = np.arange(256, dtype=np.uint8)
        _LUT = merge_ref(np.repeat(v, 256), np.tile(v, 256)).reshape(256, 256)
    return np.bincount(_LUT[np.asarray(a, np.uint8).reshape(-1), np.asarray(b, np.uint8).reshape(-1)], minlength=256)


def hist_of(regs):
    return np.bincount(np.asarray(regs, np.uint8).reshape(-1), minlength=256)


def sample_registers(rng, p, n, count):
    """`count` sketches of 2^p registers drawn from the Poisson model at n distinct elements (n any float): the largest
    value by inversion of P(max <= k) = exp(-lambda 2^-k) (k < K; the cap K takes the rest), then the two bits below it,
    each seen with probability 1 - exp(-lambda P(k)).  No hashing."""
    m, K = 1 << p, 65 - p
    lam = float(n) / m
    shape = (count, m)
    if lam == 0.0:
        return np.zeros(shape, np.uint8)
    with np.errstate(divide="ignore"):
        e = -np.log(rng.random(shape))                           # max <= k  <=>  e >= lambda 2^-k
        u = np.ceil(np.log2(lam) - np.log2(e))
    u = np.clip(u, 0, K).astype(np.int64)                        # 0: empty (e >= lambda)
    rate = lambda k: lam * np.exp2(-np.minimum(k, K - 1).astype(np.float64))
    b1 = (rng.random(shape) < -np.expm1(-rate(u - 1))) & (u >= 2)
    b0 = (rng.random(shape) < -np.expm1(-rate(u - 2))) & (u >= 3)
    r = ((u + p - 2) << 2) | (b1.astype(np.int64) << 1) | b0.astype(np.int64)
    return np.where(u == 0, 0, r).astype(np.uint8)


# ---- images -------------------------------------------------------------------------------------------------------
def image(regs, p):
    regs = np.asarray(regs, np.uint8).reshape(-1)
    assert regs.size == 1 << p
    return np.concatenate([np.frombuffer(struct.pack("<Q", 1 << p), np.uint8), regs])


def regs_of(img):
    return np.asarray(img)[..., HDR:]


SMALL_N = ("0", "1", "2", "3", "m/8", "m/2", "2m")
SATURATED_MU = (0.02, 0.2, 0.7)                                  # lambda 2^-(K-1): 2 %, 18 %, 50 % of the registers saturate


def small_n(p, which):
    m = 1 << p
    return {"0": 0, "1": 1, "2": 2, "3": 3, "m/8": m // 8, "m/2": m // 2, "2m": 2 * m}[which]


def saturated_n(p, mu):
    return mu * 2.0 ** (64 - p) * (1 << p)


def regular(rng, p):
    return image(sample_registers(rng, p, 20 << p, 1)[0], p)


def dense(rng, p):
    """n = 200 m: no register below update value 3 (P = e^-50 each), what genome-sized sketches look like"""
    return image(sample_registers(rng, p, 200 << p, 1)[0], p)


def small(rng, p, which):
    return image(sample_registers(rng, p, small_n(p, which), 1)[0], p)


def saturated(rng, p, mu):
    return image(sample_registers(rng, p, saturated_n(p, mu), 1)[0], p)


def flat(p, r):
    return image(np.full(1 << p, r, np.uint8), p)


def halves(p, r):
    regs = np.full(1 << p, r, np.uint8)
    regs[1::2] = r ^ 1
    return image(regs, p)


def flat_values(p):
    """0, an even and an odd regular value, 255"""
    return (0, 4 * p + 24, 4 * p + 45, 255)


def all_pairs(p):
    """[(image_a, image_b), ...]: over all image pairs, the register positions hold every ordered pair of valid_values(p)
    (repeated cyclically to fill the last image)"""
    v = np.array(valid_values(p), np.uint8)
    a, b = np.repeat(v, len(v)), np.tile(v, len(v))
    m = 1 << p
    n_img = -(-len(a) // m)
    idx = np.arange(n_img * m) % len(a)
    a, b = a[idx].reshape(n_img, m), b[idx].reshape(n_img, m)
    return [(image(a[i], p), image(b[i], p)) for i in range(n_img)]


# the one-pair-at-a-time merge check: 8 registers, one of them merge(a, b), seven of the largest regular value (u = 61), which
# together weigh less than any other register, so that FGRA follows the one register that differs
TINY_P, TINY_FILLER = 3, 251


def regime_images(p, seed=0):
    """the reference and query sets of the regime tests: 11 and 13 images (neither a multiple of a tile side)"""
    rng = np.random.default_rng(1000 * p + seed)
    f0, fe, fo, f255 = (flat(p, r) for r in flat_values(p))
    sm = [small(rng, p, w) for w in ("3", "m/2", "2m")]
    sat = [saturated(rng, p, mu) for mu in (0.2, 0.7)]
    reg = [regular(rng, p) for _ in range(3)]
    hv = halves(p, 4 * p + 24)
    ref = [reg[0]] + sm + sat + [f0, fo, fe, f255, hv]
    qry = [hv, f255, reg[1], fe, sat[1], fo, sm[2], f0, reg[2], sat[0], sm[1], reg[0], sm[0]]
    return np.stack(ref), np.stack(qry)
