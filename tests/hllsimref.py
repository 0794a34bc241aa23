"""numpy restatement of the HLL++ bias-table simulation (lash_hll_bias_simulate, lash_amd/csrc/hll_bias_sim.hip; DESIGN.md
"Simulated HLL++ bias tables"), step for step: S in the same floating-point order, the mean over the trials exact and rounded
once, so that its tables equal the GPU's bit for bit; plus the 6-nearest len() on register bytes (pyref.hll_len_from_regs with a tables dict)."""
from fractions import Fraction

import numpy as np

import pyref as R

U = np.uint64
GOLDEN, MUL1, MUL2, TRIAL = U(0x9E3779B97F4A7C15), U(0xBF58476D1CE4E5B9), U(0x94D049BB133111EB), U(0xD1342543DE82EF95)


def mix(x):
    """the splitmix64 step on a uint64 array (wrapping)"""
    z = x + GOLDEN
    z = (z ^ (z >> U(30))) * MUL1
    z = (z ^ (z >> U(27))) * MUL2
    return z ^ (z >> U(31))


def clz64(w):
    """leading zeros of every element of a uint64 array (64 for 0)"""
    w = w.copy()
    bits = np.zeros(w.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        t = w >> U(s)
        up = t != 0
        bits += s * up
        w = np.where(up, t, w)
    return 64 - (bits + (w != 0))


def default_points(p):
    return min(200, 5 * (1 << p) + 1)


def checkpoints(p, n_points):
    return [j * 5 * (1 << p) // (n_points - 1) for j in range(n_points)]


def estimate(p, regs):
    """E of one register state: S from 0.0 in increasing rank, then alpha * m * m / S"""
    m = float(1 << p)
    hist = np.bincount(regs, minlength=65)
    s = 0.0
    for r in range(65):
        s += float(hist[r]) * 2.0 ** -r
    return R.hll_alpha(p) * m * m / s


def trial_estimates(p, n_points, seed, t):
    m = 1 << p
    base = mix(np.array([seed], U) ^ (np.array([t], U) * TRIAL))[0]
    regs = np.zeros(m, np.int64)
    out, n_prev = [], 0
    for n_j in checkpoints(p, n_points):
        if n_j > n_prev:
            h = mix(base + np.arange(n_prev, n_j, dtype=U))
            np.maximum.at(regs, (h & U(m - 1)).astype(np.int64), clz64(h >> U(p)) - p + 1)
        n_prev = n_j
        out.append(estimate(p, regs))
    return out


def simulate(p, n_points=None, n_trials=2048, seed=42):
    """-> (n uint64, raw float64, bias float64), as Context.hll_bias_simulate returns them"""
    n_points = n_points or default_points(p)
    assert 4 <= p <= 18 and 6 <= n_points <= 5 * (1 << p) + 1
    with np.errstate(over="ignore"):
        e = [trial_estimates(p, n_points, seed, t) for t in range(n_trials)]
    n = checkpoints(p, n_points)
    # the exact sum over the trials and the exact quotient, rounded once (Fraction -> float rounds to nearest, ties to even)
    raw = [float(sum((Fraction(e[t][j]) for t in range(n_trials)), Fraction(0)) / n_trials) for j in range(n_points)]
    return np.array(n, U), np.array(raw, np.float64), np.array([r - float(c) for r, c in zip(raw, n)], np.float64)


def hll_len(p, regs, tables):
    """streaming_algorithms' len() with the 6-nearest bias of `tables` = {p: (raw list, bias list)}"""
    return R.hll_len_from_regs(p, regs, tables)
