"""The UltraLogLog estimators of ull_estimators.h (host build, `lash_ull_estimate`) against the high-precision reference of
tests/ullref.py, which shares no code with them, and against the truth on sketches sampled from the Poisson model.

Bounds (ullref.fgra_tol / ml_tol; reasoning in the issue that introduced this file):
  FGRA  |got - ref| <= (m + 1024) 2^-52 ref          m sequential additions at most, a few ulp per pow, 1/tau for the last power
  ML    |got - ref| <= 2 * 0.001 * 0.7608 / sqrt(m) ref      twice the solver's stopping step
  exact 0, +inf and register bytes.

Measured on the host, worst |got - ref| / ref over every maker (regular, small x7, saturated x3, flat x4, halves, all_pairs,
every value):
  p      3        4        8        9        10       12       15       16       18       20
  FGRA   1.0e-14  4.1e-15  2.8e-14  7.7e-14  6.1e-15  1.2e-13  1.2e-13  1.5e-11  1.0e-11  6.1e-12
  bound  2.3e-13  2.3e-13  2.8e-13  3.4e-13  4.6e-13  1.1e-12  7.5e-12  1.5e-11  5.8e-11  2.3e-10
  ML     1.1e-07  3.2e-07  3.4e-08  3.5e-09  4.8e-09  6.1e-10  5.9e-10  5.9e-10  5.9e-10  5.9e-10
  bound  5.4e-04  3.8e-04  9.5e-05  6.7e-05  4.8e-05  2.4e-05  8.4e-06  5.9e-06  3.0e-06  1.5e-06
ML never uses more than 1e-3 of its bound (the secant iteration's last step squares the error).  FGRA is at 1e-2 of its bound
or below except on almost empty sketches ("small 1", "small 3"; 0.98 of the bound at p = 16): fgra() forms z = e^(-n/m) = x^4,
which rounds to a neighbour of 1, and an empty register's term needs 1 - z ~ n/m, so m 2^-53 of relative error is built in.
A finding about the estimator's conditioning, inside the bound on every input here, and left as it is.

Saturated registers (r >= 252): before this file the FGRA term of the ideal largest values K + 2, K + 3, ... (`phi`) carried the
factor eta_X = 0.726 twice.  With 2 % / 18 % / 50 % of the registers saturated the host FGRA was 3.9e-5 / 2.4e-3 / 1.9e-2
above the reference at p = 20 (standard error 7.8e-4); 400 sampled sketches at p = 8 put its mean at +6.86 standard errors
(+1.6 %) in the 50 % case and, with phi restated as the plain series, at -1.47 (-0.3 %).  ML (the capped likelihood,
`b[63 - p] += b[64 - p]`) was unbiased before and after: -0.09 / -0.87 / -1.26 standard errors.
"""
import math

import numpy as np
import pytest

import lash_amd
import oracle_lib as O
import pyref as R
import ullref as U

P_ALL = [3, 4, 8, 9, 10, 12, 15, 16, 18, 20]


def _makers(p):
    rng = np.random.default_rng(p)
    imgs = {"regular": U.regular(rng, p)}
    for w in U.SMALL_N:
        imgs["small " + w] = U.small(rng, p, w)
    for mu in U.SATURATED_MU:
        imgs["saturated %g" % mu] = U.saturated(rng, p, mu)
    for r in U.flat_values(p):
        imgs["flat %d" % r] = U.flat(p, r)
    imgs["halves"] = U.halves(p, 4 * p + 24)
    pairs = U.all_pairs(p)
    for i in range(0, len(pairs), max(1, len(pairs) // 6)):     # (every pair of them: test_gpu_ull_pairs.py)
        a, b = pairs[i]
        imgs["all_pairs[%d] a" % i], imgs["all_pairs[%d] b" % i] = a, b
        imgs["all_pairs[%d] merged" % i] = U.image(U.merge_ref(U.regs_of(a), U.regs_of(b)), p)
    v, m = U.valid_values(p), 1 << p
    for i in range(0, len(v), m):                               # every value that exists at this p, m at a time
        imgs["values[%d:]" % i] = U.image(np.resize(np.array(v[i:i + m], np.uint8), m), p)
    return imgs


def _rel(got, want):
    """relative error; 0 / +inf must be met exactly"""
    if want == 0.0 or math.isinf(want):
        assert got == want, (got, want)
        return 0.0
    return abs(got - want) / want


@pytest.mark.parametrize("p", P_ALL)
def test_host_estimators_match_the_reference(p):
    worst = {"fgra": 0.0, "ml": 0.0}
    seen = set()
    for name, img in _makers(p).items():
        regs = U.regs_of(img)
        hist = U.hist_of(regs)
        seen |= {int(r) for r in np.nonzero(hist)[0]}
        for est, ref, tol in (("fgra", U.fgra_ref, U.fgra_tol(p)), ("ml", U.ml_ref, U.ml_tol(p))):
            err = _rel(lash_amd.ull_estimate(regs, p, est), ref(hist, p))
            worst[est] = max(worst[est], err)
            assert err <= tol, (p, name, est, err, tol)
    assert seen == set(U.valid_values(p))                       # every value that exists at this p was estimated somewhere
    print("p=%d worst relative error: fgra %.2e (bound %.2e), ml %.2e (bound %.2e)" % (p, worst["fgra"], U.fgra_tol(p), worst["ml"], U.ml_tol(p)))


def test_the_makers_reach_what_they_are_for():
    for p in P_ALL:
        rng = np.random.default_rng(p)
        special = set()
        for w in U.SMALL_N:
            h = U.hist_of(U.regs_of(U.small(rng, p, w)))
            special |= {r for r in (0, 4 * p - 4, 4 * p, 4 * p + 2) if h[r]}
            if w == "2m" and p >= 8:
                assert h[0] and h[4 * p - 4] and h[4 * p] and h[4 * p + 2] and h[4 * p + 4:252].sum()
        assert special == {0, 4 * p - 4, 4 * p, 4 * p + 2}
        m = 1 << p
        for mu in U.SATURATED_MU:
            h = U.hist_of(U.regs_of(U.saturated(rng, p, mu)))
            frac = h[252:].sum() / m
            assert abs(frac - -math.expm1(-mu)) <= 4 * math.sqrt(0.25 / m)
            assert p < 8 or mu < 0.7 or (h[252:] > 0).all()     # all four saturated bytes
        h = U.hist_of(U.regs_of(U.regular(rng, p)))
        assert h[252:].sum() == 0 and h[:4 * p + 4].sum() <= 0.02 * m     # n = 20 m: P(u <= 2) = e^-5
        h = U.hist_of(U.regs_of(U.dense(rng, p)))
        assert h[:4 * p + 4].sum() == 0 and h[252:].sum() == 0  # n = 200 m: the fast kernel's case
        a = np.concatenate([U.regs_of(x) for x, _ in U.all_pairs(p)])
        b = np.concatenate([U.regs_of(y) for _, y in U.all_pairs(p)])
        nv = len(U.valid_values(p))
        assert len(set(zip(a.tolist(), b.tolist()))) == nv * nv


def test_degenerate_returns_are_exact():
    for p in (3, 8, 16):
        empty, full = U.regs_of(U.flat(p, 0)), U.regs_of(U.flat(p, 255))
        for est, ref in (("fgra", U.fgra_ref), ("ml", U.ml_ref)):
            assert lash_amd.ull_estimate(empty, p, est) == 0.0 == ref(U.hist_of(empty), p)
            # every register saturated with both bits set: nothing was ever "not seen", a = 0
            assert lash_amd.ull_estimate(full, p, est) == math.inf == ref(U.hist_of(full), p)


def test_p26_flat():
    p = 26
    for r in U.flat_values(p):
        regs = np.full(1 << p, r, np.uint8)
        hist = np.zeros(256, np.int64)
        hist[r] = 1 << p
        assert _rel(lash_amd.ull_estimate(regs, p, "fgra"), U.fgra_ref(hist, p)) <= U.fgra_tol(p), r
        assert _rel(lash_amd.ull_estimate(regs, p, "ml"), U.ml_ref(hist, p)) <= U.ml_tol(p), r


def test_reference_rejects_values_that_do_not_exist():
    hist = np.zeros(256, np.int64)
    hist[4 * 8 + 1] = 256                                       # u = 2 with "value 0 seen"
    with pytest.raises(ValueError):
        U.fgra_ref(hist, 8)


@pytest.mark.parametrize("p", [3, 8, 12])
def test_per_register_restatement_handles_saturated_registers(p):
    """pyref.ull_fgra / ull_ml (float, per register; what the CLI tests compare with) against the 60-digit reference"""
    rng = np.random.default_rng(40 + p)
    for mu in U.SATURATED_MU:
        regs = U.regs_of(U.saturated(rng, p, mu))
        hist = U.hist_of(regs)
        assert hist[252:].sum() or p == 3
        lst = [int(r) for r in regs]
        assert R.ull_fgra(lst, p) == pytest.approx(U.fgra_ref(hist, p), rel=1e-11)
        assert R.ull_ml(lst, p) == pytest.approx(U.ml_ref(hist, p), rel=1e-11)
    assert R.ull_fgra([255] * (1 << p), p) == math.inf


@pytest.mark.parametrize("p", [3, 10, 15, 16])
def test_host_merge_equals_merge_ref_on_every_pair_of_values(p):
    for a, b in U.all_pairs(p):
        want = U.image(U.merge_ref(U.regs_of(a), U.regs_of(b)), p)
        assert np.array_equal(O.merge_images(O.ULL, p, a, b), want)
        if p <= 10:                                             # (per register in Python: slow above)
            assert bytes(U.regs_of(want)) == R.ull_merge(bytes(U.regs_of(a)), bytes(U.regs_of(b)))


# ---- the estimates against the truth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["fgra", "ml"])
def test_estimates_are_unbiased_on_sampled_sketches(est):
    """400 sketches per n at p = 8, registers drawn from the Poisson model (the number of elements is Poisson(n), so n is
    the expectation an unbiased estimator has to meet); the standard error comes from the 400 estimates themselves.
    The last three n leave 2 %, 18 % and 50 % of the registers saturated: this is what pins large_range_z, phi and ML's
    saturation line."""
    p, trials = 8, 400
    m = 1 << p
    rng = np.random.default_rng(2024)
    for n in [3, m // 2, 20 * m] + [U.saturated_n(p, mu) for mu in U.SATURATED_MU]:
        e = np.array([lash_amd.ull_estimate(r, p, est) for r in U.sample_registers(rng, p, n, trials)])
        se = e.std(ddof=1) / math.sqrt(trials)
        print("%s n=%.4g: mean/n - 1 = %+.3e = %+.2f standard errors" % (est, n, e.mean() / n - 1, (e.mean() - n) / se))
        assert abs(e.mean() - n) <= 3 * se, (est, n, e.mean() / n - 1, se / n)


# ---- one differing register among filler: what a wrong entry of the merge table would do ----------------------------------
TABLE = 0x55FAE4                                                 # lash_device.h: ull_merge_fast
TINY_P, TINY_FILLER = U.TINY_P, U.TINY_FILLER


def merge_fast_model(a, b, table=TABLE):
    hi, lo = max(a, b), min(a, b)
    d = min((hi >> 2) - (lo >> 2), 3) if lo else 3
    return hi | ((table >> (2 * (4 * d + (lo & 3)))) & 3)


def tiny_hist(r):
    hist = np.zeros(256, np.int64)
    hist[TINY_FILLER] += (1 << TINY_P) - 1
    hist[r] += 1
    return hist


def test_table_model_is_the_merge():
    v = U.valid_values(TINY_P)
    a, b = np.repeat(v, len(v)), np.tile(v, len(v))
    got = np.array([merge_fast_model(int(x), int(y)) for x, y in zip(a, b)], np.uint8)
    assert np.array_equal(got, U.merge_ref(a.astype(np.uint8), b.astype(np.uint8)))


def test_one_wrong_table_entry_moves_the_tiny_estimate_far_outside_tolerance():
    """test_gpu_ull_pairs.py gives every (a, b) its own 8-register sketch: merge(a, b) + 7 x TINY_FILLER.  Here: for each of the
    16 table entries and each wrong value of it, every (a, b) whose merged register changes moves the FGRA reference by more
    than 1e6 tolerances (the filler is light enough), and every entry is reached by some (a, b) — except where the table
    is redundant: at d = 0 the larger register already has the bits of a smaller one ending in 11, and bit 1 of one ending in 10."""
    harmless = set()
    v = U.valid_values(TINY_P)
    ok = set(v)
    tol = U.fgra_tol(TINY_P)
    for entry in range(16):
        for flip in (1, 2, 3):
            wrong = TABLE ^ (flip << (2 * entry))
            moved = 0
            for a in v:
                for b in v:
                    good, bad = merge_fast_model(a, b), merge_fast_model(a, b, wrong)
                    if good == bad:
                        continue
                    moved += 1
                    if bad not in ok:
                        continue                                # a byte no sketch holds: fgra() drops the register altogether
                    g, w = U.fgra_ref(tiny_hist(good), TINY_P), U.fgra_ref(tiny_hist(bad), TINY_P)
                    assert abs(g - w) > 1e6 * tol * g, (entry, flip, a, b, g, w)
            if not moved:
                harmless.add((entry, flip))
    assert harmless == {(2, 2), (3, 1), (3, 2), (3, 3)}
