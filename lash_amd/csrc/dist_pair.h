// dist_pair.h — the per-pair arithmetic of `lash dist` that the host (lash_dist_rows, dist_estimators.hip) and the GPU (the
// --max-dist filter, dist_filter.hip) share: one statement of the rule, compiled for both sides.
//
// Reference: /root/reference/src/utils.rs:164-167 (hmh), 272-278 (ull), 355-365 (hll); main.rs:415-423 (distance).
// Everything here is +, -, *, / on doubles with contraction off (so host and device round the same way: x86-64 has no FMA to
// contract into, gfx950 would), plus the transcendental calls: log in HLL++ linear counting, log / pow in the distance.  Those
// are the only places where the device (ocml) and the host (glibc) may disagree; dist_filter.hip bounds the disagreement.
// What stays host-only: the HLL++ bias-table branch of len() (hll_estimate_bias, dist_estimators.hip) and hyperminhash's
// 65 536-cell walk of expected_collisions for small pairs.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace lash {
namespace pairmath {

// hyperminhash's expected_collisions(n, m) where it is O(1): saturated, or both cardinalities above 2^(p+5) = 2^19 (returns true,
// *out set).  Below, the crate walks 65 536 cells (returns false).  (constants: 2^(2^q + r) = 2^74, 2^(p + 5) = 2^19,
// 2^(p - r) = 16; the crate writes them as powf calls)
__host__ __device__ inline bool hmh_ec_closed_form(double n, double m, double *out)
{
#pragma clang fp contract(off)
    if (n < m) { const double t = n; n = m; m = t; }
    if (n > 18889465931478580854784.0) { *out = 1.8446744073709552e19; return true; }                 // u64::MAX
    if (n > 524288.0) {
        const double t = (1.0 + n) / m;
        const double d = (4.0 * n / m) / (t * t);
        *out = 0.169919487159739093975315012348 * 16.0 * d + 0.5;
        return true;
    }
    return false;
}

// the 65 536-cell sum x -> the value similarity() subtracts (p = 14)
__host__ __device__ inline double hmh_ec_from_cell_sum(double x)
{
#pragma clang fp contract(off)
    return (x * 14.0 + 0.5) / 14.0;
}

// streaming_algorithms 0.3.3 len() thresholds (HLL++, Heule et al.), p = 4..18
__host__ __device__ inline double hll_threshold(int p)
{
    switch (p) {
    case 4: return 10; case 5: return 20; case 6: return 40; case 7: return 80; case 8: return 220; case 9: return 400;
    case 10: return 900; case 11: return 1800; case 12: return 3100; case 13: return 6500; case 14: return 11500;
    case 15: return 20000; case 16: return 50000; case 17: return 120000; default: return 350000;
    }
}

__host__ __device__ inline double hll_alpha(int p)
{
#pragma clang fp contract(off)
    switch (p) {
    case 4: return 0.673;
    case 5: return 0.697;
    case 6: return 0.709;
    default: return 0.7213 / (1.0 + 1.079 / (double)(1u << p));
    }
}

// len() of an HLL++ sketch from its zero-register count and sum of 2^-register, without the bias-table branch:
//   HLL_LINEAR  linear counting (*out = m ln(m / zero), *out <= the threshold)
//   HLL_RAW     alpha m^2 / sum above 5m (*out)
//   HLL_BIAS    the raw estimate *out is <= 5m: len() subtracts the HLL++ table bias from it (host only)
enum { HLL_LINEAR = 0, HLL_RAW = 1, HLL_BIAS = 2 };
__host__ __device__ inline int hll_len_regime(int p, uint64_t zero, double sum, double *out)
{
#pragma clang fp contract(off)
    const double m = (double)(1u << p);
    if (zero > 0) {
        const double h = m * std::log(m / (double)zero);
        if (h <= hll_threshold(p)) { *out = h; return HLL_LINEAR; }
    }
    const double e = hll_alpha(p) * m * m / sum;
    *out = e;
    return e <= 5.0 * m ? HLL_BIAS : HLL_RAW;
}

template <class T>
__host__ __device__ inline T compute_distance(T frac, int k, int model)
{
#pragma clang fp contract(off)
    const T kk = (T)k;
    // frac == 0 (no similarity left after the collision correction: nearly every pair of an all-vs-all): both models give exactly 1 —
    // -ln(0) / k = +inf -> min(.., 1) = 1;  1 - 0^(1/k) = 1 — without the libm call (glibc's pow(0, y) alone is 45 ns)
    if (frac == (T)0) return (T)1;
    if (model == 1) { const T d = -std::log(frac) / kk; return d < (T)1 ? d : (T)1; }      // (-frac.ln() / k).min(1)
    return (T)1 - std::pow(frac, (T)1 / kk);
}

// similarity: hmh / hll (ull = false) `.max(0.0)` (utils.rs:164, 362) — f64::max drops a NaN; ull: `if similarity < 0.0 {0.0}
// else {similarity}` (utils.rs:272-273) keeps it: two empty sketches give 0/0, model 1 then prints 1 (f64::min drops the NaN),
// model 0 NaN.  Then 2s/(1+s) (utils.rs:165-167) and the Mash distance, in f32 when fp32 (main.rs --fp32).
__host__ __device__ inline double distance_from_similarity(double sim, bool ull, int k, int model, bool fp32)
{
#pragma clang fp contract(off)
    if (ull) sim = sim < 0.0 ? 0.0 : sim;
    else if (!(sim >= 0.0)) sim = 0.0;
    const double frac = 2.0 * sim / (1.0 + sim);
    return fp32 ? (double)compute_distance<float>((float)frac, k, model) : compute_distance<double>(frac, k, model);
}

// `lash dist --containment` (not upstream): which fraction the Mash distance is taken of (include/lash_gfx950.h: LASH_MEASURE_*)
enum { MEASURE_JACCARD = 0, MEASURE_CONTAIN_QUERY = 1, MEASURE_CONTAIN_REFERENCE = 2 };

// The containment fraction of a pair with similarity s > 0 (clamped as above) and cardinalities a_r (reference), a_q (query):
//   frac_c = s/(1+s) * (a_r + a_q) / den,   den = a_q (how much of the query is in the reference) or a_r (the other way round).
// s/(1+s) * (a_r + a_q) is the shared k-mer estimate: for hll / ull, s = (a_r + a_q - u) / u, it is a_r + a_q - u exactly
// (inclusion-exclusion); for hmh it is the Jaccard-to-intersection identity.  The association is fixed here and nowhere else:
// (s / (1 + s)) * ((a_r + a_q) / den).  With a_r == a_q the second factor is 2 exactly and doubling commutes with the rounding
// of the quotient, so frac_c is the 2s/(1+s) of distance_from_similarity bit for bit: equal-sized sketches print what the
// default prints.  For fixed cardinalities frac_c does not decrease as s grows.
__host__ __device__ inline double containment_frac(double sim, double a_r, double a_q, int measure)
{
#pragma clang fp contract(off)
    const double den = measure == MEASURE_CONTAIN_QUERY ? a_q : a_r;
    return (sim / (1.0 + sim)) * ((a_r + a_q) / den);
}

// distance_from_similarity under a measure.  MEASURE_JACCARD: that function itself.  Containment: the same clamp of the similarity;
// then s <= 0 gives exactly 1 BEFORE any ratio is formed (whatever the cardinalities are, 0 and NaN included: what the filters call
// PAIR_ONE); frac_c >= 1 (one side wholly inside the other, up to estimator noise) gives +0.0 exactly without a libm call, in both
// models, f64 and f32 — -log(1) / k would be -0.0 and a frac_c above 1 a negative distance; everything else goes through
// compute_distance as the Jaccard fraction does (a NaN similarity, ull only, stays a NaN fraction).
__host__ __device__ inline double distance_from_similarity(double sim, bool ull, int k, int model, bool fp32, int measure, double a_r, double a_q)
{
#pragma clang fp contract(off)
    if (measure == MEASURE_JACCARD) return distance_from_similarity(sim, ull, k, model, fp32);
    if (ull) sim = sim < 0.0 ? 0.0 : sim;
    else if (!(sim >= 0.0)) sim = 0.0;
    if (sim <= 0.0) return 1.0;
    const double frac = containment_frac(sim, a_r, a_q, measure);
    if (fp32) {
        const float f = (float)frac;
        return f >= 1.0f ? 0.0 : (double)compute_distance<float>(f, k, model);
    }
    return frac >= 1.0 ? 0.0 : compute_distance<double>(frac, k, model);
}

// hyperminhash's similarity from C, N and expected_collisions (utils.rs:164 behind Sketch::similarity); c == 0 needs no ec
__host__ __device__ inline double hmh_similarity(double c, double n, double ec)
{
#pragma clang fp contract(off)
    if (c == 0.0) return 0.0;
    return c < ec ? 0.0 : (c - ec) / n;
}

// hll (u = len() of the union) and ull (u = the union estimate): inclusion-exclusion (utils.rs:272, 362)
__host__ __device__ inline double union_similarity(double a, double b, double u)
{
#pragma clang fp contract(off)
    return (a + b - u) / u;
}

}  // namespace pairmath
}  // namespace lash
