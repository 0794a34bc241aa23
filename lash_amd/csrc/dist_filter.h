// dist_filter.h — what the pair filters of `lash dist` share: --max-dist (dist_filter.hip), --top (dist_top.hip) and --cluster
// (dist_cluster.hip).  The block's
// statistics as the filter kernels read them, the device distance of one pair (its error analysis is at the top of dist_filter.hip),
// and the candidate layout with the scan / write kernels that compact a mask of candidates in (row, col) order.
#pragma once
#include "lash_ctx.h"
#include "dist_pair.h"

namespace lash {

constexpr uint32_t WF_TILE = 1024;                       // columns per tile: 256 lanes x 4 steps
constexpr uint32_t WF_WORDS = WF_TILE / 64;              // mask words per tile

// one candidate: block row, set column, the pair's statistics; ec_x: the small-pair cell sum of hmh, else NaN
struct WithinPair {
    uint32_t row, col, c_or_zero, n;
    double sum_or_union, ec_x;
};

struct WithinArgs {
    int algo, p, k, model, fp32;
    double limit;                                        // D + margin
    uint32_t nr, n_cols, tiles_x;
    uint64_t n_tiles;
    int64_t tri;                                         // r0 for a triangle block, else -1
    const double *row_card, *col_card;                   // row_card: the block's first row
    const uint32_t *c_or_zero, *n_counts;                // [nr][n_cols]
    const double *sum_or_union;
    const int32_t *row_small, *col_small;                // position in the set's small_idx, or -1 (row_small: the block's first row)
    const double *X;                                     // EcBlock (nrs == 0: none)
    uint32_t nrs, q_step, nqs, rbase;
};

__device__ __forceinline__ uint32_t row_end(const WithinArgs &a, uint32_t r)
{
    if (a.tri < 0) return a.n_cols;
    const int64_t e = a.tri + (int64_t)r + 1;                                          // printed columns of row r
    return e < (int64_t)a.n_cols ? (uint32_t)e : a.n_cols;
}

// The device's similarity *sim of pair (r, q).  false: the pair needs the host's arithmetic (the HLL++ bias-table regime, a
// linear-counting estimate at the threshold, a small HyperMinHash pair without a cell sum) and nothing is set.  The similarity is
// the host's bit for bit, except for HLL in linear counting, where the union is shrunk by 2^-44 so that *sim is never below the
// host's (dist_filter.hip); *sim_low is then the same expression with the union grown by 2^-44, never above the host's, and
// everywhere else equal to *sim (--cluster needs both sides, dist_cluster.hip).
__device__ inline bool pair_similarity_dev(const WithinArgs &a, uint32_t r, uint32_t q, double *sim_out, double *sim_low_out)
{
    const uint64_t at = (uint64_t)r * a.n_cols + q;
    const double rc = a.row_card[r], qc = a.col_card[q];
    double sim, sim_low;
    if (a.algo == LASH_HLL) {
        const uint32_t zero = a.c_or_zero[at];
        double u;
        const int regime = pairmath::hll_len_regime(a.p, zero, a.sum_or_union[at], &u);
        if (regime == pairmath::HLL_BIAS) return false;                               // host-only arithmetic (and maybe LASH_ERANGE)
        if (zero > 0) {
            const double m = (double)(1u << a.p), thr = pairmath::hll_threshold(a.p);
            const double h = m * log(m / (double)zero);
            if (fabs(h - thr) <= thr * 0x1p-40) return false;                           // the host's log may fall on the other side
            if (regime == pairmath::HLL_LINEAR) {
                sim_low = pairmath::union_similarity(rc, qc, u * (1.0 + 0x1p-44));     // no smaller than the host's
                u *= 1.0 - 0x1p-44;                                                    // no larger than the host's
                *sim_out = pairmath::union_similarity(rc, qc, u);
                *sim_low_out = sim_low;
                return true;
            }
        }
        sim = pairmath::union_similarity(rc, qc, u);
    } else if (a.algo == LASH_ULL) {
        sim = pairmath::union_similarity(rc, qc, a.sum_or_union[at]);
    } else {
        const double c = (double)a.c_or_zero[at], n = (double)a.n_counts[at];
        double ec = 0.0;
        if (c != 0.0 && !pairmath::hmh_ec_closed_form(qc, rc, &ec)) {
            const int32_t rs = a.row_small[r], cs = a.col_small[q];
            if (rs < 0 || cs < 0 || a.nrs == 0) return false;                           // (only NaN cardinalities get here)
            const uint32_t ri = (uint32_t)rs - a.rbase, q0 = (uint32_t)cs / a.q_step * a.q_step, nq = min(a.q_step, a.nqs - q0);
            ec = pairmath::hmh_ec_from_cell_sum(a.X[(uint64_t)a.nrs * q0 + (uint64_t)ri * nq + ((uint32_t)cs - q0)]);
        }
        sim = pairmath::hmh_similarity(c, n, ec);
    }
    *sim_out = *sim_low_out = sim;
    return true;
}

// The device's similarity *sim (pair_similarity_dev's) and the distance *d it gives; false as pair_similarity_dev.
__device__ inline bool pair_distance_dev(const WithinArgs &a, uint32_t r, uint32_t q, double *sim_out, double *d_out)
{
    double sim, sim_low;
    if (!pair_similarity_dev(a, r, q, &sim, &sim_low)) return false;
    *sim_out = sim;
    *d_out = pairmath::distance_from_similarity(sim, a.algo == LASH_ULL, a.k, a.model, a.fp32 != 0);
    return true;
}

// the block's WithinArgs from its statistics in HBM (d_c / d_n / d_u as lash_sketch_set_pair_block_device wrote them)
WithinArgs within_args(const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                       int model, int fp32, const uint32_t *d_c, const uint32_t *d_n, const double *d_u, const EcBlock &eb);

// One block of a filtered `lash dist` run, ready for a mark kernel: the pair statistics [sum_or_union f64 | c_or_zero u32 | n u32] (as
// lash_sketch_set_pair_block) and, for hmh, the small pairs' cell sums in HBM, the WithinArgs over them (a.limit is the caller's), and
// the compaction scratch [offsets u64 (n_tiles + 1) | mask u64 (n_tiles * WF_WORDS) | counts u32 (n_tiles)].  Queued on the context's
// stream; nr and n_cols are not 0.
struct WithinBlock {
    WithinArgs a;
    uint64_t *d_off, *d_mask;
    uint32_t *d_cnt;
};
int within_block(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                 int model, int fp32, int ull_estimator, WithinBlock &b);

// compaction: mask words [n_tiles][WF_WORDS] of candidates and their per-tile counts -> exclusive offsets (d_off: n_tiles + 1) -> the
// candidates with their statistics in (row, col) order, copied back into `cand` (synchronous; dist_filter.hip's scan and write kernels)
int within_compact(lash_ctx *ctx, const WithinArgs &a, const uint64_t *d_mask, const uint32_t *d_cnt, uint64_t *d_off, std::vector<WithinPair> &cand);

}  // namespace lash
