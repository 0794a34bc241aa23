// dist_filter.h — what the pair filters of `lash dist` share: --max-dist (dist_filter.hip), --top (dist_top.hip), --cluster
// (dist_cluster.hip) and --derep (dist_derep.hip).  The block's statistics as the filter kernels read them, the device similarity of one pair and the interval
// it puts around the host's distance (with the error analysis), the tile loop of the mark kernels with the mask layout the
// scan / write kernels compact in (row, col) order, and the host's exact evaluation of what comes back.
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
    int measure;                                         // pairmath::MEASURE_*: --containment (rectangles only; the mark kernel of --max-dist and the key kernel of --top read it)
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

// the position in EcBlock::X of the cell sum of a small hmh pair: rs / cs = the row's / column's place in its set's small_idx, both >= 0
__device__ __forceinline__ uint64_t small_cell(const WithinArgs &a, int32_t rs, int32_t cs)
{
    const uint32_t ri = (uint32_t)rs - a.rbase, q0 = (uint32_t)cs / a.q_step * a.q_step, nq = min(a.q_step, a.nqs - q0);
    return (uint64_t)a.nrs * q0 + (uint64_t)ri * nq + ((uint32_t)cs - q0);
}

// The device's similarity *sim of pair (r, q).  false: the pair needs the host's arithmetic (the HLL++ bias-table regime, a
// linear-counting estimate at the threshold, a small HyperMinHash pair without a cell sum) and nothing is set.  The similarity is
// the host's bit for bit, except for HLL in linear counting, where the union is shrunk by 2^-44 so that *sim is never below the
// host's; *sim_low is then the same expression with the union grown by 2^-44, never above the host's, and everywhere else equal
// to *sim (pair_interval_dev below says why).
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
            ec = pairmath::hmh_ec_from_cell_sum(a.X[small_cell(a, rs, cs)]);
        }
        sim = pairmath::hmh_similarity(c, n, ec);
    }
    *sim_out = *sim_low_out = sim;
    return true;
}

// How far the host's distance d of a placed pair can be from the device's: the one margin of the three filters.
//   f64:  -ln(f) / k with d <= 1 has |ln f| <= k <= 32: ulp(32) / k ~ 2^-47 per ulp; 1 - f^(1/k): ulp(1) = 2^-52.  ocml and glibc are
//         a few ulp apart: < 2^-44.  margin 2^-40.
//   fp32: the same in float (ocml's logf / powf: <= 2 ulp; glibc's correctly rounded or 1 ulp): ulp(1.0f) = 2^-23 per ulp of
//         d ~ 1, so a few ulp each side: < 2^-19.  margin 2^-16 (1.5e-5).
__host__ __device__ constexpr double filter_margin(bool fp32) { return fp32 ? 0x1p-16 : 0x1p-40; }

// The interval [*d_lo, *d_hi] that holds the host's exact d (dist_pair_host, in f32 under fp32) of a pair pair_similarity_dev has
// placed (its false is the fourth outcome: the pair is the host's alone, always sent back and never pruned, because it may be the
// one a run is refused on, LASH_ERANGE).
//   Identical similarity.  Up to the final log / pow the device evaluates the host's expressions (dist_pair.h: + - * / with
//     contraction off) on the host's f64 inputs: cardinalities, C / N / zero / sum / union estimates and, for small HyperMinHash
//     pairs, the same collision_gemm_kernel cell sums.  So sim == sim_low == the host's similarity bit for bit, and d_lo and d_hi
//     are one distance -/+ filter_margin, which covers the two sides' libm call on the same frac.
//   HLL linear counting, m ln(m / zero), is the exception: it calls log.  ocml's f64 log is within 1 ulp and glibc's within 1 ulp,
//     so the union estimates differ by at most 2 ulp (2^-51 relative).  pair_similarity_dev gives sim from the union shrunk by
//     2^-44 (128x that: never below the host's similarity) and sim_low from the union grown by 2^-44 (never above it), and refuses
//     an estimate within 2^-40 of the linear-counting threshold (the host may fall on the other side) like the whole bias-table
//     regime.  The distance decreases as the similarity grows, so the host's d lies in [d(sim) - margin, d(sim_low) + margin].
//   Cap.  The host's d never exceeds 1 (min(.., 1); 1 - f^(1/k) with f >= 0): d_hi = min(.., 1).
//   PAIR_ONE.  sim <= 0 means the host's similarity, never above sim, is <= 0 as well, and then d = 1.0 exactly on both sides, both
//     models, f64 and f32: no margin.  *d_lo = *d_hi = 1.
//   Containment (a.measure != MEASURE_JACCARD, CONTAIN = true; a_r / a_q: the pair's cardinalities as pair_similarity_dev read them).
//     near and far come from the rule of dist_pair.h that the host runs, distance_from_similarity(.., measure, a_r, a_q).  The
//     similarity-to-fraction step stays bit-identical: its extra + * / are the host's operations, contraction off, on the host's
//     doubles (the cardinalities in HBM are the host's).  For fixed cardinalities frac_c = s/(1+s) * (a_r + a_q) / den does not
//     decrease as s grows (up to the few ulp by which a rounded quotient of two growing numbers may, as 2s/(1+s) itself: 2^-50
//     against the 2^-44 the two similarities are apart and the 2^-40 of the margin), so the HLL linear-counting argument
//     [d(sim) - margin, d(sim_low) + margin] holds as it stands.  frac_c >= 1 gives exactly 0 on both sides, which only narrows
//     the interval.  PAIR_ONE is decided before the ratio is formed, so it stays true whatever the cardinalities are (0 and
//     NaN included).  The margin is unchanged: the same libm calls on the same fraction.
//   PAIR_NAN.  A NaN distance.  hmh / ull similarities are bit-identical and NaN goes through log / pow alike on both sides: the
//     host's d is NaN too, which no filter keeps, ranks or links.  Under hll the host decides: the pair is sent back.
enum { PAIR_INTERVAL, PAIR_ONE, PAIR_NAN };
template <bool CONTAIN = false>
__device__ inline int pair_interval_dev(const WithinArgs &a, double sim, double sim_low, double *d_lo, double *d_hi, double a_r = 0.0, double a_q = 0.0)
{
    *d_lo = *d_hi = 1.0;
    if (sim <= 0.0) return PAIR_ONE;
    const bool ull = a.algo == LASH_ULL;
    const double margin = filter_margin(a.fp32 != 0);
    double near, far;
    if constexpr (CONTAIN) {
        near = pairmath::distance_from_similarity(sim, ull, a.k, a.model, a.fp32 != 0, a.measure, a_r, a_q);
        far = sim_low == sim ? near : pairmath::distance_from_similarity(sim_low, ull, a.k, a.model, a.fp32 != 0, a.measure, a_r, a_q);
    } else {
        near = pairmath::distance_from_similarity(sim, ull, a.k, a.model, a.fp32 != 0);
        far = sim_low == sim ? near : pairmath::distance_from_similarity(sim_low, ull, a.k, a.model, a.fp32 != 0);   // (hll only)
    }
    if (near != near || far != far) return PAIR_NAN;
    *d_lo = near - margin;
    *d_hi = fmin(far + margin, 1.0);
    return PAIR_INTERVAL;
}

// The tile loop of the three mark kernels (256 threads; grid mark_grid(n_tiles), any smaller grid works).  A workgroup owns a tile of
// WF_TILE consecutive columns of one block row, tiles in row-major order; each wave takes 64 pairs at a time (step s of wave w:
// mask word s * 4 + w) and calls keep(r, q) for the printed ones, q < row_end(r), possibly with some lanes off.
// The layout within_scan_kernel / within_write_kernel (dist_filter.hip) read, stated here and nowhere else:
//   mask[tile * WF_WORDS + word]   bit l set iff pair (r, c0 + word * 64 + l) is a candidate, r = tile / tiles_x,
//                                  c0 = tile % tiles_x * WF_TILE; every word of a tile that starts before its row's end is written
//   tile_count[tile]               the tile's set bits; 0 for a tile wholly above the diagonal, whose mask words are NOT written
template <class Keep>
__device__ __forceinline__ void mark_tiles(const WithinArgs &a, uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count, Keep &&keep)
{
    __shared__ uint32_t wsum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const uint32_t r = (uint32_t)(tile / a.tiles_x), c0 = (uint32_t)(tile % a.tiles_x) * WF_TILE, c_end = row_end(a, r);
        if (c0 >= c_end) {                                                              // wholly above the diagonal
            if (threadIdx.x == 0) tile_count[tile] = 0;
            continue;
        }
        uint32_t cnt = 0;
        for (uint32_t step = 0; step < 4; ++step) {
            const uint32_t word = step * 4u + wave, q = c0 + word * 64u + lane;
            const uint64_t bits = __ballot(q < c_end && keep(r, q));
            if (lane == 0) mask[tile * WF_WORDS + word] = bits;
            cnt += (uint32_t)__popcll(bits);
        }
        if (lane == 0) wsum[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) tile_count[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

inline uint32_t mark_grid(uint64_t n_tiles) { return (uint32_t)std::min<uint64_t>(n_tiles, 1u << 20); }

// the block's WithinArgs from its statistics in HBM (d_c / d_n / d_u as lash_sketch_set_pair_block_device wrote them)
WithinArgs within_args(const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                       int model, int fp32, const uint32_t *d_c, const uint32_t *d_n, const double *d_u, const EcBlock &eb);

// One block of a filtered `lash dist` run, ready for a mark kernel: the pair statistics [sum_or_union f64 | c_or_zero u32 | n u32] (as
// lash_sketch_set_pair_block) and, for hmh, the small pairs' cell sums in HBM, the WithinArgs over them (a.limit is the caller's), and
// the compaction scratch [offsets u64 (n_tiles + 1) | mask u64 (n_tiles * WF_WORDS) | counts u32 (n_tiles)].  Queued on the context's
// stream.  within_block is what the three ABI entries do first: the argument checks they share (LASH_EINVAL), hipSetDevice, the pair
// kernels and the expected-collision GEMM.  LASH_OK with b.a.n_tiles == 0: an empty block, the entry returns LASH_OK at once.
struct WithinBlock {
    WithinArgs a;
    uint64_t *d_off, *d_mask;
    uint32_t *d_cnt;
};
int within_block(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                 int model, int fp32, int ull_estimator, WithinBlock &b, int measure = pairmath::MEASURE_JACCARD);

// compaction: mask words [n_tiles][WF_WORDS] of candidates and their per-tile counts -> exclusive offsets (d_off: n_tiles + 1) -> the
// candidates with their statistics in (row, col) order, copied back into `cand` (synchronous; dist_filter.hip's scan and write kernels)
int within_compact(lash_ctx *ctx, const WithinArgs &a, const uint64_t *d_mask, const uint32_t *d_cnt, uint64_t *d_off, std::vector<WithinPair> &cand);

// exact: one candidate of the block whose first row is r0 through the host arithmetic of lash_dist_rows.  false: that arithmetic
// refuses the pair (the HLL++ bias-table regime without tables) and *d is not set.
inline bool filter_pair_host(const WithinPair &w, const lash_sketch_set *ref, uint32_t r0, const lash_sketch_set *qry, int k, int model, int fp32,
                             const lash_hll_bias *tables, double *d, int measure = pairmath::MEASURE_JACCARD)
{
    const int algo = ref->algo;
    double ec;
    const double *ecp = nullptr;
    if (algo == LASH_HMH && !std::isnan(w.ec_x)) { ec = hmh_ec_from_cell_sum(w.ec_x); ecp = &ec; }
    return dist_pair_host(algo, ref->p, k, model, fp32, ref->card[r0 + w.row], qry->card[w.col], w.c_or_zero, w.n, w.sum_or_union, tables, ecp, d, measure);
}

// exact: the candidates in order (row-major) through filter_pair_host, each handed to each(set row, col, d, block row).  LASH_ERANGE
// at the first pair that arithmetic refuses (the one an unfiltered run reports), with *bad_pair = its place in the block; the pairs
// before it have been handed over.
template <class Each>
int filter_evaluate(const std::vector<WithinPair> &cand, const lash_sketch_set *ref, uint32_t r0, const lash_sketch_set *qry, uint32_t n_cols, int k,
                    int model, int fp32, const lash_hll_bias *tables, uint64_t *bad_pair, Each each, int measure = pairmath::MEASURE_JACCARD)
{
    for (const WithinPair &w : cand) {
        double d;
        if (!filter_pair_host(w, ref, r0, qry, k, model, fp32, tables, &d, measure)) {
            if (bad_pair) *bad_pair = (uint64_t)w.row * n_cols + w.col;
            return LASH_ERANGE;
        }
        each(r0 + w.row, w.col, d, w.row);
    }
    return LASH_OK;
}

// the rows an entry keeps: the first `cap` are stored, all are counted
struct KeptRows {
    uint32_t *row, *col;
    double *dist;
    uint64_t cap, n;
    void add(uint32_t r, uint32_t c, double d) { if (n < cap) { row[n] = r; col[n] = c; dist[n] = d; } ++n; }
};

}  // namespace lash
