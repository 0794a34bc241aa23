// dist_top.hip — `lash dist --top K`: per name, the K pairs of smallest distance, selected on the GPU while a block's pair statistics
// are still in HBM, so that only the pairs that can still be among some name's K nearest come back to the host
// (include/lash_gfx950.h: lash_sketch_set_pair_block_top).  The host evaluates each one exactly with the code lash_dist_rows runs and
// keeps per-name lists (lash_top_*, at the end of this file); the kernels only have to be sure not to miss a pair.
//
// Rank.  A pair's key is (d, row, col): its printed distance (the "same name -> 0" rule applied), then its position in the unfiltered
// output.  N_K(X) = the K smallest keys among the pairs that involve name X: a column (query) of a rectangular run, a row or a column
// of a triangle run.  NaN is never ranked.
//
// Passes over a block of rows [r0, r1) x columns [0, n_cols):
//   key      per pair the interval [lo, hi] of pair_interval_dev (dist_filter.h), which holds the host's exact d, as two
//            order-preserving 32-bit keys (hi rounded up, lo rounded down to float, so that the interval only widens).  EXACT pairs
//            have lo = hi = d and an even hi key (general pairs: odd, key | 1, which only rounds up): PAIR_ONE (d = 1.0), and the
//            row's same-name column (same_col) -> d = 0 (printed 0), still sent to the host, which must see it for LASH_ERANGE.
//            Pairs the device cannot place take no part in the selection and are always candidates.  PAIR_NAN: never a candidate
//            for hmh / ull, always one under HLL.
//   select   per column (and, in a triangle block, per row) the K-th smallest hi key Tk over the block: a radix select, four 8-bit
//            digits, histograms in LDS.  If Tk is odd, T = (decode(Tk), +inf, +inf); if it is even (exact), T = (decode(Tk), the
//            position of the rank-th pair with that key).  Fewer than K placed pairs: T = +inf.
//   combine  T = min(T_col, the caller's bound for the column's name); in a triangle block also min with the row's T and bound of
//            the same name (rows and columns are the same names there).
//   mark     a pair is a candidate iff it passes the T of its column or (triangle) of its row: an exact pair iff (d, row, col) <= T, a
//            general one iff lo <= T.d.  With max_dist, also lo <= D.  Then the scan / write compaction of dist_filter.hip.
//
// Why it cannot miss a pair of N_K(X).  The K pairs whose hi keys are <= Tk have d <= decode(Tk): those with a smaller key have
// d < decode(Tk) (keys are monotone, and no odd key decodes to 0 or 1, the only exact values, because -0 is stored as +0); those
// with key == Tk, when it is even, are exact at d = decode(Tk) and the rank-th of them in position order sits at T's position.  So K
// pairs of X have keys <= T, the K-th key of N_K(X) is <= T, and every pair of N_K(X) has key <= T: its lo <= d <= T.d, and if it is
// exact its own key is (d, position) <= T.  A T taken over a SUBSET of X's pairs (one block; only the row or only the column part
// of X in a triangle block; the caller's list from earlier blocks) is never below the true K-th key, so it is still a sound bound,
// and so is the smaller of two.  With max_dist, N_K(X) is ranked by d, so "the K nearest, then d <= D" needs nothing more.
#include "dist_filter.h"

#include <algorithm>
#include <new>

namespace lash {

namespace {

constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;        // hi: takes no part in the selection
constexpr uint32_t LO_ALWAYS = 0u;                // lo: always a candidate
constexpr uint32_t LO_NEVER = 0xFFFFFFFFu;        // lo: never a candidate
constexpr uint32_t POS_NONE = 0xFFFFFFFFu;

struct TopKey {                                   // = lash_top_key
    double d;
    uint32_t row, col;
};

__host__ __device__ inline bool key_less(const TopKey &a, const TopKey &b)
{
    if (a.d != b.d) return a.d < b.d;
    return a.row != b.row ? a.row < b.row : a.col < b.col;
}

__device__ inline TopKey key_min(const TopKey &a, const TopKey &b) { return key_less(b, a) ? b : a; }

__device__ inline uint32_t ord(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ inline float float_up(double x)
{
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, __builtin_huge_valf());
    return f;
}

__device__ inline float float_down(double x)
{
    float f = (float)x;
    if ((double)f > x) f = nextafterf(f, -__builtin_huge_valf());
    return f;
}

}  // namespace

struct TopArgs {
    const uint32_t *same_col;                     // [nr] or null
    uint32_t *hi, *lo;                            // [nr][n_cols]
    const TopKey *fc, *fr;                        // combined cutoffs: [n_cols], [nr] (triangle)
    double max_dist;                              // NaN: none
    uint32_t r0;
};

// CONTAIN: a.measure is a containment (--containment; rectangles only): the interval under that measure, from the pair's two
// cardinalities.  The Jaccard instantiation is the kernel as it was.
template <bool CONTAIN>
__global__ void __launch_bounds__(256) top_key_kernel(WithinArgs a, TopArgs t)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.n_cols) return;
    for (uint32_t r = blockIdx.y; r < a.nr; r += gridDim.y) {
        const uint64_t at = (uint64_t)r * a.n_cols + q;
        uint32_t hi, lo;
        double sim, sim_low, d_lo, d_hi;
        if (q >= row_end(a, r)) { hi = KEY_NONE; lo = LO_NEVER; }                       // above the diagonal: not printed
        else if (t.same_col && t.same_col[r] == q) { hi = ord(0.0f); lo = LO_ALWAYS; }   // prints 0; the host still evaluates it
        else if (!pair_similarity_dev(a, r, q, &sim, &sim_low)) { hi = KEY_NONE; lo = LO_ALWAYS; }
        else switch (CONTAIN ? pair_interval_dev<true>(a, sim, sim_low, &d_lo, &d_hi, a.row_card[r], a.col_card[q])
                             : pair_interval_dev<false>(a, sim, sim_low, &d_lo, &d_hi)) {
        case PAIR_ONE: hi = lo = ord(1.0f); break;                                      // exact
        case PAIR_NAN: hi = KEY_NONE; lo = a.algo == LASH_HLL ? LO_ALWAYS : LO_NEVER; break;
        default: {
            float h = float_up(d_hi);
            if (h == 0.0f) h = 0.0f;                                                    // -0 -> +0: no odd key decodes to 0
            hi = ord(h) | 1u;
            lo = ord(float_down(d_lo));
        }
        }
        t.hi[at] = hi;
        t.lo[at] = lo;
    }
}

// One workgroup per 64 columns: lane = column (each row's 64 keys are one coalesced 256-byte read), the 8 waves take every 8th row.
// Histograms [256 digits][64 columns] in LDS (64 KB): the lanes of a wave hit 64 different words whatever their digits.
constexpr uint32_t SEL_COLS = 64, SEL_WAVES = 8;

__global__ void __launch_bounds__(512) top_col_select_kernel(const uint32_t *__restrict__ hi, uint32_t nr, uint32_t n_cols, uint32_t top_k,
                                                             uint32_t r0, TopKey *__restrict__ tc)
{
    __shared__ uint32_t hist[256 * SEL_COLS];
    __shared__ uint32_t prefix[SEL_COLS], krem[SEL_COLS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = blockIdx.x * SEL_COLS + lane;
    const bool valid = c < n_cols;
    TopKey t{__builtin_huge_val(), POS_NONE, POS_NONE};
    if (nr < top_k) {                                                                   // fewer than K pairs in every column
        if (wave == 0 && valid) tc[c] = t;
        return;
    }
    if (threadIdx.x < SEL_COLS) { prefix[lane] = 0; krem[lane] = top_k; }
    for (uint32_t pass = 0; pass < 4; ++pass) {
        const uint32_t shift = 24u - 8u * pass, himask = pass ? ~0u << (shift + 8u) : 0u;
        for (uint32_t i = threadIdx.x; i < 256u * SEL_COLS; i += 64u * SEL_WAVES) hist[i] = 0;
        __syncthreads();
        const uint32_t pf = prefix[lane];
        if (valid) {
#pragma unroll 4
            for (uint32_t r = wave; r < nr; r += SEL_WAVES) {
                const uint32_t key = hi[(uint64_t)r * n_cols + c];
                if ((key & himask) == pf) atomicAdd(&hist[((key >> shift) & 255u) * SEL_COLS + lane], 1u);
            }
        }
        __syncthreads();
        if (wave == 0 && valid) {                                                       // the digit that holds the rank-th key
            const uint32_t kr = krem[lane];
            uint32_t cum = 0;
            for (uint32_t b = 0; b < 256u; ++b) {
                const uint32_t h = hist[b * SEL_COLS + lane];
                if (cum + h >= kr) { prefix[lane] = pf | (b << shift); krem[lane] = kr - cum; break; }
                cum += h;
            }
        }
        __syncthreads();
    }
    if (wave != 0 || !valid) return;
    const uint32_t tk = prefix[lane], kr = krem[lane];
    if (tk != KEY_NONE) {
        t.d = unord(tk);
        if (!(tk & 1u)) {                                                               // exact: the kr-th pair of that key, by row
            uint32_t seen = 0;
            for (uint32_t r = 0; r < nr; ++r)
                if (hi[(uint64_t)r * n_cols + c] == tk && ++seen == kr) { t.row = r0 + r; t.col = c; break; }
        }
    }
    tc[c] = t;
}

// Triangle blocks: one workgroup per row over its printed columns (contiguous keys), a 256-bin histogram per digit.
__global__ void __launch_bounds__(256) top_row_select_kernel(const uint32_t *__restrict__ hi, uint32_t nr, uint32_t n_cols, uint32_t top_k,
                                                             uint32_t r0, TopKey *__restrict__ tr)
{
    __shared__ uint32_t hist[256];
    __shared__ uint64_t wmask[4];
    __shared__ uint32_t s_prefix, s_krem, s_found;
    const uint32_t r = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = (uint64_t)r0 + r + 1;
    const uint32_t n = e < n_cols ? (uint32_t)e : n_cols;
    const uint32_t *row = hi + (uint64_t)r * n_cols;
    TopKey t{__builtin_huge_val(), POS_NONE, POS_NONE};
    if (n < top_k) {
        if (threadIdx.x == 0) tr[r] = t;
        return;
    }
    if (threadIdx.x == 0) { s_prefix = 0; s_krem = top_k; }
    for (uint32_t pass = 0; pass < 4; ++pass) {
        const uint32_t shift = 24u - 8u * pass, himask = pass ? ~0u << (shift + 8u) : 0u;
        hist[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t pf = s_prefix;
        for (uint32_t q = threadIdx.x; q < n; q += 256u) {
            const uint32_t key = row[q];
            if ((key & himask) == pf) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t kr = s_krem;
            uint32_t cum = 0;
            for (uint32_t b = 0; b < 256u; ++b) {
                if (cum + hist[b] >= kr) { s_prefix = pf | (b << shift); s_krem = kr - cum; break; }
                cum += hist[b];
            }
        }
        __syncthreads();
    }
    const uint32_t tk = s_prefix, kr = s_krem;
    if (tk == KEY_NONE) {
        if (threadIdx.x == 0) tr[r] = t;
        return;
    }
    t.d = unord(tk);
    if (tk & 1u) {
        if (threadIdx.x == 0) tr[r] = t;
        return;
    }
    // exact: the kr-th column of that key, 256 columns at a time
    uint32_t seen = 0;                                                                  // (thread 0's)
    for (uint32_t q0 = 0; q0 < n; q0 += 256u) {
        const uint32_t q = q0 + threadIdx.x;
        const uint64_t bits = __ballot(q < n && row[q] == tk);
        if (lane == 0) wmask[wave] = bits;
        if (threadIdx.x == 0) s_found = POS_NONE;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t w = 0; w < 4; ++w) {
                uint64_t m = wmask[w];
                const uint32_t cnt = (uint32_t)__popcll(m);
                if (seen + cnt >= kr) {
                    for (uint32_t j = seen + 1; j < kr; ++j) m &= m - 1;
                    s_found = q0 + w * 64u + (uint32_t)(__ffsll((long long)m) - 1);
                    break;
                }
                seen += cnt;
            }
        }
        __syncthreads();
        if (s_found != POS_NONE) break;                                                 // (uniform)
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        t.row = r0 + r;
        t.col = s_found;
        tr[r] = t;
    }
}

__global__ void __launch_bounds__(256) top_combine_kernel(const TopKey *__restrict__ tc, const TopKey *__restrict__ tr, const TopKey *__restrict__ col_bound,
                                                          const TopKey *__restrict__ row_bound, uint32_t nr, uint32_t n_cols, uint32_t r0, int tri,
                                                          TopKey *__restrict__ fc, TopKey *__restrict__ fr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_cols) {
        TopKey t = tc[i];
        if (col_bound) t = key_min(t, col_bound[i]);
        if (tri && i >= r0 && i - r0 < nr) {                                             // the same name's row in this block
            t = key_min(t, tr[i - r0]);
            if (row_bound) t = key_min(t, row_bound[i - r0]);
        }
        fc[i] = t;
    }
    if (tri && i < nr) {
        TopKey t = tr[i];
        if (row_bound) t = key_min(t, row_bound[i]);
        if (r0 + i < n_cols) {
            t = key_min(t, tc[r0 + i]);
            if (col_bound) t = key_min(t, col_bound[r0 + i]);
        }
        fr[i] = t;
    }
}

__device__ inline bool top_pass(uint32_t hi, uint32_t lo, uint32_t row, uint32_t col, const TopKey &t)
{
    if (hi & 1u) return (double)unord(lo) <= t.d;                                       // general: lo <= T.d
    const double d = unord(hi);                                                         // exact: (d, row, col) <= T
    return d < t.d || (d == t.d && (row < t.row || (row == t.row && col <= t.col)));
}

__global__ void __launch_bounds__(256) top_mark_kernel(WithinArgs a, TopArgs t, uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count)
{
    mark_tiles(a, mask, tile_count, [&](uint32_t r, uint32_t q) {
        const uint64_t at = (uint64_t)r * a.n_cols + q;
        const uint32_t lo = t.lo[at];
        if (lo == LO_ALWAYS) return true;
        if (lo == LO_NEVER) return false;
        const uint32_t hi = t.hi[at];
        if (!(t.max_dist != t.max_dist) && !((double)unord((hi & 1u) ? lo : hi) <= t.max_dist)) return false;
        return top_pass(hi, lo, t.r0 + r, q, t.fc[q]) || (a.tri >= 0 && top_pass(hi, lo, t.r0 + r, q, t.fr[r]));
    });
}

}  // namespace lash

// ---- the host accumulator: per name, the K smallest (d, row, col) keys seen so far -------------------------------------------------

struct lash_top {
    uint32_t n_names = 0, k = 0;
    bool triangle = false;
    std::vector<std::vector<lash::TopKey>> list;   // per name; trimmed to its K smallest whenever it reaches 2K
    std::vector<lash::TopKey> cut;                 // per name: the K-th key at the last trim (+inf: fewer than K seen)
};

namespace {

using lash::TopKey;

void trim(lash_top *t, uint32_t x)
{
    std::vector<TopKey> &l = t->list[x];
    if (l.size() < t->k) return;
    std::nth_element(l.begin(), l.begin() + (t->k - 1), l.end(), lash::key_less);
    l.resize(t->k);
    t->cut[x] = *std::max_element(l.begin(), l.end(), lash::key_less);
}

void push(lash_top *t, uint32_t x, const TopKey &e)
{
    if (lash::key_less(t->cut[x], e)) return;                                          // (beyond K keys already held)
    t->list[x].push_back(e);
    if (t->list[x].size() >= 2 * (size_t)t->k) trim(t, x);
}

TopKey no_key() { return TopKey{HUGE_VAL, lash::POS_NONE, lash::POS_NONE}; }

}  // namespace

extern "C" {

int lash_sketch_set_pair_block_top(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols,
                                   int triangle, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables, uint32_t top_k,
                                   double max_dist, const uint32_t *same_col, const lash_top_key *col_bound, const lash_top_key *row_bound,
                                   uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap, uint64_t *n_kept, uint64_t *bad_pair,
                                   uint64_t *n_candidates)
{
    return lash_sketch_set_pair_block_top_measure(ctx, ref, r0, r1, qry, n_cols, triangle, k, model, fp32, ull_estimator, tables, LASH_MEASURE_JACCARD, top_k,
                                                  max_dist, same_col, col_bound, row_bound, out_row, out_col, out_dist, cap, n_kept, bad_pair, n_candidates);
}

int lash_sketch_set_pair_block_top_measure(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols,
                                           int triangle, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables, int measure,
                                           uint32_t top_k, double max_dist, const uint32_t *same_col, const lash_top_key *col_bound,
                                           const lash_top_key *row_bound, uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap,
                                           uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates)
{
    using namespace lash;
    static_assert(sizeof(TopKey) == sizeof(lash_top_key), "lash_top_key layout");
    if (n_kept) *n_kept = 0;
    if (n_candidates) *n_candidates = 0;
    if (!n_kept || top_k < 1 || top_k > LASH_TOP_MAX || (cap && (!out_row || !out_col || !out_dist))) return LASH_EINVAL;
    int rc;
    WithinBlock b;
    if ((rc = within_block(ctx, ref, r0, r1, qry, n_cols, triangle, k, model, fp32, ull_estimator, b, measure)) || !b.a.n_tiles) return rc;
    const WithinArgs &a = b.a;
    const uint32_t nr = r1 - r0;
    const uint64_t np = (uint64_t)nr * n_cols;

    // selection buffers: [hi u32 (np) | lo u32 (np) | tc, fc, col_bound (n_cols) | tr, fr, row_bound (nr) TopKey | same_col u32 (nr)]
    const uint64_t nk = 3 * (uint64_t)n_cols + 3 * (uint64_t)nr;
    if ((rc = reserve(ctx, ctx->top_buf, np * 8 + nk * sizeof(TopKey) + (uint64_t)nr * 4 + 64))) return rc;
    TopKey *d_keys = static_cast<TopKey *>(ctx->top_buf.ptr);
    TopKey *d_tc = d_keys, *d_fc = d_tc + n_cols, *d_cb = d_fc + n_cols, *d_tr = d_cb + n_cols, *d_fr = d_tr + nr, *d_rb = d_fr + nr;
    uint32_t *d_hi = reinterpret_cast<uint32_t *>(d_keys + nk), *d_lo = d_hi + np, *d_same = d_lo + np;
    if (col_bound) HIPCHK(ctx, hipMemcpyAsync(d_cb, col_bound, (size_t)n_cols * sizeof(TopKey), hipMemcpyHostToDevice, ctx->stream));
    if (triangle && row_bound) HIPCHK(ctx, hipMemcpyAsync(d_rb, row_bound, (size_t)nr * sizeof(TopKey), hipMemcpyHostToDevice, ctx->stream));
    if (same_col) HIPCHK(ctx, hipMemcpyAsync(d_same, same_col, (size_t)nr * 4, hipMemcpyHostToDevice, ctx->stream));

    TopArgs t{};
    t.same_col = same_col ? d_same : nullptr;
    t.hi = d_hi; t.lo = d_lo; t.fc = d_fc; t.fr = d_fr;
    t.max_dist = max_dist;
    t.r0 = r0;
    const uint32_t gx = (n_cols + 255) / 256;
    const dim3 key_grid(gx, std::min<uint32_t>({nr, 65535u, std::max<uint32_t>(1, (1u << 20) / gx)}));
    if (measure == LASH_MEASURE_JACCARD) hipLaunchKernelGGL(top_key_kernel<false>, key_grid, dim3(256), 0, ctx->stream, a, t);
    else hipLaunchKernelGGL(top_key_kernel<true>, key_grid, dim3(256), 0, ctx->stream, a, t);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(top_col_select_kernel, dim3((n_cols + SEL_COLS - 1) / SEL_COLS), dim3(64 * SEL_WAVES), 0, ctx->stream, d_hi, nr, n_cols,
                       top_k, r0, d_tc);
    HIPCHK(ctx, hipGetLastError());
    if (triangle) {
        hipLaunchKernelGGL(top_row_select_kernel, dim3(nr), dim3(256), 0, ctx->stream, d_hi, nr, n_cols, top_k, r0, d_tr);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(top_combine_kernel, dim3((std::max(n_cols, nr) + 255) / 256), dim3(256), 0, ctx->stream, d_tc, d_tr, col_bound ? d_cb : nullptr,
                       triangle && row_bound ? d_rb : nullptr, nr, n_cols, r0, triangle ? 1 : 0, d_fc, d_fr);
    HIPCHK(ctx, hipGetLastError());

    hipLaunchKernelGGL(top_mark_kernel, dim3(mark_grid(a.n_tiles)), dim3(256), 0, ctx->stream, a, t, b.d_mask, b.d_cnt);
    HIPCHK(ctx, hipGetLastError());
    std::vector<WithinPair> cand;
    if ((rc = within_compact(ctx, a, b.d_mask, b.d_cnt, b.d_off, cand))) return rc;
    if (n_candidates) *n_candidates = cand.size();

    // the same-name rule, NaN dropped, d <= max_dist
    KeptRows kept{out_row, out_col, out_dist, cap, 0};
    rc = filter_evaluate(cand, ref, r0, qry, n_cols, k, model, fp32, tables, bad_pair, [&](uint32_t row, uint32_t col, double d, uint32_t block_row) {
        if (same_col && same_col[block_row] == col) d = 0.0;
        if (!std::isnan(d) && (std::isnan(max_dist) || d <= max_dist)) kept.add(row, col, d);
    }, measure);
    *n_kept = kept.n;
    return rc;
}

int lash_top_create(uint32_t n_names, uint32_t top_k, int triangle, lash_top **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    if (top_k < 1 || top_k > LASH_TOP_MAX) return LASH_EINVAL;
    lash_top *t = new (std::nothrow) lash_top;
    if (!t) return LASH_ENOMEM;
    t->n_names = n_names;
    t->k = top_k;
    t->triangle = triangle != 0;
    t->list.resize(n_names);
    t->cut.assign(n_names, no_key());
    *out = t;
    return LASH_OK;
}

int lash_top_add(lash_top *t, const uint32_t *row, const uint32_t *col, const double *dist, uint64_t n)
{
    if (!t || (n && (!row || !col || !dist))) return LASH_EINVAL;
    for (uint64_t i = 0; i < n; ++i)
        if (col[i] >= t->n_names || (t->triangle && row[i] >= t->n_names) || std::isnan(dist[i])) return LASH_EINVAL;
    for (uint64_t i = 0; i < n; ++i) {
        const TopKey e{dist[i], row[i], col[i]};
        push(t, col[i], e);
        if (t->triangle && row[i] != col[i]) push(t, row[i], e);
    }
    return LASH_OK;
}

int lash_top_bounds(lash_top *t, uint32_t r0, uint32_t r1, uint32_t n_cols, lash_top_key *col_bound, lash_top_key *row_bound)
{
    if (!t || r0 > r1 || n_cols > t->n_names || (t->triangle && r1 > t->n_names)) return LASH_EINVAL;
    auto bound = [&](uint32_t x) {
        trim(t, x);
        const TopKey b = t->list[x].size() >= t->k ? t->cut[x] : no_key();
        return lash_top_key{b.d, b.row, b.col};
    };
    if (col_bound) for (uint32_t c = 0; c < n_cols; ++c) col_bound[c] = bound(c);
    if (row_bound) {
        for (uint32_t r = r0; r < r1; ++r) row_bound[r - r0] = t->triangle ? bound(r) : lash_top_key{HUGE_VAL, lash::POS_NONE, lash::POS_NONE};
    }
    return LASH_OK;
}

int lash_top_merge(lash_top *dst, const lash_top *src)
{
    if (!dst || !src || dst == src || dst->n_names != src->n_names || dst->k != src->k || dst->triangle != src->triangle) return LASH_EINVAL;
    for (uint32_t x = 0; x < src->n_names; ++x)
        for (const TopKey &e : src->list[x]) push(dst, x, e);
    return LASH_OK;
}

int lash_top_result(lash_top *t, uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap, uint64_t *n)
{
    if (!t || !n || (cap && (!out_row || !out_col || !out_dist))) return LASH_EINVAL;
    std::vector<TopKey> all;
    for (uint32_t x = 0; x < t->n_names; ++x) {
        trim(t, x);
        all.insert(all.end(), t->list[x].begin(), t->list[x].end());
    }
    std::sort(all.begin(), all.end(), [](const TopKey &a, const TopKey &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    all.erase(std::unique(all.begin(), all.end(), [](const TopKey &a, const TopKey &b) { return a.row == b.row && a.col == b.col; }), all.end());
    for (uint64_t i = 0; i < all.size() && i < cap; ++i) { out_row[i] = all[i].row; out_col[i] = all[i].col; out_dist[i] = all[i].d; }
    *n = all.size();
    return LASH_OK;
}

void lash_top_free(lash_top *t) { delete t; }

}  // extern "C"
