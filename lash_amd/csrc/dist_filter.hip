// dist_filter.hip — `lash dist --max-dist D`: the pairs of a block whose distance can be <= D, found and compacted on the GPU while
// the block's pair statistics are still in HBM, so that only they come back to the host (include/lash_gfx950.h:
// lash_sketch_set_pair_block_within).  An all-vs-all of 10^5 sketches is 5 * 10^9 pairs; printing all of them is ~250 GB of text
// bound by the host, a cutoff keeps a few per row.
//
// Two passes over a block of rows [r0, r1) x columns [0, n_cols), row-major:
//   mark   a workgroup owns a tile of WF_TILE consecutive columns of one row (tiles in row-major order); each wave evaluates
//          64 pairs at a time, __ballot()s the candidates into one 64-bit mask word and the workgroup writes its count.
//          Triangle blocks: tiles that start beyond the row's diagonal write 0 and return (as the pair kernels skip them).
//   scan   one workgroup turns the per-tile counts into exclusive offsets (plain sums in a fixed order: deterministic).
//   write  every candidate lands at its tile's offset + the mask bits below it (v_mbcnt), so the output is row-major whatever
//          order the workgroups run in.  No atomics.
// A candidate is written with its statistics (and, for small HyperMinHash pairs, the expected-collision cell sum), and the host
// evaluates it exactly with the code lash_dist_rows runs: the kernel only has to be sure not to miss a pair.
//
// Why "d_dev <= D + margin" cannot miss one: the host's d is never below the device's distance of pair_similarity_dev's similarity
// minus filter_margin (dist_filter.h, above pair_interval_dev, whose lower end this is), and a pair the device cannot place is a
// candidate outright.  NaN distances (ull, two empty sketches, model 0) are candidates too; the host drops them (NaN never passes).
#include "dist_filter.h"

namespace lash {

// CONTAIN: a.measure is a containment (--containment): the distance of the same similarity under that measure, from the pair's two
// cardinalities.  The Jaccard instantiation is the kernel as it was.
template <bool CONTAIN>
__global__ void __launch_bounds__(256) within_mark_kernel(WithinArgs a, uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count)
{
    mark_tiles(a, mask, tile_count, [&](uint32_t r, uint32_t q) {
        double sim, sim_low;
        if (!pair_similarity_dev(a, r, q, &sim, &sim_low)) return true;
        if constexpr (CONTAIN)
            return !(pairmath::distance_from_similarity(sim, a.algo == LASH_ULL, a.k, a.model, a.fp32 != 0, a.measure, a.row_card[r], a.col_card[q]) > a.limit);
        else
            return !(pairmath::distance_from_similarity(sim, a.algo == LASH_ULL, a.k, a.model, a.fp32 != 0) > a.limit);   // (NaN: a candidate)
    });
}

// offsets[t] = sum of counts[0 .. t), offsets[n] = the total.  One workgroup: thread i sums a contiguous run of tiles, the 1024
// run sums are scanned in LDS, then every thread writes its run's offsets.
__global__ void __launch_bounds__(1024) within_scan_kernel(const uint32_t *__restrict__ counts, uint64_t n, uint64_t *__restrict__ offsets)
{
    __shared__ uint64_t part[1024];
    const uint64_t per = (n + 1023u) / 1024u, b = threadIdx.x * per, e = min(n, b + per);
    uint64_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {                                          // inclusive Hillis-Steele
        const uint64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t at = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; ++i) { offsets[i] = at; at += counts[i]; }
    if (threadIdx.x == 1023u) offsets[n] = part[1023];
}

__global__ void __launch_bounds__(256) within_write_kernel(WithinArgs a, const uint64_t *__restrict__ mask, const uint32_t *__restrict__ tile_count,
                                                           const uint64_t *__restrict__ offsets, WithinPair *__restrict__ out)
{
    __shared__ uint32_t before[WF_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        if (tile_count[tile] == 0) continue;                                            // (uniform across the workgroup)
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < WF_WORDS; ++w) { before[w] = s; s += (uint32_t)__popcll(mask[tile * WF_WORDS + w]); }
        }
        __syncthreads();
        const uint32_t r = (uint32_t)(tile / a.tiles_x), c0 = (uint32_t)(tile % a.tiles_x) * WF_TILE;
        const uint64_t base = offsets[tile];
        for (uint32_t step = 0; step < 4; ++step) {
            const uint32_t word = step * 4u + wave;
            const uint64_t bits = mask[tile * WF_WORDS + word];
            if (!((bits >> lane) & 1u)) continue;
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bits, 0u));
            const uint32_t q = c0 + word * 64u + lane;
            const uint64_t at = (uint64_t)r * a.n_cols + q;
            WithinPair w;
            w.row = r;
            w.col = q;
            w.c_or_zero = a.c_or_zero ? a.c_or_zero[at] : 0u;
            w.n = a.n_counts ? a.n_counts[at] : 0u;
            w.sum_or_union = a.sum_or_union ? a.sum_or_union[at] : 0.0;
            w.ec_x = __builtin_nan("");
            if (a.algo == LASH_HMH && a.nrs) {
                const int32_t rs = a.row_small[r], cs = a.col_small[q];
                if (rs >= 0 && cs >= 0) w.ec_x = a.X[small_cell(a, rs, cs)];
            }
            out[base + before[word] + below] = w;
        }
        __syncthreads();
    }
}

WithinArgs within_args(const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                       int model, int fp32, const uint32_t *d_c, const uint32_t *d_n, const double *d_u, const EcBlock &eb)
{
    const int algo = ref->algo;
    const uint32_t nr = r1 - r0;
    WithinArgs a{};
    a.algo = algo; a.p = ref->p; a.k = k; a.model = model; a.fp32 = fp32 ? 1 : 0;
    a.limit = 0.0;                                                                     // (the caller's)
    a.nr = nr; a.n_cols = n_cols;
    a.tiles_x = (n_cols + WF_TILE - 1) / WF_TILE;
    a.n_tiles = (uint64_t)nr * a.tiles_x;
    a.tri = triangle ? (int64_t)r0 : -1;
    a.row_card = static_cast<const double *>(ref->d_card.ptr) + r0;
    a.col_card = static_cast<const double *>(qry->d_card.ptr);
    a.c_or_zero = algo == LASH_ULL ? nullptr : d_c;
    a.n_counts = algo == LASH_HMH ? d_n : nullptr;
    a.sum_or_union = algo == LASH_HMH ? nullptr : d_u;
    a.row_small = static_cast<const int32_t *>(ref->d_small.ptr) + r0;
    a.col_small = static_cast<const int32_t *>(qry->d_small.ptr);
    a.X = eb.X; a.nrs = eb.nrs; a.q_step = eb.q_step; a.nqs = eb.nqs; a.rbase = eb.rbase;
    if (eb.nqs == 0) a.nrs = 0;
    return a;
}

int within_block(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols, int triangle, int k,
                 int model, int fp32, int ull_estimator, WithinBlock &b, int measure)
{
    b = WithinBlock{};
    if (measure < pairmath::MEASURE_JACCARD || measure > pairmath::MEASURE_CONTAIN_REFERENCE) return LASH_EINVAL;
    if (measure != pairmath::MEASURE_JACCARD && triangle) return LASH_EINVAL;                   // directional: no triangle
    if (!ctx || !ref || !qry || r0 > r1 || r1 > ref->n || n_cols > qry->n || k < 1 || k > 32 || (model != 0 && model != 1)) return LASH_EINVAL;
    if (ref->card.size() != ref->n || qry->card.size() != qry->n) return LASH_EINVAL;          // lash_sketch_set_cardinalities first
    if (r0 == r1 || n_cols == 0) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    int rc;
    const uint64_t np = (uint64_t)(r1 - r0) * n_cols;
    if ((rc = reserve(ctx, ctx->st_img, np * 16 + 64))) return rc;
    double *d_u = static_cast<double *>(ctx->st_img.ptr);
    uint32_t *d_c = reinterpret_cast<uint32_t *>(d_u + np), *d_n = d_c + np;
    if ((rc = lash_sketch_set_pair_block_device(ctx, ref, r0, r1, qry, n_cols, triangle, ull_estimator, d_c, d_n, d_u))) return rc;
    EcBlock eb;
    if (ref->algo == LASH_HMH && (rc = lash_set_ec_block(ctx, ref, r0, r1, qry, n_cols, eb))) return rc;
    b.a = within_args(ref, r0, r1, qry, n_cols, triangle, k, model, fp32, d_c, d_n, d_u, eb);
    b.a.measure = measure;
    const uint64_t nt = b.a.n_tiles;
    if ((rc = reserve(ctx, ctx->wf_scratch, (nt + 1) * 8 + nt * WF_WORDS * 8 + nt * 4 + 64))) return rc;
    b.d_off = static_cast<uint64_t *>(ctx->wf_scratch.ptr);
    b.d_mask = b.d_off + nt + 1;
    b.d_cnt = reinterpret_cast<uint32_t *>(b.d_mask + nt * WF_WORDS);
    return LASH_OK;
}

int within_compact(lash_ctx *ctx, const WithinArgs &a, const uint64_t *d_mask, const uint32_t *d_cnt, uint64_t *d_off, std::vector<WithinPair> &cand)
{
    int rc;
    const uint64_t nt = a.n_tiles;
    hipLaunchKernelGGL(within_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_cnt, nt, d_off);
    HIPCHK(ctx, hipGetLastError());
    uint64_t n_cand = 0;
    HIPCHK(ctx, hipMemcpyAsync(&n_cand, d_off + nt, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    cand.resize(n_cand);
    if (n_cand) {
        if ((rc = reserve(ctx, ctx->wf_out, n_cand * sizeof(WithinPair)))) return rc;
        WithinPair *d_out = static_cast<WithinPair *>(ctx->wf_out.ptr);
        hipLaunchKernelGGL(within_write_kernel, dim3(mark_grid(nt)), dim3(256), 0, ctx->stream, a, d_mask, d_cnt, d_off, d_out);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(cand.data(), d_out, n_cand * sizeof(WithinPair), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return LASH_OK;
}

}  // namespace lash

extern "C" {

int lash_sketch_set_pair_block_within(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                      uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables,
                                      double max_dist, uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap, uint64_t *n_kept,
                                      uint64_t *bad_pair, uint64_t *n_candidates)
{
    return lash_sketch_set_pair_block_within_measure(ctx, ref, r0, r1, qry, n_cols, triangle, k, model, fp32, ull_estimator, tables, LASH_MEASURE_JACCARD,
                                                     max_dist, out_row, out_col, out_dist, cap, n_kept, bad_pair, n_candidates);
}

int lash_sketch_set_pair_block_within_measure(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                              uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables,
                                              int measure, double max_dist, uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap,
                                              uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates)
{
    using namespace lash;
    if (n_kept) *n_kept = 0;
    if (n_candidates) *n_candidates = 0;
    if (!n_kept || std::isnan(max_dist) || (cap && (!out_row || !out_col || !out_dist))) return LASH_EINVAL;
    int rc;
    WithinBlock b;
    if ((rc = within_block(ctx, ref, r0, r1, qry, n_cols, triangle, k, model, fp32, ull_estimator, b, measure)) || !b.a.n_tiles) return rc;
    b.a.limit = max_dist + filter_margin(fp32 != 0);
    if (measure == LASH_MEASURE_JACCARD)
        hipLaunchKernelGGL(within_mark_kernel<false>, dim3(mark_grid(b.a.n_tiles)), dim3(256), 0, ctx->stream, b.a, b.d_mask, b.d_cnt);
    else
        hipLaunchKernelGGL(within_mark_kernel<true>, dim3(mark_grid(b.a.n_tiles)), dim3(256), 0, ctx->stream, b.a, b.d_mask, b.d_cnt);
    HIPCHK(ctx, hipGetLastError());
    std::vector<WithinPair> cand;
    if ((rc = within_compact(ctx, b.a, b.d_mask, b.d_cnt, b.d_off, cand))) return rc;
    if (n_candidates) *n_candidates = cand.size();
    KeptRows kept{out_row, out_col, out_dist, cap, 0};
    rc = filter_evaluate(cand, ref, r0, qry, n_cols, k, model, fp32, tables, bad_pair, [&](uint32_t row, uint32_t col, double d, uint32_t) {
        if (d <= max_dist) kept.add(row, col, d);
    }, measure);
    *n_kept = kept.n;
    return rc;
}

}  // extern "C"
