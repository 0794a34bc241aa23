// lash_dist_api.hip — the extern "C" entries on finished images: union of serialized sketches (Sketch::merge / HyperLogLog::union /
// UltraLogLog::merge as `lash dist` uses them, utils.rs:84-373) and the pair statistics of the all-vs-all drivers.  Split out of lash_api.hip in round 6.
#include "lash_ctx.h"
#include "lash_internal.h"

extern "C" {

int lash_merge_images_device(lash_ctx *ctx, int algo, int p, uint8_t *d_dst, const uint8_t *d_src, uint64_t n_images)
{
    if (!ctx || (n_images && (!d_dst || !d_src)) || n_images > 0x7FFFFFFFull) return LASH_EINVAL;
    lash_params prm{algo, 16, p, 0, 0};
    int rc = lash_params_check(&prm);
    if (rc) return rc;
    if (n_images == 0) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    // one pseudo work item per image: "partials" are the source images themselves (registers after the header)
    std::vector<WorkItem> items((size_t)n_images);
    std::vector<uint32_t> begin((size_t)n_images + 1);
    for (uint64_t i = 0; i < n_images; ++i) { items[i] = WorkItem{(uint32_t)i, 0, 0, 0}; begin[i] = (uint32_t)i; }
    begin[n_images] = (uint32_t)n_images;
    if ((rc = reserve(ctx, ctx->items, (size_t)(n_images + 1) * sizeof(WorkItem)))) return rc;
    if ((rc = reserve(ctx, ctx->item_begin, (size_t)(n_images + 1) * 4))) return rc;
    if ((rc = upload(ctx, ctx->items.ptr, items.data(), items.size() * sizeof(WorkItem)))) return rc;
    if ((rc = upload(ctx, ctx->item_begin.ptr, begin.data(), begin.size() * 4))) return rc;
    FinalizeArgs fa{};
    fa.partials = d_src;
    fa.items = static_cast<const WorkItem *>(ctx->items.ptr);
    fa.genome_item_begin = static_cast<const uint32_t *>(ctx->item_begin.ptr);
    fa.nvalid = nullptr;
    fa.images = d_dst;
    fa.image_bytes = image_bytes(ctx->layout, algo, p);
    fa.partial_stride = fa.image_bytes;
    fa.partial_base_off = header_bytes(ctx->layout, algo);
    fa.lay = layout_dev(ctx->layout, algo);
    fa.src_images = 1;
    const double alpha = hll_alpha(p);
    memcpy(&fa.alpha_bits, &alpha, 8);
    fa.algo = algo;
    fa.p = p;
    fa.k = 16;
    fa.accumulate = 1;
    HIPCHK(ctx, launch_finalize(fa, (uint32_t)n_images, ctx->stream));
    return LASH_OK;
}

int lash_merge_images(lash_ctx *ctx, int algo, int p, uint8_t *dst, const uint8_t *src, uint64_t n_images)
{
    if (!ctx || (n_images && (!dst || !src))) return LASH_EINVAL;
    const size_t ib = image_bytes(ctx->layout, algo, p);
    if (!ib) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    const size_t bytes = ib * (size_t)n_images;
    int rc;
    if ((rc = reserve(ctx, ctx->st_img, bytes + 64))) return rc;
    if ((rc = reserve(ctx, ctx->st_seq, bytes + 64))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_img.ptr, dst, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_seq.ptr, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = lash_merge_images_device(ctx, algo, p, static_cast<uint8_t *>(ctx->st_img.ptr),
                                  static_cast<const uint8_t *>(ctx->st_seq.ptr), n_images);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(dst, ctx->st_img.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

}  // extern "C"

namespace {

// The stand-alone pair entries run on the context's two call-scoped sets (sketch_set.hip holds all operand preparation): bind them
// to the call's images, prepare, one block of all rows against all columns.  Binding always invalidates: the host entries stage
// new contents at the address of the previous call.  One set serves both sides when the two image blocks are the same.
int pair_stats_device(lash_ctx *ctx, int algo, int p, int ull_estimator, const uint8_t *d_ref, uint32_t n_ref, const uint8_t *d_qry,
                      uint32_t n_qry, uint32_t *d_c_or_zero, uint32_t *d_n, double *d_sum_or_union)
{
    (void)hipSetDevice(ctx->device);
    if (n_ref == 0 || n_qry == 0) return LASH_OK;
    lash_sketch_set *ref = &ctx->pair_ref, *qry = d_ref == d_qry && n_ref == n_qry ? ref : &ctx->pair_qry;
    int rc;
    if ((rc = lash_set_bind(ctx, ref, algo, p, d_ref, n_ref))) return rc;
    if (qry != ref && (rc = lash_set_bind(ctx, qry, algo, p, d_qry, n_qry))) return rc;
    if ((rc = lash_sketch_set_prepare(ctx, ref, qry))) return rc;
    return lash_sketch_set_pair_block_device(ctx, ref, 0, n_ref, qry, n_qry, 0, ull_estimator, d_c_or_zero, d_n, d_sum_or_union);
}

// host buffers: stage the reference and query images, run the device form, copy back what this algorithm outputs, synchronize
int pair_stats_host(lash_ctx *ctx, int algo, int p, int ull_estimator, const uint8_t *ref_images, uint32_t n_ref, const uint8_t *qry_images,
                    uint32_t n_qry, uint32_t *out_c_or_zero, uint32_t *out_n, double *out_sum_or_union)
{
    if (n_ref == 0 || n_qry == 0) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    const size_t ib = image_bytes(ctx->layout, algo, p), rb = ib * n_ref, qb = ib * n_qry, np = (size_t)n_ref * n_qry;
    int rc;
    PairOut d;
    if ((rc = reserve(ctx, ctx->st_seq, rb + qb + 64))) return rc;
    if ((rc = lash_pair_out_reserve(ctx, np, d))) return rc;
    uint8_t *d_r = static_cast<uint8_t *>(ctx->st_seq.ptr), *d_q = d_r + rb;
    HIPCHK(ctx, hipMemcpyAsync(d_r, ref_images, rb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_q, qry_images, qb, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pair_stats_device(ctx, algo, p, ull_estimator, d_r, n_ref, d_q, n_qry, d.c, d.n, d.u))) return rc;
    return lash_pair_out_fetch(ctx, algo, np, d, out_c_or_zero, out_n, out_sum_or_union);
}

}  // namespace

extern "C" {

int lash_hmh_pair_counts_device(lash_ctx *ctx, const uint8_t *d_ref_images, uint32_t n_ref, const uint8_t *d_qry_images,
                                uint32_t n_qry, uint32_t *d_out_c, uint32_t *d_out_n)
{
    if (!ctx || ((n_ref && n_qry) && (!d_ref_images || !d_qry_images || !d_out_c || !d_out_n))) return LASH_EINVAL;
    return pair_stats_device(ctx, LASH_HMH, 0, 0, d_ref_images, n_ref, d_qry_images, n_qry, d_out_c, d_out_n, nullptr);
}

int lash_hmh_pair_counts(lash_ctx *ctx, const uint8_t *ref_images, uint32_t n_ref, const uint8_t *qry_images,
                         uint32_t n_qry, uint32_t *out_c, uint32_t *out_n)
{
    if (!ctx || ((n_ref && n_qry) && (!ref_images || !qry_images || !out_c || !out_n))) return LASH_EINVAL;
    return pair_stats_host(ctx, LASH_HMH, 0, 0, ref_images, n_ref, qry_images, n_qry, out_c, out_n, nullptr);
}

int lash_hmh_pair_expected_collisions(lash_ctx *ctx, const double *ref_card, uint32_t n_ref, const double *qry_card, uint32_t n_qry,
                                      double *out_ec)
{
    if (!ctx || ((n_ref && n_qry) && (!ref_card || !qry_card || !out_ec))) return LASH_EINVAL;
    if (n_ref == 0 || n_qry == 0) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    // the call-scoped sets, bound to cardinalities alone.  The query set and its cell vectors are kept while the values repeat.
    lash_sketch_set *ref = &ctx->pair_ref, *qry = &ctx->pair_qry;
    int rc;
    if ((rc = lash_set_bind(ctx, ref, LASH_HMH, 0, nullptr, n_ref))) return rc;
    if ((rc = lash_set_take_cardinalities(ctx, ref, ref_card))) return rc;
    if (!(qry->have_ec_vec && qry->card.size() == n_qry && std::equal(qry_card, qry_card + n_qry, qry->card.begin()))) {
        if ((rc = lash_set_bind(ctx, qry, LASH_HMH, 0, nullptr, n_qry))) return rc;
        if ((rc = lash_set_take_cardinalities(ctx, qry, qry_card))) return rc;
    }
    // O(1) regimes on the host: every pair with a large member (two small ones need the cell sum: below)
    const std::vector<uint32_t> &rs = ref->small_idx;
    std::vector<uint8_t> q_small(n_qry, 0);
    for (uint32_t j : qry->small_idx) q_small[j] = 1;
    auto r_next = rs.begin();
    for (uint32_t i = 0; i < n_ref; ++i) {
        const bool r_small = r_next != rs.end() && *r_next == i;
        if (r_small) ++r_next;
        double *row = out_ec + (size_t)i * n_qry;
        for (uint32_t j = 0; j < n_qry; ++j)
            if (!(r_small && q_small[j])) (void)hmh_ec_closed_form(qry_card[j], ref_card[i], &row[j]);
    }
    if (rs.empty() || qry->small_idx.empty()) return LASH_OK;
    if ((rc = lash_set_ec_vectors(ctx, qry))) return rc;
    // row blocks of at most 8192 small rows: 4 GiB of reference vectors at a time
    constexpr size_t R_BLOCK = 8192;
    for (size_t b = 0; b < rs.size(); b += R_BLOCK) {
        const uint32_t r0 = rs[b], r1 = b + R_BLOCK < rs.size() ? rs[b + R_BLOCK] : n_ref;
        EcBlock eb;
        if ((rc = lash_set_ec_block(ctx, ref, r0, r1, qry, n_qry, eb))) return rc;
        if ((rc = lash_set_ec_scatter(ctx, eb, ref, r0, qry, n_qry, out_ec + (size_t)r0 * n_qry))) return rc;
    }
    return LASH_OK;
}

int lash_hll_pair_union_stats_device(lash_ctx *ctx, int p, const uint8_t *d_ref_images, uint32_t n_ref,
                                     const uint8_t *d_qry_images, uint32_t n_qry, uint32_t *d_out_zero, double *d_out_sum)
{
    if (!ctx || p < 4 || p > 16 || ((n_ref && n_qry) && (!d_ref_images || !d_qry_images || !d_out_zero || !d_out_sum)))
        return LASH_EINVAL;
    return pair_stats_device(ctx, LASH_HLL, p, 0, d_ref_images, n_ref, d_qry_images, n_qry, d_out_zero, nullptr, d_out_sum);
}

int lash_hll_pair_union_stats(lash_ctx *ctx, int p, const uint8_t *ref_images, uint32_t n_ref, const uint8_t *qry_images,
                              uint32_t n_qry, uint32_t *out_zero, double *out_sum)
{
    if (!ctx || p < 4 || p > 16 || ((n_ref && n_qry) && (!ref_images || !qry_images || !out_zero || !out_sum))) return LASH_EINVAL;
    return pair_stats_host(ctx, LASH_HLL, p, 0, ref_images, n_ref, qry_images, n_qry, out_zero, nullptr, out_sum);
}

int lash_ull_pair_union_estimates_device(lash_ctx *ctx, int p, int estimator, const uint8_t *d_ref_images, uint32_t n_ref,
                                         const uint8_t *d_qry_images, uint32_t n_qry, double *d_out_est)
{
    if (!ctx || p < 3 || p > 26 || (estimator != LASH_ULL_FGRA && estimator != LASH_ULL_ML) ||
        ((n_ref && n_qry) && (!d_ref_images || !d_qry_images || !d_out_est)))
        return LASH_EINVAL;
    return pair_stats_device(ctx, LASH_ULL, p, estimator, d_ref_images, n_ref, d_qry_images, n_qry, nullptr, nullptr, d_out_est);   // (no synchronization)
}

int lash_ull_pair_union_estimates(lash_ctx *ctx, int p, int estimator, const uint8_t *ref_images, uint32_t n_ref,
                                  const uint8_t *qry_images, uint32_t n_qry, double *out_est)
{
    if (!ctx || p < 3 || p > 26 || ((n_ref && n_qry) && (!ref_images || !qry_images || !out_est))) return LASH_EINVAL;
    return pair_stats_host(ctx, LASH_ULL, p, estimator, ref_images, n_ref, qry_images, n_qry, nullptr, nullptr, out_est);
}

double lash_ull_estimate(const uint8_t *registers, int p, int estimator)
{
    if (!registers || p < 3 || p > 26) return -1.0;
    uint32_t hist[256] = {0};
    for (size_t i = 0, m = (size_t)1 << p; i < m; ++i) hist[registers[i]]++;
    auto h = [&](uint32_t r) { return hist[r]; };
    return estimator == LASH_ULL_ML ? lash::ull::ml(h, p) : lash::ull::fgra(h, p);
}

}  // extern "C"
