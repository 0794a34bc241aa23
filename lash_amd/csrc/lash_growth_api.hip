// lash_growth_api.hip — the extern "C" entries of `lash growth` (include/lash_gfx950.h: lash_sketch_set_prefix_union_*): the
// cardinality of the running union along orderings of a resident sketch set.  The register histograms of every (order, step)
// come from one launch per chunk of orders (prefix_union.hip); the host finish is the one lash_sketch_set_cardinalities uses for
// single images, so a step's number is bit for bit what the single-image entries give for the image of that union.
#include "lash_ctx.h"

namespace {

uint32_t table_words(const lash_sketch_set *s) { return (s->algo == LASH_HMH ? HMH_M * 2u : (1u << s->p)) / 4u; }

// the plan of a call: slices as asked (clamped to the word count) or chosen; orders per chunk under the histogram budget
int plan(lash_ctx *ctx, const lash_sketch_set *s, uint32_t n_orders, uint32_t len, const lash_prefix_union_opts *opts, uint32_t &slices,
         uint32_t &chunk)
{
    if (s->algo == LASH_ULL && s->p > 16) {
        char buf[160];
        snprintf(buf, sizeof buf, "prefix unions keep one order's whole table on chip: ull -p %d needs more than 64 KiB (ull is supported up to -p 16)",
                 s->p);
        ctx->err = buf;
        return LASH_EINVAL;
    }
    const uint32_t words = table_words(s);
    const uint64_t budget = opts && opts->hist_budget_bytes ? opts->hist_budget_bytes : 256ull << 20;
    const uint64_t per_order = (uint64_t)len * 256u * 4u;
    chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per_order ? budget / per_order : 1, 1), std::min<uint32_t>(std::max(n_orders, 1u), 65535u));
    slices = opts && opts->slices ? std::min(opts->slices, words) : prefix_union_default_slices(words, chunk, (uint32_t)ctx->cu_count);
    return LASH_OK;
}

}  // namespace

extern "C" {

int lash_sketch_set_prefix_union_plan(lash_ctx *ctx, const lash_sketch_set *s, uint32_t n_orders, uint32_t len, const lash_prefix_union_opts *opts,
                                      lash_prefix_union_opts *out_plan)
{
    if (!ctx || !s || !out_plan) return LASH_EINVAL;
    uint32_t slices = 0, chunk = 0;
    const int rc = plan(ctx, s, n_orders, len, opts, slices, chunk);
    if (rc) return rc;
    out_plan->slices = slices;
    out_plan->hist_budget_bytes = (uint64_t)chunk * len * 256u * 4u;
    return LASH_OK;
}

int lash_sketch_set_prefix_union_cardinalities(lash_ctx *ctx, lash_sketch_set *s, const uint32_t *orders, uint32_t n_orders, uint32_t len,
                                               int ull_estimator, const lash_hll_bias *tables, const lash_prefix_union_opts *opts,
                                               double *out_card, uint64_t *bad_index)
{
    if (!ctx || !s) return LASH_EINVAL;
    ctx->err.clear();
    if (s->device != ctx->device) return LASH_EINVAL;
    if (n_orders == 0) return LASH_OK;
    if (!orders || !out_card || len == 0) return LASH_EINVAL;
    if (s->algo == LASH_ULL && ull_estimator != LASH_ULL_FGRA && ull_estimator != LASH_ULL_ML) return LASH_EINVAL;
    uint32_t slices = 0, chunk = 0;
    int rc = plan(ctx, s, n_orders, len, opts, slices, chunk);
    if (rc) return rc;
    const uint64_t total = (uint64_t)n_orders * len;
    for (uint64_t i = 0; i < total; ++i)
        if (orders[i] >= s->n) {
            if (bad_index) *bad_index = i;
            ctx->err = "lash_sketch_set_prefix_union_cardinalities: an order names a member the set does not have";
            return LASH_EINVAL;
        }
    (void)hipSetDevice(ctx->device);

    // buffers of the call (the set and the context's scratch of other entries stay as they are)
    DevBuf d_orders, d_hist, d_fold;
    struct Free { DevBuf &a, &b, &c; ~Free() { release(a); release(b); release(c); } } guard{d_orders, d_hist, d_fold};
    const size_t chunk_words = (size_t)chunk * len * 256u;
    if ((rc = reserve(ctx, d_orders, total * 4))) return rc;
    if ((rc = reserve(ctx, d_hist, chunk_words * 4))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_orders.ptr, orders, total * 4, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> hist(chunk_words);
    std::vector<uint8_t> one;

    PrefixUnionArgs a{};
    a.img = s->d_images;
    a.stride = s->stride;
    a.hdr = s->hdr;
    a.hmh_be = s->hmh_be;
    a.len = len;
    a.n_words = table_words(s);
    a.slices = slices;
    a.hist = static_cast<uint32_t *>(d_hist.ptr);
    for (uint32_t o0 = 0; o0 < n_orders; o0 += chunk) {
        const uint32_t no = std::min(chunk, n_orders - o0);
        const size_t hb = (size_t)no * len * 256u * 4u;
        a.orders = static_cast<const uint32_t *>(d_orders.ptr) + (size_t)o0 * len;
        HIPCHK(ctx, hipMemsetAsync(d_hist.ptr, 0, hb, ctx->stream));
        HIPCHK(ctx, launch_prefix_union(a, s->algo, no, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(hist.data(), d_hist.ptr, hb, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t o = o0; o < o0 + no; ++o) {
            const uint32_t *ord = orders + (size_t)o * len;
            uint32_t folded = 0;                                      // HyperMinHash, rare ranks: d_fold holds the union of steps [0, folded)
            for (uint32_t t = 0; t < len; ++t) {
                const uint32_t *h = hist.data() + ((size_t)(o - o0) * len + t) * 256u;
                double &out = out_card[(size_t)o * len + t];
                if (s->algo == LASH_HMH) {
                    bool exact = true;
                    out = hmh_cardinality_from_hist(h, &exact);
                    if (exact) continue;
                    // a register with lz > 39: the crate's register-order sum on the real union, as lash_sketch_set_cardinalities does
                    // for a single image.  Every later step of the order comes here too, so the fold goes on from where it stopped.
                    if ((rc = reserve(ctx, d_fold, s->stride + 64))) return rc;
                    if (folded == 0) {
                        HIPCHK(ctx, hipMemcpyAsync(d_fold.ptr, s->d_images + (uint64_t)ord[0] * s->stride, s->stride, hipMemcpyDeviceToDevice, ctx->stream));
                        folded = 1;
                    }
                    for (; folded <= t; ++folded)
                        if ((rc = lash_merge_images_device(ctx, LASH_HMH, 0, static_cast<uint8_t *>(d_fold.ptr), s->d_images + (uint64_t)ord[folded] * s->stride, 1)))
                            return rc;
                    one.resize(s->stride);
                    HIPCHK(ctx, hipMemcpyAsync(one.data(), d_fold.ptr, s->stride, hipMemcpyDeviceToHost, ctx->stream));
                    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                    out = lash_hmh_cardinality(one.data() + s->hdr, (int)s->hmh_be);
                } else if (s->algo == LASH_HLL) {
                    if (hll_cardinality_from_hist(h, s->p, tables, &out) != LASH_OK) {
                        if (bad_index) *bad_index = (uint64_t)o * len + t;
                        return LASH_ERANGE;
                    }
                } else {
                    auto hh = [&](uint32_t r) { return h[r]; };
                    out = ull_estimator == LASH_ULL_ML ? lash::ull::ml(hh, s->p) : lash::ull::fgra(hh, s->p);
                }
            }
        }
    }
    return LASH_OK;
}

}  // extern "C"
