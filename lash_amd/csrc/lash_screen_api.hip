// lash_screen_api.hip — the extern "C" entries of `lash screen` (include/lash_gfx950.h: lash_sketch_set_screen_wta*): for every query of a
// resident HyperMinHash set and its list of candidate rows of a reference set, best first, the buckets each candidate holds and the
// buckets it wins when a bucket goes to the first candidate that holds it.  Per chunk of queries there are two launches
// (screen_wta.hip): the winner of every bucket of every query, then the two counts of every (query, position).  The lists are cut with
// the segment and slices lash_sketch_set_group_union_plan answers for them; a chunk holds as many queries as keep the winner tables
// (64 KiB each) under the scratch budget, at least one.
#include "lash_internal.h"

namespace {

constexpr uint64_t TABLE_BYTES = 4ull * HMH_M;                              // a query's winner table
constexpr uint64_t CHUNK_ENTRIES = 1ull << 30;                              // most list entries of a chunk: one counting workgroup each

uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

bool under_layout(const lash_ctx *ctx, const lash_sketch_set *s)
{
    return s->stride != 0 && s->hdr == header_bytes(ctx->layout, s->algo) && s->stride == image_bytes(ctx->layout, s->algo, s->p);
}

// what is refused before anything is sized by the lists
int refuse(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off)
{
    if (ref->algo != LASH_HMH || qry->algo != LASH_HMH) {
        ctx->err = std::string("lash_sketch_set_screen_wta: the ") + (ref->algo != LASH_HMH ? "reference" : "query") +
                   " set is not HyperMinHash (an hll or ull register does not identify a k-mer)";
        return LASH_EINVAL;
    }
    bool ok = cand_off[0] == 0;
    for (uint32_t q = 0; ok && q < qry->n; ++q) ok = cand_off[q] <= cand_off[q + 1];
    if (!ok) {
        ctx->err = "lash_sketch_set_screen_wta: cand_off must start at 0 and never decrease";
        return LASH_EINVAL;
    }
    if (!under_layout(ctx, ref) || !under_layout(ctx, qry)) {
        ctx->err = "lash_sketch_set_screen_wta: a set was not made under the context's layout";
        return LASH_EINVAL;
    }
    return LASH_OK;
}

bool args_ok(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off)
{
    if (!ctx || !ref || !qry || !cand_off) return false;
    ctx->err.clear();
    return ref->device == ctx->device && qry->device == ctx->device;
}

// queries [q0, q1) of one chunk: as many as keep the winner tables under the budget and the entries within a launch, at least one
uint32_t chunk_end(const uint64_t *cand_off, uint32_t n_qry, uint32_t q0, uint64_t budget)
{
    uint32_t q = q0 + 1;
    while (q < n_qry && (uint64_t)(q + 1 - q0) * TABLE_BYTES <= budget && cand_off[q + 1] - cand_off[q0] <= CHUNK_ENTRIES) ++q;
    return q;
}

int screen_wta_device(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off, const uint32_t *cand_ref,
                      const lash_group_union_opts *opts, uint32_t *d_shared, uint32_t *d_won, uint64_t *bad_index)
{
    const uint32_t n_qry = qry->n;
    const uint64_t n_entries = cand_off[n_qry];
    for (uint64_t i = 0; i < n_entries; ++i)
        if (cand_ref[i] >= ref->n) {
            if (bad_index) *bad_index = i;
            ctx->err = "lash_sketch_set_screen_wta: a list names a row the reference set does not have";
            return LASH_EINVAL;
        }
    for (uint32_t q = 0; q < n_qry; ++q)
        if (cand_off[q + 1] - cand_off[q] > CHUNK_ENTRIES) {
            ctx->err = "lash_sketch_set_screen_wta: too many candidates for one query";
            return LASH_EINVAL;
        }
    lash_group_union_opts plan{0, 0, 0};
    int rc = lash_sketch_set_group_union_plan(ctx, ref, cand_off, n_qry, opts, &plan);
    if (rc) return rc;
    const uint32_t segment = plan.segment, slices = plan.slices;
    uint32_t lanes = 1;
    while (lanes < 256u && lanes < ceil_div(HMH_M / 8u, slices)) lanes *= 2;
    const uint64_t budget = opts && opts->scratch_budget_bytes ? opts->scratch_budget_bytes : 1ull << 30;

    (void)hipSetDevice(ctx->device);
    if ((rc = reserve(ctx, ctx->sw_cand, n_entries * 4 + 64))) return rc;
    if ((rc = upload(ctx, ctx->sw_cand.ptr, cand_ref, n_entries * 4))) return rc;

    ScreenWtaArgs a{};
    a.ref = ref->d_images;
    a.ref_stride = ref->stride;
    a.ref_hdr = ref->hdr;
    a.qry = qry->d_images;
    a.qry_stride = qry->stride;
    a.qry_hdr = qry->hdr;
    a.slices = slices;
    a.lanes = lanes;
    a.out_shared = d_shared;
    a.out_won = d_won;

    std::vector<ScreenTask> tasks;
    std::vector<uint32_t> pair_table;
    for (uint32_t q0 = 0; q0 < n_qry;) {
        const uint32_t q1 = chunk_end(cand_off, n_qry, q0, budget);
        const uint64_t e0 = cand_off[q0], e1 = cand_off[q1];
        if (e1 == e0) { q0 = q1; continue; }
        tasks.clear();
        pair_table.resize(e1 - e0);
        for (uint32_t q = q0; q < q1; ++q) {
            const uint64_t b = cand_off[q], len = cand_off[q + 1] - b;
            const uint32_t n = ceil_div(len, segment);
            for (uint32_t i = 0; i < n; ++i)
                tasks.push_back(ScreenTask{b + (uint64_t)i * segment, (uint32_t)std::min<uint64_t>(segment, len - (uint64_t)i * segment), q,
                                           i * segment, q - q0, n == 1 ? 1u : 0u, 0u});
            std::fill(pair_table.begin() + (b - e0), pair_table.begin() + (b - e0 + len), q - q0);
        }
        std::vector<Section> sec = {{tasks.data(), tasks.size() * sizeof(ScreenTask), 0}, {cand_off + q0, (size_t)(q1 - q0 + 1) * 8, 0},
                                    {pair_table.data(), pair_table.size() * 4, 0}};
        const size_t total = layout_sections(sec);
        if ((rc = reserve(ctx, ctx->sw_tasks, total))) return rc;
        if ((rc = upload_sections(ctx, ctx->sw_tasks.ptr, sec, total, ctx->stream))) return rc;
        const uint64_t table_bytes = (uint64_t)(q1 - q0) * TABLE_BYTES;
        if (reserve(ctx, ctx->sw_winner, table_bytes) != LASH_OK) {
            char buf[200];
            snprintf(buf, sizeof buf, "lash_sketch_set_screen_wta: the winner tables of queries %u .. %u need %llu bytes of device memory", q0, q1 - 1,
                     (unsigned long long)table_bytes);
            ctx->err = buf;
            return LASH_ENOMEM;
        }
        HIPCHK(ctx, hipMemsetAsync(ctx->sw_winner.ptr, 0xFF, table_bytes, ctx->stream));
        const uint8_t *const base = static_cast<const uint8_t *>(ctx->sw_tasks.ptr);
        a.cand = static_cast<const uint32_t *>(ctx->sw_cand.ptr);
        a.tasks = reinterpret_cast<const ScreenTask *>(base + sec[0].off);
        a.cand_off = reinterpret_cast<const uint64_t *>(base + sec[1].off);
        a.pair_table = reinterpret_cast<const uint32_t *>(base + sec[2].off);
        a.winner = static_cast<uint32_t *>(ctx->sw_winner.ptr);
        a.n_tasks = (uint32_t)tasks.size();
        a.q0 = q0;
        a.e0 = e0;
        a.n_entries = e1 - e0;
        HIPCHK(ctx, launch_screen_winner(a, ctx->stream));
        HIPCHK(ctx, launch_screen_count(a, ctx->stream));
        q0 = q1;
    }
    return LASH_OK;
}

}  // namespace

extern "C" {

int lash_sketch_set_screen_wta_device(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off,
                                      const uint32_t *cand_ref, const lash_group_union_opts *opts, uint32_t *d_out_shared, uint32_t *d_out_won,
                                      uint64_t *bad_index)
{
    if (!args_ok(ctx, ref, qry, cand_off)) return LASH_EINVAL;
    int rc = refuse(ctx, ref, qry, cand_off);
    if (rc) return rc;
    if (cand_off[qry->n] == 0) return LASH_OK;
    if (!cand_ref || !d_out_shared || !d_out_won) return LASH_EINVAL;
    return screen_wta_device(ctx, ref, qry, cand_off, cand_ref, opts, d_out_shared, d_out_won, bad_index);
}

int lash_sketch_set_screen_wta(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off,
                               const uint32_t *cand_ref, const lash_group_union_opts *opts, uint32_t *out_shared, uint32_t *out_won,
                               uint64_t *bad_index)
{
    if (!args_ok(ctx, ref, qry, cand_off)) return LASH_EINVAL;
    int rc = refuse(ctx, ref, qry, cand_off);
    if (rc) return rc;
    const uint64_t n_entries = cand_off[qry->n];
    if (n_entries == 0) return LASH_OK;
    if (!cand_ref || !out_shared || !out_won) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    if ((rc = reserve(ctx, ctx->sw_out, n_entries * 8 + 64))) return rc;
    uint32_t *const d_shared = static_cast<uint32_t *>(ctx->sw_out.ptr), *const d_won = d_shared + n_entries;
    if ((rc = screen_wta_device(ctx, ref, qry, cand_off, cand_ref, opts, d_shared, d_won, bad_index))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_shared, d_shared, n_entries * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_won, d_won, n_entries * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

}  // extern "C"
