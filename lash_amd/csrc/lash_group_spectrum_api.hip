// lash_group_spectrum_api.hip — the extern "C" entries of `lash spectrum` (include/lash_gfx950.h: lash_sketch_set_group_spectrum*):
// for every group of members of a resident HyperMinHash set, the histogram over the 16 384 buckets of how many members hold the
// bucket's union register.  Per chunk of groups there are two phases: lash_sketch_set_group_union_device writes the chunk's union
// images (they are wanted for the union cardinality anyway), then group_spectrum.hip walks the members once more against them.
// The groups are cut with the segment and slices lash_sketch_set_group_union_plan answers; a chunk holds as many groups as keep the
// union's partials and the count tables of the groups cut into several tasks under the scratch budget, at least one.
#include "lash_ctx.h"

namespace {

constexpr uint64_t TABLE_BYTES = 4ull * HMH_M;                              // a cut group's count table
constexpr uint64_t REG_BYTES = 2ull * HMH_M;                                // a partial union of the first phase

uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

struct Cut {
    uint32_t segment = 0, fan = 0;       // the first phase's: members per task, partials per task above the first level
    uint32_t walk = 0;                   // members per task of the second phase: min(segment, GS_SEGMENT_MAX)
    uint32_t slices = 0, lanes = 0;
    uint64_t budget = 0;
};

// scratch a group of `len` members holds while its chunk runs: the partial unions of the first phase (lash_group_union_api.hip,
// group_partials) and, when the second phase cuts it, its count table
uint64_t group_scratch(uint64_t len, const Cut &c)
{
    const uint64_t even = len > c.segment ? (len + c.segment - 1) / c.segment : 0;
    const uint64_t odd = even > c.fan ? (even + c.fan - 1) / c.fan : 0;
    return (even + odd) * REG_BYTES + (len > c.walk ? TABLE_BYTES : 0);
}

uint32_t chunk_end(const uint64_t *group_off, uint32_t n_groups, uint32_t g0, const Cut &c)
{
    uint64_t held = 0;
    uint32_t g = g0;
    for (; g < n_groups && g - g0 < 0x40000000u; ++g) {
        const uint64_t s = group_scratch(group_off[g + 1] - group_off[g], c);
        if (g > g0 && held + s > c.budget) break;
        held += s;
    }
    return g;
}

bool args_ok(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off)
{
    if (!ctx || !s || !group_off) return false;
    ctx->err.clear();
    return s->device == ctx->device;
}

// what is refused before anything is sized by the lists: a set of another algorithm; offsets and a layout the union would refuse
int refuse(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, uint32_t n_groups, const lash_group_union_opts *opts,
           lash_group_union_opts *out_plan = nullptr)
{
    if (s->algo != LASH_HMH) {
        ctx->err = "lash_sketch_set_group_spectrum: the set is not HyperMinHash (an hll or ull register does not identify a k-mer)";
        return LASH_EINVAL;
    }
    lash_group_union_opts plan{0, 0, 0};
    return lash_sketch_set_group_union_plan(ctx, s, group_off, n_groups, opts, out_plan ? out_plan : &plan);
}

int group_spectrum_device(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members, uint32_t n_groups,
                          const lash_group_union_opts *opts, uint32_t *d_hist, uint8_t *d_union, uint64_t *bad_index)
{
    lash_group_union_opts plan{0, 0, 0};
    int rc = refuse(ctx, s, group_off, n_groups, opts, &plan);
    if (rc) return rc;
    const uint64_t n_members = group_off[n_groups];
    if (n_members && !members) return LASH_EINVAL;
    for (uint64_t i = 0; i < n_members; ++i)
        if (members[i] >= s->n) {
            if (bad_index) *bad_index = i;
            ctx->err = "lash_sketch_set_group_spectrum: a group names a member the set does not have";
            return LASH_EINVAL;
        }
    Cut c;
    c.segment = plan.segment;
    c.fan = std::max(plan.segment, 2u);
    c.walk = std::min(plan.segment, GS_SEGMENT_MAX);
    c.slices = plan.slices;
    c.lanes = 1;
    while (c.lanes < 256u && c.lanes < ceil_div(HMH_M / 8u, c.slices)) c.lanes *= 2;
    c.budget = opts && opts->scratch_budget_bytes ? opts->scratch_budget_bytes : 1ull << 30;
    const lash_group_union_opts run{c.segment, c.slices, c.budget};

    (void)hipSetDevice(ctx->device);
    if ((rc = reserve(ctx, ctx->gs_members, n_members * 4 + 64))) return rc;
    if ((rc = upload(ctx, ctx->gs_members.ptr, members, n_members * 4))) return rc;
    if (!d_union) {
        if ((rc = reserve(ctx, ctx->gs_union, (size_t)n_groups * s->stride + 64))) return rc;
        d_union = static_cast<uint8_t *>(ctx->gs_union.ptr);
    }
    HIPCHK(ctx, hipMemsetAsync(d_hist, 0, (size_t)(n_members + n_groups) * 4, ctx->stream));

    GroupSpectrumArgs a{};
    a.src = s->d_images;
    a.src_stride = s->stride;
    a.src_hdr = s->hdr;
    a.slices = c.slices;
    a.lanes = c.lanes;
    a.uni = d_union;
    a.uni_stride = s->stride;
    a.uni_hdr = s->hdr;
    a.hist = d_hist;

    std::vector<SpectrumTask> tasks;
    std::vector<uint64_t> table_hist, off;
    for (uint32_t g0 = 0; g0 < n_groups;) {
        const uint32_t g1 = chunk_end(group_off, n_groups, g0, c);
        // phase A: the chunk's union images
        off.assign(group_off + g0, group_off + g1 + 1);
        for (uint64_t &o : off) o -= group_off[g0];
        rc = lash_sketch_set_group_union_device(ctx, s, off.data(), members ? members + group_off[g0] : nullptr, g1 - g0, &run,
                                                d_union + (uint64_t)g0 * s->stride, nullptr);
        if (rc) return rc;
        // phase B: the members once more, against them
        tasks.clear();
        table_hist.clear();
        for (uint32_t g = g0; g < g1; ++g) {
            const uint64_t b = group_off[g], len = group_off[g + 1] - b, bins = b + g;
            if (len <= c.walk) { tasks.push_back(SpectrumTask{b, bins, (uint32_t)len, g, GS_NO_TABLE, 0u}); continue; }
            const uint32_t n = ceil_div(len, c.walk), table = (uint32_t)table_hist.size();
            for (uint32_t i = 0; i < n; ++i)
                tasks.push_back(SpectrumTask{b + (uint64_t)i * c.walk, bins, (uint32_t)std::min<uint64_t>(c.walk, len - (uint64_t)i * c.walk), g, table, 0u});
            table_hist.push_back(bins);
        }
        std::vector<Section> sec = {{tasks.data(), tasks.size() * sizeof(SpectrumTask), 0}, {table_hist.data(), table_hist.size() * 8, 0}};
        const size_t total = layout_sections(sec);
        if ((rc = reserve(ctx, ctx->gs_tasks, total))) return rc;
        if ((rc = upload_sections(ctx, ctx->gs_tasks.ptr, sec, total, ctx->stream))) return rc;
        const uint32_t n_tables = (uint32_t)table_hist.size();
        if (n_tables) {
            if (reserve(ctx, ctx->gs_counts, n_tables * TABLE_BYTES) != LASH_OK) {
                char buf[200];
                snprintf(buf, sizeof buf, "lash_sketch_set_group_spectrum: the count tables of groups %u .. %u need %llu bytes of device memory (segment %u)",
                         g0, g1 - 1, (unsigned long long)(n_tables * TABLE_BYTES), c.walk);
                ctx->err = buf;
                return LASH_ENOMEM;
            }
            HIPCHK(ctx, hipMemsetAsync(ctx->gs_counts.ptr, 0, n_tables * TABLE_BYTES, ctx->stream));
        }
        a.members = static_cast<const uint32_t *>(ctx->gs_members.ptr);
        a.tasks = reinterpret_cast<const SpectrumTask *>(static_cast<const uint8_t *>(ctx->gs_tasks.ptr) + sec[0].off);
        a.table_hist = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(ctx->gs_tasks.ptr) + sec[1].off);
        a.n_tasks = (uint32_t)tasks.size();
        a.counts = static_cast<uint32_t *>(ctx->gs_counts.ptr);
        HIPCHK(ctx, launch_group_spectrum(a, ctx->stream));
        HIPCHK(ctx, launch_group_spectrum_finish(a, n_tables, ctx->stream));
        g0 = g1;
    }
    return LASH_OK;
}

}  // namespace

extern "C" {

int lash_sketch_set_group_spectrum_device(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members,
                                          uint32_t n_groups, const lash_group_union_opts *opts, uint32_t *d_out_hist, uint8_t *d_out_union_images,
                                          uint64_t *bad_index)
{
    if (!args_ok(ctx, s, group_off)) return LASH_EINVAL;
    if (n_groups == 0) return LASH_OK;
    if (!d_out_hist) return LASH_EINVAL;
    return group_spectrum_device(ctx, s, group_off, members, n_groups, opts, d_out_hist, d_out_union_images, bad_index);
}

int lash_sketch_set_group_spectrum(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members, uint32_t n_groups,
                                   const lash_group_union_opts *opts, uint32_t *out_hist, uint8_t *out_union_images, uint64_t *bad_index)
{
    if (!args_ok(ctx, s, group_off)) return LASH_EINVAL;
    if (n_groups == 0) return LASH_OK;
    if (!out_hist) return LASH_EINVAL;
    int rc = refuse(ctx, s, group_off, n_groups, opts);                     // before a bad list sizes a buffer
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    const size_t hist_bytes = (size_t)(group_off[n_groups] + n_groups) * 4, img_bytes = (size_t)n_groups * s->stride;
    if ((rc = reserve(ctx, ctx->gs_hist, hist_bytes + 64))) return rc;
    if ((rc = reserve(ctx, ctx->gs_union, img_bytes + 64))) return rc;
    if ((rc = group_spectrum_device(ctx, s, group_off, members, n_groups, opts, static_cast<uint32_t *>(ctx->gs_hist.ptr),
                                    static_cast<uint8_t *>(ctx->gs_union.ptr), bad_index)))
        return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_hist, ctx->gs_hist.ptr, hist_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_union_images) HIPCHK(ctx, hipMemcpyAsync(out_union_images, ctx->gs_union.ptr, img_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

}  // extern "C"
