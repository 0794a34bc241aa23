// lash_group_union_api.hip — the extern "C" entries of `lash merge` (include/lash_gfx950.h: lash_sketch_set_group_union*): one
// serialized image per group of members of a resident sketch set, each the union of its members.  The host cuts the groups into
// tasks (group_union.hip says what a task is), level by level, for one chunk of groups at a time; a chunk's tasks of all levels
// go to the device in one copy and every level is one launch.
#include "lash_ctx.h"

namespace {

uint32_t table_words(const lash_sketch_set *s) { return (s->algo == LASH_HMH ? HMH_M * 2u : (1u << s->p)) / 4u; }
uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

struct Plan {
    uint32_t segment = 0, fan = 0;       // members per first-level task; partials per task above it (a segment of 1 would never shrink them)
    uint32_t slices = 0, lanes = 0;
    uint64_t budget = 0;
};

// partials a group of `len` members leaves in the two halves of the scratch buffer (levels write them in turn: the first level's
// count bounds one half, the second level's the other)
void group_partials(uint64_t len, const Plan &pl, uint64_t &even, uint64_t &odd)
{
    even = len > pl.segment ? (len + pl.segment - 1) / pl.segment : 0;
    odd = even > pl.fan ? (even + pl.fan - 1) / pl.fan : 0;
}

int check_offsets(lash_ctx *ctx, const uint64_t *group_off, uint32_t n_groups)
{
    bool ok = group_off[0] == 0;
    for (uint32_t g = 0; ok && g < n_groups; ++g) ok = group_off[g] <= group_off[g + 1];
    if (!ok) ctx->err = "lash_sketch_set_group_union: group_off must start at 0 and never decrease";
    return ok ? LASH_OK : LASH_EINVAL;
}

// segment: so that the first level has about eight workgroups per CU where the members allow it, within 8 .. 256 — a group of up to 256
// members is one task and needs no scratch, a long one is never a serial walk of more than 256 loads per thread.
// slices: one unit per thread, fewer when that would not fit a grid.
int make_plan(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, uint32_t n_groups, const lash_group_union_opts *opts, Plan &pl)
{
    if (s->stride == 0 || s->hdr != header_bytes(ctx->layout, s->algo) || s->stride != image_bytes(ctx->layout, s->algo, s->p)) {
        ctx->err = "lash_sketch_set_group_union: the set was not made under the context's layout";
        return LASH_EINVAL;
    }
    const uint32_t words = table_words(s), n_units = words / group_union_unit_words(words);
    const uint64_t members = group_off[n_groups];
    uint32_t slices = opts && opts->slices ? std::min(opts->slices, n_units) : std::max(1u, ceil_div(n_units, 256));
    const uint64_t most_tasks = std::max<uint64_t>(members, n_groups);    // (segment = 1: a task per member)
    while (slices > 1 && most_tasks * slices > 0x3FFFFFFFull) slices = (slices + 1) / 2;
    if (most_tasks * slices > 0x3FFFFFFFull) {
        ctx->err = "lash_sketch_set_group_union: too many members for one call";
        return LASH_EINVAL;
    }
    const uint32_t per_slice = ceil_div(n_units, slices);
    uint32_t lanes = 1;
    while (lanes < 256u && lanes < per_slice) lanes *= 2;
    pl.slices = slices;
    pl.lanes = lanes;
    if (opts && opts->segment) pl.segment = opts->segment;
    else {
        const uint64_t want = (members * slices + 8ull * (uint64_t)ctx->cu_count - 1) / (8ull * (uint64_t)ctx->cu_count);
        pl.segment = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 8), 256);
    }
    pl.fan = std::max(pl.segment, 2u);
    pl.budget = opts && opts->scratch_budget_bytes ? opts->scratch_budget_bytes : 1ull << 30;
    return LASH_OK;
}

// groups [g0, g1) of one chunk: as many as keep the partials under the budget and the images within a launch, at least one
uint32_t chunk_end(const uint64_t *group_off, uint32_t n_groups, uint32_t g0, const Plan &pl, uint64_t reg_bytes, uint64_t &even, uint64_t &odd)
{
    even = odd = 0;
    uint32_t g = g0;
    for (; g < n_groups && g - g0 < 0x40000000u; ++g) {
        uint64_t e, o;
        group_partials(group_off[g + 1] - group_off[g], pl, e, o);
        if (g > g0 && (even + e + odd + o) * reg_bytes > pl.budget) break;
        even += e;
        odd += o;
    }
    return g;
}

// the largest chunk's scratch: what a call allocates
uint64_t scratch_bytes(const uint64_t *group_off, uint32_t n_groups, const Plan &pl, uint64_t reg_bytes)
{
    uint64_t most = 0;
    for (uint32_t g0 = 0; g0 < n_groups;) {
        uint64_t e, o;
        g0 = chunk_end(group_off, n_groups, g0, pl, reg_bytes, e, o);
        most = std::max(most, (e + o) * reg_bytes);
    }
    return most;
}

int group_union_device(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members, uint32_t n_groups,
                       const lash_group_union_opts *opts, uint8_t *d_out, uint64_t *bad_index)
{
    int rc = check_offsets(ctx, group_off, n_groups);
    if (rc) return rc;
    const uint64_t n_members = group_off[n_groups];
    if (n_members && !members) return LASH_EINVAL;
    for (uint64_t i = 0; i < n_members; ++i)
        if (members[i] >= s->n) {
            if (bad_index) *bad_index = i;
            ctx->err = "lash_sketch_set_group_union: a group names a member the set does not have";
            return LASH_EINVAL;
        }
    Plan pl;
    if ((rc = make_plan(ctx, s, group_off, n_groups, opts, pl))) return rc;
    (void)hipSetDevice(ctx->device);
    const uint32_t words = table_words(s);
    const uint64_t reg_bytes = 4ull * words;

    if ((rc = reserve(ctx, ctx->gu_members, n_members * 4 + 64))) return rc;
    if ((rc = upload(ctx, ctx->gu_members.ptr, members, n_members * 4))) return rc;

    GroupUnionArgs a{};
    a.n_words = words;
    a.slices = pl.slices;
    a.lanes = pl.lanes;
    a.out_stride = s->stride;
    a.hdr = s->hdr;
    a.out_be = s->hmh_be;
    const LayoutDev lay = layout_dev(ctx->layout, s->algo);
    a.hdr_tpl = lay.hdr_tpl;
    const double alpha = hll_alpha(s->p);
    memcpy(&a.alpha_bits, &alpha, 8);
    a.p = s->p;

    struct Pending { uint64_t base; uint32_t n; uint32_t img; };         // a group's partials of the level below
    std::vector<GroupTask> tasks;
    std::vector<uint32_t> level_end;
    std::vector<Pending> cur, nxt;
    for (uint32_t g0 = 0; g0 < n_groups;) {
        uint64_t even = 0, odd = 0;
        const uint32_t g1 = chunk_end(group_off, n_groups, g0, pl, reg_bytes, even, odd);
        tasks.clear();
        level_end.clear();
        cur.clear();
        uint64_t slot = 0;
        for (uint32_t g = g0; g < g1; ++g) {
            const uint64_t b = group_off[g], len = group_off[g + 1] - b;
            if (len <= pl.segment) { tasks.push_back(GroupTask{b, (uint32_t)len, GU_FINAL | (g - g0)}); continue; }
            const uint32_t n = ceil_div(len, pl.segment);
            for (uint32_t i = 0; i < n; ++i)
                tasks.push_back(GroupTask{b + (uint64_t)i * pl.segment, (uint32_t)std::min<uint64_t>(pl.segment, len - (uint64_t)i * pl.segment), (uint32_t)(slot + i)});
            cur.push_back(Pending{slot, n, g - g0});
            slot += n;
        }
        level_end.push_back((uint32_t)tasks.size());
        while (!cur.empty()) {
            nxt.clear();
            slot = 0;
            for (const Pending &pe : cur) {
                if (pe.n <= pl.fan) { tasks.push_back(GroupTask{pe.base, pe.n, GU_FINAL | pe.img}); continue; }
                const uint32_t n = ceil_div(pe.n, pl.fan);
                for (uint32_t i = 0; i < n; ++i)
                    tasks.push_back(GroupTask{pe.base + (uint64_t)i * pl.fan, std::min(pl.fan, pe.n - i * pl.fan), (uint32_t)(slot + i)});
                nxt.push_back(Pending{slot, n, pe.img});
                slot += n;
            }
            level_end.push_back((uint32_t)tasks.size());
            cur.swap(nxt);
        }

        if ((rc = reserve(ctx, ctx->gu_tasks, tasks.size() * sizeof(GroupTask)))) return rc;
        if ((rc = upload(ctx, ctx->gu_tasks.ptr, tasks.data(), tasks.size() * sizeof(GroupTask)))) return rc;
        if (even + odd) {
            if (reserve(ctx, ctx->gu_part, (even + odd) * reg_bytes) != LASH_OK) {
                char buf[200];
                snprintf(buf, sizeof buf, "lash_sketch_set_group_union: the partial unions of groups %u .. %u need %llu bytes of device memory (segment %u)",
                         g0, g1 - 1, (unsigned long long)((even + odd) * reg_bytes), pl.segment);
                ctx->err = buf;
                return LASH_ENOMEM;
            }
        }
        uint8_t *const half[2] = {static_cast<uint8_t *>(ctx->gu_part.ptr), static_cast<uint8_t *>(ctx->gu_part.ptr) + even * reg_bytes};
        a.out = d_out + (uint64_t)g0 * s->stride;
        if (s->algo == LASH_HLL) {
            const size_t hb = (size_t)(g1 - g0) * 72u * 4u;
            if ((rc = reserve(ctx, ctx->gu_hist, hb))) return rc;
            HIPCHK(ctx, hipMemsetAsync(ctx->gu_hist.ptr, 0, hb, ctx->stream));
            a.hist = static_cast<uint32_t *>(ctx->gu_hist.ptr);
        }
        for (size_t lv = 0, t0 = 0; lv < level_end.size(); t0 = level_end[lv++]) {
            a.tasks = static_cast<const GroupTask *>(ctx->gu_tasks.ptr) + t0;
            a.n_tasks = level_end[lv] - (uint32_t)t0;
            if (lv == 0) {
                a.src = s->d_images; a.src_stride = s->stride; a.src_hdr = s->hdr; a.src_be = s->hmh_be;
                a.members = static_cast<const uint32_t *>(ctx->gu_members.ptr);
            } else {
                a.src = half[(lv - 1) & 1]; a.src_stride = reg_bytes; a.src_hdr = 0; a.src_be = 0;
                a.members = nullptr;
            }
            a.part = half[lv & 1];
            HIPCHK(ctx, launch_group_union(a, s->algo, ctx->stream));
        }
        if (s->algo == LASH_HLL) HIPCHK(ctx, launch_group_union_headers(a, g1 - g0, ctx->stream));
        g0 = g1;
    }
    return LASH_OK;
}

bool args_ok(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off)
{
    if (!ctx || !s || !group_off) return false;
    ctx->err.clear();
    return s->device == ctx->device;
}

}  // namespace

extern "C" {

int lash_sketch_set_group_union_plan(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, uint32_t n_groups,
                                     const lash_group_union_opts *opts, lash_group_union_opts *out_plan)
{
    if (!args_ok(ctx, s, group_off) || !out_plan) return LASH_EINVAL;
    int rc = check_offsets(ctx, group_off, n_groups);
    if (rc) return rc;
    Plan pl;
    if ((rc = make_plan(ctx, s, group_off, n_groups, opts, pl))) return rc;
    out_plan->segment = pl.segment;
    out_plan->slices = pl.slices;
    out_plan->scratch_budget_bytes = scratch_bytes(group_off, n_groups, pl, 4ull * table_words(s));
    return LASH_OK;
}

int lash_sketch_set_group_union_device(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members, uint32_t n_groups,
                                       const lash_group_union_opts *opts, uint8_t *d_out_images, uint64_t *bad_index)
{
    if (!args_ok(ctx, s, group_off)) return LASH_EINVAL;
    if (n_groups == 0) return LASH_OK;
    if (!d_out_images) return LASH_EINVAL;
    return group_union_device(ctx, s, group_off, members, n_groups, opts, d_out_images, bad_index);
}

int lash_sketch_set_group_union(lash_ctx *ctx, const lash_sketch_set *s, const uint64_t *group_off, const uint32_t *members, uint32_t n_groups,
                                const lash_group_union_opts *opts, uint8_t *out_images, uint64_t *bad_index)
{
    if (!args_ok(ctx, s, group_off)) return LASH_EINVAL;
    if (n_groups == 0) return LASH_OK;
    if (!out_images) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    const size_t bytes = (size_t)n_groups * s->stride;
    int rc = reserve(ctx, ctx->gu_out, bytes + 64);
    if (rc) return rc;
    if ((rc = group_union_device(ctx, s, group_off, members, n_groups, opts, static_cast<uint8_t *>(ctx->gu_out.ptr), bad_index))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_images, ctx->gu_out.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

}  // extern "C"
