// dist_cluster.hip — `lash dist --cluster D`: single-linkage clusters of a triangle run, joined on the GPU while a block's pair
// statistics are still in HBM (include/lash_gfx950.h: lash_sketch_set_pair_block_cluster, lash_cluster_*).  Two names are LINKED
// iff `--max-dist D` prints their pair: the host's exact distance d (dist_pair_host, in f32 under fp32) passes d <= D, NaN never.
// Clusters are the connected components of that graph.  A union-find over N labels needs at most N - 1 successful joins whatever
// the number of links, and a pair whose names are already joined needs no distance at all, so a collection with large close groups
// (10^3 genomes of one species: 5 * 10^5 links, every one a candidate, a host evaluation and a text row under --max-dist) costs
// N labels instead.
//
// State: label[N] (u32) in HBM per accumulator, and nothing else.  Invariant: label[i] <= i, and following labels from i ends at the smallest index
// joined with i so far (a root: label[x] == x).  It starts as the identity.
//
// Per block of rows [r0, r1) x columns [0, n_cols) of the lower triangle, after the pair kernels and the expected-collision GEMM:
//   mark + join   the tiles of mark_tiles (dist_filter.h).  For each printed off-diagonal pair: find both roots (reads only);
//                 same root and the device can place the pair: PRUNED, no arithmetic (hmh / ull test the roots first; hll decides
//                 first whether it can place the pair, which needs no distance).  Otherwise the interval [d_lo, d_hi] of
//                 pair_interval_dev (dist_filter.h), which holds the host's d:
//                   SURE    d_hi <= D (PAIR_ONE: 1 <= D)   -> join the two roots
//                   OUT     d_lo > D (PAIR_ONE: 1 > D), or a NaN of hmh / ull   -> nothing
//                   UNSURE  everything else, every pair the device cannot place, a NaN of hll   -> mask bit: the pair goes back to
//                           the host with its statistics (within_compact), which evaluates it exactly
//   flatten       label[i] = root(i) for every index any call has touched so far, so that the next block's finds are one hop; it
//                 also counts the roots.
//   host links    the returned pairs with d <= D are joined in the same label array by a small kernel (one thread per link), then
//                 flattened again.  Ordinary input has none.  lash_cluster_merge folds another accumulator in the same way: its
//                 labels, copied through the host, are the links (i, label[i]).
//
// Soundness.
//   A SURE pair is linked on the host: d <= d_hi <= D (or d = 1 <= D exactly), and a host link is linked by definition.  So every
//     join joins two names that --max-dist D links: label components are always subsets of true components.
//   An OUT pair is not linked: d >= d_lo > D, or d = 1 > D, or d is NaN.  Dropping it loses nothing.
//   Pruning cannot change the components: a pruned pair has both names under one root, and labels only ever record true links, so the
//     two names are already connected by true links; the pruned pair, linked or not, adds no connectivity.  The same holds for an
//     UNSURE pair whose roots are equal.  Pairs the device cannot place are never pruned: the host must see each of them, because
//     one of them may be the pair the --max-dist run fails on (LASH_ERANGE: HLL bias-table regime without tables), and that run's
//     first refused pair in (row, col) order is then this run's too.
//   Every linked pair is therefore SURE (joined), UNSURE (evaluated on the host, then joined in the same labels),
//     or redundant.  Components = connected components of the link graph.
//
// Concurrency.  A join hooks the larger root under the smaller with a 32-bit compare-and-swap at agent scope: label[hi] changes only
// from hi (a root) to a smaller index, once, so label[i] <= i holds, chains strictly descend and every find ends.  A failed swap
// means another join got there first: find again and retry (each failure is somebody's success, and there are at most N - 1).  A
// stale label read costs a longer walk, a retry or a missed prune (the pair is then evaluated, which is always right), never a wrong
// join, because roots are re-read by the swap itself.  The final partition is the set of components of the joined links, whatever
// order they arrive in, and a root is its component's smallest index, so the result does not depend on the block order,
// the workers or the scheduling.  Nothing here orders memory between workgroups beyond the atomics themselves and the kernel
// boundary.
#include "dist_filter.h"

#include <algorithm>
#include <new>
#include <numeric>

struct lash_cluster {
    int device = 0;
    uint32_t n = 0;
    uint32_t touched = 0;                        // every index >= touched is still a cluster of its own
    uint32_t *d_label = nullptr;                 // [n]
    unsigned long long *d_counts = nullptr;      // [3]: pruned, joined, roots among [0, touched)
    uint2 *d_links = nullptr;                    // host links / merged labels on their way into d_label
    size_t links_cap = 0;
};

namespace lash {

struct ClusterArgs {
    uint32_t *label;
    unsigned long long *counts;
    double max_dist;
    uint32_t r0;
};

namespace {

__device__ inline uint32_t label_load(const uint32_t *label, uint32_t i)
{
    return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline uint32_t find_root(const uint32_t *label, uint32_t i)
{
    for (;;) {
        const uint32_t p = label_load(label, i);
        if (p >= i) return i;                                                           // (p == i; > cannot happen: ends the walk anyway)
        i = p;
    }
}

// true: this call hooked one root under another
__device__ inline bool join_roots(uint32_t *label, uint32_t x, uint32_t y)
{
    for (;;) {
        x = find_root(label, x);
        y = find_root(label, y);
        if (x == y) return false;
        const uint32_t hi = x > y ? x : y, lo = x > y ? y : x;
        uint32_t expect = hi;
        if (__hip_atomic_compare_exchange_strong(label + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
    }
}

// the pair (block row r, column q), q != r0 + r; row_root = the root of r0 + r as the wave read it for this step.
// true: the pair goes back to the host.
__device__ inline bool cluster_pair(const WithinArgs &a, const ClusterArgs &c, uint32_t r, uint32_t q, uint32_t row_root, uint32_t &pruned,
                                    uint32_t &joined)
{
    const bool same = row_root == find_root(c.label, q);
    if (same && a.algo != LASH_HLL) { ++pruned; return false; }
    double sim, sim_low, d_lo, d_hi;
    if (!pair_similarity_dev(a, r, q, &sim, &sim_low)) return true;                     // the host's: never pruned
    if (same) { ++pruned; return false; }
    if (pair_interval_dev(a, sim, sim_low, &d_lo, &d_hi) == PAIR_NAN) return a.algo == LASH_HLL;
    if (d_lo > c.max_dist) return false;                                                // out
    if (!(d_hi <= c.max_dist)) return true;                                             // unsure, roots differ
    if (join_roots(c.label, c.r0 + r, q)) ++joined;                                     // sure
    return false;
}

}  // namespace

__global__ void __launch_bounds__(256) cluster_mark_kernel(WithinArgs a, ClusterArgs c, uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count)
{
    __shared__ uint32_t s_pruned, s_joined;
    if (threadIdx.x == 0) { s_pruned = 0; s_joined = 0; }
    __syncthreads();
    uint32_t pruned = 0, joined = 0;
    mark_tiles(a, mask, tile_count, [&](uint32_t r, uint32_t q) {
        // The row's root, read again for every 64 pairs: one address for the whole wave (a single request) that goes past the L1
        // like every label read.  Reading it once per tile would save three requests of a tile's ~20, but a row is new when its
        // block runs: the joins of this wave's earlier steps are what lets the later ones prune.
        const uint32_t row_root = find_root(c.label, c.r0 + r);
        return q != c.r0 + r && cluster_pair(a, c, r, q, row_root, pruned, joined);
    });
    if (pruned) atomicAdd(&s_pruned, pruned);
    if (joined) atomicAdd(&s_joined, joined);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_pruned) atomicAdd(c.counts + 0, (unsigned long long)s_pruned);
        if (s_joined) atomicAdd(c.counts + 1, (unsigned long long)s_joined);
    }
}

// label[i] = root(i) for i < n (a concurrent reader sees the old parent or the root: both are on i's chain), and the number of roots
__global__ void __launch_bounds__(256) cluster_flatten_kernel(uint32_t *__restrict__ label, uint32_t n, unsigned long long *__restrict__ counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool root = false;
    if (i < n) {
        const uint32_t r = find_root(label, i);
        root = r == i;
        if (!root) __hip_atomic_store(label + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t bits = __ballot(root);
    if ((threadIdx.x & 63u) == 0 && bits) atomicAdd(counts + 2, (unsigned long long)__popcll(bits));
}

// links the host confirmed (or another accumulator's labels): one join each; both ends are below n (checked by the caller)
__global__ void __launch_bounds__(256) cluster_link_kernel(uint32_t *__restrict__ label, const uint2 *__restrict__ links, uint32_t n_links)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_links) join_roots(label, links[i].x, links[i].y);
}

}  // namespace lash

namespace {

// label[i] = root(i) over everything touched so far; *roots = the accumulator's number of clusters.  Synchronizes the stream.
hipError_t flatten_and_count(lash_cluster *c, hipStream_t stream, uint64_t *roots)
{
    unsigned long long in_touched = 0;
    hipError_t e = hipMemsetAsync(c->d_counts + 2, 0, sizeof(unsigned long long), stream);
    if (e == hipSuccess && c->touched) {
        hipLaunchKernelGGL(lash::cluster_flatten_kernel, dim3((c->touched + 255) / 256), dim3(256), 0, stream, c->d_label, c->touched, c->d_counts);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&in_touched, c->d_counts + 2, sizeof in_touched, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    *roots = in_touched + (c->n - c->touched);
    return e;
}

// joins `links` (both ends < c->n) in the label array and flattens.  Synchronizes the stream.
hipError_t apply_links(lash_cluster *c, hipStream_t stream, const std::vector<uint2> &links, uint64_t *roots)
{
    hipError_t e = hipSuccess;
    if (links.size() > c->links_cap) {
        if (c->d_links) { e = hipStreamSynchronize(stream); (void)hipFree(c->d_links); c->d_links = nullptr; c->links_cap = 0; }
        const size_t want = links.size() + links.size() / 4 + 64;
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_links), want * sizeof(uint2));
        if (e != hipSuccess) return e;
        c->links_cap = want;
    }
    e = hipMemcpyAsync(c->d_links, links.data(), links.size() * sizeof(uint2), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lash::cluster_link_kernel, dim3(((uint32_t)links.size() + 255) / 256), dim3(256), 0, stream, c->d_label, c->d_links,
                       (uint32_t)links.size());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return flatten_and_count(c, stream, roots);                                          // (`links` is read before this returns)
}

// for every name the smallest index of its cluster, from the labels as they are (flattened or not)
int host_labels(const lash_cluster *c, std::vector<uint32_t> &lab)
{
    lab.resize(c->n);
    if (!c->n) return LASH_OK;
    (void)hipSetDevice(c->device);
    if (hipMemcpy(lab.data(), c->d_label, (size_t)c->n * 4, hipMemcpyDeviceToHost) != hipSuccess) return LASH_EHIP;
    for (uint32_t i = 0; i < c->n; ++i) {
        if (lab[i] > i) return LASH_EHIP;                                                  // (the invariant; never seen)
        lab[i] = lab[lab[i]];                                                              // lab[j] for j < i is already a root
    }
    return LASH_OK;
}

}  // namespace

extern "C" {

int lash_cluster_create(lash_ctx *ctx, uint32_t n, lash_cluster **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    if (!ctx) return LASH_EINVAL;
    lash_cluster *c = new (std::nothrow) lash_cluster;
    if (!c) return LASH_ENOMEM;
    c->device = ctx->device;
    c->n = n;
    std::vector<uint32_t> identity(n);
    std::iota(identity.begin(), identity.end(), 0u);
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->d_label), (size_t)n * 4 + 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_counts), 3 * sizeof(unsigned long long));
    if (e == hipSuccess && n) e = hipMemcpy(c->d_label, identity.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        lash_cluster_free(c);
        return fail(ctx, e == hipErrorOutOfMemory ? LASH_ENOMEM : LASH_EHIP, "lash_cluster_create", e);
    }
    *out = c;
    return LASH_OK;
}

void lash_cluster_free(lash_cluster *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_label) (void)hipFree(c->d_label);
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->d_links) (void)hipFree(c->d_links);
    delete c;
}

int lash_sketch_set_pair_block_cluster(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols,
                                       int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables, double max_dist,
                                       lash_cluster *cluster, lash_cluster_stats *stats, uint64_t *bad_pair)
{
    using namespace lash;
    if (stats) *stats = lash_cluster_stats{};
    if (!cluster || std::isnan(max_dist) || r1 > cluster->n || n_cols > cluster->n || !ctx || cluster->device != ctx->device) return LASH_EINVAL;
    int rc;
    WithinBlock b;
    if ((rc = within_block(ctx, ref, r0, r1, qry, n_cols, 1, k, model, fp32, ull_estimator, b)) || !b.a.n_tiles) return rc;
    const WithinArgs &a = b.a;

    ClusterArgs c{};
    c.label = cluster->d_label;
    c.counts = cluster->d_counts;
    c.max_dist = max_dist;
    c.r0 = r0;
    HIPCHK(ctx, hipMemsetAsync(cluster->d_counts, 0, 3 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(cluster_mark_kernel, dim3(mark_grid(a.n_tiles)), dim3(256), 0, ctx->stream, a, c, b.d_mask, b.d_cnt);
    HIPCHK(ctx, hipGetLastError());
    cluster->touched = std::max({cluster->touched, r1, n_cols});                               // blocks may come in any order
    unsigned long long counts[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(counts, cluster->d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
    uint64_t roots = 0;
    HIPCHK(ctx, flatten_and_count(cluster, ctx->stream, &roots));
    std::vector<WithinPair> cand;
    if ((rc = within_compact(ctx, a, b.d_mask, b.d_cnt, b.d_off, cand))) return rc;

    std::vector<uint2> links;
    rc = filter_evaluate(cand, ref, r0, qry, n_cols, k, model, fp32, tables, bad_pair, [&](uint32_t row, uint32_t col, double d, uint32_t) {
        if (d <= max_dist) links.push_back(make_uint2(row, col));
    });
    if (rc) return rc;
    if (!links.empty()) HIPCHK(ctx, apply_links(cluster, ctx->stream, links, &roots));
    if (stats) {
        uint64_t pairs = 0;                                                                    // the printed off-diagonal pairs
        for (uint32_t r = r0; r < r1; ++r) pairs += std::min<uint64_t>((uint64_t)r + 1, n_cols) - (r < n_cols ? 1 : 0);
        stats->pairs = pairs;
        stats->pruned = counts[0];
        stats->joined_on_device = counts[1];
        stats->sent_to_host = cand.size();
        stats->clusters = roots;
    }
    return LASH_OK;
}

int lash_cluster_merge(lash_cluster *dst, const lash_cluster *src)
{
    if (!dst || !src || dst == src || dst->n != src->n) return LASH_EINVAL;
    std::vector<uint32_t> lab;
    const int rc = host_labels(src, lab);
    if (rc != LASH_OK) return rc;
    std::vector<uint2> links;
    for (uint32_t i = 0; i < dst->n; ++i)
        if (lab[i] != i) links.push_back(make_uint2(i, lab[i]));
    if (links.empty()) return LASH_OK;
    (void)hipSetDevice(dst->device);
    dst->touched = dst->n;
    uint64_t roots = 0;
    return apply_links(dst, nullptr, links, &roots) == hipSuccess ? LASH_OK : LASH_EHIP;       // (the device's default stream)
}

int lash_cluster_labels(const lash_cluster *c, uint32_t *out)
{
    if (!c || (c->n && !out)) return LASH_EINVAL;
    std::vector<uint32_t> lab;
    const int rc = host_labels(c, lab);
    if (rc != LASH_OK) return rc;
    std::copy(lab.begin(), lab.end(), out);
    return LASH_OK;
}

}  // extern "C"
