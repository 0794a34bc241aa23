// dist_tree.hip — `lash dist --tree` / `--cluster D --linkage average|complete`: agglomerative clustering of the N x N matrix of printed
// distances, merged on the GPU (include/lash_gfx950.h: lash_tree_*).  The matrix stays where the pair kernels' results already go, in
// device memory, and 2N - 1 nodes come back instead of N^2 cells.
//
// The rule.  Slots 0..N-1 hold one leaf each (size 1, height 0).  Step s = 0..N-2: among active slots i < j take the pair
// with the smallest key (D[i][j], i, j); record merge s = (node of i, node of j, D[i][j], size_i + size_j); node N + s lives on in slot
// i, slot j retires; for every other active k
//   average   D[i][k] = (size_i * D[i][k] + size_j * D[j][k]) / (size_i + size_j)     two products, one sum, one quotient, each rounded
//   single    D[i][k] = min(D[i][k], D[j][k])
//   complete  D[i][k] = max(D[i][k], D[j][k])
// and D[k][i] the same number.  Only + * / min max on doubles, contraction off, and one arg-min with a total order: the result is a
// function of the input bits, so a numpy model reproduces it bit for bit (tests/tree_model.py).
//
// State in device memory: D [N][N] f64 (the only large allocation), per row the cached minimum key (d, column) over active columns
// other than the row itself, sizes, active flags, node ids, the chosen pair of the current step, the list of rows to rescan, and the
// merge list.  lash_tree_build queues, per step, three plain launches on the context's stream and synchronizes once after the last:
//   select   one workgroup reduces the N cached keys to the global (d, i, j).  A row r with cached column c stands for the pair
//            (min(r, c), max(r, c)); the row i* of the true minimum pair (i*, j*) caches exactly j* (a lower column with the same d
//            would make a smaller pair key), so the minimum over rows is the minimum over pairs.  It appends the merge, updates
//            sizes, flags and node ids, and leaves (i, j, size_i, size_j) for the next kernel.
//   update   one thread per slot k: reads D[i][k] and D[j][k] (two coalesced rows), writes D[i][k] (coalesced) and D[k][i] (one
//            8-byte store per row: N strided stores).  Row k's cache: when its cached column is neither i nor j, the new (D[k][i], i)
//            replaces it iff it is the smaller key.  When it is i or j and the new D[k][i] is <= the cached d, (D[k][i], i) is the
//            row's minimum again (every other column's key was above the cached one, and i is below every column that tied with
//            it), so it is patched in place; otherwise the row goes on the rescan list.  Row i always does; row j's cache is retired.
//   rescan   one workgroup per listed row: coalesced 8-byte loads of the full row, the minimum (d, column) over active columns by
//            a wave64 shuffle reduction and one LDS round over the workgroup's four waves; equal d: the lower column.
// The first fill of the cache is one rescan of every row.  Cost per step: O(N) plus N per rescanned row.  A row is rescanned only
// when its nearest slot was merged AND moved away from it, which single linkage never does (min never grows) and a matrix of equal
// distances never does either (the patch above); the worst case, every row's nearest being the merged slot and moving away at every
// step, is O(N^2) per step.
//
// Later launches read what earlier ones left in device memory; the kernel boundary on one stream is the only ordering used.  There is
// no host round trip per step, no graph capture and no grid-wide synchronization.
#include "dist_tree.h"

#include <new>

#pragma clang fp contract(off)

namespace lash {

constexpr uint32_t TREE_SELECT_THREADS = 1024;    // one workgroup; tests/test_gpu_tree.py sizes around these three constants
constexpr uint32_t TREE_UPDATE_THREADS = 256;     // one thread per slot
constexpr uint32_t TREE_RESCAN_THREADS = 256;     // one workgroup per listed row
constexpr uint32_t TREE_RESCAN_GRID = 512;        // workgroups of a rescan launch; each takes list entries b, b + grid, ...

struct TreeStep { uint32_t i, j, size_i, size_j; };

struct TreeState {
    double *D;
    double *min_d;                                // [n] cached minimum key of every row: (min_d, min_c); a retired row: (+inf, NONE)
    uint32_t *min_c;
    uint32_t *size, *node;                        // [n]
    uint8_t *active;                              // [n]
    uint32_t *list;                               // [n] rows to rescan
    uint32_t *list_n;                             // [1]
    unsigned long long *rescanned;                // [1] rows rescanned by the steps before the current one
    TreeStep *step;                               // [1]
    lash_tree_merge *merges;                      // [n - 1]
    uint32_t n;
    int linkage;
};

// D[r][c] = D[c][r] = v for the staged rows [r0, r1) x columns [0, r]; stage is row-major [r1 - r0][ld]
__global__ void __launch_bounds__(256) tree_scatter_kernel(double *__restrict__ D, const double *__restrict__ stage, uint32_t n, uint32_t r0, uint32_t ld)
{
    const uint32_t r = r0 + blockIdx.y;
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c > r) return;                                                                          // (r < n and c <= r < n: the caller checked r1 <= n)
    const double v = stage[(size_t)blockIdx.y * ld + c];
    D[(size_t)r * n + c] = v;
    if (c != r) D[(size_t)c * n + r] = v;
}

__global__ void __launch_bounds__(256) tree_init_kernel(TreeState t)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < t.n) {
        t.size[k] = 1;
        t.node[k] = k;
        t.active[k] = 1;
        t.list[k] = k;                                                                          // the first fill: every row
        t.min_d[k] = HUGE_VAL;
        t.min_c[k] = TREE_NONE;
    }
    if (k == 0) { *t.list_n = t.n; *t.rescanned = 0; }
}

__global__ void __launch_bounds__(TREE_RESCAN_THREADS) tree_rescan_kernel(TreeState t)
{
    __shared__ double s_d[TREE_RESCAN_THREADS / 64];
    __shared__ uint32_t s_a[TREE_RESCAN_THREADS / 64], s_b[TREE_RESCAN_THREADS / 64];
    const uint32_t n_list = *t.list_n;                                                          // (<= n: one entry per slot at most)
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        const uint32_t r = t.list[e];
        const double *row = t.D + (size_t)r * t.n;
        double d = HUGE_VAL;
        uint32_t c_min = TREE_NONE, zero = 0;
        for (uint32_t c = threadIdx.x; c < t.n; c += TREE_RESCAN_THREADS) {
            if (c == r || !t.active[c]) continue;
            const double v = row[c];
            if (v < d || c_min == TREE_NONE) { d = v; c_min = c; }                              // (columns ascend per thread: a tie keeps the lower)
        }
        block_min_key<TREE_RESCAN_THREADS / 64>(d, c_min, zero, s_d, s_a, s_b);
        if (threadIdx.x == 0) {
            t.min_d[r] = c_min == TREE_NONE ? HUGE_VAL : d;
            t.min_c[r] = c_min;
        }
        __syncthreads();                                                                        // s_* are reused by the next entry
    }
}

__global__ void __launch_bounds__(TREE_SELECT_THREADS) tree_select_kernel(TreeState t, uint32_t s)
{
    __shared__ double s_d[TREE_SELECT_THREADS / 64];
    __shared__ uint32_t s_a[TREE_SELECT_THREADS / 64], s_b[TREE_SELECT_THREADS / 64];
    double d = HUGE_VAL;
    uint32_t a = TREE_NONE, b = TREE_NONE;
    for (uint32_t r = threadIdx.x; r < t.n; r += TREE_SELECT_THREADS) {
        const uint32_t c = t.min_c[r];
        if (c == TREE_NONE) continue;
        const double v = t.min_d[r];
        const uint32_t lo = r < c ? r : c, hi = r < c ? c : r;
        if (key_less(v, lo, hi, d, a, b)) { d = v; a = lo; b = hi; }
    }
    block_min_key<TREE_SELECT_THREADS / 64>(d, a, b, s_d, s_a, s_b);
    if (threadIdx.x == 0) {
        // (a pair always exists: step s < n - 1 has n - s >= 2 active slots, each with a cached column; were the state ever broken,
        // nothing is indexed with it: the build sees the marker and fails)
        if (a >= t.n || b >= t.n) {
            lash_tree_merge none;
            none.a = none.b = TREE_NONE; none.height = 0.0; none.size = 0;
            t.merges[s] = none;
            *t.step = TreeStep{TREE_NONE, TREE_NONE, 0, 0};
            return;
        }
        const uint32_t si = t.size[a], sj = t.size[b];
        lash_tree_merge m;
        m.a = t.node[a]; m.b = t.node[b]; m.height = d; m.size = si + sj;
        t.merges[s] = m;
        *t.step = TreeStep{a, b, si, sj};
        t.size[a] = si + sj;
        t.node[a] = t.n + s;
        t.active[b] = 0;
        *t.rescanned += *t.list_n;                                                              // the list of the step before is done
        *t.list_n = 0;
    }
}

__global__ void __launch_bounds__(TREE_UPDATE_THREADS) tree_update_kernel(TreeState t)
{
    const uint32_t k = blockIdx.x * TREE_UPDATE_THREADS + threadIdx.x;
    if (k >= t.n) return;
    const TreeStep st = *t.step;
    if (st.i >= t.n || st.j >= t.n) return;
    if (k == st.j) { t.min_d[k] = HUGE_VAL; t.min_c[k] = TREE_NONE; return; }                    // retired
    if (k == st.i) { t.list[atomicAdd(t.list_n, 1u)] = k; return; }                             // its whole row changes
    if (!t.active[k]) return;
    const double dik = t.D[(size_t)st.i * t.n + k], djk = t.D[(size_t)st.j * t.n + k];
    double v;
    if (t.linkage == LASH_LINKAGE_AVERAGE) {
        const double wi = (double)st.size_i, wj = (double)st.size_j;
        const double pi = wi * dik, pj = wj * djk;                                              // (contraction is off: four roundings)
        v = (pi + pj) / (wi + wj);
    } else if (t.linkage == LASH_LINKAGE_SINGLE) v = djk < dik ? djk : dik;
    else v = djk > dik ? djk : dik;
    t.D[(size_t)st.i * t.n + k] = v;
    t.D[(size_t)k * t.n + st.i] = v;
    const double cd = t.min_d[k];
    const uint32_t cc = t.min_c[k];
    if (cc == st.i || cc == st.j) {
        if (v <= cd) { t.min_d[k] = v; t.min_c[k] = st.i; }
        else t.list[atomicAdd(t.list_n, 1u)] = k;                                               // (at most one entry per slot: the list holds n)
    } else if (v < cd || (v == cd && st.i < cc)) { t.min_d[k] = v; t.min_c[k] = st.i; }
}

}  // namespace lash

namespace {

int tree_error(lash_ctx *ctx, const char *text)
{
    ctx->err = text;
    return LASH_EINVAL;
}

}  // namespace

extern "C" {

int lash_tree_create(lash_ctx *ctx, uint32_t n, lash_tree **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    if (!ctx) return LASH_EINVAL;
    lash_tree *t = new (std::nothrow) lash_tree;
    if (!t) return LASH_ENOMEM;
    t->device = ctx->device;
    t->n = n;
    t->row_set.assign(n, 0);
    (void)hipSetDevice(ctx->device);
    const size_t bytes = (size_t)n * n * sizeof(double);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->d_D), bytes + 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char buf[160];
        snprintf(buf, sizeof buf, "lash_tree_create: the %u x %u distance matrix needs %llu bytes of device memory: %s", n, n,
                 (unsigned long long)bytes, hipGetErrorString(e));
        ctx->err = buf;
        delete t;
        return e == hipErrorOutOfMemory ? LASH_ENOMEM : LASH_EHIP;
    }
    *out = t;
    return LASH_OK;
}

void lash_tree_free(lash_ctx *ctx, lash_tree *t)
{
    (void)ctx;
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->d_D) (void)hipFree(t->d_D);
    if (t->d_stage) (void)hipFree(t->d_stage);
    delete t;
}

int lash_tree_set_rows(lash_ctx *ctx, lash_tree *t, uint32_t r0, uint32_t r1, const double *d)
{
    using namespace lash;
    if (!ctx || !t || t->device != ctx->device || r0 > r1 || r1 > t->n || (r1 > r0 && !d)) return LASH_EINVAL;
    if (t->built) return tree_error(ctx, "lash_tree_set_rows: the tree has been built");
    if (r0 == r1) return LASH_OK;
    (void)hipSetDevice(t->device);
    const uint32_t ld = r1;
    for (uint32_t r = r0; r < r1; ++r) {
        const double *row = d + (size_t)(r - r0) * ld;
        for (uint32_t c = 0; c <= r && !(t->has_nan && t->has_inf); ++c) {
            const double v = row[c];
            if (v != v) { if (!t->has_nan) { t->has_nan = true; t->nan_row = r; t->nan_col = c; } }
            else if (std::isinf(v) && !t->has_inf) { t->has_inf = true; t->inf_row = r; t->inf_col = c; }
        }
        t->row_set[r] = 1;
    }
    // pieces of at most ~64 MB of rows (and 65 535 rows: the grid's y) go through one staging buffer
    const uint32_t piece = (uint32_t)std::min<size_t>(65535, std::max<size_t>(1, (size_t(8) << 20) / ld));
    const size_t want = (size_t)std::min<uint32_t>(piece, r1 - r0) * ld;
    if (want > t->stage_cap) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (t->d_stage) { (void)hipFree(t->d_stage); t->d_stage = nullptr; t->stage_cap = 0; }
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&t->d_stage), want * sizeof(double)));
        t->stage_cap = want;
    }
    for (uint32_t a = r0; a < r1; a += piece) {
        const uint32_t b = std::min<uint64_t>((uint64_t)a + piece, r1);
        HIPCHK(ctx, hipMemcpyAsync(t->d_stage, d + (size_t)(a - r0) * ld, (size_t)(b - a) * ld * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(tree_scatter_kernel, dim3((b + 255) / 256, b - a), dim3(256), 0, ctx->stream, t->d_D, t->d_stage, t->n, a, ld);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                                           // the staging buffer and `d` are free again
    }
    return LASH_OK;
}

int lash_tree_get_rows(lash_ctx *ctx, const lash_tree *t, uint32_t r0, uint32_t r1, double *out)
{
    if (!ctx || !t || t->device != ctx->device || r0 > r1 || r1 > t->n || (r1 > r0 && !out)) return LASH_EINVAL;
    if (t->built) return tree_error(ctx, "lash_tree_get_rows: the tree has been built (the build consumes the matrix)");
    if (r0 == r1) return LASH_OK;
    (void)hipSetDevice(t->device);
    HIPCHK(ctx, hipMemcpyAsync(out, t->d_D + (size_t)r0 * t->n, (size_t)(r1 - r0) * t->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

int lash_tree_build(lash_ctx *ctx, lash_tree *t, int linkage, lash_tree_merge *out, lash_tree_stats *stats)
{
    using namespace lash;
    if (stats) *stats = lash_tree_stats{};
    if (!ctx || !t || t->device != ctx->device) return LASH_EINVAL;
    const uint32_t n = t->n;
    if (linkage != LASH_LINKAGE_AVERAGE && linkage != LASH_LINKAGE_SINGLE && linkage != LASH_LINKAGE_COMPLETE)
        return tree_error(ctx, "lash_tree_build: linkage must be LASH_LINKAGE_AVERAGE, _SINGLE or _COMPLETE");
    if (t->built) return tree_error(ctx, "lash_tree_build: the tree has been built (the build consumes the matrix)");
    if (n > 1 && !out) return LASH_EINVAL;
    char buf[160];
    for (uint32_t r = 0; r < n; ++r)
        if (!t->row_set[r]) {
            snprintf(buf, sizeof buf, "lash_tree_build: row %u has not been set", r);
            return tree_error(ctx, buf);
        }
    if (t->has_nan) {
        snprintf(buf, sizeof buf, "lash_tree_build: the distance of row %u and col %u is NaN: the linkage is undefined", t->nan_row, t->nan_col);
        return tree_error(ctx, buf);
    }
    t->built = true;
    if (stats) stats->bytes = (uint64_t)n * n * sizeof(double);
    if (n < 2) return LASH_OK;
    (void)hipSetDevice(t->device);

    // the small state, one allocation: 8-byte fields first
    const size_t n8 = ((size_t)n + 7) & ~size_t(7);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~size_t(15); return o; };
    const size_t o_min_d = take(n8 * 8), o_merges = take((size_t)(n - 1) * sizeof(lash_tree_merge)), o_resc = take(8), o_step = take(sizeof(TreeStep)),
                 o_min_c = take(n8 * 4), o_size = take(n8 * 4), o_node = take(n8 * 4), o_list = take(n8 * 4), o_list_n = take(4), o_active = take(n8);
    uint8_t *base = nullptr;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&base), at));
    struct Guard { uint8_t *p; ~Guard() { (void)hipFree(p); } } guard{base};
    TreeState s{};
    s.D = t->d_D;
    s.min_d = reinterpret_cast<double *>(base + o_min_d);
    s.merges = reinterpret_cast<lash_tree_merge *>(base + o_merges);
    s.rescanned = reinterpret_cast<unsigned long long *>(base + o_resc);
    s.step = reinterpret_cast<TreeStep *>(base + o_step);
    s.min_c = reinterpret_cast<uint32_t *>(base + o_min_c);
    s.size = reinterpret_cast<uint32_t *>(base + o_size);
    s.node = reinterpret_cast<uint32_t *>(base + o_node);
    s.list = reinterpret_cast<uint32_t *>(base + o_list);
    s.list_n = reinterpret_cast<uint32_t *>(base + o_list_n);
    s.active = base + o_active;
    s.n = n;
    s.linkage = linkage;

    hipStream_t st = ctx->stream;
    const uint32_t n_blocks = (n + TREE_UPDATE_THREADS - 1) / TREE_UPDATE_THREADS;
    const uint32_t rescan_grid = std::min(n, TREE_RESCAN_GRID);
    hipLaunchKernelGGL(tree_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, s);
    hipLaunchKernelGGL(tree_rescan_kernel, dim3(rescan_grid), dim3(TREE_RESCAN_THREADS), 0, st, s);
    HIPCHK(ctx, hipGetLastError());
    for (uint32_t step = 0; step + 1 < n; ++step) {
        hipLaunchKernelGGL(tree_select_kernel, dim3(1), dim3(TREE_SELECT_THREADS), 0, st, s, step);
        hipLaunchKernelGGL(tree_update_kernel, dim3(n_blocks), dim3(TREE_UPDATE_THREADS), 0, st, s);
        hipLaunchKernelGGL(tree_rescan_kernel, dim3(rescan_grid), dim3(TREE_RESCAN_THREADS), 0, st, s);
        if ((step & 1023u) == 1023u) HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipGetLastError());
    unsigned long long rescanned = 0;
    uint32_t last_list = 0;
    HIPCHK(ctx, hipMemcpyAsync(out, s.merges, (size_t)(n - 1) * sizeof(lash_tree_merge), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&rescanned, s.rescanned, sizeof rescanned, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&last_list, s.list_n, sizeof last_list, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i + 1 < n; ++i)
        if (out[i].a == TREE_NONE) return tree_error(ctx, "lash_tree_build: no pair left to merge (internal error)");
    if (stats) {
        stats->steps = n - 1;
        stats->rescanned_rows = rescanned + last_list;
    }
    return LASH_OK;
}

}  // extern "C"
