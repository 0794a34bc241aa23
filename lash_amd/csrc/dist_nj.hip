// dist_nj.hip — `lash dist --tree --nj`: a neighbour-joining tree of the N x N matrix of printed distances, joined on the GPU
// (include/lash_gfx950.h: lash_tree_build_nj).  It works on the lash_tree matrix that dist_tree.hip creates and fills.
//
// The rule.  Slots 0..n-1 hold one leaf each; the slot index is the label that breaks ties.  R[i] starts from +0.0 and
// takes D[i][c] for c = 0, 1, .., n-1 in that order, c = i skipped, each add rounded.  Join step s = 0, 1, .. while r >= 3 (r = active
// slots, w = (double)(r - 2)): for active i < j
//   Q = ((w * D[i][j]) - R[i]) - R[j]                             three separately rounded operations
// and the pair with the smallest key (Q, i, j) is joined:
//   len_i = D[i][j] * 0.5 + (R[i] - R[j]) / (2.0 * w)      len_j = D[i][j] - len_i      join s = (node of i, node of j, len_i, len_j)
// for every other active k
//   v = ((D[i][k] + D[j][k]) - D[i][j]) * 0.5      R[k] = ((R[k] - D[i][k]) - D[j][k]) + v      D[i][k] = D[k][i] = v
// then R[i] = ((R[i] + R[j]) - (double)r * D[i][j]) * 0.5; node n + s lives on in slot i, slot j retires.  At r = 2 the closing record
// (node of i, node of j, D[i][j], 0) for the remaining slots i < j.  n - 1 records for n >= 2.  Lengths may be negative and are reported
// as computed.  Row sums are carried, never re-summed: that is part of the rule, so the result is a function of the input bits and a
// numpy model reproduces it bit for bit (tests/nj_model.py).  The rule is worded on slot labels, not on where a row lies in memory.
//
// lash_tree_build_nj queues plain launches on the context's stream and synchronizes once after the last:
//   rowsum   once: one thread per row i, columns ascending, reading D[c][i] (the mirror holds the same bits; these loads coalesce)
//   scan     per step, the hot kernel: up to NJ_SCAN_GRID workgroups take the active rows grid-strided (the triangle makes rows unequal,
//            striding balances them; a retired row is skipped whole).  The threads stride the columns above the row's diagonal with
//            16-byte loads from the first even element on (the head and the tail element, where there is one, are 8-byte loads of thread
//            0), form Q from D, R[] and active[] (small: they stay in L2) and keep their minimum key; a wave64 shuffle reduction and one
//            LDS round give the workgroup's, which goes to part[blockIdx.x].  A minimum under a total order is the same in any order.
//   select   one workgroup reduces part[], writes the join with both lengths, the new R[i], node and active, and leaves (i, j, D[i][j])
//            for update.  A broken state (no pair) writes a marker and indexes nothing; the build then fails.
//   update   one thread per slot k: v, R[k], D[i][k] (coalesced) and D[k][i] (one 8-byte store per row).
//   closing  once, one thread: the record of the last two slots.
// The scan reads the active rows' upper parts, retired columns included: 8 * sum over r of about r * N / 2 bytes, about 2 N^3 in all.
#include "dist_tree.h"

#pragma clang fp contract(off)

namespace lash {

constexpr uint32_t NJ_SCAN_THREADS = 256;         // a workgroup sweeps 2 x 256 columns at a time; tests/test_gpu_nj.py sizes around these
constexpr uint32_t NJ_SCAN_GRID = 1024;           // workgroups of a scan launch; above it a workgroup takes rows b, b + grid, ...
constexpr uint32_t NJ_SELECT_THREADS = 1024;      // one workgroup: one thread per entry of part[]
constexpr uint32_t NJ_UPDATE_THREADS = 256;       // one thread per slot
static_assert(NJ_SCAN_GRID <= NJ_SELECT_THREADS, "select reads one entry of part[] per thread");

struct NjStep { uint32_t i, j; double dij; };

struct NjState {
    double *D;                                    // [n][n]
    double *R;                                    // [n] the carried row sums
    double *part_q;                               // [NJ_SCAN_GRID] the workgroups' minimum keys of the current step
    uint32_t *part_i, *part_j;
    uint32_t *node;                               // [n]
    uint8_t *active;                              // [n]
    NjStep *step;                                 // [1]
    lash_nj_join *joins;                          // [n - 1]
    uint32_t n;
};

__global__ void __launch_bounds__(256) nj_rowsum_kernel(NjState t)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.n) return;
    double sum = 0.0;
    for (uint32_t c = 0; c < t.n; ++c)
        if (c != i) sum = sum + t.D[(size_t)c * t.n + i];
    t.R[i] = sum;
    t.node[i] = i;
    t.active[i] = 1;
}

__global__ void __launch_bounds__(NJ_SCAN_THREADS) nj_scan_kernel(NjState t, double w)
{
    __shared__ double s_d[NJ_SCAN_THREADS / 64];
    __shared__ uint32_t s_a[NJ_SCAN_THREADS / 64], s_b[NJ_SCAN_THREADS / 64];
    const uint32_t n = t.n;
    double q = HUGE_VAL;
    uint32_t a = TREE_NONE, b = TREE_NONE;
    for (uint32_t i = blockIdx.x; i + 1 < n; i += gridDim.x) {                                  // (row n - 1 has no column above it)
        if (!t.active[i]) continue;
        const double ri = t.R[i];
        const double *row = t.D + (size_t)i * n;
        auto look = [&](double d, uint32_t j) {                                                 // (i < j < n)
            if (!t.active[j]) return;
            const double wd = w * d;
            const double v = (wd - ri) - t.R[j];
            if (key_less(v, i, j, q, a, b)) { q = v; a = i; b = j; }
        };
        // columns [i + 1, n): D is 256-byte aligned, so element i * n + j is 16-byte aligned iff it is even
        const uint32_t c0 = i + 1;
        const uint32_t p0 = c0 + (uint32_t)(((size_t)i * n + c0) & 1u);                         // (<= n)
        if (threadIdx.x == 0 && p0 != c0) look(row[c0], c0);
        for (uint32_t c = p0 + 2u * threadIdx.x; c + 1 < n; c += 2u * NJ_SCAN_THREADS) {
            const double2 d = *reinterpret_cast<const double2 *>(row + c);
            look(d.x, c);
            look(d.y, c + 1);
        }
        if (threadIdx.x == 0 && ((n - p0) & 1u)) look(row[n - 1], n - 1);                       // (p0 < n here: the pairs left one over)
    }
    block_min_key<NJ_SCAN_THREADS / 64>(q, a, b, s_d, s_a, s_b);
    if (threadIdx.x == 0) { t.part_q[blockIdx.x] = q; t.part_i[blockIdx.x] = a; t.part_j[blockIdx.x] = b; }
}

// step s with r active slots; part[] holds n_part keys
__global__ void __launch_bounds__(NJ_SELECT_THREADS) nj_select_kernel(NjState t, uint32_t s, uint32_t n_part, uint32_t r)
{
    __shared__ double s_d[NJ_SELECT_THREADS / 64];
    __shared__ uint32_t s_a[NJ_SELECT_THREADS / 64], s_b[NJ_SELECT_THREADS / 64];
    double q = HUGE_VAL;
    uint32_t a = TREE_NONE, b = TREE_NONE;
    for (uint32_t p = threadIdx.x; p < n_part; p += NJ_SELECT_THREADS) {
        const double pq = t.part_q[p];
        const uint32_t pa = t.part_i[p], pb = t.part_j[p];
        if (key_less(pq, pa, pb, q, a, b)) { q = pq; a = pa; b = pb; }
    }
    block_min_key<NJ_SELECT_THREADS / 64>(q, a, b, s_d, s_a, s_b);
    if (threadIdx.x == 0) {
        // (a pair always exists: r >= 3 active slots; were the state ever broken, nothing is indexed with it: the build sees the marker)
        if (a >= t.n || b >= t.n) {
            lash_nj_join none;
            none.a = none.b = TREE_NONE; none.len_a = none.len_b = 0.0;
            t.joins[s] = none;
            *t.step = NjStep{TREE_NONE, TREE_NONE, 0.0};
            return;
        }
        const double dij = t.D[(size_t)a * t.n + b], ri = t.R[a], rj = t.R[b];
        const double w = (double)(r - 2u);
        const double half = dij * 0.5, diff = ri - rj, twice = 2.0 * w;
        lash_nj_join m;
        m.a = t.node[a]; m.b = t.node[b];
        m.len_a = half + diff / twice;
        m.len_b = dij - m.len_a;
        t.joins[s] = m;
        *t.step = NjStep{a, b, dij};
        const double both = ri + rj, off = (double)r * dij;
        t.R[a] = (both - off) * 0.5;
        t.node[a] = t.n + s;
        t.active[b] = 0;
    }
}

__global__ void __launch_bounds__(NJ_UPDATE_THREADS) nj_update_kernel(NjState t)
{
    const uint32_t k = blockIdx.x * NJ_UPDATE_THREADS + threadIdx.x;
    if (k >= t.n) return;
    const NjStep st = *t.step;
    if (st.i >= t.n || st.j >= t.n) return;
    if (k == st.i || k == st.j || !t.active[k]) return;
    const double dik = t.D[(size_t)st.i * t.n + k], djk = t.D[(size_t)st.j * t.n + k];
    const double sum = dik + djk;
    const double v = (sum - st.dij) * 0.5;
    const double less = t.R[k] - dik;
    t.R[k] = (less - djk) + v;
    t.D[(size_t)st.i * t.n + k] = v;
    t.D[(size_t)k * t.n + st.i] = v;
}

// r = 2: the record of the two slots that are left, at joins[n - 2]
__global__ void nj_closing_kernel(NjState t)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t i = TREE_NONE, j = TREE_NONE, left = 0;
    for (uint32_t k = 0; k < t.n; ++k)
        if (t.active[k]) {
            if (left == 0) i = k;
            else if (left == 1) j = k;
            ++left;
        }
    lash_nj_join m;
    if (left != 2) { m.a = m.b = TREE_NONE; m.len_a = m.len_b = 0.0; }
    else { m.a = t.node[i]; m.b = t.node[j]; m.len_a = t.D[(size_t)i * t.n + j]; m.len_b = 0.0; }
    t.joins[t.n - 2] = m;
}

}  // namespace lash

extern "C" int lash_tree_build_nj(lash_ctx *ctx, lash_tree *t, lash_nj_join *out, lash_tree_stats *stats)
{
    using namespace lash;
    if (stats) *stats = lash_tree_stats{};
    if (!ctx || !t || t->device != ctx->device) return LASH_EINVAL;
    const uint32_t n = t->n;
    char buf[160];
    auto refuse = [&]() { ctx->err = buf; return LASH_EINVAL; };
    if (t->built) { snprintf(buf, sizeof buf, "lash_tree_build_nj: the tree has been built (the build consumes the matrix)"); return refuse(); }
    if (n > 1 && !out) return LASH_EINVAL;
    for (uint32_t r = 0; r < n; ++r)
        if (!t->row_set[r]) { snprintf(buf, sizeof buf, "lash_tree_build_nj: row %u has not been set", r); return refuse(); }
    if (t->has_nan) {
        snprintf(buf, sizeof buf, "lash_tree_build_nj: the distance of row %u and col %u is NaN: the tree is undefined", t->nan_row, t->nan_col);
        return refuse();
    }
    if (t->has_inf) {
        snprintf(buf, sizeof buf, "lash_tree_build_nj: the distance of row %u and col %u is not finite: neighbour joining would subtract "
                                  "infinities", t->inf_row, t->inf_col);
        return refuse();
    }
    t->built = true;
    if (stats) stats->bytes = (uint64_t)n * n * sizeof(double);
    if (n < 2) return LASH_OK;
    (void)hipSetDevice(t->device);

    // the small state, one allocation: 8-byte fields first
    const size_t n8 = ((size_t)n + 7) & ~size_t(7);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~size_t(15); return o; };
    const size_t o_R = take(n8 * 8), o_part_q = take((size_t)NJ_SCAN_GRID * 8), o_joins = take((size_t)(n - 1) * sizeof(lash_nj_join)),
                 o_step = take(sizeof(NjStep)), o_part_i = take((size_t)NJ_SCAN_GRID * 4), o_part_j = take((size_t)NJ_SCAN_GRID * 4),
                 o_node = take(n8 * 4), o_active = take(n8);
    uint8_t *base = nullptr;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&base), at));
    struct Guard { uint8_t *p; ~Guard() { (void)hipFree(p); } } guard{base};
    NjState s{};
    s.D = t->d_D;
    s.R = reinterpret_cast<double *>(base + o_R);
    s.part_q = reinterpret_cast<double *>(base + o_part_q);
    s.joins = reinterpret_cast<lash_nj_join *>(base + o_joins);
    s.step = reinterpret_cast<NjStep *>(base + o_step);
    s.part_i = reinterpret_cast<uint32_t *>(base + o_part_i);
    s.part_j = reinterpret_cast<uint32_t *>(base + o_part_j);
    s.node = reinterpret_cast<uint32_t *>(base + o_node);
    s.active = base + o_active;
    s.n = n;

    hipStream_t st = ctx->stream;
    const uint32_t n_blocks = (n + NJ_UPDATE_THREADS - 1) / NJ_UPDATE_THREADS;
    const uint32_t scan_grid = std::min(n - 1, NJ_SCAN_GRID);                                   // rows 0 .. n - 2 have columns above them
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3((n + 255) / 256), dim3(256), 0, st, s);
    HIPCHK(ctx, hipGetLastError());
    for (uint32_t step = 0; step + 2 < n; ++step) {
        const uint32_t r = n - step;
        hipLaunchKernelGGL(nj_scan_kernel, dim3(scan_grid), dim3(NJ_SCAN_THREADS), 0, st, s, (double)(r - 2));
        hipLaunchKernelGGL(nj_select_kernel, dim3(1), dim3(NJ_SELECT_THREADS), 0, st, s, step, scan_grid, r);
        hipLaunchKernelGGL(nj_update_kernel, dim3(n_blocks), dim3(NJ_UPDATE_THREADS), 0, st, s);
        if ((step & 1023u) == 1023u) HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(nj_closing_kernel, dim3(1), dim3(1), 0, st, s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, s.joins, (size_t)(n - 1) * sizeof(lash_nj_join), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i + 1 < n; ++i)
        if (out[i].a == TREE_NONE) { snprintf(buf, sizeof buf, "lash_tree_build_nj: no pair left to join (internal error)"); return refuse(); }
    if (stats) stats->steps = n - 1;
    return LASH_OK;
}
