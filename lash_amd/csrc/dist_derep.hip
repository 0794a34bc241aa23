// dist_derep.hip — `lash dist --derep D`: greedy representatives of a triangle run, chosen while a block's pair statistics are still in
// HBM (include/lash_gfx950.h: lash_sketch_set_pair_block_derep, lash_derep_*).  Two names are WITHIN D iff `--max-dist D` prints their
// pair: the host's exact distance d (dist_pair_host, in f32 under fp32) passes d <= D, NaN never.  Walking the names in row order,
// name i is a REPRESENTATIVE iff no representative j < i is within D of it, and otherwise a MEMBER of the first such j.  This is
// greedy incremental clustering (CD-HIT, dRep, skDER): not transitive, and first, not nearest — which is what lets the device prune:
// a column that is not a representative needs no distance at all, and a row that has surely found a representative needs nothing
// beyond it.
//
// State: rep[N] (u32) in HBM per accumulator with a host mirror: rep[i] == i a representative, rep[i] == j < i a member of j,
// 0xFFFFFFFF undecided.  Blocks arrive in row order, contiguous from 0 (`decided` rows so far): a row is decided from the
// representatives among the rows before it, so every column q < r0 of a block is decided when the block runs and stays so.
//
// Per block of rows [r0, r1) x columns [0, n_cols) of the lower triangle, after the pair kernels and the expected-collision GEMM:
//   mark   the tiles of mark_tiles (dist_filter.h).  For each pair strictly below the diagonal: a column q < r0 that is not a
//          representative is PRUNED before any arithmetic.  Otherwise (a representative, or an in-block column q >= r0, which the host
//          decides in this same call) the interval [d_lo, d_hi] of pair_interval_dev, which holds the host's d:
//            OUT       d_lo > D (PAIR_ONE: 1 > D), or a NaN of hmh / ull             -> nothing
//            SURE HIT  q < r0 and d_hi <= D (PAIR_ONE: 1 <= D)                      -> mask bit, first_sure[r] = min(first_sure[r], q)
//            UNSURE    everything else, every pair the device cannot place, a NaN of hll   -> mask bit
//   trim   over the mask words only, no distance arithmetic: clears the bits of the columns > first_sure[r] and rewrites the tile
//          counts.  A row with a sure hit in an earlier block then brings back that hit and the undecided or unplaceable pairs
//          before it, and nothing from its own block (whose columns are all >= r0 > first_sure[r]).
//   host   within_compact, then a walk over the candidates in (row, col) order with the host's exact arithmetic: a row stops at its
//          first column that is a representative (in-block columns have just been decided by this walk) with d <= D; that column is
//          its representative, and without one the row is a representative itself.  rep[r0, r1) goes back to the device.
//
// Soundness.
//   The row's answer is the smallest representative column q with d(row, q) <= D.  Call it q*.
//   Pruned columns are not representatives: they cannot be q* and the walk of the contract skips them too.
//   An OUT pair has d > D or NaN: it is not q* and it is not a pair the host refuses (the device placed it).
//   first_sure[r] = f means d(row, f) <= d_hi <= D for a representative f, so q* <= f: no column > f matters, neither for the answer nor
//     for the refusal, because the contract's walk stops at q* <= f.  The bit of f itself stays.
//   Every representative (or in-block) column q <= f, or any q when the row has no sure hit, with d <= D is SURE or UNSURE, hence a
//     candidate; so is every pair the device cannot place.  The host walk therefore meets, in column order, every pair the contract's
//     walk could stop at or be refused on, evaluates each exactly, and skips in-block columns that turned out to be members without
//     evaluating them.  LASH_ERANGE is returned iff it meets a refused pair before the row stops.
//
// Concurrency.  rep is read-only while a block's kernels run (only columns q < r0 are read, and they were uploaded before).  The only
// write shared between workgroups is atomicMin on first_sure[r], a 32-bit vector atomic whose result does not depend on the order;
// the trim kernel runs after the mark kernel on the same stream.
#include "dist_filter.h"

#include <algorithm>
#include <new>

struct lash_derep {
    int device = 0;
    uint32_t n = 0;
    uint32_t decided = 0;                        // rows [0, decided) are decided, on the device and in `rep`
    uint32_t representatives = 0;                // among them
    uint32_t *d_rep = nullptr;                   // [n]
    uint32_t *d_first = nullptr;                 // [first_cap]: the block's first sure hit per row
    size_t first_cap = 0;
    unsigned long long *d_counts = nullptr;      // [2]: pruned as not a representative, bits the trim cleared
    std::vector<uint32_t> rep;                   // the host mirror
};

namespace lash {

constexpr uint32_t DEREP_UNDECIDED = 0xFFFFFFFFu;

struct DerepArgs {
    const uint32_t *rep;
    uint32_t *first_sure;                        // [nr], DEREP_UNDECIDED = none
    unsigned long long *counts;
    double max_dist;
    uint32_t r0;
};

namespace {

// the pair (block row r, column q) strictly below the diagonal.  true: the pair goes back to the host.
__device__ inline bool derep_pair(const WithinArgs &a, const DerepArgs &c, uint32_t r, uint32_t q, uint32_t &pruned)
{
    const bool earlier = q < c.r0;
    if (earlier && c.rep[q] != q) { ++pruned; return false; }                            // not a representative: no arithmetic
    double sim, sim_low, d_lo, d_hi;
    if (!pair_similarity_dev(a, r, q, &sim, &sim_low)) return true;                     // the host's
    if (pair_interval_dev(a, sim, sim_low, &d_lo, &d_hi) == PAIR_NAN) return a.algo == LASH_HLL;
    if (d_lo > c.max_dist) return false;                                                // out
    if (earlier && d_hi <= c.max_dist) atomicMin(c.first_sure + r, q);                  // a sure hit
    return true;
}

}  // namespace

__global__ void __launch_bounds__(256) derep_mark_kernel(WithinArgs a, DerepArgs c, uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count)
{
    __shared__ uint32_t s_pruned;
    if (threadIdx.x == 0) s_pruned = 0;
    __syncthreads();
    uint32_t pruned = 0;
    mark_tiles(a, mask, tile_count, [&](uint32_t r, uint32_t q) { return q < c.r0 + r && derep_pair(a, c, r, q, pruned); });
    if (pruned) atomicAdd(&s_pruned, pruned);
    __syncthreads();
    if (threadIdx.x == 0 && s_pruned) atomicAdd(c.counts + 0, (unsigned long long)s_pruned);
}

// One wave per tile: lane w < WF_WORDS owns mask word w.  Clears the bits of the columns beyond the row's first sure hit and rewrites
// the tile's count.  A tile with count 0 is skipped: nothing to clear, and above the diagonal its words were never written.
__global__ void __launch_bounds__(256) derep_trim_kernel(uint32_t tiles_x, uint64_t n_tiles, const uint32_t *__restrict__ first_sure,
                                                         uint64_t *__restrict__ mask, uint32_t *__restrict__ tile_count,
                                                         unsigned long long *__restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t tile = (uint64_t)blockIdx.x * 4u + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * 4u) {
        if (tile_count[tile] == 0) continue;                                            // (uniform across the wave)
        const uint32_t r = (uint32_t)(tile / tiles_x), c0 = (uint32_t)(tile % tiles_x) * WF_TILE;
        const uint32_t fs = first_sure[r];
        if (fs == DEREP_UNDECIDED || (uint64_t)fs >= (uint64_t)c0 + WF_TILE - 1u) continue;   // no hit, or at / beyond the tile's last column
        uint32_t kept = 0, cleared = 0;
        if (lane < WF_WORDS) {
            const uint64_t at = tile * WF_WORDS + lane;
            const uint64_t w0 = (uint64_t)c0 + lane * 64u;                              // the word's first column
            const uint64_t old = mask[at];
            uint64_t now = old;
            if (w0 > fs) now = 0;
            else if (fs - w0 < 63u) now = old & ((2ull << (fs - w0)) - 1ull);           // columns w0 .. fs
            if (now != old) mask[at] = now;
            kept = (uint32_t)__popcll(now);
            cleared = (uint32_t)__popcll(old) - kept;
        }
        for (uint32_t d = 8; d; d >>= 1) { kept += __shfl_xor(kept, d); cleared += __shfl_xor(cleared, d); }   // over lanes 0 .. 15
        if (lane == 0 && cleared) {
            tile_count[tile] = kept;
            atomicAdd(counts + 1, (unsigned long long)cleared);
        }
    }
}

}  // namespace lash

extern "C" {

int lash_derep_create(lash_ctx *ctx, uint32_t n, lash_derep **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    if (!ctx) return LASH_EINVAL;
    lash_derep *c = new (std::nothrow) lash_derep;
    if (!c) return LASH_ENOMEM;
    c->device = ctx->device;
    c->n = n;
    c->rep.assign(n, lash::DEREP_UNDECIDED);
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->d_rep), (size_t)n * 4 + 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_counts), 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->d_rep, 0xFF, (size_t)n * 4 + 4);
    if (e != hipSuccess) {
        lash_derep_free(c);
        return fail(ctx, e == hipErrorOutOfMemory ? LASH_ENOMEM : LASH_EHIP, "lash_derep_create", e);
    }
    *out = c;
    return LASH_OK;
}

void lash_derep_free(lash_derep *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_rep) (void)hipFree(c->d_rep);
    if (c->d_first) (void)hipFree(c->d_first);
    if (c->d_counts) (void)hipFree(c->d_counts);
    delete c;
}

int lash_sketch_set_pair_block_derep(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry, uint32_t n_cols,
                                     int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables, double max_dist, lash_derep *acc,
                                     lash_derep_stats *stats, uint64_t *bad_pair)
{
    using namespace lash;
    if (stats) *stats = lash_derep_stats{};
    if (!acc || std::isnan(max_dist) || !ctx || acc->device != ctx->device) return LASH_EINVAL;
    if (r0 != acc->decided || r1 > acc->n || n_cols > acc->n || n_cols < r1) return LASH_EINVAL;   // in row order, every column below its rows
    int rc;
    WithinBlock b;
    if ((rc = within_block(ctx, ref, r0, r1, qry, n_cols, 1, k, model, fp32, ull_estimator, b)) || !b.a.n_tiles) return rc;
    const WithinArgs &a = b.a;
    const uint32_t nr = r1 - r0;

    if (nr > acc->first_cap) {
        if (acc->d_first) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(acc->d_first); acc->d_first = nullptr; acc->first_cap = 0; }
        const size_t want = (size_t)nr + nr / 4 + 64;
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&acc->d_first), want * 4));
        acc->first_cap = want;
    }
    DerepArgs c{};
    c.rep = acc->d_rep;
    c.first_sure = acc->d_first;
    c.counts = acc->d_counts;
    c.max_dist = max_dist;
    c.r0 = r0;
    HIPCHK(ctx, hipMemsetAsync(acc->d_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(acc->d_first, 0xFF, (size_t)nr * 4, ctx->stream));
    hipLaunchKernelGGL(derep_mark_kernel, dim3(mark_grid(a.n_tiles)), dim3(256), 0, ctx->stream, a, c, b.d_mask, b.d_cnt);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(derep_trim_kernel, dim3(mark_grid((a.n_tiles + 3) / 4)), dim3(256), 0, ctx->stream, a.tiles_x, a.n_tiles, acc->d_first, b.d_mask,
                       b.d_cnt, acc->d_counts);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(counts, acc->d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<WithinPair> cand;
    if ((rc = within_compact(ctx, a, b.d_mask, b.d_cnt, b.d_off, cand))) return rc;         // (synchronizes: counts are here)

    // the walk: candidates are in (row, col) order; a row stops at its first representative column within D
    std::vector<uint32_t> &rep = acc->rep;
    uint64_t evaluated = 0;
    uint32_t reps = 0;
    size_t at = 0;
    for (uint32_t row = r0; row < r1; ++row) {
        uint32_t found = row;
        for (; at < cand.size() && cand[at].row == row - r0; ++at) {
            const WithinPair &w = cand[at];
            if (found != row || rep[w.col] != w.col) continue;                              // the row has stopped; an in-block member
            double d;
            ++evaluated;
            if (!filter_pair_host(w, ref, r0, qry, k, model, fp32, tables, &d)) {
                if (bad_pair) *bad_pair = (uint64_t)w.row * n_cols + w.col;
                std::fill(rep.begin() + r0, rep.begin() + r1, DEREP_UNDECIDED);
                return LASH_ERANGE;
            }
            if (d <= max_dist) found = w.col;
        }
        rep[row] = found;
        reps += found == row;
    }
    HIPCHK(ctx, hipMemcpyAsync(acc->d_rep + r0, rep.data() + r0, (size_t)nr * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    acc->decided = r1;
    acc->representatives += reps;
    if (stats) {
        uint64_t pairs = 0;                                                                    // the printed off-diagonal pairs
        for (uint32_t r = r0; r < r1; ++r) pairs += r;
        stats->pairs = pairs;
        stats->pruned_not_rep = counts[0];
        stats->pruned_after_hit = counts[1];
        stats->sent_to_host = cand.size();
        stats->evaluated = evaluated;
        stats->representatives = acc->representatives;
    }
    return LASH_OK;
}

int lash_derep_result(const lash_derep *c, uint32_t *out)
{
    if (!c || (c->n && !out) || c->decided != c->n) return LASH_EINVAL;
    std::copy(c->rep.begin(), c->rep.end(), out);
    return LASH_OK;
}

}  // extern "C"
