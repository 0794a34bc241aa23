// prefix_union.hip — register histograms of the running union along orderings of a resident sketch set (`lash growth`,
// include/lash_gfx950.h: lash_sketch_set_prefix_union_cardinalities).
//
// For order o and step t the union U(o, t) = image[order[o][0]] ∪ ... ∪ image[order[o][t]] is a sketch like any other, and its
// cardinality needs only the histogram of its registers (sketch_set.hip: sketch_hist_kernel makes that of one image).  The fold is
// a stream: one workgroup owns (order, register slice), keeps its slice of the running table in LDS, reads its slice of the next
// image per step, merges with the sketch's own rule (merge_word, sketch_rules.h) and keeps the histogram up to date by moving one
// count from the old bin to the new one for every register that changed — early steps change most registers, late steps almost
// none, so the cost of a late step is its loads.
//
// Registers are independent, so slices never talk to each other: they exist so that a run with few orderings still fills the
// chip.  A slice is a contiguous run of whole 32-bit words; thread i of the workgroup owns words i, i + 256, ... of it for the
// whole launch, so the table needs no barrier at all.  What is shared is the histogram: the step's changes are collected as
// signed deltas in LDS (two buffers in turn: one barrier per step), thread b keeps bin b's running count in a register and adds
// it into the step's 256-bin row in global memory.  Rows are zeroed before the launch and every contribution is an integer
// atomic add, so the row is the same sum whatever the slice count, the chunking of the orders or the timing.
//
// The order list is known in advance: the loads of step t + 1 are issued before step t is merged, so a step's barrier and
// atomics run under the next step's memory latency.  PU_PREFETCH words per thread are read ahead; a slice with more than
// 256 * PU_PREFETCH words (only when the caller asks for fewer slices than the default) reads the rest in the step itself.
#include "sketch_rules.h"

namespace lash {

namespace {

constexpr uint32_t PU_THREADS = 256;
constexpr uint32_t PU_PREFETCH = 4;

// bin of register r of a word in register order: HyperMinHash = the 6-bit leading-zero field of the u16, else the byte
template <int ALGO>
__device__ __forceinline__ uint32_t pu_bin(uint32_t w, uint32_t r)
{
    if constexpr (ALGO == 0) return (w >> (16u * r + 10u)) & 63u;
    else return (w >> (8u * r)) & 0xFFu;
}

template <int ALGO>
__global__ void __launch_bounds__(PU_THREADS) prefix_union_kernel(PrefixUnionArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t pu_lds[];
    constexpr uint32_t REGS = ALGO == 0 ? 2u : 4u;                        // registers per word
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, o = blockIdx.y;
    // slices: contiguous runs of whole words, sizes differing by at most one (the first n_words % slices are the longer ones)
    const uint32_t q = a.n_words / a.slices, rem = a.n_words % a.slices;
    const uint32_t w0 = slice * q + (slice < rem ? slice : rem), cnt = q + (slice < rem ? 1u : 0u);
    uint32_t *const tab = pu_lds;                                         // [q + 1] the slice of the running table, register order
    uint32_t *const delta = pu_lds + (q + 1u);                            // [2][256] the step's changes, per bin (wrapping)
    for (uint32_t i = tid; i < cnt; i += PU_THREADS) tab[i] = 0u;         // (the thread's own words)
    delta[tid] = 0u;
    delta[256u + tid] = 0u;
    uint32_t mine = tid == 0u ? cnt * REGS : 0u;                          // bin `tid` of the slice's histogram: an empty table is all zeros
    __syncthreads();

    const uint32_t be = ALGO == 0 ? a.hmh_be : 0u;
    const uint32_t *const ord = a.orders + (uint64_t)o * a.len;
    uint32_t *const rows = a.hist + (uint64_t)o * a.len * 256u;
    auto image = [&](uint32_t t) { return a.img + (uint64_t)ord[t] * a.stride + a.hdr + 4ull * w0; };
    uint32_t nxt[PU_PREFETCH];
    auto fetch = [&](const uint8_t *src) {
#pragma unroll
        for (uint32_t k = 0; k < PU_PREFETCH; ++k) {
            const uint32_t i = tid + k * PU_THREADS;
            nxt[k] = i < cnt ? load_u32_any(src + 4ull * i) : 0u;
        }
    };
    auto merge = [&](uint32_t i, uint32_t v, uint32_t *d) {
        const uint32_t old = tab[i], m = merge_word<ALGO>(old, hmh_img_order(v, be));
        if (m == old) return;
        tab[i] = m;
#pragma unroll
        for (uint32_t r = 0; r < REGS; ++r) {
            const uint32_t bo = pu_bin<ALGO>(old, r), bn = pu_bin<ALGO>(m, r);
            if (bo != bn) { atomicSub(&d[bo], 1u); atomicAdd(&d[bn], 1u); }
        }
    };
    fetch(image(0));
    for (uint32_t t = 0; t < a.len; ++t) {
        uint32_t cur[PU_PREFETCH];
#pragma unroll
        for (uint32_t k = 0; k < PU_PREFETCH; ++k) cur[k] = nxt[k];
        const uint8_t *const src = image(t);
        if (t + 1u < a.len) fetch(image(t + 1u));                         // in flight while this step merges, syncs and adds
        uint32_t *const d = delta + (t & 1u) * 256u;
#pragma unroll
        for (uint32_t k = 0; k < PU_PREFETCH; ++k) {
            const uint32_t i = tid + k * PU_THREADS;
            if (i < cnt) merge(i, cur[k], d);
        }
        for (uint32_t i = tid + PU_PREFETCH * PU_THREADS; i < cnt; i += PU_THREADS) merge(i, load_u32_any(src + 4ull * i), d);
        __syncthreads();
        // d is written again at step t + 2, after the barrier of step t + 1: one barrier per step is enough
        mine += d[tid];
        d[tid] = 0u;
        if (mine) atomicAdd(&rows[(uint64_t)t * 256u + tid], mine);
    }
}

}  // namespace

uint32_t prefix_union_default_slices(uint32_t n_words, uint32_t n_orders, uint32_t cu_count)
{
    // every word read ahead (at most PU_PREFETCH per thread), about 8 workgroups per CU when the orders alone do not give them, and
    // no slice below one word per thread unless the table itself is smaller
    const uint32_t lo = (n_words + PU_THREADS * PU_PREFETCH - 1) / (PU_THREADS * PU_PREFETCH);
    const uint32_t hi = std::max(1u, n_words / PU_THREADS);
    const uint32_t want = (8u * cu_count + n_orders - 1) / std::max(1u, n_orders);
    return std::max(lo, std::min(hi, std::max(1u, want)));
}

hipError_t launch_prefix_union(const PrefixUnionArgs &args, int algo, uint32_t n_orders, hipStream_t stream)
{
    if (n_orders == 0 || args.len == 0) return hipSuccess;
    if (args.slices == 0 || args.slices > args.n_words || n_orders > 65535u) return hipErrorInvalidValue;
    const uint32_t lds = (args.n_words / args.slices + 1u + 512u) * 4u;
    const dim3 grid(args.slices, n_orders);
    switch (algo) {
    case 0: return launch_dyn_lds(prefix_union_kernel<0>, grid, dim3(PU_THREADS), lds, stream, args);
    case 1: return launch_dyn_lds(prefix_union_kernel<1>, grid, dim3(PU_THREADS), lds, stream, args);
    case 2: return launch_dyn_lds(prefix_union_kernel<2>, grid, dim3(PU_THREADS), lds, stream, args);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace lash
