// group_union.hip — unions of groups of serialized sketches (`lash merge`, include/lash_gfx950.h: lash_sketch_set_group_union).
//
// The union of sketches is the sketch of the union, register by register, under the sketch's own rule (merge_word, sketch_rules.h):
// a fold with no state but the register itself.  So a thread OWNS registers — a unit of four 32-bit words, one 16-byte load — and
// walks the sources of its task: nothing is shared, no table sits in LDS, no barrier is needed, and the table may be of any size
// (two words at ull p = 3, 64 MiB at ull p = 26).  The walk is unrolled by eight: eight independent 16-byte loads per thread are in
// flight before the first merge waits for one, every source byte is read once, and the lanes of a wave read neighbouring units.
//
// Work is cut three ways so that 50 000 groups of two and one group of 100 000 both fill the chip (lash_group_union_api.hip plans it):
//   tasks    a group of up to `segment` members is one task that writes the caller's image; a longer one is cut into segments, each
//            folded into a partial (a bare register table in scratch memory), and the partials are folded again by the same kernel,
//            level after level, until one task is left for the image.  The rules are commutative, associative and idempotent: the cut
//            changes no bit.
//   slices   an image's units are cut into contiguous runs, one workgroup (or part of one) each; a thread strides over its run
//   lanes    a run shorter than 256 units takes only `lanes` threads, and the workgroup 256 / lanes tasks side by side
// A final task also writes the header: HyperMinHash / UltraLogLog have nothing to compute for it; HyperLogLog's needs the histogram
// of the finished registers, which the slices add — integers, atomically — into 72 bins per image, and one wave per image turns
// into (zero, sum) afterwards with the code lash_merge_images uses (write_hll_header_wave), so the header is the same function of the
// registers there and here.
#include "sketch_rules.h"

namespace lash {

namespace {

constexpr uint32_t GU_THREADS = 256;
constexpr uint32_t GU_LDS_TASKS = 16;      // tasks of a workgroup that get a histogram in LDS; with more (tables below 256 registers) the few
                                           // registers of a task go straight to the image's bins in global memory

template <int W> struct GuUnit;
template <> struct GuUnit<4> {
    typedef uint4 type;
    static __device__ __forceinline__ uint4 load(const uint8_t *p) { return load16_any(p); }
    static __device__ __forceinline__ void store(uint8_t *p, uint4 v) { __builtin_memcpy(p, &v, 16); }
    static __device__ __forceinline__ uint4 zero() { return make_uint4(0u, 0u, 0u, 0u); }
    template <int ALGO> static __device__ __forceinline__ uint4 merge(uint4 a, uint4 b)
    { return make_uint4(merge_word<ALGO>(a.x, b.x), merge_word<ALGO>(a.y, b.y), merge_word<ALGO>(a.z, b.z), merge_word<ALGO>(a.w, b.w)); }
    static __device__ __forceinline__ uint4 order(uint4 v, uint32_t be)
    { return make_uint4(hmh_img_order(v.x, be), hmh_img_order(v.y, be), hmh_img_order(v.z, be), hmh_img_order(v.w, be)); }
    static __device__ __forceinline__ uint32_t word(uint4 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
};
template <> struct GuUnit<1> {
    typedef uint32_t type;
    static __device__ __forceinline__ uint32_t load(const uint8_t *p) { return load_u32_any(p); }
    static __device__ __forceinline__ void store(uint8_t *p, uint32_t v) { store_u32_any(p, v); }
    static __device__ __forceinline__ uint32_t zero() { return 0u; }
    template <int ALGO> static __device__ __forceinline__ uint32_t merge(uint32_t a, uint32_t b) { return merge_word<ALGO>(a, b); }
    static __device__ __forceinline__ uint32_t order(uint32_t v, uint32_t be) { return hmh_img_order(v, be); }
    static __device__ __forceinline__ uint32_t word(uint32_t v, int) { return v; }
};

// HyperLogLog: a thread's tally of the registers it finished.  Ranks below 8 — nearly all of them — are counted in eight 8-bit fields
// and leave as one atomic per rank every 15 units (240 registers: a field cannot overflow); the others go one by one.
struct GuTally {
    uint64_t packed = 0;
    uint32_t words = 0;
    __device__ __forceinline__ void add(uint32_t *hist, uint32_t v)
    {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t rho = (v >> (8 * b)) & 0xFFu;
            if (rho < 8u) packed += 1ull << (8u * rho);
            else atomicAdd(&hist[rho < 71u ? rho : 71u], 1u);
        }
        if (++words == 60u) flush(hist);
    }
    __device__ __forceinline__ void flush(uint32_t *hist)
    {
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r) {
            const uint32_t c = (uint32_t)(packed >> (8u * r)) & 0xFFu;
            if (c) atomicAdd(&hist[r], c);
        }
        packed = 0; words = 0;
    }
};

// L0: the first level (sources are the set's images, named by `members`)
template <int ALGO, int W, bool L0>
__global__ void __launch_bounds__(GU_THREADS) group_union_kernel(GroupUnionArgs a)
{
    typedef GuUnit<W> U;
    typedef typename U::type V;
    __shared__ uint32_t lds_hist[GU_LDS_TASKS * 72u];
    __shared__ uint32_t lds_img[GU_LDS_TASKS];                             // the image a task of this workgroup finishes, or ~0
    const uint32_t tid = threadIdx.x, L = a.lanes, tpb = GU_THREADS / L;
    const uint32_t sub = tid / L, lane = tid - sub * L;
    const uint32_t slice = blockIdx.x % a.slices, task = (blockIdx.x / a.slices) * tpb + sub;
    const bool in_lds = ALGO == 1 && tpb <= GU_LDS_TASKS;
    if constexpr (ALGO == 1) {
        if (in_lds) {
            for (uint32_t i = tid; i < tpb * 72u; i += GU_THREADS) lds_hist[i] = 0u;
            if (tid < tpb) lds_img[tid] = 0xFFFFFFFFu;
            __syncthreads();
        }
    }
    if (task < a.n_tasks) {
        const GroupTask t = a.tasks[task];
        const bool fin = (t.dst & GU_FINAL) != 0u;
        const uint32_t d = t.dst & ~GU_FINAL;
        // the slice's run of units: sizes differ by at most one (the first n_units % slices runs are the longer ones)
        const uint32_t n_units = a.n_words / (uint32_t)W, q = n_units / a.slices, rem = n_units % a.slices;
        const uint32_t u0 = slice * q + (slice < rem ? slice : rem), cnt = q + (slice < rem ? 1u : 0u);
        uint8_t *const img = a.out + (uint64_t)d * a.out_stride;
        uint8_t *const dst = fin ? img + a.hdr : a.part + (uint64_t)d * a.n_words * 4ull;
        const uint32_t dst_be = fin && ALGO == 0 ? a.out_be : 0u, src_be = ALGO == 0 ? a.src_be : 0u;
        uint32_t *hist = nullptr;
        if constexpr (ALGO == 1) {
            if (fin) hist = in_lds ? lds_hist + sub * 72u : a.hist + (uint64_t)d * 72u;
            if (fin && in_lds && lane == 0u) lds_img[sub] = d;
        }
        GuTally tally;
        for (uint32_t u = lane; u < cnt; u += L) {
            const uint64_t off = 4ull * (uint32_t)W * (u0 + u);
            V acc = U::zero();
#pragma unroll 8
            for (uint32_t j = 0; j < t.count; ++j) {
                const uint64_t s = L0 ? (uint64_t)a.members[t.src_begin + j] : t.src_begin + j;
                acc = U::template merge<ALGO>(acc, U::order(U::load(a.src + s * a.src_stride + a.src_hdr + off), src_be));
            }
            U::store(dst + off, U::order(acc, dst_be));
            if constexpr (ALGO == 1) {
                if (fin) {
#pragma unroll
                    for (int i = 0; i < W; ++i) tally.add(hist, U::word(acc, i));
                }
            }
        }
        if constexpr (ALGO == 1) {
            if (fin) tally.flush(hist);
        } else {
            // lash_merge_images' header (finalize_kernel); a group without members is the empty sketch as the sketch kernels write it
            if (fin && slice == 0u && lane == 0u && a.hdr) {
                const uint64_t n_regs = ALGO == 0 ? HMH_M : (1ull << a.p), z = t.count ? 0ull : n_regs;
                write_header(img, a.hdr_tpl, a.alpha_bits, n_regs, z, (double)z, ALGO == 0 ? HMH_P : a.p);
            }
        }
    }
    if constexpr (ALGO == 1) {
        if (in_lds) {
            __syncthreads();
            for (uint32_t i = tid; i < tpb * 72u; i += GU_THREADS) {
                const uint32_t d = lds_img[i / 72u], c = lds_hist[i];
                if (d != 0xFFFFFFFFu && c) atomicAdd(&a.hist[(uint64_t)d * 72u + i % 72u], c);
            }
        }
    }
}

// one wave per image: (zero, sum) and the rest of the header from the finished registers' histogram
__global__ void __launch_bounds__(64) group_union_hll_headers_kernel(GroupUnionArgs a)
{
    write_hll_header_wave(a.out + (uint64_t)blockIdx.x * a.out_stride, a.hdr_tpl, a.hist + (uint64_t)blockIdx.x * 72u, a.alpha_bits, a.p, nullptr);
}

template <int ALGO, int W>
hipError_t launch_level(const GroupUnionArgs &a, dim3 grid, hipStream_t stream)
{
    if (a.members) hipLaunchKernelGGL((group_union_kernel<ALGO, W, true>), grid, dim3(GU_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((group_union_kernel<ALGO, W, false>), grid, dim3(GU_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

// a unit is four words wherever the table is made of whole ones (everything but ull p = 3: two words)
uint32_t group_union_unit_words(uint32_t n_words) { return n_words % 4u == 0u ? 4u : 1u; }

hipError_t launch_group_union(const GroupUnionArgs &a, int algo, hipStream_t stream)
{
    if (a.n_tasks == 0) return hipSuccess;
    const uint32_t W = group_union_unit_words(a.n_words), n_units = a.n_words / W;
    if (a.slices == 0 || a.slices > n_units || a.lanes == 0 || a.lanes > GU_THREADS || (a.lanes & (a.lanes - 1u))) return hipErrorInvalidValue;
    const uint32_t tpb = GU_THREADS / a.lanes;
    const uint64_t blocks = (uint64_t)((a.n_tasks + tpb - 1u) / tpb) * a.slices;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks);
    switch (algo * 2 + (W == 4u ? 1 : 0)) {
    case 0: return launch_level<0, 1>(a, grid, stream);
    case 1: return launch_level<0, 4>(a, grid, stream);
    case 2: return launch_level<1, 1>(a, grid, stream);
    case 3: return launch_level<1, 4>(a, grid, stream);
    case 4: return launch_level<2, 1>(a, grid, stream);
    case 5: return launch_level<2, 4>(a, grid, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_group_union_headers(const GroupUnionArgs &a, uint32_t n_images, hipStream_t stream)
{
    if (n_images == 0) return hipSuccess;
    hipLaunchKernelGGL(group_union_hll_headers_kernel, dim3(n_images), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lash
