// group_spectrum.hip — the k-mer sharing spectrum of groups of HyperMinHash sketches (`lash spectrum`, include/lash_gfx950.h:
// lash_sketch_set_group_spectrum).
//
// A bucket's union register is the largest register over the group's members; it belongs to one k-mer of the union, and the members
// whose register equals it are the members that hold that k-mer.  The histogram of that number over the occupied buckets is a uniform
// sample of the group's multiplicity spectrum.  The union images come from group_union.hip; this file counts.
//
// Work is cut as group_union.hip cuts it — tasks of up to `segment` members, slices of contiguous 16-byte units, lanes for short
// runs — and a thread OWNS a unit of eight 16-bit registers: it loads the union's unit once and walks its task's members with eight
// independent 16-byte loads in flight, adding "equal" into eight 16-bit fields of four words (a task holds at most 65 535 members).
// Equality and "not 0" do not depend on the byte order of the registers as long as both sides are in the same one, so nothing is
// swapped.  Nothing is shared during the walk: no table in LDS, no barrier.
//   a group that is one task   is final in registers.  Counts 0..3 — all there is in a pairs workload, 16 384 per group — are tallied in
//       four 16-bit fields per thread, summed over the task's lanes of a wave with shuffles, and leave as one add per bin and wave into
//       the workgroup's histogram in LDS; other counts below the LDS bound go there one by one; the workgroup then adds every non-zero
//       bin to the group's bins in global memory once.  Counts at or above the bound go to global memory directly.
//   a group cut into several   adds its non-zero counts into the group's count table (uint32[16384], zeroed) in scratch memory, and
//       one finishing launch bins the tables of the chunk.
// Every sum is a sum of integers added atomically: the bins do not depend on segment, slices, lanes or the scratch budget.
#include "sketch_rules.h"

namespace lash {

namespace {

constexpr uint32_t GS_THREADS = 256;
constexpr uint32_t GS_LDS_TASKS = 16;      // most tasks of a workgroup that share the LDS histogram (more: runs below 16 units, straight to global memory)
constexpr uint32_t GS_BINS = 4096;         // LDS bins of a workgroup, split evenly over its tasks: 256 each at the least
constexpr uint32_t GS_SMALL = 4;           // counts tallied in registers and reduced over the wave
constexpr uint32_t GS_FINISH_SLICES = 8;   // workgroups per count table of the finishing launch: 2048 counts, eight per thread

// x = a ^ b of two words of two registers: 1 at bit 0 / bit 16 where the low / high register is equal (no carry crosses bit 15)
__device__ __forceinline__ uint32_t zero_halves(uint32_t x) { return (~(((x & 0x7FFF7FFFu) + 0x7FFF7FFFu) | x) & 0x80008000u) >> 15; }

__device__ __forceinline__ uint32_t word_of(uint4 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

__global__ void __launch_bounds__(GS_THREADS) group_spectrum_kernel(GroupSpectrumArgs a)
{
    __shared__ uint32_t lds_hist[GS_BINS];
    const uint32_t tid = threadIdx.x, L = a.lanes, tpb = GS_THREADS / L;
    const uint32_t sub = tid / L, lane = tid - sub * L;
    const uint32_t slice = blockIdx.x % a.slices, task = (blockIdx.x / a.slices) * tpb + sub;
    const bool in_lds = tpb <= GS_LDS_TASKS;
    const uint32_t bins = GS_BINS / (in_lds ? tpb : GS_THREADS);
    SpectrumTask t{};
    bool fin = false;
    if (task < a.n_tasks) {
        t = a.tasks[task];
        fin = t.table == GS_NO_TABLE;
    }
    uint32_t *const mine = lds_hist + sub * bins;                            // (in_lds only)
    const uint32_t nb = fin && in_lds ? (t.count + 1u < bins ? t.count + 1u : bins) : 0u;
    if (in_lds) {
        for (uint32_t b = lane; b < nb; b += L) mine[b] = 0u;
        __syncthreads();
    }
    uint64_t small = 0;                                                      // four 16-bit tallies: a thread has at most 8 units, 64 registers
    if (task < a.n_tasks) {
        const uint32_t n_units = HMH_M / 8u, q = n_units / a.slices, rem = n_units % a.slices;
        const uint32_t u0 = slice * q + (slice < rem ? slice : rem), cnt = q + (slice < rem ? 1u : 0u);
        uint32_t *const bin = a.hist + t.hist_begin;
        for (uint32_t u = lane; u < cnt; u += L) {
            const uint64_t off = 16ull * (u0 + u);
            const uint4 U = load16_any(a.uni + (uint64_t)t.group * a.uni_stride + a.uni_hdr + off);
            uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll 8
            for (uint32_t j = 0; j < t.count; ++j) {
                const uint4 v = load16_any(a.src + (uint64_t)a.members[t.src_begin + j] * a.src_stride + a.src_hdr + off);
                c[0] += zero_halves(v.x ^ U.x);
                c[1] += zero_halves(v.y ^ U.y);
                c[2] += zero_halves(v.z ^ U.z);
                c[3] += zero_halves(v.w ^ U.w);
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                c[w] &= (zero_halves(word_of(U, w)) ^ 0x00010001u) * 0xFFFFu;                     // an empty bucket is held by nobody
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t n = (c[w] >> (16 * h)) & 0xFFFFu;
                    if (fin) {
                        if (n < GS_SMALL) small += 1ull << (16u * n);
                        else if (n < nb) atomicAdd(&mine[n], 1u);
                        else atomicAdd(&bin[n], 1u);
                    } else if (n) atomicAdd(&a.counts[(uint64_t)t.table * HMH_M + 8u * (u0 + u) + 2u * (uint32_t)w + (uint32_t)h], n);
                }
            }
        }
    }
    // the small tallies of a task's lanes in this wave (every lane takes part: a thread without a final task holds zeros)
    uint32_t lo = (uint32_t)small, hi = (uint32_t)(small >> 32);
    const uint32_t span = L < 64u ? L : 64u;
    for (uint32_t o = 1; o < span; o <<= 1) {
        lo += __shfl_xor(lo, (int)o);
        hi += __shfl_xor(hi, (int)o);
    }
    if (fin && (tid & (span - 1u)) == 0u) {
        const uint32_t s[GS_SMALL] = {lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu, hi >> 16};
#pragma unroll
        for (uint32_t b = 0; b < GS_SMALL; ++b)
            if (s[b]) atomicAdd(b < nb ? &mine[b] : &a.hist[t.hist_begin + b], s[b]);
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = lane; b < nb; b += L) {
            const uint32_t n = mine[b];
            if (n) atomicAdd(&a.hist[t.hist_begin + b], n);
        }
    }
}

// the count tables of the groups that were cut: GS_FINISH_SLICES workgroups per table, eight counts per thread
__global__ void __launch_bounds__(GS_THREADS) group_spectrum_finish_kernel(GroupSpectrumArgs a)
{
    __shared__ uint32_t lds_hist[GS_BINS];
    const uint32_t tid = threadIdx.x, table = blockIdx.x / GS_FINISH_SLICES, slice = blockIdx.x % GS_FINISH_SLICES;
    for (uint32_t b = tid; b < GS_BINS; b += GS_THREADS) lds_hist[b] = 0u;
    __syncthreads();
    uint32_t *const bin = a.hist + a.table_hist[table];
    const uint32_t *const src = a.counts + (uint64_t)table * HMH_M + 8u * (slice * GS_THREADS + tid);
    const uint4 lo = *reinterpret_cast<const uint4 *>(src), hi = *reinterpret_cast<const uint4 *>(src + 4);
    const uint32_t n[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (n[i] < GS_BINS) atomicAdd(&lds_hist[n[i]], 1u);
        else atomicAdd(&bin[n[i]], 1u);
    }
    __syncthreads();
    for (uint32_t b = tid; b < GS_BINS; b += GS_THREADS) {
        const uint32_t c = lds_hist[b];
        if (c) atomicAdd(&bin[b], c);
    }
}

}  // namespace

hipError_t launch_group_spectrum(const GroupSpectrumArgs &a, hipStream_t stream)
{
    if (a.n_tasks == 0) return hipSuccess;
    if (a.slices == 0 || a.slices > HMH_M / 8u || a.lanes == 0 || a.lanes > GS_THREADS || (a.lanes & (a.lanes - 1u))) return hipErrorInvalidValue;
    // a thread's small tallies are 16-bit fields summed over a wave: at most 8 units a thread
    if ((uint64_t)a.slices * a.lanes * 8u < HMH_M / 8u) return hipErrorInvalidValue;
    const uint32_t tpb = GS_THREADS / a.lanes;
    const uint64_t blocks = (uint64_t)((a.n_tasks + tpb - 1u) / tpb) * a.slices;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_spectrum_kernel, dim3((uint32_t)blocks), dim3(GS_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_group_spectrum_finish(const GroupSpectrumArgs &a, uint32_t n_tables, hipStream_t stream)
{
    if (n_tables == 0) return hipSuccess;
    if ((uint64_t)n_tables * GS_FINISH_SLICES > 0x7FFFFFFFull) return hipErrorInvalidValue;
    static_assert(GS_FINISH_SLICES * GS_THREADS * 8u == HMH_M, "a finishing workgroup takes 2048 counts");
    hipLaunchKernelGGL(group_spectrum_finish_kernel, dim3(n_tables * GS_FINISH_SLICES), dim3(GS_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lash
