// screen_wta.hip — winner-takes-all containment of HyperMinHash sketches (`lash screen`, include/lash_gfx950.h:
// lash_sketch_set_screen_wta).
//
// A bucket's register identifies one sampled k-mer (group_spectrum.hip): reference i HOLDS bucket b of a query iff the
// query's register there is not 0 and the reference's equals it.  A query comes with a list of candidate references, best first; a
// bucket is credited to the first candidate of the list that holds it, and every candidate is counted twice: the buckets it holds
// (shared) and the buckets it won.
//
// Two launches per chunk of queries; the kernel boundary between them is what makes the winner tables visible to every XCD.
//   screen_winner_kernel  work is cut as group_union.hip cuts it — tasks of up to `segment` consecutive positions of one query's list,
//       slices of contiguous 16-byte units, lanes for short runs — and a thread OWNS a unit of eight registers: it loads the query's
//       unit once and walks its task's candidates with eight independent 16-byte loads in flight.  Positions ascend within a task, so
//       the first candidate that holds a bucket is the task's smallest: the walk keeps it and compares no positions.  Equality and
//       "not 0" do not depend on the byte order of the registers as long as both sides are in the same one, so nothing is swapped.
//       Nothing is shared during the walk: no table in LDS, no barrier.
//         a list that is one task   stores its eight winners with two 16-byte stores;
//         a list cut into several   takes the minimum into the query's winner table (uint32[16384], filled with SW_NONE) atomically,
//                                   and only for the buckets that found a holder.
//   screen_count_kernel   one workgroup per (query, position): every thread takes eight units, loads the query's unit, the candidate's
//       unit and the eight winners, and adds "holds" into shared and "holds and the winner is this position" into won; the sums go over
//       the wave with shuffles and over the four waves through LDS.
// Every result is a minimum or a sum of integers: it does not depend on segment, slices, lanes or the scratch budget.
#include "sketch_rules.h"

namespace lash {

namespace {

constexpr uint32_t SW_THREADS = 256;
constexpr uint32_t SW_UNITS = HMH_M / 8u;                                    // 16-byte units of a register table

// x = a ^ b of two words of two registers: 1 at bit 0 / bit 16 where the low / high register is equal (no carry crosses bit 15)
__device__ __forceinline__ uint32_t zero_halves(uint32_t x) { return (~(((x & 0x7FFF7FFFu) + 0x7FFF7FFFu) | x) & 0x80008000u) >> 15; }

__global__ void __launch_bounds__(SW_THREADS) screen_winner_kernel(ScreenWtaArgs a)
{
    const uint32_t tid = threadIdx.x, L = a.lanes, tpb = SW_THREADS / L;
    const uint32_t sub = tid / L, lane = tid - sub * L;
    const uint32_t slice = blockIdx.x % a.slices, task = (blockIdx.x / a.slices) * tpb + sub;
    if (task >= a.n_tasks) return;
    const ScreenTask t = a.tasks[task];
    const uint32_t q = SW_UNITS / a.slices, rem = SW_UNITS % a.slices;
    const uint32_t u0 = slice * q + (slice < rem ? slice : rem), cnt = q + (slice < rem ? 1u : 0u);
    const uint8_t *const qimg = a.qry + (uint64_t)t.query * a.qry_stride + a.qry_hdr;
    const uint32_t *const list = a.cand + t.src_begin;
    for (uint32_t u = lane; u < cnt; u += L) {
        const uint64_t off = 16ull * (u0 + u);
        const uint4 Q = load16_any(qimg + off);
        const uint32_t qw[4] = {Q.x, Q.y, Q.z, Q.w};
        uint32_t found[4] = {0u, 0u, 0u, 0u};                                // bit 0 / bit 16: the low / high register has its winner
        uint32_t win[8] = {SW_NONE, SW_NONE, SW_NONE, SW_NONE, SW_NONE, SW_NONE, SW_NONE, SW_NONE};
#pragma unroll
        for (int w = 0; w < 4; ++w) found[w] = zero_halves(qw[w]);           // an empty bucket is held by nobody: closed before the walk
#pragma unroll 8
        for (uint32_t j = 0; j < t.count; ++j) {
            const uint4 v = load16_any(a.ref + (uint64_t)list[j] * a.ref_stride + a.ref_hdr + off);
            const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
            const uint32_t pos = t.pos0 + j;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t eq = zero_halves(vw[w] ^ qw[w]), fresh = eq & ~found[w];
                found[w] |= eq;
                if (fresh & 1u) win[2 * w] = pos;
                if (fresh & 0x10000u) win[2 * w + 1] = pos;
            }
        }
        uint32_t *const dst = a.winner + (uint64_t)t.table * HMH_M + 8u * (u0 + u);
        if (t.single) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(win[0], win[1], win[2], win[3]);
            *reinterpret_cast<uint4 *>(dst + 4) = make_uint4(win[4], win[5], win[6], win[7]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (win[i] != SW_NONE) atomicMin(&dst[i], win[i]);
        }
    }
}

__global__ void __launch_bounds__(SW_THREADS) screen_count_kernel(ScreenWtaArgs a)
{
    __shared__ uint32_t part[2][SW_THREADS / 64u];
    const uint32_t tid = threadIdx.x, e = blockIdx.x;                        // e: the entry of the chunk's part of the list
    const uint32_t table = a.pair_table[e];
    const uint32_t query = a.q0 + table;
    const uint32_t pos = (uint32_t)(a.e0 + e - a.cand_off[table]);
    const uint8_t *const qimg = a.qry + (uint64_t)query * a.qry_stride + a.qry_hdr;
    const uint8_t *const rimg = a.ref + (uint64_t)a.cand[a.e0 + e] * a.ref_stride + a.ref_hdr;
    const uint32_t *const wtab = a.winner + (uint64_t)table * HMH_M;
    uint32_t shared = 0, won = 0;
#pragma unroll
    for (uint32_t i = 0; i < SW_UNITS / SW_THREADS; ++i) {
        const uint32_t u = i * SW_THREADS + tid;
        const uint4 Q = load16_any(qimg + 16ull * u), v = load16_any(rimg + 16ull * u);
        const uint4 wl = *reinterpret_cast<const uint4 *>(wtab + 8u * u), wh = *reinterpret_cast<const uint4 *>(wtab + 8u * u + 4u);
        const uint32_t qw[4] = {Q.x, Q.y, Q.z, Q.w}, vw[4] = {v.x, v.y, v.z, v.w};
        const uint32_t win[8] = {wl.x, wl.y, wl.z, wl.w, wh.x, wh.y, wh.z, wh.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t holds = zero_halves(vw[w] ^ qw[w]) & ~zero_halves(qw[w]);
            shared += (holds & 1u) + (holds >> 16);
            won += ((holds & 1u) & (uint32_t)(win[2 * w] == pos)) + ((holds >> 16) & (uint32_t)(win[2 * w + 1] == pos));
        }
    }
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        shared += __shfl_xor(shared, (int)o);
        won += __shfl_xor(won, (int)o);
    }
    if ((tid & 63u) == 0u) {
        part[0][tid >> 6] = shared;
        part[1][tid >> 6] = won;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0, w = 0;
#pragma unroll
        for (uint32_t i = 0; i < SW_THREADS / 64u; ++i) {
            s += part[0][i];
            w += part[1][i];
        }
        a.out_shared[a.e0 + e] = s;
        a.out_won[a.e0 + e] = w;
    }
}

}  // namespace

hipError_t launch_screen_winner(const ScreenWtaArgs &a, hipStream_t stream)
{
    if (a.n_tasks == 0) return hipSuccess;
    if (a.slices == 0 || a.slices > SW_UNITS || a.lanes == 0 || a.lanes > SW_THREADS || (a.lanes & (a.lanes - 1u))) return hipErrorInvalidValue;
    const uint32_t tpb = SW_THREADS / a.lanes;
    const uint64_t blocks = (uint64_t)((a.n_tasks + tpb - 1u) / tpb) * a.slices;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(screen_winner_kernel, dim3((uint32_t)blocks), dim3(SW_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_screen_count(const ScreenWtaArgs &a, hipStream_t stream)
{
    if (a.n_entries == 0) return hipSuccess;
    if (a.n_entries > 0x7FFFFFFFull) return hipErrorInvalidValue;
    static_assert(SW_UNITS % SW_THREADS == 0, "a counting thread takes whole units");
    hipLaunchKernelGGL(screen_count_kernel, dim3((uint32_t)a.n_entries), dim3(SW_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lash
