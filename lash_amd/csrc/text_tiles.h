// text_tiles.h — what the device passes over raw text share (fasta_index.hip, fasta_coords.hip, fasta_windows.hip, fasta_translate.hip,
// fastq_check.hip).  They all walk a buffer in tiles of 4 KiB, one workgroup of 256 threads per tile and 16 bytes per thread (a "lane"), in
// the shape count, scan, ordered write: a lane finds its bytes of interest as a 16-bit mask, the masks' popcounts are prefixed inside the
// workgroup, the tiles' counts are scanned by one workgroup, and a second pass writes every hit at tile base + prefix.  No atomics, and
// nothing depends on scheduling.  (pack_kernels.hip and sketch_rules.h have scans of their own on the sketch path; dist_filter.hip's is
// another algorithm.)
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lash {

constexpr uint32_t TEXT_LANE = 16;                 // bytes per thread
constexpr uint32_t TEXT_TILE = 256 * TEXT_LANE;    // bytes per workgroup: 4096

// bit i: byte i of the 8 in x equals c
__device__ __forceinline__ uint32_t eq_mask8(uint64_t x, uint8_t c)
{
    const uint64_t z = x ^ (0x0101010101010101ull * c);
    const uint64_t nz = ((z & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | z;     // high bit of a byte set <=> the byte is non-zero
    return (uint32_t)((((~nz >> 7) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

// bit i: byte i of the 16 in lo, hi equals c
__device__ __forceinline__ uint32_t eq_mask16(uint64_t lo, uint64_t hi, uint8_t c) { return eq_mask8(lo, c) | (eq_mask8(hi, c) << 8); }

// the lane's bytes raw[at, at + 16) as two little-endian words, and which of them lie before `total` (bit i: byte i does); the others are
// zero.  One 16-byte load where 16 bytes are there, the buffer's last few one by one.
__device__ __forceinline__ uint32_t lane_load(const uint8_t *__restrict__ raw, uint64_t at, uint64_t total, uint64_t &lo, uint64_t &hi)
{
    lo = hi = 0;
    if (at >= total) return 0u;
    const uint64_t avail = total - at;
    if (avail >= TEXT_LANE) {
        uint4 q;
        __builtin_memcpy(&q, raw + at, 16);
        lo = q.x | ((uint64_t)q.y << 32);
        hi = q.z | ((uint64_t)q.w << 32);
        return 0xFFFFu;
    }
    for (uint32_t i = 0; i < (uint32_t)avail; ++i) {
        const uint64_t b = raw[at + i];
        if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u));
    }
    return (1u << (uint32_t)avail) - 1u;
}

// number of j in [0, n) with a[j] <= x, and with a[j] < x (a ascending)
__device__ __forceinline__ uint32_t count_le(const uint64_t *a, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint32_t count_lt(const uint64_t *a, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// the record of byte `at` in the tile that begins at tile0 (start[0] == 0, so there is one): one search of start[] per tile, the same for every
// lane, then one among the records that begin inside the tile (mostly none)
__device__ __forceinline__ uint32_t record_of(const uint64_t *start, uint32_t n, uint64_t tile0, uint64_t at)
{
    const uint32_t rt = count_le(start, n, tile0) - 1u;
    const uint32_t in_tile = count_le(start + rt + 1u, n - rt - 1u, tile0 + TEXT_TILE - 1u);
    return rt + count_le(start + rt + 1u, in_tile, at);
}

// exclusive prefix of `mine` over the 256 threads of the workgroup; *sum = their total.  wsum: 4 words of LDS.  Every thread of the workgroup
// calls it (there is a barrier inside): leave early only after it.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t mine, uint32_t *wsum, uint32_t *sum)
{
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63u) >= d) incl += v; }
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = incl - mine;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) pre += wsum[w];
    *sum = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return pre;
}

// the 1024 threads of one workgroup: out[i] = in[0] + ... + in[i - 1] for i in [0, n), *total = in[0] + ... + in[n - 1].  Every thread takes
// a run of ceil(n / 1024) elements, thread 0 scans the 1024 run sums.  in and out may be the same array; part: 1024 T of LDS.
template <typename T>
__device__ __forceinline__ void run_scan_1024(const T *in, T *out, uint32_t n, T *part, T *total)
{
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t t0 = (uint32_t)min((uint64_t)n, (uint64_t)threadIdx.x * per), t1 = (uint32_t)min((uint64_t)n, (uint64_t)t0 + per);
    T s = 0;
    for (uint32_t t = t0; t < t1; ++t) s += in[t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { T acc = 0; for (uint32_t i = 0; i < 1024; ++i) { const T v = part[i]; part[i] = acc; acc += v; } *total = acc; }
    __syncthreads();
    T acc = part[threadIdx.x];
    for (uint32_t t = t0; t < t1; ++t) { const T v = in[t]; out[t] = acc; acc += v; }
}

// one workgroup: d_out[i] = d_in[0] + ... + d_in[i - 1] for i in [0, n], d_out[n] the total (n + 1 entries); d_out may be d_in (text_tiles.hip)
hipError_t launch_tile_scan(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
hipError_t launch_tile_scan(const uint64_t *d_in, uint64_t *d_out, uint32_t n, hipStream_t stream);

}  // namespace lash
