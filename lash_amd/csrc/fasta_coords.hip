// fasta_coords.hip — the sequence coordinates of the records of a FASTA index, on the device: which bytes of the buffer are sequence bytes,
// and the rank of each among them.  fasta_index.hip finds the records; the stages that rewrite their sequences (fasta_windows.hip,
// fasta_translate.hip) start from these coordinates.
//
// Rules: the sequence bytes of record r are the bytes after its header line's '\n' up to start[r + 1] that are neither LF nor CR (every
// other byte counts: N, lower case, a stray '>').  Their 0-based rank in the record is the coordinate; L_r is their number.
//
// Passes over the 4 KiB tiles of text_tiles.h (16 bytes per lane; count, scan; no atomics, nothing depends on scheduling):
//   1. fc_seqbegin_kernel  one thread per record walks its header line: seq_begin[r]
//   2. fc_count_kernel     per tile: a 16-bit mask of sequence bytes per lane and the lane's rank inside the tile (one u32), a count per tile
//   3. launch_tile_scan    one workgroup: exclusive 64-bit scan of the tile counts
//   4. fc_seq0_kernel      per record: rank of its first sequence byte in the whole buffer (seq0[r]); L_r = seq0[r + 1] - seq0[r]
// What is left for the next stage (FastaCoords): the lane words, the tile bases, seq_begin[] and seq0[].  The rank of the sequence byte at
// bit b of lane word w in tile t is tile_base[t] + (w >> 16) + popcount(w & ((1 << b) - 1)).  Traffic: the input is read once, 4 bytes per 16
// of lane words are written.
#include <hip/hip_runtime.h>

#include "lash_kernels.h"
#include "text_tiles.h"

namespace lash {

__global__ void __launch_bounds__(256) fc_seqbegin_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ start, uint32_t n,
                                                          uint64_t *__restrict__ seq_begin)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint64_t end = start[r + 1u];
    uint64_t p = start[r];
    while (p < end && raw[p] != '\n') ++p;
    seq_begin[r] = p < end ? p + 1u : end;                          // a header with no line end: the record has no sequence
}

__global__ void __launch_bounds__(256) fc_count_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ start,
                                                       const uint64_t *__restrict__ seq_begin, uint32_t n, uint32_t *__restrict__ lanes,
                                                       uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t wsum[4];
    const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE, at = tile0 + threadIdx.x * 16ull;
    uint64_t lo, hi;
    const uint32_t valid = lane_load(raw, at, total, lo, hi);
    uint32_t m = ~(eq_mask16(lo, hi, '\n') | eq_mask16(lo, hi, '\r')) & valid;
    if (valid) {
        // header bytes [start[r], seq_begin[r]) of every record that touches these 16 bytes are no sequence
        for (uint32_t r = record_of(start, n, tile0, at); r < n && start[r] < at + 16u; ++r) {
            const uint64_t sb = seq_begin[r];
            if (sb <= at) continue;
            const uint32_t a = start[r] > at ? (uint32_t)(start[r] - at) : 0u, b = sb < at + 16u ? (uint32_t)(sb - at) : 16u;
            m &= ~(((1u << b) - 1u) & ~((1u << a) - 1u));
        }
    }
    uint32_t sum;
    const uint32_t pre = block_scan_256((uint32_t)__builtin_popcount(m), wsum, &sum);
    lanes[(uint64_t)blockIdx.x * 256u + threadIdx.x] = (pre << 16) | m;      // pre <= 4080
    if (threadIdx.x == 0u) tile_cnt[blockIdx.x] = sum;
}

// sequence bytes before position pos (pos <= total)
__device__ __forceinline__ uint64_t fc_rank(const uint32_t *lanes, const uint64_t *tile_base, uint32_t n_tiles, uint64_t total, uint64_t pos)
{
    if (pos >= total) return tile_base[n_tiles];
    const uint32_t w = lanes[pos >> 4];
    return tile_base[pos / TEXT_TILE] + (w >> 16) + (uint32_t)__builtin_popcount(w & ((1u << (uint32_t)(pos & 15u)) - 1u));
}

// nothing lies between seq_begin[r] and seq_begin[r + 1] but the sequence of r and the header of r + 1: L_r is the difference of the ranks
__global__ void __launch_bounds__(256) fc_seq0_kernel(const uint64_t *__restrict__ seq_begin, uint32_t n, uint64_t total,
                                                      const uint32_t *__restrict__ lanes, const uint64_t *__restrict__ tile_base, uint32_t n_tiles,
                                                      uint64_t *__restrict__ seq0)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r <= n) seq0[r] = fc_rank(lanes, tile_base, n_tiles, total, r < n ? seq_begin[r] : total);
}

// scratch: [lanes: n_tiles * 256 u32 | tile_base: n_tiles + 1 u64 | seq_begin: n u64 | seq0: n + 1 u64] (a multiple of 8 bytes)
size_t fasta_coords_scratch_bytes(uint32_t n_tiles, uint32_t n_records)
{
    return (size_t)n_tiles * 1024 + ((size_t)n_tiles + 1) * 8 + ((size_t)n_records * 2 + 1) * 8 + 64;
}

FastaCoords fasta_coords_view(uint8_t *d_scratch, uint32_t n_tiles, uint32_t n_records)
{
    FastaCoords c;
    c.lanes = reinterpret_cast<uint32_t *>(d_scratch);
    c.tile_base = reinterpret_cast<uint64_t *>(d_scratch + (size_t)n_tiles * 1024);
    c.seq_begin = c.tile_base + n_tiles + 1;
    c.seq0 = c.seq_begin + n_records;
    return c;
}

hipError_t launch_fasta_coords(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                               uint8_t *d_scratch, hipStream_t stream)
{
    const FastaCoords c = fasta_coords_view(d_scratch, n_tiles, n_records);
    uint32_t *lanes = const_cast<uint32_t *>(c.lanes);
    uint64_t *tile_base = const_cast<uint64_t *>(c.tile_base), *seq_begin = const_cast<uint64_t *>(c.seq_begin), *seq0 = const_cast<uint64_t *>(c.seq0);
    hipLaunchKernelGGL(fc_seqbegin_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, d_raw, d_start, n_records, seq_begin);
    if (n_tiles) hipLaunchKernelGGL(fc_count_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_start, seq_begin, n_records, lanes, tile_base);
    const hipError_t e = launch_tile_scan(tile_base, tile_base, n_tiles, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fc_seq0_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, seq_begin, n_records, total, lanes, tile_base, n_tiles, seq0);
    return hipGetLastError();
}

}  // namespace lash
