// fasta_translate.hip — six-frame translation of FASTA records, made on the device (`lash sketch --translate`; lash_fasta_translate[_device]).
// fasta_index.hip finds the records and fasta_coords.hip gives every sequence byte its coordinate; this stage writes the six
// reading frames of every record as residues into one buffer, cut into segments at stops and ambiguous codons, so that the amino-acid
// route (LASH_F_AMINO, aa_sketch_kernel) sketches them unchanged with the segments as its records.
//
// Rules (k-independent): the sequence bytes S[0..L) of a record are those of fasta_coords.hip.  A base is one of ACGTacgt, every other byte
// is no base.  Frames 0, 1, 2 read S from offset f; frames 3, 4, 5 read the reverse complement R[t] = comp(S[L - 1 - t]) from offset f - 3;
// frame f has n_f = max(0, (L - o) / 3) codons, a trailing partial codon is dropped.  Three bases translate by NCBI table 1 ('*' for a stop),
// a codon with a no-base gives 'X'; '*' and 'X' are break bytes.  Record r takes 6 + 2 * max(0, L - 2) bytes at out_base[r]: its frames in
// order, each its n_f residues and one '*'.  A segment ends after every break byte: seg_off[0] = 0, seg_off[s + 1] = position after the
// s-th break; rec_seg[r] = the first segment of record r (out_base[r] is always a segment boundary: the byte before it ends a frame).
//
// Passes (no atomics, nothing depends on scheduling):
//   1. launch_fasta_coords          lane words, tile bases and seq0[r]: the coordinate of every sequence byte
//   2. tr_size_kernel + scan        the closed-form record sizes, scanned to out_base[r]; the host reads the total B and makes room
//   3. tr_term_kernel               one thread per record: the six frame terminators
//   4. tr_map_kernel                per 4 KiB tile of the INPUT, 16 bytes per lane: the sequence byte at coordinate i >= 2 completes the codon
//                                   that starts at s = i - 2; it is residue s / 3 of frame s % 3 and, reverse-complemented, residue t / 3 of
//                                   frame 3 + t % 3 with t = L - 3 - s.  A lane looks back over at most two sequence bytes before its own
//                                   (across line ends and tile boundaries), so every input byte is decoded once and stored twice
//   5. tr_count_kernel + scan       break bytes per 4 KiB tile of the OUTPUT, scanned; the host reads the total n_seg and makes room
//   6. tr_segoff_kernel             re-reads the output tile and stores the position after each break at its rank
//   7. tr_recseg_kernel             rec_seg[r] = the index of out_base[r] in seg_off
#include <hip/hip_runtime.h>

#include "lash_kernels.h"
#include "text_tiles.h"

namespace lash {

// base order T, C, A, G: the order of the codon table below; the complement of code x is x ^ 2
__device__ const uint8_t TR_CODON[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

// 0..3 for T C A G in either case, 4 for every other byte
__device__ __forceinline__ uint32_t tr_base_code(uint32_t byte)
{
    const uint32_t c = byte & 0xDFu, i = (c >> 1) & 3u;                    // A 0x41 -> 0, C 0x43 -> 1, T 0x54 -> 2, G 0x47 -> 3
    const uint32_t letter = (0x47544341u >> (8u * i)) & 0xFFu;             // 'A' 'C' 'T' 'G'
    return c == letter ? (0xC6u >> (2u * i)) & 3u : 4u;                    // A -> 2, C -> 1, T -> 0, G -> 3
}

__device__ __forceinline__ uint8_t tr_residue(const uint8_t *tab, uint32_t a, uint32_t b, uint32_t c)
{
    return (a | b | c) & 4u ? (uint8_t)'X' : tab[(a << 4) | (b << 2) | c];
}

// where the frames of a record of L sequence bytes start inside its 6 + 2 * max(0, L - 2) bytes, and how many codons each holds
struct TrFrames {
    uint64_t n[3], fs[6];
    __device__ __forceinline__ explicit TrFrames(uint64_t L)
    {
        n[0] = L / 3u;
        n[1] = L >= 1u ? (L - 1u) / 3u : 0u;
        n[2] = L >= 2u ? (L - 2u) / 3u : 0u;
        fs[0] = 0;
        for (int f = 1; f < 6; ++f) fs[f] = fs[f - 1] + n[(f - 1) % 3] + 1u;
    }
};

__global__ void __launch_bounds__(256) tr_size_kernel(const uint64_t *__restrict__ seq0, uint32_t n, uint64_t *__restrict__ out_base)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint64_t L = seq0[r + 1u] - seq0[r];
    out_base[r] = 6u + 2u * (L > 2u ? L - 2u : 0u);
}

__global__ void __launch_bounds__(256) tr_term_kernel(const uint64_t *__restrict__ seq0, const uint64_t *__restrict__ out_base, uint32_t n,
                                                      uint8_t *__restrict__ out)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const TrFrames fr(seq0[r + 1u] - seq0[r]);
    const uint64_t base = out_base[r];
#pragma unroll
    for (int f = 0; f < 6; ++f) out[base + fr.fs[f] + fr.n[f % 3]] = '*';
}

__global__ void __launch_bounds__(256) tr_map_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ start, uint32_t n,
                                                     const uint32_t *__restrict__ lanes, const uint64_t *__restrict__ tile_base,
                                                     const uint64_t *__restrict__ seq0, const uint64_t *__restrict__ out_base, uint8_t *__restrict__ out)
{
    __shared__ uint8_t tab[64];
    if (threadIdx.x < 64u) tab[threadIdx.x] = TR_CODON[threadIdx.x];
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE, at = tile0 + threadIdx.x * 16ull;
    const uint32_t word = lanes[(uint64_t)blockIdx.x * 256u + threadIdx.x];
    uint32_t m = word & 0xFFFFu;
    if (!m) return;                                                 // (a lane past the end of the buffer has no bit set)
    uint64_t lo, hi;
    (void)lane_load(raw, at, total, lo, hi);
    const uint64_t g = tile_base[blockIdx.x] + (word >> 16);        // rank of the lane's first sequence byte in the whole buffer
    const uint32_t first = (uint32_t)__builtin_ctz(m);
    uint32_t r = record_of(start, n, tile0, at + first);
    uint64_t i = g - seq0[r], L = seq0[r + 1u] - seq0[r], base = out_base[r];
    TrFrames fr(L);
    // the two sequence bytes before the lane's first: the same record's, behind nothing but line ends
    uint32_t q1 = 4u, q2 = 4u;                                      // codes at coordinates i - 1 and i - 2
    if (i >= 1u) {
        uint64_t p = at + first;
        do --p; while (raw[p] == '\n' || raw[p] == '\r');
        q1 = tr_base_code(raw[p]);
        if (i >= 2u) {
            do --p; while (raw[p] == '\n' || raw[p] == '\r');
            q2 = tr_base_code(raw[p]);
        }
    }
    // the codon that ends at coordinate i starts at s = i - 2: s % 3 == (i + 1) % 3, s / 3 == (i + 1) / 3 - 1; its mirror starts at t = L - 1 - i.
    // One division per lane (and per record that begins in it); from there the four numbers advance by counting
    uint32_t sm = (uint32_t)((i + 1u) % 3u), tm = (uint32_t)((L - 1u - i) % 3u);
    uint64_t sq1 = (i + 1u) / 3u, tq = (L - 1u - i) / 3u;
    while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctz(m);
        const uint64_t pos = at + bit;
        m &= m - 1u;
        if (r + 1u < n && start[r + 1u] <= pos) {                   // the first sequence byte of a later record: coordinate 0
            do ++r; while (r + 1u < n && start[r + 1u] <= pos);
            L = seq0[r + 1u] - seq0[r];
            base = out_base[r];
            fr = TrFrames(L);
            i = 0;
            sm = 1u; sq1 = 0; tm = (uint32_t)((L - 1u) % 3u); tq = (L - 1u) / 3u;
            q1 = q2 = 4u;
        }
        const uint32_t q0 = tr_base_code((uint32_t)((bit < 8u ? lo >> (8u * bit) : hi >> (8u * (bit - 8u))) & 0xFFu));
        if (i >= 2u) {
            out[base + (sm == 0u ? fr.fs[0] : sm == 1u ? fr.fs[1] : fr.fs[2]) + sq1 - 1u] = tr_residue(tab, q2, q1, q0);
            out[base + (tm == 0u ? fr.fs[3] : tm == 1u ? fr.fs[4] : fr.fs[5]) + tq] = tr_residue(tab, q0 ^ 2u, q1 ^ 2u, q2 ^ 2u);   // (4 ^ 2 keeps bit 2)
        }
        q2 = q1;
        q1 = q0;
        ++i;
        if (++sm == 3u) { sm = 0u; ++sq1; }
        if (tm == 0u) { tm = 2u; --tq; } else --tm;                 // (past the record's last byte these wrap; the next byte starts a record)
    }
}

// which of the lane's 16 output bytes are break bytes
__device__ __forceinline__ uint32_t tr_break_mask(const uint8_t *__restrict__ out, uint64_t bytes, uint64_t at)
{
    uint64_t lo, hi;
    const uint32_t valid = lane_load(out, at, bytes, lo, hi);
    return (eq_mask16(lo, hi, '*') | eq_mask16(lo, hi, 'X')) & valid;
}

__global__ void __launch_bounds__(256) tr_count_kernel(const uint8_t *__restrict__ out, uint64_t bytes, uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t wsum[4];
    const uint32_t m = tr_break_mask(out, bytes, (uint64_t)blockIdx.x * TEXT_TILE + threadIdx.x * 16ull);
    uint32_t sum;
    (void)block_scan_256((uint32_t)__builtin_popcount(m), wsum, &sum);
    if (threadIdx.x == 0u) tile_cnt[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256) tr_segoff_kernel(const uint8_t *__restrict__ out, uint64_t bytes, const uint64_t *__restrict__ tile_base,
                                                        uint64_t *__restrict__ seg_off)
{
    __shared__ uint32_t wsum[4];
    const uint64_t at = (uint64_t)blockIdx.x * TEXT_TILE + threadIdx.x * 16ull;
    uint32_t m = tr_break_mask(out, bytes, at), sum;
    uint64_t rank = tile_base[blockIdx.x] + block_scan_256((uint32_t)__builtin_popcount(m), wsum, &sum);
    while (m) {
        seg_off[++rank] = at + (uint32_t)__builtin_ctz(m) + 1u;     // the s-th break byte ends segment s: seg_off[s + 1]
        m &= m - 1u;
    }
}

__global__ void __launch_bounds__(256) tr_recseg_kernel(const uint64_t *__restrict__ seg_off, uint64_t n_seg, const uint64_t *__restrict__ out_base,
                                                        uint32_t n, uint64_t *__restrict__ rec_seg)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > n) return;
    const uint64_t x = out_base[r];                                 // (out_base[n] = the buffer's size = seg_off[n_seg])
    uint64_t lo = 0, hi = n_seg;                                    // the first s with seg_off[s] >= x: it is equal
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (seg_off[mid] < x) lo = mid + 1; else hi = mid; }
    rec_seg[r] = lo;
}

hipError_t launch_fasta_translate_sizes(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                        uint8_t *d_scratch, uint64_t *d_out_base, hipStream_t stream)
{
    const hipError_t e = launch_fasta_coords(d_raw, total, d_start, n_records, n_tiles, d_scratch, stream);
    if (e != hipSuccess) return e;
    const FastaCoords c = fasta_coords_view(d_scratch, n_tiles, n_records);
    hipLaunchKernelGGL(tr_size_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, c.seq0, n_records, d_out_base);
    return launch_tile_scan(d_out_base, d_out_base, n_records, stream);
}

hipError_t launch_fasta_translate_write(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                        uint8_t *d_scratch, const uint64_t *d_out_base, uint64_t out_bytes, uint8_t *d_out, uint64_t *d_tile_cnt,
                                        hipStream_t stream)
{
    const FastaCoords c = fasta_coords_view(d_scratch, n_tiles, n_records);
    hipLaunchKernelGGL(tr_term_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, c.seq0, d_out_base, n_records, d_out);
    if (n_tiles && n_records)
        hipLaunchKernelGGL(tr_map_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_start, n_records, c.lanes, c.tile_base, c.seq0, d_out_base,
                           d_out);
    const uint32_t n_out_tiles = (uint32_t)((out_bytes + TEXT_TILE - 1u) / TEXT_TILE);
    if (n_out_tiles) hipLaunchKernelGGL(tr_count_kernel, dim3(n_out_tiles), dim3(256), 0, stream, d_out, out_bytes, d_tile_cnt);
    return launch_tile_scan(d_tile_cnt, d_tile_cnt, n_out_tiles, stream);
}

hipError_t launch_fasta_translate_segments(const uint8_t *d_out, uint64_t out_bytes, const uint64_t *d_tile_base, const uint64_t *d_out_base,
                                           uint32_t n_records, uint64_t n_seg, uint64_t *d_seg_off, uint64_t *d_rec_seg, hipStream_t stream)
{
    const uint32_t n_out_tiles = (uint32_t)((out_bytes + TEXT_TILE - 1u) / TEXT_TILE);
    hipError_t e = hipMemsetAsync(d_seg_off, 0, 8, stream);         // seg_off[0] = 0
    if (e != hipSuccess) return e;
    if (n_out_tiles) hipLaunchKernelGGL(tr_segoff_kernel, dim3(n_out_tiles), dim3(256), 0, stream, d_out, out_bytes, d_tile_base, d_seg_off);
    hipLaunchKernelGGL(tr_recseg_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, d_seg_off, n_seg, d_out_base, n_records, d_rec_seg);
    return hipGetLastError();
}

}  // namespace lash
