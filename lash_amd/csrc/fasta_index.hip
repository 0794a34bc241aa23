// fasta_index.hip — the record index of raw multi-FASTA bytes, on the device: where every record starts, how long its id is and which
// file it belongs to (`lash sketch --per-record`; lash_fasta_index[_device]).  The raw-file route sketches one image per FILE; a FASTA
// record is itself a well-formed FASTA file, so with the record starts as file offsets that route sketches one image per record
// unchanged.  What was missing is the thing that finds the records.
//
// Rules (needletail's, the ones pack_kernels.hip applies when it sets record breaks): a record starts at a file's first byte, which must
// be '>', and at every '>' whose preceding byte IN THE SAME FILE is '\n'; a '>' anywhere else starts nothing.  The id is what follows
// the '>' up to the first space / TAB / CR / LF or the end of the file.
//
// Four small kernels over the 4 KiB tiles of the whole buffer (text_tiles.h: count, scan, ordered write):
//   1. fa_mark_kernel   per tile: 16 bytes per lane + the byte before them -> a 16-bit mask of record starts per lane, a count per tile;
//                       the files that begin inside a lane's 16 bytes are looked up in the sorted offset table
//   2. launch_tile_scan one workgroup: exclusive scan of the tile counts; the total is the number of records
//   3. fa_write_kernel  per tile: start[] and file[] of its records at tile base + prefix inside the tile (wave scan, no atomics: the
//                       order is file order then byte order whatever the scheduling)
//   4. fa_id_kernel     one thread per record walks its header for id_len[]
// Traffic: the mark pass reads every byte once and writes 2 bytes of mask per 16; the other passes touch only masks, counts and headers
// (kernel times: profiles/r08/per_record.txt).
#include <hip/hip_runtime.h>

#include "lash_kernels.h"
#include "text_tiles.h"

namespace lash {

__global__ void __launch_bounds__(256) fa_mark_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ file_off,
                                                      uint32_t n_files, uint16_t *__restrict__ masks, uint32_t *__restrict__ cnt,
                                                      uint32_t *__restrict__ bad)
{
    __shared__ uint32_t wsum[4];
    const uint64_t at = (uint64_t)blockIdx.x * TEXT_TILE + threadIdx.x * 16ull;
    uint32_t m = 0;
    uint64_t lo, hi;
    if (lane_load(raw, at, total, lo, hi)) {                        // (at < total; the zero bytes past the end are neither '>' nor '\n')
        const uint32_t gt = eq_mask16(lo, hi, '>'), nl = eq_mask16(lo, hi, '\n');
        const uint32_t prev = at > 0 && raw[at - 1] == '\n' ? 1u : 0u;
        m = gt & ((nl << 1) | prev) & 0xFFFFu;
        // files that begin inside these 16 bytes: their first byte is a record start whatever precedes it, and must be '>'
        // (one search of the table per tile, the same for every lane; a lane searches only among the files of its tile: mostly none)
        const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE;
        const uint32_t jt = count_lt(file_off, n_files, tile0), je = jt + count_lt(file_off + jt, n_files - jt, tile0 + TEXT_TILE);
        for (uint32_t j = jt + count_lt(file_off + jt, je - jt, at); j < je && file_off[j] < at + 16; ++j) {
            if (file_off[j + 1] == file_off[j]) continue;          // an empty file holds no record
            const uint32_t bit = 1u << (uint32_t)(file_off[j] - at);
            if (gt & bit) m |= bit;
            else { m &= ~bit; bad[0] = 1u; }
        }
    }
    masks[(uint64_t)blockIdx.x * 256u + threadIdx.x] = (uint16_t)m;
    uint32_t s = (uint32_t)__builtin_popcount(m);                   // only the tile's total is wanted here: a reduce, not block_scan_256
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(256) fa_write_kernel(const uint16_t *__restrict__ masks, const uint32_t *__restrict__ base,
                                                       const uint64_t *__restrict__ file_off, uint32_t n_files, uint32_t n_records,
                                                       uint64_t *__restrict__ start, uint32_t *__restrict__ file)
{
    __shared__ uint32_t wsum[4];
    uint32_t m = masks[(uint64_t)blockIdx.x * 256u + threadIdx.x];
    const uint32_t mine = (uint32_t)__builtin_popcount(m);
    uint32_t sum;
    const uint32_t pre = block_scan_256(mine, wsum, &sum);         // (the barrier is in there: before any lane leaves)
    if (!m) return;
    uint32_t r = base[blockIdx.x] + pre;
    const uint64_t at = (uint64_t)blockIdx.x * TEXT_TILE + threadIdx.x * 16ull;
    // the file of the lane's first record: the last one that begins at or before it (of several at one offset the last, the non-empty one)
    uint32_t f = count_lt(file_off, n_files, at + (uint32_t)__builtin_ctz(m) + 1u) - 1u;
    while (m) {
        const uint64_t pos = at + (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        while (f + 1u < n_files && file_off[f + 1u] <= pos) ++f;
        if (r < n_records) { start[r] = pos; file[r] = f; }
        ++r;
    }
}

__global__ void __launch_bounds__(256) fa_id_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ file_off,
                                                    uint32_t n_records, uint64_t *__restrict__ start, const uint32_t *__restrict__ file,
                                                    uint32_t *__restrict__ id_len)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r == 0) start[n_records] = total;                          // record r is [start[r], start[r + 1]); the last one ends with its file
    if (r >= n_records) return;
    const uint64_t s = start[r] + 1u, end = min(total, file_off[file[r] + 1u]);
    uint64_t p = s;
    for (; p < end; ++p) {
        const uint8_t c = raw[p];
        if (c == ' ' || c == '\t' || c == '\r' || c == '\n') break;
    }
    id_len[r] = (uint32_t)min(p - s, (uint64_t)0xFFFFFFFFu);
}

// scratch: [masks: n_tiles * 256 u16 | cnt: n_tiles u32 | base: n_tiles + 1 u32 | bad: 1 u32], 16-byte aligned sections
size_t fasta_index_scratch_bytes(uint32_t n_tiles) { return (size_t)n_tiles * 512 + (((size_t)n_tiles * 4 + 15) & ~(size_t)15) + (size_t)n_tiles * 4 + 64; }

static void fa_sections(uint8_t *scratch, uint32_t n_tiles, uint16_t *&masks, uint32_t *&cnt, uint32_t *&base, uint32_t *&bad)
{
    masks = reinterpret_cast<uint16_t *>(scratch);
    cnt = reinterpret_cast<uint32_t *>(scratch + (size_t)n_tiles * 512);
    base = reinterpret_cast<uint32_t *>(scratch + (size_t)n_tiles * 512 + (((size_t)n_tiles * 4 + 15) & ~(size_t)15));
    bad = base + n_tiles + 1;
}

hipError_t launch_fasta_mark(const uint8_t *d_raw, uint64_t total, const uint64_t *d_file_off, uint32_t n_files, uint32_t n_tiles,
                             uint8_t *d_scratch, const uint32_t **d_n_records_and_bad, hipStream_t stream)
{
    uint16_t *masks; uint32_t *cnt, *base, *bad;
    fa_sections(d_scratch, n_tiles, masks, cnt, base, bad);
    hipError_t e = hipMemsetAsync(base + n_tiles, 0, 8, stream);   // the total (n_tiles == 0: nothing writes it) and the flag
    if (e != hipSuccess) return e;
    if (n_tiles) {
        hipLaunchKernelGGL(fa_mark_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_file_off, n_files, masks, cnt, bad);
        if ((e = launch_tile_scan(cnt, base, n_tiles, stream)) != hipSuccess) return e;    // base[t] = records before tile t, base[n_tiles] = all of them
    }
    *d_n_records_and_bad = base + n_tiles;                         // [0] records, [1] a file does not begin with '>'
    return hipGetLastError();
}

hipError_t launch_fasta_write(const uint8_t *d_raw, uint64_t total, const uint64_t *d_file_off, uint32_t n_files, uint32_t n_tiles,
                              uint8_t *d_scratch, uint32_t n_records, uint64_t *d_start, uint32_t *d_file, uint32_t *d_id_len, hipStream_t stream)
{
    uint16_t *masks; uint32_t *cnt, *base, *bad;
    fa_sections(d_scratch, n_tiles, masks, cnt, base, bad);
    if (n_tiles && n_records)
        hipLaunchKernelGGL(fa_write_kernel, dim3(n_tiles), dim3(256), 0, stream, masks, base, d_file_off, n_files, n_records, d_start, d_file);
    hipLaunchKernelGGL(fa_id_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, d_raw, total, d_file_off, n_records, d_start, d_file, d_id_len);
    return hipGetLastError();
}

}  // namespace lash
