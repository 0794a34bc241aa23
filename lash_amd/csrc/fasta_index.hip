// fasta_index.hip — the record index of raw multi-FASTA bytes, on the device: where every record starts, how long its id is and which
// file it belongs to (`lash sketch --per-record`; lash_fasta_index[_device]).  The raw-file route sketches one image per FILE; a FASTA
// record is itself a well-formed FASTA file, so with the record starts as file offsets that route sketches one image per record
// unchanged.  What was missing is the thing that finds the records.
//
// Rules (needletail's, the ones pack_kernels.hip applies when it sets record breaks): a record starts at a file's first byte, which must
// be '>', and at every '>' whose preceding byte IN THE SAME FILE is '\n'; a '>' anywhere else starts nothing.  The id is what follows
// the '>' up to the first space / TAB / CR / LF or the end of the file.
//
// Four small kernels over 4 KiB tiles of the whole buffer (the shape of fastq_check.hip and dist_filter.h: count, scan, ordered write):
//   1. fa_mark_kernel   per tile: 16 bytes per lane + the byte before them -> a 16-bit mask of record starts per lane, a count per tile;
//                       the files that begin inside a lane's 16 bytes are looked up in the sorted offset table
//   2. fa_scan_kernel   one workgroup: exclusive scan of the tile counts; the total is the number of records
//   3. fa_write_kernel  per tile: start[] and file[] of its records at tile base + prefix inside the tile (wave scan, no atomics: the
//                       order is file order then byte order whatever the scheduling)
//   4. fa_id_kernel     one thread per record walks its header for id_len[]
// Traffic: the mark pass reads every byte once and writes 2 bytes of mask per 16; the other passes touch only masks, counts and headers
// (kernel times: profiles/r08/per_record.txt).
#include <hip/hip_runtime.h>

#include "lash_kernels.h"

namespace lash {

constexpr uint32_t FA_TILE = 4096;           // bytes per tile = 256 threads x 16

// bit i: byte i of the 8 in x equals c
__device__ __forceinline__ uint32_t eq_mask8(uint64_t x, uint8_t c)
{
    const uint64_t z = x ^ (0x0101010101010101ull * c);
    const uint64_t nz = ((z & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | z;     // high bit of a byte set <=> the byte is non-zero
    return (uint32_t)((((~nz >> 7) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

// first j in [0, n) with off[j] >= x (n when there is none)
__device__ __forceinline__ uint32_t lower_bound_off(const uint64_t *off, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(256) fa_mark_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ file_off,
                                                      uint32_t n_files, uint16_t *__restrict__ masks, uint32_t *__restrict__ cnt,
                                                      uint32_t *__restrict__ bad)
{
    __shared__ uint32_t wsum[4];
    const uint64_t at = (uint64_t)blockIdx.x * FA_TILE + threadIdx.x * 16ull;
    uint32_t m = 0;
    if (at < total) {
        const uint64_t avail = total - at;
        uint64_t lo = 0, hi = 0;
        if (avail >= 16) {
            uint4 q;
            __builtin_memcpy(&q, raw + at, 16);
            lo = q.x | ((uint64_t)q.y << 32);
            hi = q.z | ((uint64_t)q.w << 32);
        } else {
            for (uint32_t i = 0; i < (uint32_t)avail; ++i) {       // the buffer's last bytes; a zero byte is neither '>' nor '\n'
                const uint64_t b = raw[at + i];
                if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u));
            }
        }
        const uint32_t gt = eq_mask8(lo, '>') | (eq_mask8(hi, '>') << 8);
        const uint32_t nl = eq_mask8(lo, '\n') | (eq_mask8(hi, '\n') << 8);
        const uint32_t prev = at > 0 && raw[at - 1] == '\n' ? 1u : 0u;
        m = gt & ((nl << 1) | prev) & 0xFFFFu;
        // files that begin inside these 16 bytes: their first byte is a record start whatever precedes it, and must be '>'
        // (one search of the table per tile, the same for every lane; a lane searches only among the files of its tile: mostly none)
        const uint64_t tile0 = (uint64_t)blockIdx.x * FA_TILE;
        const uint32_t jt = lower_bound_off(file_off, n_files, tile0), je = jt + lower_bound_off(file_off + jt, n_files - jt, tile0 + FA_TILE);
        for (uint32_t j = jt + lower_bound_off(file_off + jt, je - jt, at); j < je && file_off[j] < at + 16; ++j) {
            if (file_off[j + 1] == file_off[j]) continue;          // an empty file holds no record
            const uint32_t bit = 1u << (uint32_t)(file_off[j] - at);
            if (gt & bit) m |= bit;
            else { m &= ~bit; bad[0] = 1u; }
        }
    }
    masks[(uint64_t)blockIdx.x * 256u + threadIdx.x] = (uint16_t)m;
    uint32_t s = (uint32_t)__builtin_popcount(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: base[t] = records before tile t, base[n_tiles] = all of them
__global__ void __launch_bounds__(1024) fa_scan_kernel(const uint32_t *__restrict__ cnt, uint32_t n_tiles, uint32_t *__restrict__ base)
{
    __shared__ uint32_t part[1024];
    const uint32_t per = (n_tiles + 1023u) / 1024u, t0 = min(n_tiles, threadIdx.x * per), t1 = min(n_tiles, t0 + per);
    uint32_t s = 0;
    for (uint32_t t = t0; t < t1; ++t) s += cnt[t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t acc = 0; for (uint32_t i = 0; i < 1024; ++i) { const uint32_t v = part[i]; part[i] = acc; acc += v; } base[n_tiles] = acc; }
    __syncthreads();
    uint32_t acc = part[threadIdx.x];
    for (uint32_t t = t0; t < t1; ++t) { base[t] = acc; acc += cnt[t]; }
}

__global__ void __launch_bounds__(256) fa_write_kernel(const uint16_t *__restrict__ masks, const uint32_t *__restrict__ base,
                                                       const uint64_t *__restrict__ file_off, uint32_t n_files, uint32_t n_records,
                                                       uint64_t *__restrict__ start, uint32_t *__restrict__ file)
{
    __shared__ uint32_t wsum[4];
    uint32_t m = masks[(uint64_t)blockIdx.x * 256u + threadIdx.x];
    const uint32_t mine = (uint32_t)__builtin_popcount(m);
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63u) >= d) incl += v; }
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (!m) return;
    uint32_t r = base[blockIdx.x] + incl - mine;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) r += wsum[w];
    const uint64_t at = (uint64_t)blockIdx.x * FA_TILE + threadIdx.x * 16ull;
    // the file of the lane's first record: the last one that begins at or before it (of several at one offset the last, the non-empty one)
    uint32_t f = lower_bound_off(file_off, n_files, at + (uint32_t)__builtin_ctz(m) + 1u) - 1u;
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

uint32_t fasta_index_tile_bytes() { return FA_TILE; }

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
        hipLaunchKernelGGL(fa_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, n_tiles, base);
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
