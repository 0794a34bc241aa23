// fasta_windows.hip — fixed-length windows of FASTA records, built on the device (`lash sketch --window W`; lash_fasta_windows[_device]).
// fasta_index.hip finds the records; this stage cuts every record's sequence into windows of W bases and writes each window out as a
// one-record FASTA file (">\n", the window's bytes, "\n"), so that the raw-file route sketches one image per window unchanged.  A window
// is not a byte range of the input: it starts mid-line, has no header and holds line ends, so it has to be built.
//
// Rules: the sequence bytes of record r are the bytes after its header line's '\n' up to start[r + 1] that are neither LF nor CR (every
// other byte counts: N, lower case, a stray '>').  Their 0-based rank in the record is the coordinate.  A record of L sequence bytes has
// ceil(L / W) windows, window j = coordinates [jW, min(L, (j + 1)W)); L = 0 gives none.  Windows come in record order, then j.
//
// Passes over the 4 KiB tiles of fasta_index.hip (16 bytes per lane; count, scan, ordered write; no atomics, nothing depends on scheduling):
//   1. fw_seqbegin_kernel  one thread per record walks its header line: seq_begin[r]
//   2. fw_count_kernel     per tile: a 16-bit mask of sequence bytes per lane and the lane's rank inside the tile (one u32), a count per tile
//   3. fw_scan_kernel      one workgroup: exclusive 64-bit scan of the tile counts
//   4. fw_rec_kernel       per record: rank of its first sequence byte in the whole buffer (seq0[r]), hence L_r and its window count
//   5. fw_scan_kernel      ... scanned to win_base[r]; the host reads the two totals (sequence bytes S, windows n) and makes room
//   6. fw_fill_kernel      one thread per window: record[], begin[], length[], off[] and the window's three framing bytes
//   7. fw_scatter_kernel   per tile: sequence byte of global rank g, in window w, goes to out[g + 3w + 2]
// The output holds exactly S + 3n bytes.  Traffic: the input is read twice (count, scatter), 4 bytes per 16 of lane words are written and
// read, and every sequence byte is written once: about 2.5 bytes moved per input byte.
#include <hip/hip_runtime.h>

#include "lash_kernels.h"

namespace lash {

constexpr uint32_t FW_TILE = 4096;           // bytes per tile = 256 threads x 16 (fasta_index.hip's)

// bit i: byte i of the 8 in x equals c
__device__ __forceinline__ uint32_t fw_eq_mask8(uint64_t x, uint8_t c)
{
    const uint64_t z = x ^ (0x0101010101010101ull * c);
    const uint64_t nz = ((z & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | z;
    return (uint32_t)((((~nz >> 7) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

// number of j in [0, n) with a[j] <= x (a ascending)
__device__ __forceinline__ uint32_t fw_count_le(const uint64_t *a, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// the record of byte `at` (start[0] == 0, so there is one): one search of start[] per tile, the same for every lane, then one among the
// records that begin inside the tile (mostly none)
__device__ __forceinline__ uint32_t fw_record_of(const uint64_t *start, uint32_t n, uint64_t tile0, uint64_t at)
{
    const uint32_t rt = fw_count_le(start, n, tile0) - 1u;
    const uint32_t in_tile = fw_count_le(start + rt + 1u, n - rt - 1u, tile0 + FW_TILE - 1u);
    return rt + fw_count_le(start + rt + 1u, in_tile, at);
}

__global__ void __launch_bounds__(256) fw_seqbegin_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ start, uint32_t n,
                                                          uint64_t *__restrict__ seq_begin)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint64_t end = start[r + 1u];
    uint64_t p = start[r];
    while (p < end && raw[p] != '\n') ++p;
    seq_begin[r] = p < end ? p + 1u : end;                          // a header with no line end: the record has no sequence
}

__global__ void __launch_bounds__(256) fw_count_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ start,
                                                       const uint64_t *__restrict__ seq_begin, uint32_t n, uint32_t *__restrict__ lanes,
                                                       uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t wsum[4];
    const uint64_t tile0 = (uint64_t)blockIdx.x * FW_TILE, at = tile0 + threadIdx.x * 16ull;
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
            for (uint32_t i = 0; i < (uint32_t)avail; ++i) {
                const uint64_t b = raw[at + i];
                if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u));
            }
        }
        const uint32_t valid = avail >= 16 ? 0xFFFFu : (1u << (uint32_t)avail) - 1u;
        const uint32_t le = fw_eq_mask8(lo, '\n') | (fw_eq_mask8(hi, '\n') << 8) | fw_eq_mask8(lo, '\r') | (fw_eq_mask8(hi, '\r') << 8);
        m = ~le & valid;
        // header bytes [start[r], seq_begin[r]) of every record that touches these 16 bytes are no sequence
        for (uint32_t r = fw_record_of(start, n, tile0, at); r < n && start[r] < at + 16u; ++r) {
            const uint64_t sb = seq_begin[r];
            if (sb <= at) continue;
            const uint32_t a = start[r] > at ? (uint32_t)(start[r] - at) : 0u, b = sb < at + 16u ? (uint32_t)(sb - at) : 16u;
            m &= ~(((1u << b) - 1u) & ~((1u << a) - 1u));
        }
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(m);
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63u) >= d) incl += v; }
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = incl - mine;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) pre += wsum[w];
    lanes[(uint64_t)blockIdx.x * 256u + threadIdx.x] = (pre << 16) | m;      // pre <= 4080
    if (threadIdx.x == 255u) tile_cnt[blockIdx.x] = pre + mine;
}

// one workgroup, in place: a[i] = a[0] + ... + a[i - 1] for i in [0, n], a[n] the total
__global__ void __launch_bounds__(1024) fw_scan_kernel(uint64_t *__restrict__ a, uint32_t n)
{
    __shared__ uint64_t part[1024];
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t t0 = (uint32_t)min((uint64_t)n, (uint64_t)threadIdx.x * per), t1 = (uint32_t)min((uint64_t)n, (uint64_t)t0 + per);
    uint64_t s = 0;
    for (uint32_t t = t0; t < t1; ++t) s += a[t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint64_t acc = 0; for (uint32_t i = 0; i < 1024; ++i) { const uint64_t v = part[i]; part[i] = acc; acc += v; } a[n] = acc; }
    __syncthreads();
    uint64_t acc = part[threadIdx.x];
    for (uint32_t t = t0; t < t1; ++t) { const uint64_t v = a[t]; a[t] = acc; acc += v; }
}

// sequence bytes before position pos (pos <= total)
__device__ __forceinline__ uint64_t fw_rank(const uint32_t *lanes, const uint64_t *tile_base, uint32_t n_tiles, uint64_t total, uint64_t pos)
{
    if (pos >= total) return tile_base[n_tiles];
    const uint32_t w = lanes[pos >> 4];
    return tile_base[pos / FW_TILE] + (w >> 16) + (uint32_t)__builtin_popcount(w & ((1u << (uint32_t)(pos & 15u)) - 1u));
}

__global__ void __launch_bounds__(256) fw_rec_kernel(const uint64_t *__restrict__ seq_begin, uint32_t n, uint64_t total,
                                                     const uint32_t *__restrict__ lanes, const uint64_t *__restrict__ tile_base, uint32_t n_tiles,
                                                     uint64_t window, uint64_t *__restrict__ seq0, uint64_t *__restrict__ win_cnt)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > n) return;
    // nothing between seq_begin[r] and seq_begin[r + 1] but the sequence of r and the header of r + 1: L_r is the difference of the ranks
    const uint64_t a = fw_rank(lanes, tile_base, n_tiles, total, r < n ? seq_begin[r] : total);
    seq0[r] = a;
    if (r == n) return;
    const uint64_t len = fw_rank(lanes, tile_base, n_tiles, total, r + 1u < n ? seq_begin[r + 1u] : total) - a;
    win_cnt[r] = len / window + (len % window ? 1u : 0u);
}

__global__ void __launch_bounds__(256) fw_fill_kernel(const uint64_t *__restrict__ seq0, const uint64_t *__restrict__ win_base, uint32_t n,
                                                      uint64_t window, uint64_t n_win, uint64_t *__restrict__ record, uint64_t *__restrict__ begin,
                                                      uint64_t *__restrict__ length, uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w == 0) off[n_win] = seq0[n] + 3u * n_win;
    if (w >= n_win) return;
    const uint32_t r = fw_count_le(win_base, n, w) - 1u;           // the last record with win_base[r] <= w: it has win_base[r + 1] > w
    const uint64_t j = w - win_base[r], len_r = seq0[r + 1u] - seq0[r], b = j * window, len = min(window, len_r - b), o = seq0[r] + b + 3u * w;
    record[w] = r;
    begin[w] = b;
    length[w] = len;
    off[w] = o;
    out[o] = '>';
    out[o + 1u] = '\n';
    out[o + 2u + len] = '\n';
}

__global__ void __launch_bounds__(256) fw_scatter_kernel(const uint8_t *__restrict__ raw, uint64_t total, const uint64_t *__restrict__ start,
                                                         uint32_t n, const uint32_t *__restrict__ lanes, const uint64_t *__restrict__ tile_base,
                                                         const uint64_t *__restrict__ seq0, const uint64_t *__restrict__ win_base, uint64_t window,
                                                         uint8_t *__restrict__ out)
{
    const uint64_t tile0 = (uint64_t)blockIdx.x * FW_TILE, at = tile0 + threadIdx.x * 16ull;
    const uint32_t word = lanes[(uint64_t)blockIdx.x * 256u + threadIdx.x];
    uint32_t m = word & 0xFFFFu;
    if (!m) return;                                                 // (a lane past the end of the buffer has no bit set)
    uint64_t g = tile_base[blockIdx.x] + (word >> 16);              // rank of the lane's first sequence byte in the whole buffer
    uint32_t r = fw_record_of(start, n, tile0, at + (uint32_t)__builtin_ctz(m));
    // one division per lane; from there the window advances by counting
    uint64_t i = g - seq0[r], w = win_base[r] + i / window, rem = i % window;
    while (m) {
        const uint64_t pos = at + (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        if (r + 1u < n && start[r + 1u] <= pos) {                   // the first sequence byte of a later record: its window 0, coordinate 0
            do ++r; while (r + 1u < n && start[r + 1u] <= pos);
            w = win_base[r];
            rem = 0;
        } else if (rem == window) { ++w; rem = 0; }
        out[g + 3u * w + 2u] = raw[pos];
        ++g;
        ++rem;
    }
}

// scratch: [lanes: n_tiles * 256 u32 | tile_base: n_tiles + 1 u64 | seq_begin: n u64 | seq0: n + 1 u64 | win_base: n + 1 u64]
size_t fasta_windows_scratch_bytes(uint32_t n_tiles, uint32_t n_records)
{
    return (size_t)n_tiles * 1024 + ((size_t)n_tiles + 1) * 8 + ((size_t)n_records * 3 + 2) * 8 + 64;
}

static void fw_sections(uint8_t *scratch, uint32_t n_tiles, uint32_t n, uint32_t *&lanes, uint64_t *&tile_base, uint64_t *&seq_begin,
                        uint64_t *&seq0, uint64_t *&win_base)
{
    lanes = reinterpret_cast<uint32_t *>(scratch);
    tile_base = reinterpret_cast<uint64_t *>(scratch + (size_t)n_tiles * 1024);
    seq_begin = tile_base + n_tiles + 1;
    seq0 = seq_begin + n;
    win_base = seq0 + n + 1;
}

void fasta_windows_rank_view(uint8_t *d_scratch, uint32_t n_tiles, uint32_t n_records, const uint32_t **d_lanes, const uint64_t **d_tile_base,
                             const uint64_t **d_seq0)
{
    uint32_t *lanes; uint64_t *tile_base, *seq_begin, *seq0, *win_base;
    fw_sections(d_scratch, n_tiles, n_records, lanes, tile_base, seq_begin, seq0, win_base);
    *d_lanes = lanes;
    *d_tile_base = tile_base;
    *d_seq0 = seq0;
}

hipError_t launch_scan_u64(uint64_t *d_a, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(fw_scan_kernel, dim3(1), dim3(1024), 0, stream, d_a, n);
    return hipGetLastError();
}

hipError_t launch_fasta_windows_count(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                      uint64_t window, uint8_t *d_scratch, const uint64_t **d_seq_bytes, const uint64_t **d_n_windows,
                                      hipStream_t stream)
{
    uint32_t *lanes; uint64_t *tile_base, *seq_begin, *seq0, *win_base;
    fw_sections(d_scratch, n_tiles, n_records, lanes, tile_base, seq_begin, seq0, win_base);
    hipLaunchKernelGGL(fw_seqbegin_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, d_raw, d_start, n_records, seq_begin);
    if (n_tiles) hipLaunchKernelGGL(fw_count_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_start, seq_begin, n_records, lanes, tile_base);
    hipLaunchKernelGGL(fw_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_base, n_tiles);
    hipLaunchKernelGGL(fw_rec_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, seq_begin, n_records, total, lanes, tile_base, n_tiles, window,
                       seq0, win_base);
    hipLaunchKernelGGL(fw_scan_kernel, dim3(1), dim3(1024), 0, stream, win_base, n_records);
    *d_seq_bytes = seq0 + n_records;
    *d_n_windows = win_base + n_records;
    return hipGetLastError();
}

hipError_t launch_fasta_windows_write(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                      uint64_t window, uint8_t *d_scratch, uint64_t n_windows, uint64_t *d_record, uint64_t *d_begin,
                                      uint64_t *d_length, uint64_t *d_off, uint8_t *d_out, hipStream_t stream)
{
    uint32_t *lanes; uint64_t *tile_base, *seq_begin, *seq0, *win_base;
    fw_sections(d_scratch, n_tiles, n_records, lanes, tile_base, seq_begin, seq0, win_base);
    hipLaunchKernelGGL(fw_fill_kernel, dim3((uint32_t)(n_windows / 256u + 1u)), dim3(256), 0, stream, seq0, win_base, n_records, window, n_windows,
                       d_record, d_begin, d_length, d_off, d_out);
    if (n_tiles && n_windows)
        hipLaunchKernelGGL(fw_scatter_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_start, n_records, lanes, tile_base, seq0, win_base,
                           window, d_out);
    return hipGetLastError();
}

}  // namespace lash
