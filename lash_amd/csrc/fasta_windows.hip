// fasta_windows.hip — fixed-length windows of FASTA records, built on the device (`lash sketch --window W`; lash_fasta_windows[_device]).
// fasta_index.hip finds the records and fasta_coords.hip gives every sequence byte its coordinate; this stage cuts every record's sequence
// into windows of W bases and writes each window out as a one-record FASTA file (">\n", the window's bytes, "\n"), so that the raw-file route
// sketches one image per window unchanged.  A window is not a byte range of the input: it starts mid-line, has no header and holds line
// ends, so it has to be built.
//
// Rules: a record of L sequence bytes (fasta_coords.hip) has ceil(L / W) windows, window j = coordinates [jW, min(L, (j + 1)W)); L = 0 gives
// none.  Windows come in record order, then j.
//
// Passes (no atomics, nothing depends on scheduling):
//   1. launch_fasta_coords  lane words, tile bases and seq0[r]: the coordinate of every sequence byte
//   2. fw_wincnt_kernel     per record: its window count from L_r = seq0[r + 1] - seq0[r]
//   3. launch_tile_scan     ... scanned to win_base[r]; the host reads the two totals (sequence bytes S, windows n) and makes room
//   4. fw_fill_kernel       one thread per window: record[], begin[], length[], off[] and the window's three framing bytes
//   5. fw_scatter_kernel    per 4 KiB tile of the input: sequence byte of global rank g, in window w, goes to out[g + 3w + 2]
// The output holds exactly S + 3n bytes.  Traffic: the input is read twice (coordinates, scatter), 4 bytes per 16 of lane words are written
// and read, and every sequence byte is written once: about 2.5 bytes moved per input byte.
#include <hip/hip_runtime.h>

#include "lash_kernels.h"
#include "text_tiles.h"

namespace lash {

__global__ void __launch_bounds__(256) fw_wincnt_kernel(const uint64_t *__restrict__ seq0, uint32_t n, uint64_t window, uint64_t *__restrict__ win_cnt)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint64_t len = seq0[r + 1u] - seq0[r];
    win_cnt[r] = len / window + (len % window ? 1u : 0u);
}

__global__ void __launch_bounds__(256) fw_fill_kernel(const uint64_t *__restrict__ seq0, const uint64_t *__restrict__ win_base, uint32_t n,
                                                      uint64_t window, uint64_t n_win, uint64_t *__restrict__ record, uint64_t *__restrict__ begin,
                                                      uint64_t *__restrict__ length, uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w == 0) off[n_win] = seq0[n] + 3u * n_win;
    if (w >= n_win) return;
    const uint32_t r = count_le(win_base, n, w) - 1u;              // the last record with win_base[r] <= w: it has win_base[r + 1] > w
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
    const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE, at = tile0 + threadIdx.x * 16ull;
    const uint32_t word = lanes[(uint64_t)blockIdx.x * 256u + threadIdx.x];
    uint32_t m = word & 0xFFFFu;
    if (!m) return;                                                 // (a lane past the end of the buffer has no bit set)
    uint64_t g = tile_base[blockIdx.x] + (word >> 16);              // rank of the lane's first sequence byte in the whole buffer
    uint32_t r = record_of(start, n, tile0, at + (uint32_t)__builtin_ctz(m));
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

// scratch: [the coordinates: fasta_coords_scratch_bytes | win_base: n + 1 u64]
size_t fasta_windows_scratch_bytes(uint32_t n_tiles, uint32_t n_records)
{
    return fasta_coords_scratch_bytes(n_tiles, n_records) + ((size_t)n_records + 1) * 8;
}

static uint64_t *fw_win_base(uint8_t *d_scratch, uint32_t n_tiles, uint32_t n_records)
{
    return reinterpret_cast<uint64_t *>(d_scratch + fasta_coords_scratch_bytes(n_tiles, n_records));
}

hipError_t launch_fasta_windows_count(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                      uint64_t window, uint8_t *d_scratch, const uint64_t **d_seq_bytes, const uint64_t **d_n_windows,
                                      hipStream_t stream)
{
    const hipError_t e = launch_fasta_coords(d_raw, total, d_start, n_records, n_tiles, d_scratch, stream);
    if (e != hipSuccess) return e;
    const FastaCoords c = fasta_coords_view(d_scratch, n_tiles, n_records);
    uint64_t *win_base = fw_win_base(d_scratch, n_tiles, n_records);
    hipLaunchKernelGGL(fw_wincnt_kernel, dim3(n_records / 256u + 1u), dim3(256), 0, stream, c.seq0, n_records, window, win_base);
    *d_seq_bytes = c.seq0 + n_records;
    *d_n_windows = win_base + n_records;
    return launch_tile_scan(win_base, win_base, n_records, stream);
}

hipError_t launch_fasta_windows_write(const uint8_t *d_raw, uint64_t total, const uint64_t *d_start, uint32_t n_records, uint32_t n_tiles,
                                      uint64_t window, uint8_t *d_scratch, uint64_t n_windows, uint64_t *d_record, uint64_t *d_begin,
                                      uint64_t *d_length, uint64_t *d_off, uint8_t *d_out, hipStream_t stream)
{
    const FastaCoords c = fasta_coords_view(d_scratch, n_tiles, n_records);
    const uint64_t *win_base = fw_win_base(d_scratch, n_tiles, n_records);
    hipLaunchKernelGGL(fw_fill_kernel, dim3((uint32_t)(n_windows / 256u + 1u)), dim3(256), 0, stream, c.seq0, win_base, n_records, window, n_windows,
                       d_record, d_begin, d_length, d_off, d_out);
    if (n_tiles && n_windows)
        hipLaunchKernelGGL(fw_scatter_kernel, dim3(n_tiles), dim3(256), 0, stream, d_raw, total, d_start, n_records, c.lanes, c.tile_base, c.seq0,
                           win_base, window, d_out);
    return hipGetLastError();
}

}  // namespace lash
