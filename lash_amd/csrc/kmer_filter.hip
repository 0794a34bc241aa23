// kmer_filter.hip — the k-mer abundance filter of `lash sketch --min-count M` (lash_kmer_filter_*, lash_sketch_files_raw_filtered): drop
// the k-mers a file holds fewer than M times before they reach the sketch.  A sequencing error makes up to k k-mers that exist nowhere
// else; in a read set they can outnumber the real ones (Mash -m, sourmash and Dashing filter the same way).  Not in the reference.
//
// Two passes over the pack stage's output (2-bit words, record-start bitmap, nvalid), each walking the stream as sketch_kernel does — a
// lane owns 4 consecutive words = 64 k-mer start positions, the windows, the reverse complement and the validity mask are the helpers of
// sketch_rules.h — so all three walks see the same k-mers at the same positions:
//   kmer_count_kernel   every valid occurrence increments two cells of its file's table (a count-min sketch with two rows sharing one
//                       array; lash_kernels.h gives the addresses).  A cell is a byte of a 32-bit word and saturates at 255: the increment is
//                       a compare-and-swap on the word that adds 1 << (8 * (i & 3)) only while that byte is below 255, so no carry ever reaches
//                       the neighbouring cell, and a lane that loads a saturated cell issues no atomic at all (a homopolymer run would
//                       otherwise hammer one word from every lane).  Saturating adds commute: the cells are min(255, occurrences that
//                       map there) whatever the order of lanes, launches or chunks.
//   kmer_keep_kernel    after the whole file has been counted: keep bit i <=> position i starts a valid k-mer and both its cells are >= M.
//                       One bit per base beside brk; sketch_kernel<REGS_LDS_KEEP> ANDs them into its validity mask.
// A k-mer with a true count >= M always passes (its cells count at least its own occurrences); one with a smaller count passes only
// when collisions lift BOTH cells.
#include <algorithm>

#include "sketch_rules.h"

namespace lash {

// the walk both kernels share; KEEP_PASS: read the cells and write keep bits instead of counting
template <int KMODE, bool KEEP_PASS>
__device__ __forceinline__ void kmer_filter_walk(const KmerFilterArgs &a)
{
    const int k = a.k;
    KParams kp{};                                                          // the window fields only: nothing is hashed with xxh3 here
    kp.set_window<KMODE>(k);
    const uint32_t cm = a.comp_mask;
    for (uint32_t g = blockIdx.y; g < a.n_genomes; g += gridDim.y) {
        const GenomeDesc gd = a.genomes[g];
        const uint64_t L = a.nvalid[g];
        if (L < (uint64_t)k) continue;
        const uint64_t nk = L - (uint64_t)k + 1;                           // k-mer start positions of the genome (< 2^32 - 64)
        const uint32_t nk_words = (uint32_t)((nk + 15) >> 4);              // word w holds a k-mer start <=> w < nk_words
        const uint32_t *__restrict__ w = a.words + gd.word_off;
        const bool multi_rec = gd.format != 0u || gd.rec_end - gd.rec_begin > 1;   // (as sketch_kernel; always true here: the filter takes raw files only, format != 0)
        const uint32_t *__restrict__ bk = a.brk + gd.brk_off;
        uint32_t *cells = a.cells + a.cell_word[g];
        const uint32_t sh = 64u - (uint32_t)a.log2_cells[g];
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * SKETCH_WORDS_PER_THREAD;
        for (uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SKETCH_WORDS_PER_THREAD; w0 < nk_words; w0 += stride) {
            // words w0 .. w0 + 5 (the genome is followed by PAD_WORDS readable words), break bits of positions 16 w0 .. 16 w0 + 95
            const uint4 q = *reinterpret_cast<const uint4 *>(w + w0);
            const uint32_t c[6] = {q.x, q.y, q.z, q.w, w[w0 + 4], KMODE == KM_GT16 ? w[w0 + 5] : 0u};
            const uint32_t bi = (uint32_t)(w0 >> 1);
            const uint32_t b0 = multi_rec ? bk[bi] : 0u, b1 = multi_rec ? bk[bi + 1] : 0u, b2 = multi_rec ? bk[bi + 2] : 0u;
            const uint64_t kv = kmer_valid_mask(b0, b1, b2, (uint32_t)(w0 * 16), (uint32_t)nk, k);
            uint64_t keep = 0;
#pragma unroll
            for (int wi = 0; wi < SKETCH_WORDS_PER_THREAD; ++wi) {
                const uint32_t c0 = c[wi], c1 = c[wi + 1], c2 = c[wi + 2];
                const uint32_t r0 = rcword(c0, cm), r1 = rcword(c1, cm), r2 = (KMODE == KM_GT16) ? rcword(c2, cm) : 0u;
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {
                    if (!((kv >> (wi * 16 + r)) & 1ull)) continue;
                    uint32_t can_lo, can_hi = 0;
                    canon_kmer<KMODE, 0>(r, c0, c1, c2, r0, r1, r2, kp, can_lo, can_hi);
                    const uint64_t key = ((uint64_t)can_hi << 32) | can_lo;
                    const uint64_t i1 = (key * KMER_FILTER_MUL1) >> sh, i2 = ((key ^ (key >> 32)) * KMER_FILTER_MUL2) >> sh;
                    if constexpr (KEEP_PASS) {
                        const uint8_t *cb = reinterpret_cast<const uint8_t *>(cells);
                        const uint32_t n1 = cb[i1], n2 = cb[i2];
                        if ((n1 < n2 ? n1 : n2) >= a.min_count) keep |= 1ull << (wi * 16 + r);
                    } else {
                        for (int j = 0; j < 2; ++j) {
                            const uint64_t i = j ? i2 : i1;
                            if (j && i2 == i1) break;                         // both addresses in one cell: counted once
                            uint32_t *wp = cells + (i >> 2);
                            const uint32_t s = ((uint32_t)i & 3u) * 8u;
                            uint32_t seen = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            while (((seen >> s) & 255u) != 255u) {            // saturated: nothing to add, no atomic
                                const uint32_t was = atomicCAS(wp, seen, seen + (1u << s));
                                if (was == seen) break;
                                seen = was;
                            }
                        }
                    }
                }
            }
            if constexpr (KEEP_PASS) {
                uint32_t *kb = a.keep + gd.brk_off + bi;
                kb[0] = (uint32_t)keep;
                kb[1] = (uint32_t)(keep >> 32);
            }
        }
    }
}

template <int KMODE>
__global__ void __launch_bounds__(256) kmer_count_kernel(KmerFilterArgs a) { kmer_filter_walk<KMODE, false>(a); }
template <int KMODE>
__global__ void __launch_bounds__(256) kmer_keep_kernel(KmerFilterArgs a) { kmer_filter_walk<KMODE, true>(a); }

template <bool KEEP_PASS>
static hipError_t launch_filter(const KmerFilterArgs &args, uint64_t max_bytes, hipStream_t stream)
{
    if (args.n_genomes == 0 || max_bytes == 0) return hipSuccess;
    const uint64_t per_block = 256ull * SKETCH_WORDS_PER_THREAD * 16;       // bases one workgroup takes per trip
    const uint32_t gx = (uint32_t)std::min<uint64_t>(2048, (max_bytes + per_block - 1) / per_block);
    const dim3 grid(gx, std::min(args.n_genomes, 65535u));
    void (*kern)(KmerFilterArgs);
    if constexpr (KEEP_PASS) kern = args.k == 16 ? kmer_keep_kernel<KM_16> : args.k < 16 ? kmer_keep_kernel<KM_LT16> : kmer_keep_kernel<KM_GT16>;
    else kern = args.k == 16 ? kmer_count_kernel<KM_16> : args.k < 16 ? kmer_count_kernel<KM_LT16> : kmer_count_kernel<KM_GT16>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_kmer_count(const KmerFilterArgs &args, uint64_t max_bytes, hipStream_t stream) { return launch_filter<false>(args, max_bytes, stream); }
hipError_t launch_kmer_keep(const KmerFilterArgs &args, uint64_t max_bytes, hipStream_t stream) { return launch_filter<true>(args, max_bytes, stream); }

}  // namespace lash
