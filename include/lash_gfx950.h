/*
 * lash_gfx950.h — C ABI of liblash_gfx950.so: the MI355X (gfx950) drop-in for lash's sketching hot path.
 *
 * What it replaces.  In the reference the per-k-mer plug-in boundary is
 *     trait KmerSketch { fn new(Option<u32>); fn add_kmer(&mut self, masked: u64, seed: u64); fn save(&self, w) }
 * (/root/reference/src/utils.rs:377-386) with a single caller, the per-file closure of `sketch_files`
 * (utils.rs:452-508).  A per-k-mer FFI call is meaningless for a GPU, so the boundary is that closure widened
 * to a batch:  records of many files in  ->  the byte images `S::save` would have written out
 * (utils.rs:400-402, 415-417, 431-433), in file order (utils.rs:509, 571-573).  A Rust host `write_all`s the
 * images into its zstd encoder unchanged; INTEGRATION.md shows the `extern "C"` block.
 *
 * Rules of the ABI: plain pointers and sizes only; the caller allocates and frees every buffer; the library owns
 * only what hangs off a lash_ctx / lash_packed; no exceptions or aborts cross the boundary (0 = OK, <0 = error);
 * a lash_ctx is used by one host thread at a time; there is NO CPU fallback — without a HIP device every compute
 * entry returns LASH_ENODEV.
 */
#ifndef LASH_GFX950_H
#define LASH_GFX950_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASH_ABI_VERSION 5

/* error codes */
#define LASH_OK       0
#define LASH_EINVAL  (-1)   /* bad algo / k / p / arguments: mirrors the panics at utils.rs:500-502, main.rs:245 and
                               the expect()s at utils.rs:408,423 */
#define LASH_ENODEV  (-2)   /* no usable HIP device */
#define LASH_EHIP    (-3)   /* HIP runtime error; text via lash_ctx_last_error() */
#define LASH_ENOMEM  (-4)
#define LASH_ERANGE  (-6)   /* HyperLogLog estimate <= 5 * 2^p: streaming_algorithms subtracts a bias read from the HLL++
                               empirical tables there; the tables are not in this build, so the case is refused */
#define LASH_EFORMAT (-7)   /* lash_sketch_files_raw_device: a FASTQ file's line structure broke; see lash_ctx_format_errors() */
#define LASH_ELIMIT  (-5)   /* a genome has more than 2^32-64 bases in one call (split it and merge images) */

/* -a {hmh,hll,ull}  (main.rs:69-76, 210-246) */
#define LASH_HMH 0
#define LASH_HLL 1
#define LASH_ULL 2

/* flags */
#define LASH_F_HMH_X_LOW   1u  /* SURVEY App. D switch U1: take x (bucket, lz) from the LOW 64 bits of xxh3_128
                                  (per call; OR-ed with the context layout's hmh_x_low) */
#define LASH_F_ACCUMULATE  2u  /* out_images already hold sketches of the same algo/p: union the new ones in */
#define LASH_F_AMINO       8u  /* the amino-acid branch of sketch_files (utils.rs:511-563; `aa`, which main.rs:198 hard-wires to false and
                                  whose --aa flag is commented out at main.rs:97-104): records are upper-cased, records whose RAW
                                  length is below k skipped, every byte outside the 20 residue letters deleted (filter_out_a,
                                  utils.rs:43-55), 5-bit codes, k 1..=12 (utils.rs:554 panics above), no reverse complement,
                                  mask_aa_bits (utils.rs:66-76), add_kmer as for nucleotides.  lash_sketch_batch[_async/_device] and
                                  lash_sketch_files_raw (host parse); the packed / raw-device entries return LASH_EINVAL */
#define LASH_F_NO_DIRECT   4u  /* lash_sketch_batch[_device]: pack first (ASCII -> 2-bit stream in HBM -> sketch), the route raw
                                  FASTA / FASTQ bytes always take.  By default the sketch kernels read the record bytes
                                  themselves and apply filter_out_n (utils.rs:33-41) on the fly: clean stretches as they are,
                                  deleted bytes by junction walks / in-LDS compaction, soft-masked genomes by a compacting
                                  kernel.  Same images either way; the flag exists for A/B runs */

#define LASH_F_STREAM_ONLY 16u /* lash_sketch_batch[_device]: skip the optimistic pass, every genome goes through the compacting
                                  kernel (stream_sketch_kernel) — what the context does by itself while batches keep turning out
                                  soft-masked.  Same images; for A/B runs and tests */

#define LASH_F_NO_SOLE     32u /* (ABI v5) every sketch entry: do not use the persistent small-genome kernel (sole_kernels.hip), which by
                                  default takes the genomes of a call that are at most LASH_SOLE_MAX bytes long (environment,
                                  default 393216; 0 = never) when the sketch's table fits 64 KiB of LDS — a resident workgroup streams
                                  whole genomes through an LDS ring instead of one workgroup per genome.  Same images; for A/B
                                  runs and tests */

typedef struct lash_ctx lash_ctx;        /* one per (host thread, GPU): stream, workspace, scratch */
typedef struct lash_packed lash_packed;  /* device-resident 2-bit genomes produced by lash_pack_* */

typedef struct {
    int32_t  algo;    /* LASH_HMH / LASH_HLL / LASH_ULL                                        */
    int32_t  k;       /* 1..=32 (utils.rs:466-502)                                             */
    int32_t  p;       /* HLL 4..=16, ULL 3..=26, ignored for HMH (main.rs:212-213)             */
    uint32_t flags;   /* LASH_F_*                                                              */
    uint64_t seed;    /* -s (main.rs:88-95); handed to xxh3 exactly as utils.rs:397,412,428 do  */
} lash_params;

/* ---- layout: the crate-internal rules of the reference's dependencies, as data ----------------------------------------
 * lash's k-mer values, register rules and `save` bytes are fixed inside kmerutils 0.0.14, hyperminhash 0.1.4,
 * streaming_algorithms 0.3.3 and ultraloglog 0.1.6 (Cargo.lock:917,713,1834,2012; called at utils.rs:397,412,428,464-499
 * and 401,416,432).  Those crates are not in the reference tree, so each rule that could not be verified here (SURVEY App. D,
 * U1-U5) is ONE field of this struct; the default is the hypothesis of SURVEY App. A.  tools/ref_probe/ produces images with
 * the real `lash` and fits this struct to them; a mismatch is then a field change, not a code change.
 * Header templates are strings of field codes written before the register array, all little-endian (bincode fixint):
 *   'a' alpha f64 | 'z' zero u64 | 'Z' zero u32 | 's' sum f64 | 'p' p u8 | 'P' p u32 | 'Q' p u64 |
 *   'l' register count u64 | 'L' register count u32 */
typedef struct {
    uint8_t base_code[4];     /* U5  2-bit codes of 'A','C','G','T' (a permutation of 0..3)                 {0,1,2,3} */
    uint8_t kmer_lsb_first;   /* U5  0: a k-mer's first base is its MOST significant 2 bits; 1: least                0 */
    uint8_t hmh_x_low;        /* U1  0: x (bucket, lz) = high 64 bits of xxh3_128, y = low; 1: swapped               0 */
    uint8_t hmh_reg_be;       /* U2  HyperMinHash registers saved as u16 little- (0) or big-endian (1)               0 */
    uint8_t hll_bucket_high;  /* U3  0: HLL bucket = low p bits of the hash, rho from the rest; 1: top p bits        0 */
    char    hmh_header[8];    /* U2  ""       */
    char    hll_header[8];    /* U3  "azspl"  */
    char    ull_header[8];    /* U4  "l"      */
    uint8_t fastq_skip_bad;   /* U6  what lash's record loop sees after a MALFORMED FASTQ record.  The loop is
                                     `while let Some(res) = reader.next() { if let Ok(rec) = res {..} }` (utils.rs:457-458): it
                                     keeps calling next() after an Err.  0: needletail's iterator is finished by the error — the
                                     records before it stand, nothing after it is seen.  1: the iterator goes on — the malformed
                                     record is dropped, reading resumes at the next line that starts with '@' and whose line
                                     after next starts with '+'.  tools/ref_probe carries two such files                  0 */
    uint8_t aa_code_zero_based; /* U7 amino-acid sketches (LASH_F_AMINO): kmerutils' 5-bit residue codes over "ACDEFGHIKLMNPQRSTVWY" in
                                     that order — 0: A = 1 ... Y = 20, 1: A = 0 ... Y = 19                                  0 */
    uint8_t reserved[6];      /*     zero */
} lash_layout;                /* 40 bytes */

/* Sums over every sketch call since lash_ctx_enable_timing(ctx, 1) (HIP events on the ctx stream). */
typedef struct {
    float    pack_ms;           /* ASCII -> 2-bit + record-break bitmap (incl. the small table uploads); calls
                                   that took the direct route spend nothing here: their dirty-genome pack is
                                   queued behind the direct pass and counted in sketch_ms */
    float    sketch_ms;         /* k-mer / xxh3 / register-update kernels (direct pass + the compacting kernel for handed-over genomes) */
    float    finalize_ms;       /* partial-sketch reduction + byte images                                  */
    uint32_t calls;             /* sketch calls summed                                                     */
    uint32_t sketch_launches;   /* launches of the sketch kernel summed                                    */
    uint32_t sketch_workgroups; /* workgroups of the last sketch launch                                    */
    uint32_t direct_launches;   /* launches of the direct (ASCII-reading) sketch kernel summed              */
    uint64_t kmers;             /* valid k-mers hashed, device-counted, summed                             */
    uint64_t bases_last;        /* bases that survived filter_out_n in the last call                       */
    uint64_t packed_bytes;      /* 2-bit words + break bitmap read by the sketch kernel, summed            */
    float    direct_ms;         /* the part of sketch_ms spent in the direct (ASCII-reading) sketch kernel */
    uint32_t defer_launches;    /* of sketch_launches: HyperMinHash with deferred signatures (batches of long work items)  */
    uint32_t sole_launches;     /* (ABI v5) launches of the persistent small-genome kernel summed (sole_kernels.hip)         */
} lash_timing;

/* ---- library / context ---------------------------------------------------------------------------------- */
int         lash_abi_version(void);
int         lash_device_count(void);                       /* 0 when no GPU is visible */
const char *lash_strerror(int code);
int         lash_ctx_create(lash_ctx **out, int device);   /* device >= 0 */
void        lash_ctx_destroy(lash_ctx *ctx);
int         lash_ctx_set_stream(lash_ctx *ctx, void *hip_stream);   /* run on the caller's hipStream_t (NULL = own) */
int         lash_ctx_synchronize(lash_ctx *ctx);
const char *lash_ctx_last_error(lash_ctx *ctx);
int         lash_ctx_enable_timing(lash_ctx *ctx, int on); /* (re)starts the sums; HIP events around each stage */
int         lash_ctx_get_timing(lash_ctx *ctx, lash_timing *out);   /* synchronizes the stream */

/* Page-locked host memory for the buffers handed to lash_sketch_batch (optional: pageable memory works, pinned memory
 * lets the H2D copy run at PCIe speed).  Free with lash_host_free_pinned. */
void       *lash_host_alloc_pinned(size_t bytes);
void        lash_host_free_pinned(void *p);

/* ---- parameters / sizes (host only, no GPU needed) -------------------------------------------------------- */
int         lash_params_check(const lash_params *prm);     /* LASH_OK or LASH_EINVAL */
size_t      lash_sketch_image_bytes(int algo, int p);      /* bytes S::save writes per sketch (default layout); 0 if invalid */

/* ---- layout (host only) ------------------------------------------------------------------------------------------ */
void        lash_layout_default(lash_layout *out);
int         lash_layout_check(const lash_layout *lay);     /* LASH_OK or LASH_EINVAL */
/* "key=value,..." on top of the default: codes=ACGT (the four letters in code order) kmer=msb|lsb hmh_x=high|low
 * hmh_reg=le|be hll_bucket=low|high hmh_hdr= hll_hdr=azspl ull_hdr=l fastq_err=stop|skip aa_codes=one|zero.  NULL / "" = the default. */
int         lash_layout_parse(const char *spec, lash_layout *out);
size_t      lash_layout_header_bytes(const lash_layout *lay, int algo);
size_t      lash_layout_image_bytes(const lash_layout *lay, int algo, int p);   /* lay NULL = default; 0 if invalid */
/* Every entry below that reads or writes images through `ctx` uses the context's layout (default until set). */
int         lash_ctx_set_layout(lash_ctx *ctx, const lash_layout *lay);         /* NULL = back to the default */
int         lash_ctx_get_layout(lash_ctx *ctx, lash_layout *out);

/* ---- the hot path --------------------------------------------------------------------------------------- */
/* Replaces the body of files.par_iter().map(...) (utils.rs:450-509) for a batch of files ("genomes").
 *   seq            concatenated record sequences exactly as needletail's seqrec.seq() yields them (utils.rs:459):
 *                  no headers, no line ends; any byte other than upper-case A C G T is deleted (utils.rs:33-41)
 *   rec_off        n_rec+1 byte offsets into seq (record r = [rec_off[r], rec_off[r+1]))
 *   genome_rec_off n_genomes+1 record indices (genome g owns records [genome_rec_off[g], genome_rec_off[g+1]))
 *   out_images     n_genomes * lash_sketch_image_bytes() bytes, genome order
 * Host-resident buffers; copies in, runs, copies out, synchronizes. */
int lash_sketch_batch(lash_ctx *ctx, const lash_params *prm,
                      const uint8_t *seq, const uint64_t *rec_off, uint64_t n_rec,
                      const uint64_t *genome_rec_off, uint32_t n_genomes, uint8_t *out_images);

/* The same, without the wait: queues copy-in, kernels and copy-out and returns.  Two staging slots and separate copy streams
 * inside the context let the H2D copy of the NEXT call and the D2H copy of the PREVIOUS one overlap this call's kernels, so
 * a host that streams batches runs at the PCIe rate.  seq / rec_off / out_images must stay valid and
 * untouched until lash_ctx_synchronize(ctx) (or until two further _async calls have been made); give them page-locked memory
 * (lash_host_alloc_pinned) — copies from pageable memory are staged by the runtime and do not overlap.  genome_rec_off is
 * consumed before the call returns. */
int lash_sketch_batch_async(lash_ctx *ctx, const lash_params *prm,
                            const uint8_t *seq, const uint64_t *rec_off, uint64_t n_rec,
                            const uint64_t *genome_rec_off, uint32_t n_genomes, uint8_t *out_images);

/* Same with seq / rec_off / out_images already in device memory (asynchronous on the ctx stream).
 * The two small per-genome tables stay on the host: genome_byte_off[g] == rec_off[genome_rec_off[g]]. */
int lash_sketch_batch_device(lash_ctx *ctx, const lash_params *prm,
                             const uint8_t *d_seq, const uint64_t *d_rec_off, uint64_t n_rec,
                             const uint64_t *genome_rec_off, const uint64_t *genome_byte_off,
                             uint32_t n_genomes, uint8_t *d_out_images);

/* File bytes in: the FASTA / FASTQ parse itself runs on the device, so the host only reads (or
 * inflates) files into one buffer.  file_fmt[g] is LASH_FMT_FASTA ('>' files) or LASH_FMT_FASTQ ('@' files, 4-line
 * records); file g is bytes [file_off[g], file_off[g+1]) of raw, uncompressed.  Semantics are needletail's
 * (utils.rs:453-459) followed by the same path as lash_sketch_batch: one sketch per file. */
#define LASH_FMT_FASTA 1
#define LASH_FMT_FASTQ 2
int lash_sketch_files_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off,
                          const uint8_t *file_fmt, uint32_t n_files, uint8_t *out_images);
int lash_sketch_files_raw_device(lash_ctx *ctx, const lash_params *prm, const uint8_t *d_raw, const uint64_t *file_off,
                                 const uint8_t *file_fmt, uint32_t n_files, uint8_t *d_out_images);
/* Malformed FASTQ.  needletail's iterator ends with an error at a record that is not header / sequence / '+' / quality and
 * lash keeps the records before it (`while let Some(Ok(..))`, utils.rs:457).  The device parse counts lines modulo 4 and
 * cannot stop mid-file, but it CHECKS needletail's rules in full: a line in phase 0 must start with '@', one in phase 2 with
 * '+' (pack_kernels.hip); a quality line must be as long as its sequence line, CR stripped, and the file must end on a whole
 * record (fastq_check.hip, round 3 — a second scan over newline positions).  Files that fail:
 *   lash_sketch_files_raw         (bytes on the host) re-does each such file through a host parse that stops at the first
 *                                 malformed record (or drops it: layout.fastq_skip_bad) and lash_sketch_batch — exact reference
 *                                 semantics, returns LASH_OK;
 *   lash_sketch_files_raw_device  (bytes only in HBM) leaves their images unreliable; the next lash_ctx_synchronize() returns
 *                                 LASH_EFORMAT.  The flagged set equals the set of files lash_fastq_valid_prefix(buf, n) < n
 *                                 (tests/test_gpu_rawfiles.py holds them side by side).
 * Either way the indices of those files (of the last raw call) are available here: returns how many, copies up to `cap`.
 * The first byte of a file must be '>' or '@' (parse_fastx_file fails otherwise, utils.rs:453): LASH_EINVAL from both. */
uint32_t lash_ctx_format_errors(lash_ctx *ctx, uint32_t *file_index, uint32_t cap);

/* One sketch per FASTA RECORD (`lash sketch --per-record`; Mash's -i): viral / plasmid databases, metagenome assemblies and contig sets come as
 * one multi-FASTA with 10^4 - 10^6 records.  lash_fasta_index finds the records of a batch of raw, uncompressed FASTA files on the device
 * (fasta_index.hip), in file order then byte order:
 *   start[r]   byte offset of record r's '>' in the buffer, r in [0, n_records]; the extra entry is file_off[n_files], so record r is
 *              bytes [start[r], start[r + 1]) (a file's last record ends where the next file begins)
 *   id_len[r]  length of the record id: the header bytes after '>' up to the first space, TAB, CR, LF or the end of the file (may be 0)
 *   file[r]    index of the file the record belongs to
 * Rules (needletail's): a record starts at a file's first byte and at every '>' whose preceding byte in the same file is '\n'; a '>'
 * anywhere else starts nothing; every record counts whatever its sequence.  An empty file holds no record.  file_off[0] must be 0.  A
 * file whose first byte is not '>' (every FASTQ file): LASH_EINVAL.  _device: the bytes are in device memory, file_off stays on the
 * host; both entries synchronize the context's stream once (the number of records sizes the result).  Each accessor is one copy to
 * the host.  Free with lash_rec_index_free.  An index made by lash_fasta_index keeps its device copy of the bytes until it is freed.
 * lash_sketch_records_raw sketches records [r0, r1) of an index made from the same raw / file_off: one image per record, exactly what
 * lash_sketch_files_raw gives for the same records written one per file — it IS that call, with start[r0 .. r1] as its file offsets, so
 * the HyperLogLog `sum` replay and lash_ctx_format_errors / lash_ctx_hll_inexact_sums work as there, with record indices relative to
 * r0 where that entry has file indices.  A caller bounds the bytes of images in flight by the width of [r0, r1).  With an index made by
 * lash_fasta_index from this same `raw` pointer (unchanged since) the bytes are not copied to the device again.  LASH_F_AMINO:
 * LASH_EINVAL. */
typedef struct lash_rec_index lash_rec_index;
int      lash_fasta_index(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, lash_rec_index **out);
int      lash_fasta_index_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, lash_rec_index **out);
uint64_t lash_rec_index_n_records(const lash_rec_index *index);
int      lash_rec_index_start(lash_ctx *ctx, const lash_rec_index *index, uint64_t *out);    /* n_records + 1 */
int      lash_rec_index_id_len(lash_ctx *ctx, const lash_rec_index *index, uint32_t *out);   /* n_records */
int      lash_rec_index_file(lash_ctx *ctx, const lash_rec_index *index, uint32_t *out);     /* n_records */
void     lash_rec_index_free(lash_ctx *ctx, lash_rec_index *index);
int      lash_sketch_records_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files,
                                 const lash_rec_index *index, uint64_t r0, uint64_t r1, uint8_t *out_images);

/* One sketch per fixed-length WINDOW of every FASTA record (`lash sketch --window W`): which stretch of a chromosome is the prophage, which
 * part of a contig is the contaminant.  lash_fasta_windows cuts the records of an index (made from the same raw / file_off on the same
 * context) into windows on the device (fasta_coords.hip, fasta_windows.hip):
 *   sequence bytes  of a record: the bytes after its header line's '\n' up to start[r + 1] that are neither '\n' nor '\r'; every other
 *                   byte counts (N, lower case, a stray '>').  Their 0-based rank in the record is the coordinate.
 *   windows         a record of L sequence bytes has ceil(L / window) of them, window j = coordinates [j * window, min(L, (j + 1) * window));
 *                   L = 0 gives none; the last, shorter one is kept.  No window spans two records.  Order: record order, then j.
 *   record[w]       the record (of the index) window w lies in;  begin[w]  its first coordinate;  length[w]  its bases, 1 .. window
 * Every window is written as a one-record FASTA file (">\n", its bytes, "\n") into one device buffer the window index owns until it is
 * freed: lash_win_index_bytes bytes at lash_win_index_buffer_device, window w at offset[w] (n_windows + 1 entries), ready for
 * lash_sketch_files_raw_device.  lash_sketch_windows_raw sketches windows [w0, w1) of it: one image per window, exactly what
 * lash_sketch_files_raw gives for those files; the HyperLogLog `sum` replay and lash_ctx_format_errors / lash_ctx_hll_inexact_sums work as
 * there, with indices relative to w0.  With an index made by lash_fasta_index from this same `raw` pointer the bytes are not sent again;
 * _device: the bytes are in device memory.  Both synchronize the context's stream once (the totals size the result).  window = 0, an
 * index of another context or buffer, w0 > w1, w1 > n_windows, LASH_F_AMINO: LASH_EINVAL; no room for the buffer: LASH_ENOMEM; 2^32
 * windows or more: LASH_ELIMIT. */
typedef struct lash_win_index lash_win_index;
int      lash_fasta_windows(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *index,
                            uint64_t window, lash_win_index **out);
int      lash_fasta_windows_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *index,
                                   uint64_t window, lash_win_index **out);
uint64_t lash_win_index_n_windows(const lash_win_index *windows);
uint64_t lash_win_index_bytes(const lash_win_index *windows);
const uint8_t *lash_win_index_buffer_device(const lash_win_index *windows);
int      lash_win_index_record(lash_ctx *ctx, const lash_win_index *windows, uint64_t *out);  /* n_windows */
int      lash_win_index_begin(lash_ctx *ctx, const lash_win_index *windows, uint64_t *out);   /* n_windows */
int      lash_win_index_length(lash_ctx *ctx, const lash_win_index *windows, uint64_t *out);  /* n_windows */
int      lash_win_index_offset(lash_ctx *ctx, const lash_win_index *windows, uint64_t *out);  /* n_windows + 1 */
int      lash_sketch_windows_raw(lash_ctx *ctx, const lash_params *prm, const lash_win_index *windows, uint64_t w0, uint64_t w1,
                                 uint8_t *out_images);
void     lash_win_index_free(lash_ctx *ctx, lash_win_index *windows);

/* Six-frame PROTEIN sketches of nucleotide FASTA (`lash sketch --translate`): genomes too far apart for nucleotide k-mers are compared in protein
 * space, and a user with assemblies has no proteins.  lash_fasta_translate translates the records of an index (made from the same raw / file_off
 * on the same context) on the device (fasta_coords.hip, fasta_translate.hip) into one buffer the result owns until it is freed.  The rule does not depend on k:
 *   sequence bytes  S[0..L) of a record: as for lash_fasta_windows (the bytes after the header line's LF that are neither LF nor CR)
 *   bases           ACGTacgt, case ignored (soft-masked sequence translates like any other); every other byte, N and U included, is no base
 *   frames          f = 0, 1, 2 read S from offset f; f = 3, 4, 5 read the reverse complement R[t] = comp(S[L - 1 - t]) from offset f - 3;
 *                   frame f has n_f = max(0, floor((L - offset) / 3)) codons, a trailing partial codon is dropped
 *   codons          three bases: the standard genetic code (NCBI table 1; table 11 maps codons alike), a stop gives '*'; a codon with a
 *                   no-base gives 'X'.  '*' and 'X' are BREAK BYTES
 *   buffer          records in index order, frames 0..5 in order, each frame its n_f bytes and one '*': record r takes 6 + 2 * max(0, L_r - 2) bytes
 *   segments        a segment ends after every break byte: segment s = bytes [seg_off[s], seg_off[s + 1]), seg_off[0] = 0, as many segments
 *                   as break bytes, a segment may be one byte long; rec_seg[r] (n_records + 1 entries) = the first segment of record r
 * lash_sketch_translated sketches groups of records: group g = records [group_rec_off[g], group_rec_off[g + 1]) of the index (ascending,
 * within [0, n_records]; they need not start at 0 or cover everything), one image per group: the LASH_F_AMINO sketch whose records are the
 * group's segments.  It is lash_sketch_batch_device with LASH_F_AMINO OR-ed into prm->flags on (buffer, seg_off, the groups' segment and byte
 * offsets), the images copied to the host, the stream synchronized; LASH_F_ACCUMULATE, LASH_F_HMH_X_LOW and the context's layout (aa_codes
 * included) apply.  A segment's trailing break byte counts toward its raw length and is deleted by the amino-acid filter, so no k-mer spans a
 * stop, an ambiguous codon, two frames or two records, and a segment of fewer than k residues yields none.  A sketch made this way and a
 * LASH_F_AMINO sketch of a proteome hold the same kind of k-mers.
 * With an index made by lash_fasta_index from this same `raw` pointer the bytes are not sent again; _device: the bytes are in device memory.
 * Both synchronize the context's stream (the totals size the result).  Device memory: the buffer is about twice the sequence bytes and seg_off
 * about 0.75 bytes per base of random DNA: budget 5 x the raw bytes with the input and the scratch.  LASH_EINVAL: an index or a translation
 * of another context or buffer, group offsets descending or beyond n_records, k outside 1..12; LASH_ENOMEM: no room; LASH_ELIMIT: 2^32
 * segments or more in one group. */
typedef struct lash_tr_index lash_tr_index;
int      lash_fasta_translate(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *index,
                              lash_tr_index **out);
int      lash_fasta_translate_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *index,
                                     lash_tr_index **out);
uint64_t lash_tr_index_n_segments(const lash_tr_index *translated);
uint64_t lash_tr_index_bytes(const lash_tr_index *translated);
const uint8_t *lash_tr_index_buffer_device(const lash_tr_index *translated);
int      lash_tr_index_seg_off(lash_ctx *ctx, const lash_tr_index *translated, uint64_t *out);   /* n_segments + 1 */
int      lash_tr_index_rec_seg(lash_ctx *ctx, const lash_tr_index *translated, uint64_t *out);   /* n_records + 1 */
int      lash_sketch_translated(lash_ctx *ctx, const lash_params *prm, const lash_tr_index *translated, const uint64_t *group_rec_off,
                                uint32_t n_groups, uint8_t *out_images);
void     lash_tr_index_free(lash_ctx *ctx, lash_tr_index *translated);

/* K-mer abundance filter (`lash sketch --min-count M`; Mash -m, not upstream): a k-mer a file holds fewer than M times stays out of its
 * sketch.  A sequencing error makes up to k k-mers that exist nowhere else, and in a read set they can outnumber the real ones.
 *   key      the masked canonical k-mer value the reference hands to add_kmer (utils.rs:464-499), as a u64 for all three sketch types
 *            (HyperMinHash: before its truncation to 32 bits); both strands are one key; counted per file over all its records
 *   table    each file has 2^L saturating byte counters (L = log2_cells[file], 10..36), zero at creation.  Every valid k-mer occurrence
 *            increments cells  i1 = (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - L)  and
 *            i2 = ((key ^ (key >> 32)) * 0xC2B2AE3D27D4EB4F mod 2^64) >> (64 - L)  — one cell once when i1 == i2 — up to 255, exactly
 *   keep     after the whole file has been counted an occurrence is kept iff min(cell[i1], cell[i2]) >= min_count; kept occurrences go
 *            through add_kmer as ever, dropped ones are not hashed into the sketch
 * Two passes, count everything and then test: the result depends on neither thread order nor batching.  Every k-mer with a true count
 * >= M is in the sketch; one with a smaller count gets in only through collisions in BOTH of its cells.  min_count = 1 keeps everything:
 * the images are byte for byte those of lash_sketch_files_raw.
 *   create       one L per file; LASH_EINVAL outside 10..36, LASH_ENOMEM when the tables do not fit the device
 *   count_raw    adds the k-mers of raw / file_off / file_fmt (as lash_sketch_files_raw takes them) to the tables.  May be called once per
 *                chunk of files streamed in pieces cut between records: no k-mer spans records, so the cells equal one call's.  Only
 *                prm->k and the context's layout fix the key: one filter serves every algo, p and seed
 *   counts       the 2^L cells of one file, one byte each
 *   sketch_files_raw_filtered   lash_sketch_files_raw with the keep rule; min_count 1..255; honours LASH_F_ACCUMULATE (chunks of a file
 *                counted whole beforehand give the image of one call).  Always the pack-first route on the sliced kernel.  Supported where
 *                the sketch's registers are a plain table in LDS: hmh, hll p <= 15, ull p <= 14
 * LASH_EINVAL: LASH_F_AMINO, n_files different from the filter's, a filter of another device, min_count outside 1..255, a precision
 * without a filtered launch (lash_ctx_last_error names the limits).  Malformed FASTQ as in lash_sketch_files_raw on both calls: the records
 * needletail's iterator yields are counted and sketched, the file is listed by lash_ctx_format_errors.  HyperLogLog files that end with a
 * register above 53 - p are NOT replayed (the replay would have to run on the filtered stream): their `sum` is the correctly rounded sum
 * over the final registers and they stay reported by lash_ctx_hll_inexact_sums.  All four calls synchronize the context's stream. */
typedef struct lash_kmer_filter lash_kmer_filter;
int  lash_kmer_filter_create(lash_ctx *ctx, uint32_t n_files, const uint8_t *log2_cells, lash_kmer_filter **out);
int  lash_kmer_filter_count_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off,
                                const uint8_t *file_fmt, uint32_t n_files, lash_kmer_filter *f);
int  lash_kmer_filter_counts(lash_ctx *ctx, const lash_kmer_filter *f, uint32_t file, uint8_t *out);
int  lash_sketch_files_raw_filtered(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off,
                                    const uint8_t *file_fmt, uint32_t n_files, const lash_kmer_filter *f,
                                    uint32_t min_count, uint8_t *out_images);
void lash_kmer_filter_free(lash_ctx *ctx, lash_kmer_filter *f);

/* HyperLogLog images carry `sum` = sum_j 2^-m[j] (f64).  streaming_algorithms keeps it incrementally per k-mer (sum -= 2^-old;
 * sum += 2^-new); that is exactly the sum over the final registers as long as every register is <= 53 - p, and the HIP path
 * writes that sum.  A register above 53 - p (one k-mer in 2^(52-p): p = 14 -> 1 in 2.7e11) makes the incremental value depend
 * on the order of its f64 roundings — it can differ from the correctly rounded sum written here by the terms below the
 * 2^(p-53) grid (< 2^(p-52) absolute, ~1e-14 relative: the low bits of those 8 header bytes); registers, `zero` and every
 * other byte are unaffected.  This call synchronizes the context's stream and lists
 * the genomes of the LAST HyperLogLog sketch call that are in that corner (indices into that call's genomes; returns how many,
 * writes at most `cap`).  tests/test_gpu_hll_corner.py holds k-mers that reach it. */
uint32_t lash_ctx_hll_inexact_sums(lash_ctx *ctx, uint32_t *genome_index, uint32_t cap);
/* Round 4: the corner is closed for per-genome sketches.  For a flagged genome the library finds the k-mer(s) that put a register
 * above 53 - p by a binary search over PREFIXES of the genome's records (each probe an ordinary sketch call), takes the incremental
 * sum up to there from the prefix's own (exact) header, performs that k-mer's `sum -= 2^-old; sum += 2^-new` in IEEE double as
 * the crate does, and adds the exact net change of the steps that follow: the 8 bytes then equal the oracle's
 * (tests/test_gpu_hll_corner.py asserts byte equality).  lash_sketch_batch and lash_sketch_files_raw do this themselves before they
 * return (lash_ctx_hll_inexact_sums() then reports nothing); after lash_sketch_batch_device / _async call this with the same
 * arguments once the caller may wait: it synchronizes, patches `sum` in d_images and clears the report.  What stays flagged:
 * calls with LASH_F_ACCUMULATE (the registers already in the image are not the library's to replay — the CLI's streamed chunks
 * of one huge file) and the raw-bytes device entry.  ~25 small sketch calls per flagged genome, i.e. nothing on average. */
int lash_hll_replay_sums_device(lash_ctx *ctx, const lash_params *prm, const uint8_t *d_seq, const uint64_t *d_rec_off, uint64_t n_rec,
                                const uint64_t *genome_rec_off, uint32_t n_genomes, uint8_t *d_images);
/* (ABI v5) The same for ONE FILE STREAMED IN CHUNKS with LASH_F_ACCUMULATE (the CLI's --stream-mb; utils.rs:457-505 reads the file's records
 * in order into one sketch, so the reference's `sum` is the incremental value over the whole file).  Call after each chunk's
 * lash_sketch_files_raw: raw / n_bytes / fmt = the chunk as it was handed over, image_before = the file's image before that call,
 * image_after = after it (host memory, patched in place), carry[2] + *have_carry = state the caller keeps per file (zero-initialised).
 * While no register is above 53 - p nothing happens.  A chunk that lifts one there is replayed — prefix sketches of the chunk united with
 * image_before's registers locate the k-mers, their updates are done in IEEE double as the crate does — and from then on every later
 * chunk's exact net change is added to the carried value: image_after's `sum` equals the reference's after every chunk
 * (tests/test_gpu_hll_corner.py asserts byte equality for --stream-mb 1). */
int lash_hll_replay_streamed_chunk(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, uint64_t n_bytes, int fmt,
                                   const uint8_t *image_before, uint8_t *image_after, double *carry, int *have_carry);
/* Host-side twin of the device checks (what the library itself runs on a flagged file; the `lash` CLI no longer pre-validates —
 * it hands the bytes over and reads lash_ctx_format_errors): the length of the longest prefix of `buf` that is a sequence of
 * well-formed records — '@' header, sequence, '+' line, quality of EQUAL length (CR stripped); the last record may lack its
 * final newline.  == n for a well-formed file, 0 if the first byte is not '@'.  What follows the prefix is what needletail's
 * iterator never yields; lash_fastq_neutralise_tail overwrites such a tail (inside a batch buffer whose file offsets must stay
 * contiguous) with a well-formed stand-in that contributes no base.  Host only. */
uint64_t lash_fastq_valid_prefix(const uint8_t *buf, uint64_t n);
void     lash_fastq_neutralise_tail(uint8_t *tail, uint64_t n);
/* Both in one, for either setting of layout.fastq_skip_bad: overwrites, in place, every byte needletail's iterator would not
 * turn into a record — skip_bad 0: what follows the first malformed record (lash_fastq_neutralise_tail); skip_bad 1: each
 * malformed stretch up to the next plausible record start ('@' + 'x'..., which makes it part of that record's header line), the
 * last one as a tail — so that the device parse of the buffer yields exactly the reference's records.  File offsets stay as
 * they are.  Returns the number of bytes overwritten (0: a well-formed file).  Host only. */
uint64_t lash_fastq_sanitize(uint8_t *buf, uint64_t n, int skip_bad);

/* Two-stage form for callers that keep genomes resident in HBM as 2-bit (0.28 B/base incl. break bitmap):
 * pack once, sketch many times (other k / algo / seed; a packed batch belongs to the base codes / k-mer bit order of the layout it was packed
 * under: after lash_ctx_set_layout changes those, lash_sketch_packed_device returns LASH_EINVAL).  The pack stage performs filter_out_n + KSeq::new
 * (utils.rs:459,464) and records where records begin so that no k-mer spans two records (utils.rs:457-464). */
int  lash_pack_device(lash_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_rec_off, uint64_t n_rec,
                      const uint64_t *genome_rec_off, const uint64_t *genome_byte_off, uint32_t n_genomes,
                      lash_packed **out);
int  lash_sketch_packed_device(lash_ctx *ctx, const lash_params *prm, const lash_packed *pk, uint8_t *d_out_images);
void lash_packed_free(lash_ctx *ctx, lash_packed *pk);
uint64_t lash_packed_bytes(const lash_packed *pk);          /* device bytes held */

/* Union of serialized sketches, image-wise: dst[i] = dst[i] U src[i]
 * (hyperminhash union / HyperLogLog::union / UltraLogLog::merge, utils.rs:171,261,357). */
int lash_merge_images_device(lash_ctx *ctx, int algo, int p, uint8_t *d_dst, const uint8_t *d_src, uint64_t n_images);
int lash_merge_images(lash_ctx *ctx, int algo, int p, uint8_t *dst, const uint8_t *src, uint64_t n_images);

/* dist side, HyperMinHash: the register scan of hyperminhash's Sketch::similarity for every (reference, query) pair
 * (/root/reference/src/utils.rs:150-167):  out_c[r * n_qry + q] = #{i : a_i != 0 and a_i == b_i},
 * out_n[r * n_qry + q] = #{i : a_i != 0 or b_i != 0}.  Images are 32 768-byte HMH sketches as written by `save`. */
int lash_hmh_pair_counts_device(lash_ctx *ctx, const uint8_t *d_ref_images, uint32_t n_ref, const uint8_t *d_qry_images,
                                uint32_t n_qry, uint32_t *d_out_c, uint32_t *d_out_n);
int lash_hmh_pair_counts(lash_ctx *ctx, const uint8_t *ref_images, uint32_t n_ref, const uint8_t *qry_images,
                         uint32_t n_qry, uint32_t *out_c, uint32_t *out_n);

/* dist side, HyperLogLog: for every (reference, query) pair the two numbers `len()` needs from the union sketch
 * (/root/reference/src/utils.rs:355-363: ref_hll.union(q_hll); ref_hll.len()):
 * out_zero[r * n_qry + q] = #{i : max(a_i, b_i) == 0},  out_sum[r * n_qry + q] = sum_i 2^-max(a_i, b_i).
 * Images are HLL sketches of precision p as written by `save` (33-byte header + 2^p registers).
 * (p >= 10 runs through per-threshold bitmaps and popcounts, which needs the range of register values first: the device entry
 * synchronizes the stream while it prepares them, as lash_sketch_set_prepare does.) */
int lash_hll_pair_union_stats_device(lash_ctx *ctx, int p, const uint8_t *d_ref_images, uint32_t n_ref,
                                     const uint8_t *d_qry_images, uint32_t n_qry, uint32_t *d_out_zero, double *d_out_sum);
int lash_hll_pair_union_stats(lash_ctx *ctx, int p, const uint8_t *ref_images, uint32_t n_ref, const uint8_t *qry_images,
                              uint32_t n_qry, uint32_t *out_zero, double *out_sum);

/* dist side, UltraLogLog (/root/reference/src/utils.rs:186-288): for every (reference, query) pair the distinct-count
 * estimate of the merged sketch — UltraLogLog::merge (utils.rs:260-262) followed by get_distinct_count_estimate()
 * (estimator LASH_ULL_FGRA) or MaximumLikelihoodEstimator.estimate() (LASH_ULL_ML), utils.rs:265-269:
 * out_est[r * n_qry + q].  Images are ULL sketches of precision p as written by `save`. */
#define LASH_ULL_FGRA 0
#define LASH_ULL_ML   1
int lash_ull_pair_union_estimates_device(lash_ctx *ctx, int p, int estimator, const uint8_t *d_ref_images, uint32_t n_ref,
                                         const uint8_t *d_qry_images, uint32_t n_qry, double *d_out_est);
int lash_ull_pair_union_estimates(lash_ctx *ctx, int p, int estimator, const uint8_t *ref_images, uint32_t n_ref,
                                  const uint8_t *qry_images, uint32_t n_qry, double *out_est);
/* The same two estimators for ONE sketch (utils.rs:213-217), host only: `registers` = the 2^p state bytes (no header). */
double lash_ull_estimate(const uint8_t *registers, int p, int estimator);

/* ---- dist side, host arithmetic (no GPU): what is O(sketches) or O(pairs) in utils.rs:84-373 ------------------------------
 * HLL++ empirical bias tables.  streaming_algorithms' `len()` (utils.rs:315, 355-363) subtracts, when its raw estimate is
 * <= 5 * 2^p, the mean bias of the 6 nearest samples of a per-precision table of Monte-Carlo measurements (Heule et al. 2013,
 * appendix; the crate carries them as constants).  The numbers are neither in /root/reference nor derivable, so they are NOT
 * in this library: lash_hll_bias_load reads them from a text file ('#' comments; "p <p> <n>" then n lines "<raw> <bias>", any
 * subset of p = 4..18) that tools/ref_probe/extract_hll_bias.py writes from the crate's source.  With `tables` NULL (or no
 * table for p) that regime returns LASH_ERANGE instead of a different estimate.
 * The tables are measurements, so they can also be MADE: lash_hll_bias_simulate repeats the Monte-Carlo of the HLL++ paper on
 * the GPU (hll_bias_sim.hip, DESIGN.md "Simulated HLL++ bias tables") and its arrays go to lash_hll_bias_from_arrays.  Those
 * numbers are regenerated, not the crate's: estimates are unbiased with them, but not digit for digit what the reference prints. */
typedef struct lash_hll_bias lash_hll_bias;
int  lash_hll_bias_load(const char *path, lash_hll_bias **out);               /* LASH_EINVAL: cannot open; LASH_EFORMAT: malformed */
int  lash_hll_bias_from_arrays(lash_hll_bias **inout, int p, const double *raw, const double *bias, uint32_t n);  /* *inout NULL: created */
int  lash_hll_bias_has(const lash_hll_bias *tables, int p);
void lash_hll_bias_free(lash_hll_bias *tables);
/* One precision's table by simulation (the only entry of this group that needs the GPU).  n_trials random sets (0 = 2048, at most
 * 2^20) are grown to 5 * 2^p distinct elements each; at the n_points checkpoints n_j = j * 5 * 2^p / (n_points - 1) (0 =
 * lash_hll_bias_default_points(p) = min(200, 5 * 2^p + 1); 6 <= n_points <= 5 * 2^p + 1) the raw estimate alpha m^2 / sum of every set is
 * taken: out_raw[j] = its mean over the sets (exact sum, exact quotient, rounded once to the nearest double), out_bias[j] = out_raw[j] - n_j, out_n[j] = n_j (out_n may be NULL).  The
 * arrays hold n_points entries (the default count when 0 was passed).  Hash, register rule and summation orders are fixed: the same
 * (p, n_points, n_trials, seed) gives the same bits on every run and device.  Synchronous.  LASH_EINVAL: p outside 4..18, n_points or
 * n_trials out of range, NULL ctx / out_raw / out_bias. */
int      lash_hll_bias_simulate(lash_ctx *ctx, int p, uint32_t n_points, uint32_t n_trials, uint64_t seed, uint64_t *out_n, double *out_raw,
                                double *out_bias);
uint32_t lash_hll_bias_default_points(int p);                                  /* 0 for p outside 4..18 */
/* Per-sketch cardinalities from the register bytes (no header): hyperminhash's LogLog-beta (`cardinality()`, utils.rs:170-173),
 * streaming_algorithms' `len()` (utils.rs:315), lash_ull_estimate above. */
double lash_hmh_cardinality(const uint8_t *registers, int big_endian);
int    lash_hll_cardinality(const uint8_t *registers, int p, const lash_hll_bias *tables, double *out);
/* The distance the reference prints for every pair of an [n_ref x n_qry] block, from the GPU's pair statistics and the
 * per-sketch cardinalities: similarity (hmh: C, N + expected-collision correction, utils.rs:164; hll: len() of the union from
 * zero / sum, utils.rs:355-362; ull: the union estimate, utils.rs:272) -> .max(0) -> 2s/(1+s) -> model 1: min(-ln(f)/k, 1),
 * model 0: 1 - f^(1/k) (main.rs:415-423), in f32 arithmetic when fp32 (main.rs --fp32).  The caller applies the
 * "same name -> 0" rule (main.rs:452-453).  hmh: c_or_zero = C, n_counts = N; hll: c_or_zero = zero, sum_or_union = sum;
 * ull: sum_or_union = union estimates.  LASH_ERANGE: a union fell into the HLL bias-table regime and `tables` does not cover
 * it (*bad_pair = its index). */
int    lash_dist_rows(int algo, int p, int k, int model, int fp32, uint32_t n_ref, uint32_t n_qry, const double *ref_card,
                      const double *qry_card, const uint32_t *c_or_zero, const uint32_t *n_counts, const double *sum_or_union,
                      const lash_hll_bias *tables, const double *hmh_ec, double *out_dist, uint64_t *bad_pair);
/* hmh_ec (HyperMinHash only, may be NULL): hyperminhash's expected_collisions(n, m) per pair, [n_ref x n_qry], as
 * lash_hmh_pair_expected_collisions / lash_sketch_set_hmh_expected_collisions compute them on the GPU; READ ONLY for pairs whose two
 * cardinalities are both <= 2^19 (every other pair is a closed form, taken here).  NULL: those pairs are computed here on the host,
 * a walk over 65 536 cells with four pow() each (4 ms to 0.2 s PER PAIR, as in the crate): viruses, plasmids, short contigs. */

/* The measure a distance is taken of (`lash dist --containment`, not upstream).  s: the similarity above after its clamp; a_r / a_q:
 * the reference's / the query's cardinality.
 *   LASH_MEASURE_JACCARD            frac = 2s/(1+s): the reference's Mash distance, what every entry without a measure computes
 *   LASH_MEASURE_CONTAIN_QUERY      frac = s/(1+s) * (a_r + a_q) / a_q: how much of the query is in the reference
 *   LASH_MEASURE_CONTAIN_REFERENCE  frac = s/(1+s) * (a_r + a_q) / a_r: how much of the reference is in the query
 * s/(1+s) * (a_r + a_q) estimates the shared k-mers (hll / ull: a_r + a_q - union exactly).  s <= 0 gives d = 1 exactly, frac >= 1
 * gives d = +0 exactly, otherwise the model's distance of frac as for the Jaccard fraction; with a_r == a_q frac is 2s/(1+s) bit for
 * bit (csrc/dist_pair.h states the rule once, for the host and the device).  Containment is directional: the _measure entries below
 * take rectangles only, triangle != 0 with a containment is LASH_EINVAL, as is any other value of `measure`.  Each _measure entry is
 * its namesake with one more argument, and its namesake is the entry with LASH_MEASURE_JACCARD. */
#define LASH_MEASURE_JACCARD 0
#define LASH_MEASURE_CONTAIN_QUERY 1
#define LASH_MEASURE_CONTAIN_REFERENCE 2
int    lash_dist_rows_measure(int algo, int p, int k, int model, int fp32, uint32_t n_ref, uint32_t n_qry, const double *ref_card,
                              const double *qry_card, const uint32_t *c_or_zero, const uint32_t *n_counts, const double *sum_or_union,
                              const lash_hll_bias *tables, const double *hmh_ec, int measure, double *out_dist, uint64_t *bad_pair);

/* ---- dist side, resident form: all-vs-all on whole collections (BASELINE configs[3]: 10^5 sketches, 5 * 10^9 printed pairs) ----
 * `lash dist` keeps both sketch files in memory for the run (utils.rs:95-127, 202-242, 303-337), takes one cardinality per
 * sketch (utils.rs:170-173, 213-219, 314-315) and walks reference rows x query columns — the lower triangle only when both are
 * the same files (utils.rs:150-180).  A lash_sketch_set is the device-side counterpart: N serialized sketches resident in HBM,
 * uploaded (or adopted from device memory, e.g. the result of an all-gather) ONCE, plus what the pair kernels derive from them
 * once: HyperMinHash register bit planes, HyperLogLog threshold bitmaps.
 *   create          images: n_images serialized sketches of (algo, p) in the context's layout, host memory; member i of the set is
 *                   images[order[i]] (order NULL: member i = image i, n == n_images) — `order` is how a caller puts the set into
 *                   the reference's hash-map key order so that the printed triangle is the set's lower triangle
 *   create_device   adopts d_images (n sketches, set order) without copying; they must outlive the set
 *   cardinalities   per-member distinct-count estimates, the same numbers as lash_hmh_cardinality / lash_hll_cardinality /
 *                   lash_ull_estimate give for each image: register histograms on the GPU, O(histogram) finish on the host.
 *                   LASH_ERANGE: an HLL member fell into the bias-table regime and `tables` does not cover it (*bad_index)
 *   prepare         builds what pair_block needs for this (reference, query) combination (may be the same set); call it once,
 *                   from one thread, before the first pair_block of the combination.  Not needed for correctness: without it
 *                   pair_block falls back to the kernels that read the images themselves (several times slower)
 *   pair_block      statistics of set rows [r0, r1) of `ref` against columns [0, n_cols) of `qry`, row-major [r1 - r0][n_cols]:
 *                   hmh: out_c_or_zero = C, out_n = N (lash_hmh_pair_counts); hll: out_c_or_zero = zero, out_sum_or_union = sum
 *                   (lash_hll_pair_union_stats); ull: out_sum_or_union = the union estimate (lash_ull_pair_union_estimates).
 *                   triangle != 0 (the rows and the columns are the same names in the same order, normally the same set): only
 *                   entries with column <= r0 + row are defined — tiles wholly above the diagonal are skipped
 *                   (utils.rs:158-160).  A caller that wants the triangle passes n_cols = r1.
 *                   Sets are read-only here: several contexts (host threads) of the same device may call pair_block on the
 *                   same prepared sets concurrently.  _device: outputs in device memory, asynchronous on the context's stream. */
typedef struct lash_sketch_set lash_sketch_set;
int      lash_sketch_set_create(lash_ctx *ctx, int algo, int p, const uint8_t *images, uint32_t n_images, const uint32_t *order, uint32_t n,
                                lash_sketch_set **out);
int      lash_sketch_set_create_device(lash_ctx *ctx, int algo, int p, const uint8_t *d_images, uint32_t n, lash_sketch_set **out);
void     lash_sketch_set_free(lash_ctx *ctx, lash_sketch_set *set);
uint32_t lash_sketch_set_size(const lash_sketch_set *set);
int      lash_sketch_set_cardinalities(lash_ctx *ctx, lash_sketch_set *set, int ull_estimator, const lash_hll_bias *tables,
                                       double *out_card, uint32_t *bad_index);
int      lash_sketch_set_prepare(lash_ctx *ctx, lash_sketch_set *ref, lash_sketch_set *qry);
int      lash_sketch_set_pair_block(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                    uint32_t n_cols, int triangle, int ull_estimator, uint32_t *out_c_or_zero, uint32_t *out_n,
                                    double *out_sum_or_union);
int      lash_sketch_set_pair_block_device(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                           uint32_t n_cols, int triangle, int ull_estimator, uint32_t *d_c_or_zero, uint32_t *d_n,
                                           double *d_sum_or_union);
/* pair_block_within: `lash dist --max-dist`.  The same block as pair_block, but what comes back is only its pairs whose distance d
 * (lash_dist_rows' number, before the "same name -> 0" rule, which is the caller's) passes d <= max_dist; NaN never passes.  The pair
 * statistics, HyperMinHash's expected collisions of small pairs and a filter kernel run on the device; only the candidates the filter
 * lets through are copied back, and each is evaluated here exactly as lash_dist_rows evaluates it.  Survivors are written in (row,
 * col) order — out_row[i] is the set row (r0 <= row < r1), out_col[i] the column, out_dist[i] d — the first `cap` of them; *n_kept
 * is their full count (> cap: call again with larger buffers; the result is deterministic).  n_candidates (may be NULL): how many
 * pairs the filter kernel passed to the host.  LASH_ERANGE with *bad_pair = (row - r0) * n_cols + col of the first such pair in
 * (row, col) order exactly when lash_dist_rows would refuse the block (an HLL union in the bias-table regime that `tables` does
 * not cover).  Needs lash_sketch_set_cardinalities on both sets; prepare as for pair_block.  triangle / n_cols as pair_block;
 * k, model, fp32, tables as lash_dist_rows.  max_dist NaN: LASH_EINVAL. */
int      lash_sketch_set_pair_block_within(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                           uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator,
                                           const lash_hll_bias *tables, double max_dist, uint32_t *out_row, uint32_t *out_col,
                                           double *out_dist, uint64_t cap, uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates);
/* the same under `measure` (LASH_MEASURE_*, above lash_dist_rows_measure): d is lash_dist_rows_measure's number */
int      lash_sketch_set_pair_block_within_measure(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                                   uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator,
                                                   const lash_hll_bias *tables, int measure, double max_dist, uint32_t *out_row, uint32_t *out_col,
                                                   double *out_dist, uint64_t cap, uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates);

/* pair_block_top: `lash dist --top K`.  A pair's rank key is (d, row, col): d its printed distance (lash_dist_rows' number, in f32
 * under fp32, with the "same name -> 0" rule), then its position in the unfiltered output; NaN is never ranked.  N_K(X) = the K
 * smallest keys among the pairs of name X: a column of a rectangular run; a row or a column of a triangle run.  The block runs as
 * pair_block_within (statistics, expected collisions, then a selection on the device: dist_top.hip) and comes back as the exact
 * (row, col, d) of a SUPERSET of the block's pairs that can be in some N_K given the bounds, in (row, col) order, NaN dropped, and
 * with max_dist (NaN: none) only d <= max_dist.  top_k in [1, LASH_TOP_MAX].  same_col (may be NULL): per block row the column that
 * carries the row's name (LASH_TOP_NO_COLUMN: none) — that pair's d is 0.  col_bound (per column) / row_bound (per block row,
 * triangle only), may be NULL: the caller's current K-th key for that name (lash_top_bounds), or d = +inf.  cap / *n_kept /
 * *bad_pair / *n_candidates (the pairs the device passed to the host) and LASH_ERANGE: as pair_block_within.
 * lash_top: the host-side per-name lists that make N_K from those blocks (the command line and Python share it):
 *   create   n_names: the columns (rectangular) or the set (triangle, rows and columns are the same names)
 *   add      a block's result: each pair goes to its column's list and, in a triangle run, to its row's (the diagonal once)
 *   bounds   col_bound [0, n_cols) and row_bound [r0, r1) for the next block (rectangular: row_bound gets +inf)
 *   merge    another accumulator's lists (one per worker / device)
 *   result   every kept pair, in (row, col) order, each once: the rows `--top` prints; *n the count (> cap: call again) */
#define LASH_TOP_MAX 1024u
#define LASH_TOP_NO_COLUMN 0xFFFFFFFFu
typedef struct lash_top_key { double d; uint32_t row, col; } lash_top_key;
int      lash_sketch_set_pair_block_top(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                        uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator,
                                        const lash_hll_bias *tables, uint32_t top_k, double max_dist, const uint32_t *same_col,
                                        const lash_top_key *col_bound, const lash_top_key *row_bound, uint32_t *out_row, uint32_t *out_col,
                                        double *out_dist, uint64_t cap, uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates);
/* the same under `measure` (LASH_MEASURE_*): ranked by lash_dist_rows_measure's number; a containment is a rectangle, so per column */
int      lash_sketch_set_pair_block_top_measure(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                                uint32_t n_cols, int triangle, int k, int model, int fp32, int ull_estimator,
                                                const lash_hll_bias *tables, int measure, uint32_t top_k, double max_dist, const uint32_t *same_col,
                                                const lash_top_key *col_bound, const lash_top_key *row_bound, uint32_t *out_row, uint32_t *out_col,
                                                double *out_dist, uint64_t cap, uint64_t *n_kept, uint64_t *bad_pair, uint64_t *n_candidates);
typedef struct lash_top lash_top;
int      lash_top_create(uint32_t n_names, uint32_t top_k, int triangle, lash_top **out);
int      lash_top_add(lash_top *t, const uint32_t *row, const uint32_t *col, const double *dist, uint64_t n);
int      lash_top_bounds(lash_top *t, uint32_t r0, uint32_t r1, uint32_t n_cols, lash_top_key *col_bound, lash_top_key *row_bound);
int      lash_top_merge(lash_top *dst, const lash_top *src);
int      lash_top_result(lash_top *t, uint32_t *out_row, uint32_t *out_col, double *out_dist, uint64_t cap, uint64_t *n);
void     lash_top_free(lash_top *t);

/* pair_block_cluster: `lash dist --cluster D`, single-linkage clusters of a triangle run (rows and columns are the same names in the
 * same order).  Two names are LINKED iff pair_block_within with the same arguments returns their pair: the exact d passes
 * d <= max_dist, NaN never; the diagonal plays no part.  Clusters are the connected components of the links.  The block runs as
 * pair_block_within with triangle = 1 (statistics, expected collisions), then a mark-and-join kernel (dist_cluster.hip): a pair whose
 * names are already in one cluster is pruned without arithmetic, a pair that is surely linked joins the two clusters in a label array
 * in device memory (a union-find, compare-and-swap on roots), a pair that is surely not linked is dropped, and only the pairs the
 * device cannot decide (within the margin of max_dist, or host-only arithmetic) come back; each of those is evaluated here exactly
 * and, when linked, joined in the same label array.  Blocks may run in any order and be spread over several accumulators (one per worker, each
 * with the context of its device); the labels do not depend on it.  LASH_ERANGE and *bad_pair as pair_block_within (pairs the device
 * cannot place are never pruned).  max_dist NaN, r1 or n_cols beyond the accumulator's n, an accumulator of another device: LASH_EINVAL.
 * lash_cluster:
 *   create   n names, each a cluster of its own; the label array lives on ctx's device
 *   merge    folds another accumulator's clusters into dst (src's labels go through the host and are joined on dst's device, on
 *            its default stream); src is unchanged
 *   labels   out[i] = the smallest index of the cluster of i, for all n
 * stats (may be NULL), per call: pairs = the block's printed off-diagonal pairs; pruned = already in one cluster, no distance
 * computed; joined_on_device = successful joins (at most n - 1 over an accumulator's life); sent_to_host = the pairs that came
 * back; clusters = the accumulator's number of clusters after the block. */
typedef struct lash_cluster lash_cluster;
typedef struct lash_cluster_stats { uint64_t pairs, pruned, joined_on_device, sent_to_host, clusters; } lash_cluster_stats;
int      lash_cluster_create(lash_ctx *ctx, uint32_t n, lash_cluster **out);
void     lash_cluster_free(lash_cluster *c);
int      lash_sketch_set_pair_block_cluster(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                            uint32_t n_cols, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables,
                                            double max_dist, lash_cluster *cluster, lash_cluster_stats *stats, uint64_t *bad_pair);
int      lash_cluster_merge(lash_cluster *dst, const lash_cluster *src);
int      lash_cluster_labels(const lash_cluster *c, uint32_t *out);

/* pair_block_derep: `lash dist --derep D`, greedy representatives of a triangle run (rows and columns are the same names in the same
 * order, which is the priority order).  Two names are WITHIN max_dist iff pair_block_within with the same arguments returns their
 * pair: the exact d passes d <= max_dist, NaN never; the diagonal plays no part.  Name i is a representative iff no representative
 * j < i is within max_dist of it, and otherwise a member of the FIRST such j in row order (not the nearest; not transitive).  The block
 * runs as pair_block_within with triangle = 1 (statistics, expected collisions), then a mark kernel and a trim kernel
 * (dist_derep.hip): a column of an earlier block that is not a representative is pruned before any arithmetic, a pair that is surely
 * farther than max_dist is dropped, the first column of an earlier block that is surely within it is recorded per row and every pair
 * beyond it is cleared, and what is left comes back: that hit, the pairs before it the device cannot decide (within the margin of
 * max_dist, or host-only arithmetic), and for a row without such a hit its in-block candidates too.  They are walked here row by row,
 * in column order, with the exact arithmetic, each row stopping at its first representative within max_dist.  LASH_ERANGE with
 * *bad_pair (as pair_block_within) iff that walk meets a pair the arithmetic refuses before the row stops; pairs beyond a row's
 * stop do not matter.  Blocks depend on each other: they must arrive in row order, contiguous from 0, on one accumulator.
 * LASH_EINVAL: max_dist NaN, r0 not the number of rows decided so far, r1 or n_cols beyond the accumulator's n, n_cols < r1, an
 * accumulator of another device.
 * lash_derep:
 *   create   n names, all undecided; rep[] lives on ctx's device with a mirror on the host
 *   result   out[i] = i for a representative, else the representative i is a member of, for all n; LASH_EINVAL before every name
 *            is decided
 * stats (may be NULL), per call: pairs = the block's printed off-diagonal pairs; pruned_not_rep = columns skipped without a distance;
 * pruned_after_hit = mask bits the trim cleared; sent_to_host = the pairs that came back; evaluated = those the walk computed;
 * representatives = the accumulator's count after the block. */
typedef struct lash_derep lash_derep;
typedef struct lash_derep_stats { uint64_t pairs, pruned_not_rep, pruned_after_hit, sent_to_host, evaluated, representatives; } lash_derep_stats;
int      lash_derep_create(lash_ctx *ctx, uint32_t n, lash_derep **out);
void     lash_derep_free(lash_derep *d);
int      lash_sketch_set_pair_block_derep(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                          uint32_t n_cols, int k, int model, int fp32, int ull_estimator, const lash_hll_bias *tables,
                                          double max_dist, lash_derep *acc, lash_derep_stats *stats, uint64_t *bad_pair);
int      lash_derep_result(const lash_derep *d, uint32_t *out);

/* lash_tree: `lash dist --tree` and `--cluster D --linkage average|complete`, agglomerative clustering of an n x n matrix of f64
 * distances held in device memory (dist_tree.hip), n - 1 merges back.  The rule: slots 0..n-1 hold one leaf each (size 1, height 0);
 * step s = 0..n-2 takes, among active slots i < j, the pair with the smallest key (D[i][j], i, j), records merge s = (node of i,
 * node of j, D[i][j], size_i + size_j), lets the new node n + s live on in slot i and retires slot j; for every other active k,
 * D[i][k] = D[k][i] becomes
 *   LASH_LINKAGE_AVERAGE   (size_i * D[i][k] + size_j * D[j][k]) / (size_i + size_j), each operation a separately rounded f64 one
 *   LASH_LINKAGE_SINGLE    min(D[i][k], D[j][k])
 *   LASH_LINKAGE_COMPLETE  max(D[i][k], D[j][k])
 * Node ids follow the scipy convention (leaves 0..n-1, the node of step s is n + s).  The result is a function of the input bits.
 * lash_tree (every entry takes the context of the tree's device, else LASH_EINVAL):
 *   create     allocates the n x n f64 matrix on ctx's device; LASH_ENOMEM with a last-error text that states the bytes needed
 *   set_rows   d is host memory, row-major [r1 - r0][r1]; only columns <= row are read (the triangle) and each value lands at D[r][c]
 *              and D[c][r].  Blocks may arrive in any order and any split; a cell set twice keeps the later value
 *   get_rows   full rows [r1 - r0][n] as they stand, before build only (how tests see the mirror)
 *   build      out holds n - 1 merges in step order; the whole merge loop is queued on ctx's stream (three plain launches per step,
 *              no host round trip per step) and synchronized once.  It consumes the matrix.  LASH_EINVAL, with a last-error text: a
 *              row that was never set, a NaN among the cells set_rows read (the text names row and col), a linkage other than the
 *              three, a second build.  n < 2 has no merges and out may be NULL
 *   free       the matrix and everything else
 * stats (may be NULL): steps = n - 1; rescanned_rows = rows whose cached nearest slot had to be recomputed from the full row, the
 * first fill of n rows included; bytes = the matrix, 8 n^2. */
typedef struct lash_tree lash_tree;
typedef struct lash_tree_merge { uint32_t a, b; double height; uint32_t size; } lash_tree_merge;
typedef struct lash_tree_stats { uint64_t steps, rescanned_rows, bytes; } lash_tree_stats;
#define LASH_LINKAGE_AVERAGE  0
#define LASH_LINKAGE_SINGLE   1
#define LASH_LINKAGE_COMPLETE 2
int      lash_tree_create(lash_ctx *ctx, uint32_t n, lash_tree **out);
int      lash_tree_set_rows(lash_ctx *ctx, lash_tree *t, uint32_t r0, uint32_t r1, const double *d);
int      lash_tree_get_rows(lash_ctx *ctx, const lash_tree *t, uint32_t r0, uint32_t r1, double *out);
int      lash_tree_build(lash_ctx *ctx, lash_tree *t, int linkage, lash_tree_merge *out, lash_tree_stats *stats);
void     lash_tree_free(lash_ctx *ctx, lash_tree *t);

/* lash_tree_build_nj: `lash dist --tree --nj`, a neighbour-joining tree of the same lash_tree matrix (dist_nj.hip; create / set_rows /
 * get_rows / free as above).  The rule: slots 0..n-1 hold one leaf each, the slot index being the label that breaks ties.  R[i] starts
 * from +0.0 and takes D[i][c] for c = 0, 1, .., n-1 in that order, c = i skipped, each add rounded.  Join step s = 0, 1, .. while r >= 3
 * (r = active slots, w = (double)(r - 2)): for active i < j, Q = ((w * D[i][j]) - R[i]) - R[j], three separately rounded operations;
 * the pair with the smallest key (Q, i, j) is joined with
 *   len_i = D[i][j] * 0.5 + (R[i] - R[j]) / (2.0 * w)      len_j = D[i][j] - len_i      join s = (node of i, node of j, len_i, len_j)
 * and for every other active k
 *   v = ((D[i][k] + D[j][k]) - D[i][j]) * 0.5      R[k] = ((R[k] - D[i][k]) - D[j][k]) + v      D[i][k] = D[k][i] = v
 * then R[i] = ((R[i] + R[j]) - (double)r * D[i][j]) * 0.5; node n + s lives on in slot i and slot j retires.  At r = 2 the closing
 * record (node of i, node of j, D[i][j], 0) of the remaining slots i < j.  out holds n - 1 records for n >= 2 (n - 2 joins, then the
 * closing record), none for n < 2 (out may be NULL).  Lengths may be negative and are reported as computed.  Row sums are carried,
 * never re-summed: the result is a function of the input bits.
 * The join loop is queued on ctx's stream (three plain launches per step, no host round trip per step) and synchronized once.  It
 * consumes the matrix, as lash_tree_build does.  LASH_EINVAL, with a last-error text: a row that was never set, a second build (of
 * either kind), a NaN or an infinite value among the cells set_rows read (the text names row and col; inf - inf would put a NaN into
 * the arg-min).  stats (may be NULL): steps = records written, rescanned_rows = 0, bytes = 8 n^2. */
typedef struct lash_nj_join { uint32_t a, b; double len_a, len_b; } lash_nj_join;
int      lash_tree_build_nj(lash_ctx *ctx, lash_tree *t, lash_nj_join *out, lash_tree_stats *stats);

/* lash_tree_build_pcoa: `lash dist --pcoa K`, principal coordinates (PCoA, classical MDS) of the same lash_tree matrix (dist_pcoa.hip;
 * create / set_rows / get_rows / free as above; n >= 2, k 1..16).  The rule: A = -1/2 D o D (every cell, the diagonal included, as set);
 * B[i][j] = A[i][j] - (r[i] + r[j]) + g, r the row means of A and g the mean of r (Gower centring, in place on the device).  The axes are
 * the k' = min(k, n - 1) ALGEBRAICALLY largest eigenpairs (theta_a, v_a) of B, theta_1 >= theta_2 >= ..., |v_a|_2 = 1 -- not the largest
 * in size: sketch distances are not Euclidean, B has negative eigenvalues and one of them may exceed theta_k in size.  The sign of v_a
 * makes its component of largest size positive (ties: the lowest row).
 *   out_eigenvalues[a] = theta_a            out_coords[i * k + a] = v_a[i] * sqrt(max(theta_a, 0))
 * so an axis with theta_a <= 0 is all +0.0, and so is every entry a >= k' (B has at most n - 1 non-zero eigenvalues).  Where eigenvalues
 * coincide, any orthonormal basis of their eigenspace is a valid answer.
 * The solver is a subspace iteration on B + sigma I with min(n, max(2k, k + 8)) vectors and a Rayleigh-Ritz step per iteration; the Ritz
 * values are sorted algebraically, so a negative eigenvalue the subspace holds costs a spare vector; sigma = |B|_F / 1000 + 1.1 times the
 * Frobenius norm of B outside the subspace covers the negative eigenvalues it does not hold, renewed every iteration.  A converged
 * answer is accepted only if theta_k' + sigma >= 0 (then no eigenvalue outside the subspace exceeds theta_k'); otherwise the solve is
 * repeated from the start vectors with sigma >= -lambda_min(B) throughout, which ranks algebraically.  It stops when |B v_a - theta_a v_a|_2 <=
 * tol * max(theta_1, 0) holds for every a <= k', the residuals being those of B itself, computed on the device.  tol <= 0 means 1e-10,
 * max_iter = 0 means 2000.  Otherwise LASH_EINVAL with a last-error text that gives the iterations done and the worst relative residual,
 * and the outputs are untouched.  Everything is queued on ctx's stream; per iteration two 32 x 32 matrices come to the host (Q^T B Q, solved
 * there by cyclic Jacobi, and the Gram matrix of the residual vectors, whose diagonal holds the squared norms) with one status word,
 * and the 32 x 32 Ritz vectors and 32 Ritz values go back.  No floating-point atomics, every reduction a fixed tree, start vectors from splitmix64 with a fixed
 * seed: two builds of the same matrix bits give the same output bits, whatever order and split set_rows received.
 * It consumes the matrix, as lash_tree_build does.  LASH_EINVAL, with a last-error text: k outside 1..16, a second build (of any kind),
 * n < 2, a row that was never set, a NaN or an infinite value among the cells set_rows read (the text names row and col).
 * stats (may be NULL): iterations (of both passes together, as max_iter counts them); products = B Q products, each reading the matrix once; bytes = 8 n^2; worst_residual = the largest of
 * the k' relative residuals at exit; shift = the last sigma; trace = the sum of B[i][i], which theta_a is divided by for the share of an
 * axis (it can pass 1 in sum when negative eigenvalues exist). */
typedef struct lash_pcoa_stats { uint64_t iterations, products, bytes; double worst_residual, shift, trace; } lash_pcoa_stats;
int      lash_tree_build_pcoa(lash_ctx *ctx, lash_tree *t, uint32_t k, double tol, uint32_t max_iter, double *out_eigenvalues, double *out_coords,
                              lash_pcoa_stats *stats);

/* HyperMinHash sets: hyperminhash's expected_collisions(n, m) for the pairs of a block in which BOTH sketches hold at most 2^19
 * distinct k-mers (the regime in which the crate walks 65 536 cells per pair; lash_hmh_pair_expected_collisions below):
 * out_ec[(r - r0) * n_cols + c] for exactly those pairs — the other entries are left untouched, lash_dist_rows derives theirs in
 * O(1) — and *n_small_pairs says how many there were (0: out_ec was not touched and may be NULL).  Both sets must have had
 * lash_sketch_set_cardinalities called (the set keeps them); lash_sketch_set_prepare builds the query side's cell vectors once. */
int      lash_sketch_set_hmh_expected_collisions(lash_ctx *ctx, const lash_sketch_set *ref, uint32_t r0, uint32_t r1, const lash_sketch_set *qry,
                                                 uint32_t n_cols, double *out_ec, uint64_t *n_small_pairs);

/* hyperminhash's expected_collisions(n, m) for every pair of an [n_ref x n_qry] block from the per-sketch cardinalities (host
 * arrays in, host array out).  Above 2^19 (either sketch) the crate's closed form; below, the 65 536-cell sum as a product of
 * per-sketch cell-probability vectors: one vector kernel per sketch, one f64 MFMA matrix product per block (dist_kernels.hip).
 * Summation order differs from the crate's loop: agreement ~1e-13 relative.  The query vectors are kept on the device while
 * consecutive calls pass the same qry_card values (row blocks of one `dist` run). */
int    lash_hmh_pair_expected_collisions(lash_ctx *ctx, const double *ref_card, uint32_t n_ref, const double *qry_card, uint32_t n_qry,
                                         double *out_ec);

/* ---- growth: the cardinality of the running union along orderings of a set (`lash growth`, prefix_union.hip) ----
 * orders holds n_orders index lists of `len` members each, every entry < the set's size; a list need not be a permutation (repeats
 * are legal and change nothing).  out_card[o * len + t] is the distinct-count estimate of U(o, t) = member orders[o][0] U ... U member
 * orders[o][t], bit for bit what lash_hmh_cardinality / lash_hll_cardinality / lash_ull_estimate give for the image of that union (the
 * number lash_sketch_set_cardinalities returns for a single image): one workgroup per (order, slice of the register table) folds the
 * images in LDS and keeps the register histogram up to date, the O(histogram) finish runs on the host.  A HyperMinHash step whose
 * union holds a register with more than 39 leading zeros is re-folded with lash_merge_images_device and summed in register order.
 *   opts (may be NULL; a zero field = the library chooses)
 *     slices             the table is cut into that many contiguous runs of whole 32-bit words, sizes differing by at most one word
 *                        (clamped to the word count); one workgroup per (order, slice)
 *     hist_budget_bytes  bound on the device histogram buffer, orders in flight x len x 1 KiB: the orders go in chunks under it, at
 *                        least one order per chunk [256 MiB]
 *   The numbers do not depend on opts: the histograms are sums of integers.
 *   LASH_EINVAL  NULL arguments, len == 0 with n_orders > 0, an index >= the set's size (*bad_index = its position in orders), a bad
 *                ull_estimator for an UltraLogLog set, a table that does not fit on chip: supported are hmh, hll (p 4-16) and ull p 3-16
 *                (lash_ctx_last_error says so for ull p >= 17)
 *   LASH_ERANGE  an HLL union fell into the bias-table regime and `tables` does not cover it; *bad_index = o * len + t of the first
 *                such entry in (order, step) order
 * The set's own state (the cardinalities it has taken, what prepare built) is left untouched.  Synchronous.
 * _plan: what a call with these arguments would run with — out_plan->slices, and out_plan->hist_budget_bytes = the bytes of the
 * histogram buffer it allocates.  Same LASH_EINVAL for an unsupported table. */
typedef struct { uint32_t slices; uint64_t hist_budget_bytes; } lash_prefix_union_opts;   /* 0 = the library chooses */
int lash_sketch_set_prefix_union_cardinalities(lash_ctx *ctx, lash_sketch_set *set, const uint32_t *orders, uint32_t n_orders,
                                               uint32_t len, int ull_estimator, const lash_hll_bias *tables,
                                               const lash_prefix_union_opts *opts /* may be NULL */,
                                               double *out_card /* [n_orders][len] */, uint64_t *bad_index);
int lash_sketch_set_prefix_union_plan(lash_ctx *ctx, const lash_sketch_set *set, uint32_t n_orders, uint32_t len,
                                      const lash_prefix_union_opts *opts, lash_prefix_union_opts *out_plan);

/* ---- merge: one sketch per group of members of a set (`lash merge`, group_union.hip) ----
 * The groups are a CSR list: group g holds members[group_off[g] .. group_off[g + 1]), indices into the set; group_off[0] = 0 and the
 * offsets never decrease.  Groups may overlap, a member may repeat within a group, a group may be empty.  Image g of the output
 * (n_groups serialized images in the context's layout, back to back) is byte for byte what lash_merge_images leaves when the members
 * are folded into the image of an empty sketch one after another, header included; an empty group is that empty image.  The fold runs
 * on the device: a thread owns registers and walks members, a group longer than `segment` members is folded into partial unions in
 * scratch memory which are folded again (group_union.hip).
 *   opts (may be NULL; a zero field = the library chooses)
 *     segment               members per task of the first level; partial unions are folded max(segment, 2) at a time
 *     slices                workgroups an image's registers are cut over (clamped to the number of 16-byte units)
 *     scratch_budget_bytes  bound on the partial unions held at once: the groups go in chunks under it, at least one group per chunk
 *                           (a single group may exceed it) [1 GiB]
 *   The bytes do not depend on opts: the merge rules are commutative, associative and idempotent.
 *   LASH_EINVAL  NULL arguments, offsets that do not start at 0 or decrease, a member >= the set's size (*bad_index = its position in
 *                members), a set made under another layout than the context's
 *   LASH_ENOMEM  the partial unions of one chunk do not fit the device (lash_ctx_last_error names the groups and the bytes)
 * The set's own state is left untouched.  The host form is synchronous; _device writes to device memory and is asynchronous on the
 * context's stream (the lists are copied before it returns).
 * _plan: what a call with these offsets would run with — segment, slices, and scratch_budget_bytes = the scratch bytes it allocates. */
typedef struct { uint32_t segment; uint32_t slices; uint64_t scratch_budget_bytes; } lash_group_union_opts;   /* 0 = the library chooses */
int lash_sketch_set_group_union(lash_ctx *ctx, const lash_sketch_set *set, const uint64_t *group_off, const uint32_t *members,
                                uint32_t n_groups, const lash_group_union_opts *opts /* may be NULL */,
                                uint8_t *out_images /* host, n_groups images */, uint64_t *bad_index);
int lash_sketch_set_group_union_device(lash_ctx *ctx, const lash_sketch_set *set, const uint64_t *group_off, const uint32_t *members,
                                       uint32_t n_groups, const lash_group_union_opts *opts /* may be NULL */,
                                       uint8_t *d_out_images /* device, n_groups images */, uint64_t *bad_index);
int lash_sketch_set_group_union_plan(lash_ctx *ctx, const lash_sketch_set *set, const uint64_t *group_off, uint32_t n_groups,
                                     const lash_group_union_opts *opts, lash_group_union_opts *out_plan);

/* ---- spectrum: how the union's k-mers are shared inside a group (`lash spectrum`, group_spectrum.hip) ----
 * HyperMinHash sets only.  The groups are the CSR list of lash_sketch_set_group_union above (overlaps, repeats and empty groups are
 * legal; a member listed twice counts twice).  With r[j][b] the 16 384 16-bit registers of member j's image, for a group G of n members:
 *   U_b = max over j in G of r[j][b]                       the union's register: one k-mer of the union, drawn uniformly from the
 *                                                          bucket's distinct k-mers
 *   c_b = #{ j in G : r[j][b] == U_b } if U_b != 0, else 0  the members that hold that k-mer
 *   hist[c] = #{ b : c_b == c }, c = 0 .. n                 hist[0] = the empty buckets; the bins sum to 16 384
 * so hist[1 .. n] over the occupied buckets is a uniform sample, of up to 16 384 k-mers, of the group's multiplicity spectrum: the
 * distinct k-mers held by exactly c members are about hist[c] / (16384 - hist[0]) x the union's cardinality.  For a group of two,
 * hist[2] and 16384 - hist[0] are the C and N of lash_hmh_pair_counts.  All of it is exact integer work.
 *   out_hist          uint32 bins, CSR: group g's n_g + 1 bins at out_hist[group_off[g] + g .. group_off[g + 1] + g], group_off[n_groups]
 *                     + n_groups in all
 *   out_union_images  may be NULL; else n_groups images, byte for byte lash_sketch_set_group_union's (the fold runs anyway: the counts
 *                     are taken against it, and the union's cardinality is what scales the bins)
 *   opts              as for lash_sketch_set_group_union, and lash_sketch_set_group_union_plan answers for segment and slices;
 *                     scratch_budget_bytes bounds the union's partials together with the count tables (64 KiB for each group longer
 *                     than min(segment, 65 535) members) of a chunk of groups, at least one group per chunk
 *   The bins do not depend on opts: they are sums of integers.
 *   LASH_EINVAL  what lash_sketch_set_group_union refuses (*bad_index = the position in members of a member >= the set's size), and a
 *                set that is not HyperMinHash: an hll or ull register does not identify a k-mer (lash_ctx_last_error says so)
 *   LASH_ENOMEM  the scratch of one chunk does not fit the device
 * The set's own state is left untouched.  The host form is synchronous; _device writes to device memory and is asynchronous on the
 * context's stream (the lists are copied before it returns). */
int lash_sketch_set_group_spectrum(lash_ctx *ctx, const lash_sketch_set *set, const uint64_t *group_off, const uint32_t *members,
                                   uint32_t n_groups, const lash_group_union_opts *opts /* may be NULL */,
                                   uint32_t *out_hist /* host */, uint8_t *out_union_images /* host, may be NULL */, uint64_t *bad_index);
int lash_sketch_set_group_spectrum_device(lash_ctx *ctx, const lash_sketch_set *set, const uint64_t *group_off, const uint32_t *members,
                                          uint32_t n_groups, const lash_group_union_opts *opts /* may be NULL */,
                                          uint32_t *d_out_hist /* device */, uint8_t *d_out_union_images /* device, may be NULL */,
                                          uint64_t *bad_index);

/* ---- screen: winner-takes-all containment of queries against candidate references (`lash screen`, screen_wta.hip) ----
 * HyperMinHash sets only, both.  With q[b] the 16 384 16-bit registers of a query's image and r_i[b] those of reference row i:
 *   reference i HOLDS bucket b  iff  q[b] != 0 and r_i[b] == q[b]     the query's sampled k-mer of the bucket is one of the reference's
 * Every query row j of `qry` has a candidate list L_j = (i_0, i_1, ...) = cand_ref[cand_off[j] .. cand_off[j + 1]) of rows of `ref`;
 * POSITION IS PRIORITY, i_0 is best.  For the list of one query:
 *   winner[b] = the smallest position t such that i_t holds b, NONE (0xFFFFFFFF) if no candidate holds b
 *   shared[t] = #{ b : i_t holds b }                                   the C of lash_hmh_pair_counts for the pair (i_t, query)
 *   won[t]    = #{ b : winner[b] == t }                                the buckets credited to i_t when each goes to its best holder
 * so won[t] <= shared[t]; the sum of won over a list is the number of buckets some candidate holds, at most the query's occupied
 * buckets; a row listed twice wins nothing at its later position; an empty list gives nothing.  Lists may overlap.  All of it is exact
 * integer work, and equality and "not 0" do not depend on the layout's register byte order.
 *   cand_off          n_qry + 1 offsets, n_qry = the query set's size; cand_off[0] = 0 and the offsets never decrease
 *   out_shared,       uint32, cand_off[n_qry] each: entry cand_off[j] + t belongs to position t of query j's list
 *   out_won
 *   opts              as for lash_sketch_set_group_union: segment = the positions of a list one task walks, slices = the workgroups an
 *                     image's registers are cut over (lash_sketch_set_group_union_plan on the reference set and cand_off answers for
 *                     both); scratch_budget_bytes bounds the winner tables (64 KiB per query) of a chunk of queries, at least one
 *                     query per chunk [1 GiB]
 *   The counts do not depend on opts: they are minima and sums of integers.
 *   LASH_EINVAL  NULL arguments, offsets that do not start at 0 or decrease, a cand_ref entry >= the reference set's size (*bad_index =
 *                its position in cand_ref), a set that is not HyperMinHash: an hll or ull register does not identify a k-mer
 *                (lash_ctx_last_error says which set), a set made under another layout than the context's
 *   LASH_ENOMEM  the winner tables of one chunk do not fit the device
 * cand_off[n_qry] == 0 is LASH_OK and touches nothing.  Both sets' own state (the cardinalities they have taken, what prepare built) is
 * left untouched.  The host form is synchronous; _device writes to device memory and is asynchronous on the context's stream (the
 * lists are copied before it returns). */
int lash_sketch_set_screen_wta(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry,
                               const uint64_t *cand_off /* n_qry + 1, CSR over the query set's rows */,
                               const uint32_t *cand_ref /* reference rows, best first */, const lash_group_union_opts *opts /* may be NULL */,
                               uint32_t *out_shared /* host */, uint32_t *out_won /* host */, uint64_t *bad_index);
int lash_sketch_set_screen_wta_device(lash_ctx *ctx, const lash_sketch_set *ref, const lash_sketch_set *qry, const uint64_t *cand_off,
                                      const uint32_t *cand_ref, const lash_group_union_opts *opts /* may be NULL */,
                                      uint32_t *d_out_shared /* device */, uint32_t *d_out_won /* device */, uint64_t *bad_index);

/* Synthetic genomes of SURVEY.md §8(d) generated in HBM (bench / tests): genome ids first..first+n-1,
 * n_bases ASCII bytes each, written back to back at d_out. */
int lash_synth_genomes_device(lash_ctx *ctx, uint64_t first_genome, uint32_t n_genomes, uint64_t n_bases, uint8_t *d_out);

#ifdef __cplusplus
}
#endif
#endif
