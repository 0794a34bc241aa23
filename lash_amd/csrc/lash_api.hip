// lash_api.hip — the extern "C" boundary of liblash_gfx950.so (include/lash_gfx950.h): library / context / layout entries and the sketch
// entries (record batches, packed genomes, raw files).  Round 6 moved the planning behind them to lash_plan.hip, the HyperLogLog `sum`
// replay to lash_hll_replay.hip and the merge / dist-side entries to lash_dist_api.hip (lash_internal.h declares what they share).
//
// Reference side of the boundary: the per-file closure of sketch_files
// (/root/reference/src/utils.rs:452-508) and KmerSketch::{new,add_kmer,save} (utils.rs:377-434).
// There is no CPU fallback here: every compute entry needs a HIP device.
#include "lash_ctx.h"
#include "lash_internal.h"


// ===============================================================================================================

namespace lashi {

// needletail's record rules for uncompressed input as lash uses it (utils.rs:453-459), on the host: the exact
// path for the rare file the device parse flags.  FASTA: '>' header line, sequence lines up to the next line that starts with
// '>', line ends stripped.  FASTQ: '@' header, sequence line, '+' line, quality line of the same length; iteration STOPS at
// the first record that breaks this (the records before it stand).  Returns the offset at which the iteration stopped
// (n when the whole buffer parsed); seq / rec_off may be NULL (validation only).
// `bad` (FASTQ, may be NULL): the byte ranges [first, second) that are not part of any record the iteration yields.
size_t parse_fastx_strict(const uint8_t *d, size_t n, std::vector<uint8_t> *seq, std::vector<uint64_t> *rec_off, bool skip_bad,
                                 std::vector<std::pair<size_t, size_t>> *bad)
{
    auto line_end = [&](size_t p) { const void *q = memchr(d + p, '\n', n - p); return q ? (size_t)((const uint8_t *)q - d) : n; };
    size_t i = 0;
    if (n && d[0] == '>') {
        while (i < n) {
            i = line_end(i);
            if (i < n) ++i;
            while (i < n && d[i] != '>') {
                size_t e = line_end(i), stop = e;
                while (stop > i && d[stop - 1] == '\r') --stop;
                if (seq) seq->insert(seq->end(), d + i, d + stop);
                i = e < n ? e + 1 : n;
            }
            if (rec_off) rec_off->push_back(seq ? seq->size() : 0);
        }
        return n;
    }
    while (i < n) {
        const size_t rec = i;
        bool ok = false;
        do {
            if (d[i] != '@') break;
            const size_t e = line_end(i);
            if (e >= n) break;
            const size_t s = e + 1, se = line_end(s);
            if (se >= n) break;
            const size_t pl = se + 1;
            if (pl >= n || d[pl] != '+') break;
            const size_t pe = line_end(pl);
            if (pe >= n) break;
            const size_t ql = pe + 1, qe = line_end(ql);
            size_t sl = se - s, qn = qe - ql;
            while (sl && d[s + sl - 1] == '\r') --sl;
            while (qn && d[ql + qn - 1] == '\r') --qn;
            if (sl != qn) break;
            if (seq) seq->insert(seq->end(), d + s, d + s + sl);
            if (rec_off) rec_off->push_back(seq ? seq->size() : 0);
            i = qe < n ? qe + 1 : n;
            ok = true;
        } while (false);
        if (ok) continue;
        if (!skip_bad) { if (bad) bad->emplace_back(rec, n); return rec; }      // the iterator is finished by the error
        // layout.fastq_skip_bad: resume at the next plausible record start after `rec`
        size_t c = line_end(rec), resume = n;
        while (c < n) {
            const size_t ls = c + 1;
            if (ls >= n) break;
            if (d[ls] == '@') {
                const size_t l1 = line_end(ls), l2 = l1 < n ? line_end(l1 + 1) : n;
                if (l2 < n && l2 + 1 < n && d[l2 + 1] == '+') { resume = ls; break; }
            }
            c = line_end(ls);
        }
        if (bad) bad->emplace_back(rec, resume);
        i = resume;
    }
    return n;
}

}  // namespace lashi

extern "C" {

int lash_abi_version(void) { return LASH_ABI_VERSION; }

int lash_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *lash_strerror(int code)
{
    switch (code) {
    case LASH_OK: return "ok";
    case LASH_EINVAL: return "invalid argument (algorithm must be hmh/hll/ull, k 1..=32, hll p 4..=16, ull p 3..=26)";
    case LASH_ENODEV: return "no usable HIP device (liblash_gfx950 has no CPU fallback)";
    case LASH_EHIP: return "HIP runtime error";
    case LASH_ENOMEM: return "out of device memory";
    case LASH_ERANGE: return "HyperLogLog estimate <= 5 * 2^p needs the HLL++ bias tables of streaming_algorithms, which this build does not have (sketch with a smaller -p)";
    case LASH_EFORMAT: return "malformed FASTQ record (the images of the files listed by lash_ctx_format_errors are unreliable)";
    case LASH_ELIMIT: return "a genome exceeds 2^32-64 bytes in one call; split it and merge the images";
    default: return "unknown error";
    }
}

void *lash_host_alloc_pinned(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void lash_host_free_pinned(void *p)
{
    if (p) (void)hipHostFree(p);
}

int lash_params_check(const lash_params *prm)
{
    if (!prm) return LASH_EINVAL;
    if (prm->k < 1 || prm->k > 32) return LASH_EINVAL;                    // utils.rs:500-502
    if ((prm->flags & LASH_F_AMINO) && prm->k > 12) return LASH_EINVAL;   // utils.rs:554: "k-mer length for amino acid must be 1-12"
    switch (prm->algo) {
    case LASH_HMH: return LASH_OK;                                        // precision ignored, main.rs:212-213
    case LASH_HLL: return (prm->p >= 4 && prm->p <= 16) ? LASH_OK : LASH_EINVAL;
    case LASH_ULL: return (prm->p >= 3 && prm->p <= 26) ? LASH_OK : LASH_EINVAL;
    default: return LASH_EINVAL;                                          // main.rs:245
    }
}

size_t lash_sketch_image_bytes(int algo, int p) { return image_bytes(kDefaultLayout, algo, p); }

void lash_layout_default(lash_layout *out) { if (out) *out = kDefaultLayout; }

int lash_layout_check(const lash_layout *lay) { return lay && layout_ok(*lay) ? LASH_OK : LASH_EINVAL; }

size_t lash_layout_header_bytes(const lash_layout *lay, int algo)
{
    if (algo < LASH_HMH || algo > LASH_ULL) return 0;
    return (size_t)header_bytes(lay ? *lay : kDefaultLayout, algo);
}

size_t lash_layout_image_bytes(const lash_layout *lay, int algo, int p)
{
    if (lay && !layout_ok(*lay)) return 0;
    return image_bytes(lay ? *lay : kDefaultLayout, algo, p);
}

int lash_layout_parse(const char *spec, lash_layout *out)
{
    if (!out) return LASH_EINVAL;
    lash_layout lay = kDefaultLayout;
    std::string text = spec ? spec : "";
    size_t pos = 0;
    while (pos < text.size()) {
        size_t end = text.find(',', pos);
        if (end == std::string::npos) end = text.size();
        const std::string item = text.substr(pos, end - pos);
        pos = end + 1;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) return LASH_EINVAL;
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        auto two = [&](const char *zero, const char *one, uint8_t &dst) {
            if (val == zero) { dst = 0; return true; }
            if (val == one) { dst = 1; return true; }
            return false;
        };
        auto hdr = [&](char (&dst)[8]) {
            if (val.size() > 7) return false;
            memset(dst, 0, 8);
            memcpy(dst, val.data(), val.size());
            return true;
        };
        bool ok;
        if (key == "codes") {
            ok = val.size() == 4;
            for (size_t c = 0; ok && c < 4; ++c) {
                const char *at = strchr("ACGT", val[c]);
                if (!at || !val[c]) { ok = false; break; }
                lay.base_code[at - "ACGT"] = (uint8_t)c;
            }
        } else if (key == "kmer") ok = two("msb", "lsb", lay.kmer_lsb_first);
        else if (key == "hmh_x") ok = two("high", "low", lay.hmh_x_low);
        else if (key == "hmh_reg") ok = two("le", "be", lay.hmh_reg_be);
        else if (key == "hll_bucket") ok = two("low", "high", lay.hll_bucket_high);
        else if (key == "hmh_hdr") ok = hdr(lay.hmh_header);
        else if (key == "hll_hdr") ok = hdr(lay.hll_header);
        else if (key == "ull_hdr") ok = hdr(lay.ull_header);
        else if (key == "fastq_err") ok = two("stop", "skip", lay.fastq_skip_bad);
        else if (key == "aa_codes") ok = two("one", "zero", lay.aa_code_zero_based);
        else ok = false;
        if (!ok) return LASH_EINVAL;
    }
    if (!layout_ok(lay)) return LASH_EINVAL;
    *out = lay;
    return LASH_OK;
}

int lash_ctx_set_layout(lash_ctx *ctx, const lash_layout *lay)
{
    if (!ctx) return LASH_EINVAL;
    if (lay && !layout_ok(*lay)) return LASH_EINVAL;
    ctx->layout = lay ? *lay : kDefaultLayout;
    return LASH_OK;
}

int lash_ctx_get_layout(lash_ctx *ctx, lash_layout *out)
{
    if (!ctx || !out) return LASH_EINVAL;
    *out = ctx->layout;
    return LASH_OK;
}

int lash_ctx_create(lash_ctx **out, int device)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    int n = lash_device_count();
    if (n <= 0) return LASH_ENODEV;
    if (device < 0 || device >= n) return LASH_EINVAL;
    lash_ctx *ctx = new (std::nothrow) lash_ctx();
    if (!ctx) return LASH_ENOMEM;
    ctx->device = device;
    ctx->scratch.owned_by_ctx = true;
    hipDeviceProp_t prop;
    const bool ok = hipSetDevice(device) == hipSuccess && hipGetDeviceProperties(&prop, device) == hipSuccess &&
                    hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        lash_ctx_destroy(ctx);
        return LASH_EHIP;
    }
    ctx->own_stream = true;
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = ctx;
    return LASH_OK;
}

void lash_ctx_destroy(lash_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    release(ctx->sole_tab);
    release(ctx->sole_brk);
    release(ctx->sole_state);
    for (DevBuf *b : {&ctx->items, &ctx->item_begin, &ctx->item_kmers, &ctx->partials, &ctx->gregs, &ctx->counter, &ctx->st_seq, &ctx->st_rec,
                      &ctx->st_img, &ctx->hll_flags, &ctx->ec_ref, &ctx->ec_qry, &ctx->ec_x, &ctx->ec_card, &ctx->wf_scratch, &ctx->wf_out, &ctx->top_buf,
                      &ctx->fa_off, &ctx->fa_scratch, &ctx->fc_scratch, &ctx->kf_keep, &ctx->gu_members, &ctx->gu_tasks, &ctx->gu_part, &ctx->gu_hist,
                      &ctx->gu_out, &ctx->gs_members, &ctx->gs_tasks, &ctx->gs_counts, &ctx->gs_union, &ctx->gs_hist,
                      &ctx->sw_cand, &ctx->sw_tasks, &ctx->sw_winner, &ctx->sw_out})
        release(*b);
    {
        lash_packed &sc = ctx->scratch;
        for (DevBuf *b : {&sc.words, &sc.brk, &sc.tables, &sc.tiles, &sc.lookback, &sc.tile_begin_c, &sc.brk_bytes, &sc.fq})
            release(*b);
    }
    release(ctx->pair_ref);
    release(ctx->pair_qry);
    for (auto &s : ctx->ev_pool)
        for (auto &e : s.e)
            if (e) (void)hipEventDestroy(e);
    if (ctx->probe_host) (void)hipHostFree(ctx->probe_host);
    if (ctx->probe_ev) (void)hipEventDestroy(ctx->probe_ev);
    for (auto &sl : ctx->slot) {
        if (sl.busy && sl.d2h) (void)hipEventSynchronize(sl.d2h);
        for (DevBuf *b : {&sl.seq, &sl.rec, &sl.img}) release(*b);
        for (hipEvent_t e : {sl.h2d, sl.kern, sl.d2h}) if (e) (void)hipEventDestroy(e);
    }
    if (ctx->h2d_stream) (void)hipStreamDestroy(ctx->h2d_stream);
    if (ctx->d2h_stream) (void)hipStreamDestroy(ctx->d2h_stream);
    for (auto &hs : ctx->ring) {
        if (hs.done) (void)hipEventDestroy(hs.done);
        if (hs.ptr) (void)hipHostFree(hs.ptr);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int lash_ctx_set_stream(lash_ctx *ctx, void *hip_stream)
{
    if (!ctx) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->own_stream = false;
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    if (!hip_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return LASH_OK;
}

static int read_format_errors(lash_ctx *ctx)
{
    const uint32_t n = ctx->raw_files_pending;
    ctx->raw_files_pending = 0;
    ctx->bad_files.clear();
    if (!n || !ctx->scratch.d_dirty) return LASH_OK;
    std::vector<uint32_t> fl(n);
    HIPCHK(ctx, hipMemcpy(fl.data(), ctx->scratch.d_dirty + 3 * (size_t)n + 1, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t g = 0; g < n; ++g)
        if (fl[g]) ctx->bad_files.push_back(g);
    return LASH_OK;
}

static int check_pack_flag(lash_ctx *ctx, const lash_packed *pk)
{
    if (!pk || !pk->error_flag) return LASH_OK;
    uint32_t f = 0;
    HIPCHK(ctx, hipMemcpy(&f, pk->error_flag, 4, hipMemcpyDeviceToHost));
    if (f) { ctx->err = "pack kernel: look-back spin bound exceeded (results invalid)"; return LASH_EHIP; }
    return LASH_OK;
}

int lash_ctx_synchronize(lash_ctx *ctx)
{
    if (!ctx) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &sl : ctx->slot)                                   // results of lash_sketch_batch_async are in the caller's buffers
        if (sl.busy) { HIPCHK(ctx, hipEventSynchronize(sl.d2h)); sl.busy = false; }
    if (ctx->raw_files_pending) {                                // FASTQ structure flags of the last raw-file call
        const int rc = read_format_errors(ctx);
        if (rc) return rc;
        if (!ctx->bad_files.empty()) return LASH_EFORMAT;
    }
    for (const lash_packed *pk : ctx->last_packed) {
        const int rc = check_pack_flag(ctx, pk);
        if (rc) return rc;
    }
    return LASH_OK;
}

const char *lash_ctx_last_error(lash_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int lash_ctx_enable_timing(lash_ctx *ctx, int on)
{
    if (!ctx) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timing = on != 0;
    ctx->ev_used = 0;
    ctx->cur_ev = nullptr;
    ctx->last = lash_timing{};
    ctx->counter_zeroed = false;                                  // the k-mer census restarts as well
    return LASH_OK;
}

int lash_ctx_get_timing(lash_ctx *ctx, lash_timing *out)
{
    if (!ctx || !out) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    lash_timing t = ctx->last;
    t.pack_ms = t.sketch_ms = t.finalize_ms = t.direct_ms = 0.f;
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        const EvSet &s = ctx->ev_pool[i];
        if (!s.done) continue;
        float ms = 0.f;
        if (s.pack) { HIPCHK(ctx, hipEventElapsedTime(&ms, s.e[0], s.e[1])); t.pack_ms += ms; }
        HIPCHK(ctx, hipEventElapsedTime(&ms, s.e[2], s.e[3])); t.sketch_ms += ms;
        HIPCHK(ctx, hipEventElapsedTime(&ms, s.e[3], s.e[4])); t.finalize_ms += ms;
        if (s.direct) { HIPCHK(ctx, hipEventElapsedTime(&ms, s.e[6], s.e[5])); t.direct_ms += ms; }
    }
    t.kmers = 0;
    t.bases_last = 0;
    if (ctx->counter.ptr && ctx->counter_zeroed) {
        unsigned long long c = 0;
        HIPCHK(ctx, hipMemcpy(&c, ctx->counter.ptr, 8, hipMemcpyDeviceToHost));
        t.kmers = c;
    }
    if (ctx->last_sole_only && ctx->counter.ptr && ctx->counter_zeroed) {   // the last call ran on the persistent kernel alone: its own count
        unsigned long long b = 0;
        HIPCHK(ctx, hipMemcpy(&b, static_cast<const uint8_t *>(ctx->counter.ptr) + 8, 8, hipMemcpyDeviceToHost));
        t.bases_last = b;
    }
    for (const lash_packed *pk : ctx->last_packed) {
        if (!pk->n_genomes) continue;
        std::vector<uint64_t> nv(pk->n_genomes);
        HIPCHK(ctx, hipMemcpy(nv.data(), pk->d_nvalid, nv.size() * 8, hipMemcpyDeviceToHost));
        for (uint64_t v : nv) t.bases_last += v;
        if (pk->direct) {                                          // bytes deleted: by the direct pass in the genomes it kept, by
            const uint32_t n = pk->n_genomes;                      // the compacting kernel in the ones it took over
            std::vector<uint32_t> fl(5 * (size_t)n + 2);
            HIPCHK(ctx, hipMemcpy(fl.data(), pk->d_dirty, fl.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t g = 0; g < n; ++g)
                t.bases_last -= fl[g] ? fl[4 * (size_t)n + 2 + g] : fl[2 * (size_t)n + 1 + g];
        }
    }
    *out = t;
    return LASH_OK;
}

int lash_pack_device(lash_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_rec_off, uint64_t n_rec,
                     const uint64_t *genome_rec_off, const uint64_t *genome_byte_off, uint32_t n_genomes,
                     lash_packed **out)
{
    if (!ctx || !out) return LASH_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    lash_packed *pk = new (std::nothrow) lash_packed();
    if (!pk) return LASH_ENOMEM;
    int rc = n_genomes && (!genome_rec_off || !genome_byte_off) ? LASH_EINVAL : LASH_OK;
    if (rc == LASH_OK)
        rc = pack_into(ctx, pk, ctx->stream, nullptr, d_seq, n_genomes ? d_seq + genome_byte_off[n_genomes] : d_seq, d_rec_off, n_rec,
                       genome_rec_off, genome_byte_off, n_genomes);
    if (rc) { lash_packed_free(ctx, pk); return rc; }
    *out = pk;
    return LASH_OK;
}

void lash_packed_free(lash_ctx *ctx, lash_packed *pk)
{
    if (!pk || pk->owned_by_ctx) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (auto it = ctx->last_packed.begin(); it != ctx->last_packed.end();)
            it = (*it == pk) ? ctx->last_packed.erase(it) : it + 1;
    }
    for (DevBuf *b : {&pk->words, &pk->brk, &pk->tables, &pk->tiles, &pk->lookback, &pk->tile_begin_c, &pk->brk_bytes, &pk->fq})
        release(*b);
    delete pk;
}

uint64_t lash_packed_bytes(const lash_packed *pk)
{
    return pk ? pk->words.cap + pk->brk.cap + pk->tables.cap : 0;
}

int lash_sketch_packed_device(lash_ctx *ctx, const lash_params *prm, const lash_packed *pk, uint8_t *d_out_images)
{
    if (!ctx || !pk || (pk->n_genomes && !d_out_images)) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    if (prm->flags & LASH_F_AMINO) return LASH_EINVAL;                   // packed genomes are 2-bit nucleotides
    // the words carry the code table of the layout they were packed under (base codes, and their swap for kmer_lsb_first): another layout's
    // reverse complement and canonical order would read them wrongly — refuse instead of sketching something else
    if (pk->code_tab4 != layout_dev(ctx->layout, prm->algo).code_tab4) {
        ctx->err = "lash_sketch_packed_device: the context's layout changed its base codes / k-mer bit order since lash_pack_device";
        return LASH_EINVAL;
    }
    (void)hipSetDevice(ctx->device);
    if ((rc = timing_begin(ctx))) return rc;
    ctx->last_packed.clear();
    ctx->last_sole_only = false;
    ctx->last.calls += 1;
    return sketch_from(ctx, prm, pk, d_out_images, ctx->cur_ev);
}

int lash_sketch_batch_device(lash_ctx *ctx, const lash_params *prm, const uint8_t *d_seq, const uint64_t *d_rec_off,
                             uint64_t n_rec, const uint64_t *genome_rec_off, const uint64_t *genome_byte_off,
                             uint32_t n_genomes, uint8_t *d_out_images)
{
    if (!ctx || (n_genomes && (!d_out_images || !genome_rec_off || !genome_byte_off))) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    ctx->last_packed.clear();
    ctx->last_sole_only = false;
    ctx->last.calls += 1;
    if (n_genomes == 0) return LASH_OK;
    if (prm->flags & LASH_F_AMINO) return sketch_aa(ctx, prm, d_seq, d_rec_off, n_rec, genome_rec_off, genome_byte_off, n_genomes, d_out_images);

    // One packed batch, one stream.  Packing chunk c+1 on a second stream while chunk c is sketched was measured and
    // rejected (DESIGN.md "Rejected"): the pack workgroups' LDS fragments the CU's 160 KiB so that only one 64 KiB
    // sketch workgroup fits, and the step got 20-40 % slower.
    if ((rc = timing_begin(ctx))) return rc;
    EvSet *ev = ctx->cur_ev;
    TraceScope trace_scope(ctx->trace);
    TRACE("call");
    static const bool env_no_direct = getenv("LASH_NO_DIRECT") != nullptr;          // A/B knob for tools/
    // A genome that turns out dirty late has cost a wasted direct pass, so the optimistic pass only pays while most of a
    // batch is clean (break-even near 20 % dirty).  Feedback from the previous direct call, read without waiting:
    if (ctx->probe_pending && hipEventQuery(ctx->probe_ev) == hipSuccess) {
        ctx->dirty_frac = ctx->probe_tiles ? (float)ctx->probe_host[0] / (float)ctx->probe_tiles : 0.f;
        ctx->probe_pending = false;
    }
    // (the alternative k-mer / bucket rules of a non-default layout exist for packed input only)
    bool direct = !(prm->flags & LASH_F_NO_DIRECT) && !env_no_direct;
    bool stream_first = false;
    if (direct && ctx->dirty_frac > 0.2f) {
        if (++ctx->direct_skipped < 8) stream_first = true;     // skip the optimistic pass; try it again every 8th call
        else ctx->direct_skipped = 0;
    }
    static const bool env_stream_first = getenv("LASH_STREAM_FIRST") != nullptr;     // A/B knob for tools/ (like LASH_NO_DIRECT)
    ctx->scratch.stream_first = (stream_first || env_stream_first || (prm->flags & LASH_F_STREAM_ONLY)) && direct;
    ctx->last_sole_only = false;
    if (direct) {
        // Nothing but small genomes (a viral / plasmid / amplicon collection): the persistent kernel takes the whole call, planned
        // from the byte offsets alone — no descriptors, no work items, no pack tables (sole_kernels.hip; VERDICT r4 next #1: the
        // host loops over genomes were 17 ms per 10^6 genomes)
        const SolePlan sp = make_sole_plan(prm->algo, prm->p, n_genomes, (uint32_t)ctx->cu_count);
        const uint64_t smax = sole_max_bytes(ctx, prm, sp);
        bool all_small = smax != 0 && genome_byte_off[n_genomes] >= 16, any_multi = false;   // (the kernel loads 16 bytes at a time, from inside the buffer)
        bool identity = n_rec == n_genomes;                            // genome g IS record g: its byte offsets are the resident record offsets
        for (uint32_t g = 0; g < n_genomes && all_small; ++g) {
            if (genome_byte_off[g + 1] < genome_byte_off[g] || genome_rec_off[g + 1] < genome_rec_off[g] || genome_rec_off[g + 1] > n_rec) return LASH_EINVAL;
            all_small = genome_byte_off[g + 1] - genome_byte_off[g] <= smax;
            any_multi = any_multi || genome_rec_off[g + 1] - genome_rec_off[g] > 1;
            identity = identity && genome_rec_off[g] == g && genome_rec_off[g + 1] == (uint64_t)g + 1;
        }
        if (all_small) {
            rc = sole_call(ctx, prm, sp, n_genomes, ev, [&] {
                return sole_run(ctx, prm, sp, smax, d_seq, genome_byte_off[n_genomes], d_rec_off, n_rec, any_multi, identity, genome_byte_off, nullptr,
                                n_genomes, d_out_images, nullptr);
            });
            if (rc) return rc;
            ctx->last_sole_only = true;
            ctx->cur_ev = nullptr;
            return LASH_OK;
        }
    }
    rc = pack_into(ctx, &ctx->scratch, ctx->stream, ev, d_seq, d_seq + genome_byte_off[n_genomes], d_rec_off, n_rec,
                   genome_rec_off, genome_byte_off, n_genomes, nullptr, direct);
    if (rc) return rc;
    rc = sketch_from(ctx, prm, &ctx->scratch, d_out_images, ev);
    ctx->cur_ev = nullptr;
    return rc;
}

int lash_sketch_batch_async(lash_ctx *ctx, const lash_params *prm, const uint8_t *seq, const uint64_t *rec_off, uint64_t n_rec,
                            const uint64_t *genome_rec_off, uint32_t n_genomes, uint8_t *out_images)
{
    if (!ctx || !rec_off || !genome_rec_off || (n_genomes && !out_images)) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    for (uint64_t r = 0; r < n_rec; ++r)
        if (rec_off[r + 1] < rec_off[r]) return LASH_EINVAL;
    const uint64_t seq_bytes = rec_off[n_rec];
    if (seq_bytes && !seq) return LASH_EINVAL;
    std::vector<uint64_t> gbo(n_genomes + 1);
    for (uint32_t g = 0; g <= n_genomes; ++g) {
        if (genome_rec_off[g] > n_rec) return LASH_EINVAL;
        gbo[g] = rec_off[genome_rec_off[g]];
    }
    if (!ctx->h2d_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->h2d_stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
        for (auto &sl : ctx->slot)
            for (hipEvent_t *e : {&sl.h2d, &sl.kern, &sl.d2h}) HIPCHK(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    lash_ctx::AsyncSlot &sl = ctx->slot[ctx->slot_next++ & 1u];
    if (sl.busy) { HIPCHK(ctx, hipEventSynchronize(sl.d2h)); sl.busy = false; }   // the batch two calls ago has landed
    const size_t img_bytes = (size_t)n_genomes * image_bytes(ctx->layout, prm->algo, prm->p);
    auto grow = [&](DevBuf &b, size_t bytes) -> int {            // the slot is idle: no stream uses its buffers
        if (bytes <= b.cap) return LASH_OK;
        release(b);
        const size_t want = bytes + bytes / 8 + 256;
        HIPCHK(ctx, hipMalloc(&b.ptr, want));
        b.cap = want;
        return LASH_OK;
    };
    if ((rc = grow(sl.seq, seq_bytes + 64))) return rc;
    if ((rc = grow(sl.rec, (size_t)(n_rec + 1) * 8))) return rc;
    if ((rc = grow(sl.img, img_bytes + 64))) return rc;
    if (seq_bytes) HIPCHK(ctx, hipMemcpyAsync(sl.seq.ptr, seq, seq_bytes, hipMemcpyHostToDevice, ctx->h2d_stream));
    HIPCHK(ctx, hipMemcpyAsync(sl.rec.ptr, rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, ctx->h2d_stream));
    if ((prm->flags & LASH_F_ACCUMULATE) && img_bytes)
        HIPCHK(ctx, hipMemcpyAsync(sl.img.ptr, out_images, img_bytes, hipMemcpyHostToDevice, ctx->h2d_stream));
    HIPCHK(ctx, hipEventRecord(sl.h2d, ctx->h2d_stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, sl.h2d, 0));
    rc = lash_sketch_batch_device(ctx, prm, static_cast<const uint8_t *>(sl.seq.ptr), static_cast<const uint64_t *>(sl.rec.ptr), n_rec,
                                  genome_rec_off, gbo.data(), n_genomes, static_cast<uint8_t *>(sl.img.ptr));
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(sl.kern, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->d2h_stream, sl.kern, 0));
    if (img_bytes) HIPCHK(ctx, hipMemcpyAsync(out_images, sl.img.ptr, img_bytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    HIPCHK(ctx, hipEventRecord(sl.d2h, ctx->d2h_stream));
    sl.busy = true;
    return LASH_OK;
}

int lash_sketch_batch(lash_ctx *ctx, const lash_params *prm, const uint8_t *seq, const uint64_t *rec_off, uint64_t n_rec,
                      const uint64_t *genome_rec_off, uint32_t n_genomes, uint8_t *out_images)
{
    int rc = lash_sketch_batch_async(ctx, prm, seq, rec_off, n_rec, genome_rec_off, n_genomes, out_images);
    if (rc) return rc;
    if ((rc = lash_ctx_synchronize(ctx))) return rc;
    if (prm->algo == LASH_HLL && n_genomes && !(prm->flags & LASH_F_AMINO)) {
        // genomes with a register above 53 - p: their `sum` as the reference's incremental rule leaves it (hll_replay_sums)
        const std::vector<uint32_t> flagged = hll_flagged(ctx);
        if (!flagged.empty()) {
            const lash_ctx::AsyncSlot &sl = ctx->slot[(ctx->slot_next - 1u) & 1u];           // this call's device copies
            std::vector<uint32_t> left;
            rc = hll_replay_sums(ctx, prm, static_cast<const uint8_t *>(sl.seq.ptr), static_cast<const uint64_t *>(sl.rec.ptr), rec_off,
                                 genome_rec_off, static_cast<uint8_t *>(sl.img.ptr), out_images, flagged, left);
        }
    }
    return rc;
}

int lash_sketch_files_raw_device(lash_ctx *ctx, const lash_params *prm, const uint8_t *d_raw, const uint64_t *file_off,
                                 const uint8_t *file_fmt, uint32_t n_files, uint8_t *d_out_images)
{
    if (!ctx || (n_files && (!d_out_images || !file_off || !file_fmt))) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    if (prm->flags & LASH_F_AMINO) return LASH_EINVAL;                   // the device-side parse feeds the nucleotide pack stage only
    (void)hipSetDevice(ctx->device);
    if (ctx->raw_files_pending) {                                // flags of an earlier raw call nobody has looked at yet
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = read_format_errors(ctx))) return rc;
        if (!ctx->bad_files.empty()) return LASH_EFORMAT;
    }
    ctx->bad_files.clear();
    ctx->last_packed.clear();
    ctx->last_sole_only = false;
    ctx->last.calls += 1;
    if (n_files == 0) return LASH_OK;
    if ((rc = timing_begin(ctx))) return rc;
    EvSet *ev = ctx->cur_ev;
    rc = pack_into(ctx, &ctx->scratch, ctx->stream, ev, d_raw, d_raw + file_off[n_files], nullptr, 0, nullptr, file_off, n_files,
                   file_fmt);
    if (rc) return rc;
    rc = sketch_from(ctx, prm, &ctx->scratch, d_out_images, ev);
    ctx->cur_ev = nullptr;
    if (rc == LASH_OK) ctx->raw_files_pending = n_files;
    return rc;
}

uint32_t lash_ctx_format_errors(lash_ctx *ctx, uint32_t *file_index, uint32_t cap)
{
    if (!ctx) return 0;
    const uint32_t n = (uint32_t)ctx->bad_files.size();
    for (uint32_t i = 0; i < n && i < cap && file_index; ++i) file_index[i] = ctx->bad_files[i];
    return n;
}

uint64_t lash_fastq_valid_prefix(const uint8_t *buf, uint64_t n)
{
    if (!buf || n == 0) return 0;
    if (buf[0] != '@') return 0;
    return (uint64_t)parse_fastx_strict(buf, (size_t)n, nullptr, nullptr);
}

uint64_t lash_fastq_sanitize(uint8_t *buf, uint64_t n, int skip_bad)
{
    if (!buf || n == 0 || buf[0] != '@') return 0;
    std::vector<std::pair<size_t, size_t>> bad;
    parse_fastx_strict(buf, (size_t)n, nullptr, nullptr, skip_bad != 0, &bad);
    uint64_t changed = 0;
    for (const auto &b : bad) {
        if (b.second >= n) lash_fastq_neutralise_tail(buf + b.first, n - b.first);
        else {                                                     // becomes the head of the next record's header line
            buf[b.first] = '@';
            for (size_t i = b.first + 1; i < b.second; ++i) buf[i] = 'x';
        }
        changed += b.second - b.first;
    }
    return changed;
}

void lash_fastq_neutralise_tail(uint8_t *tail, uint64_t n)
{
    // a well-formed stand-in that contributes no base: ONE record with an empty sequence, "@xxx...\n\n+\n\n", or what fits of it
    if (!tail || n == 0) return;
    static const char end5[] = "\n\n+\n\n";
    tail[0] = '@';
    if (n >= 6) {
        for (uint64_t i = 1; i < n - 5; ++i) tail[i] = 'x';
        memcpy(tail + n - 5, end5, 5);
    } else {
        for (uint64_t i = 1; i < n; ++i) tail[i] = (uint8_t)end5[i - 1];
    }
}

int lash_sketch_files_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off,
                          const uint8_t *file_fmt, uint32_t n_files, uint8_t *out_images)
{
    return files_raw_staged(ctx, prm, raw, nullptr, file_off, file_fmt, n_files, out_images);
}

}  // extern "C"

// lash_sketch_files_raw; d_raw != NULL: the bytes of `raw` are already in device memory there (lash_sketch_records_raw: the record index
// keeps the copy it was made from), so nothing is staged and file_off may start anywhere in the buffer.  raw == NULL with d_raw: the bytes
// exist on the device only (lash_sketch_windows_raw: the rewritten windows); the rare file that is redone on the host is fetched from there
int lashi::files_raw_staged(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint8_t *d_raw, const uint64_t *file_off,
                            const uint8_t *file_fmt, uint32_t n_files, uint8_t *out_images)
{
    if (!ctx || !file_off || (n_files && (!out_images || !file_fmt))) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    const uint64_t bytes = file_off[n_files];
    if (bytes && !raw && (!d_raw || (prm->flags & LASH_F_AMINO))) return LASH_EINVAL;
    if (prm->flags & LASH_F_AMINO) {
        // protein FASTA / FASTQ: parsed here on the host with needletail's record rules, sketched by the record entry
        std::vector<uint8_t> seq;
        std::vector<uint64_t> rec_off(1, 0), goff(1, 0);
        for (uint32_t g = 0; g < n_files; ++g) {
            const uint8_t *f = raw + file_off[g];
            const size_t n = (size_t)(file_off[g + 1] - file_off[g]);
            if (n == 0 || (f[0] != '>' && f[0] != '@')) return LASH_EINVAL;
            parse_fastx_strict(f, n, &seq, &rec_off, ctx->layout.fastq_skip_bad != 0);
            goff.push_back(rec_off.size() - 1);
        }
        const uint8_t dummy = 0;
        return lash_sketch_batch(ctx, prm, seq.empty() ? &dummy : seq.data(), rec_off.data(), rec_off.size() - 1, goff.data(), n_files, out_images);
    }
    const size_t ib = image_bytes(ctx->layout, prm->algo, prm->p), img_bytes = (size_t)n_files * ib;
    if (!d_raw && (rc = reserve(ctx, ctx->st_seq, bytes + 64))) return rc;
    if ((rc = reserve(ctx, ctx->st_img, img_bytes + 64))) return rc;
    if (!d_raw && bytes) HIPCHK(ctx, hipMemcpyAsync(ctx->st_seq.ptr, raw, bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((prm->flags & LASH_F_ACCUMULATE) && img_bytes)
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_img.ptr, out_images, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = lash_sketch_files_raw_device(ctx, prm, d_raw ? d_raw : static_cast<const uint8_t *>(ctx->st_seq.ptr), file_off, file_fmt, n_files,
                                      static_cast<uint8_t *>(ctx->st_img.ptr));
    if (rc) return rc;
    // files whose FASTQ structure broke are re-done below from the caller's copy of the images (accumulate) or from scratch:
    // their device images are not copied back over out_images
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (const lash_packed *pk : ctx->last_packed)
        if ((rc = check_pack_flag(ctx, pk))) return rc;
    if ((rc = read_format_errors(ctx))) return rc;
    std::vector<uint32_t> bad = ctx->bad_files;
    const size_t n_malformed = bad.size();
    // HyperLogLog files with a register above 53 - p, taken NOW: the per-file redo calls below overwrite the device flags
    std::vector<uint32_t> corner;
    if (prm->algo == LASH_HLL) corner = hll_flagged(ctx);
    if (prm->algo == LASH_HLL && !(prm->flags & LASH_F_ACCUMULATE)) {
        // ... go the same way as the malformed ones — host parse, record entry — which replays their incremental `sum`
        // (hll_replay_sums): one file in ~10^4 at p = 14
        for (uint32_t g : corner)
            if (std::find(bad.begin(), bad.end(), g) == bad.end()) bad.push_back(g);
    }
    if (bad.empty()) {
        if (img_bytes) HIPCHK(ctx, hipMemcpy(out_images, ctx->st_img.ptr, img_bytes, hipMemcpyDeviceToHost));
        return LASH_OK;                                            // (an accumulating call's corner files stay flagged on the device)
    }
    std::vector<uint8_t> is_bad(n_files, 0);
    for (uint32_t g : bad) is_bad[g] = 1;
    for (uint32_t g = 0; g < n_files;) {                          // copy back the runs of good images
        if (is_bad[g]) { ++g; continue; }
        uint32_t e = g;
        while (e < n_files && !is_bad[e]) ++e;
        HIPCHK(ctx, hipMemcpy(out_images + (size_t)g * ib, static_cast<uint8_t *>(ctx->st_img.ptr) + (size_t)g * ib, (size_t)(e - g) * ib,
                              hipMemcpyDeviceToHost));
        g = e;
    }
    for (uint32_t g : bad) {                                       // exact reference semantics for the malformed ones
        std::vector<uint8_t> seq;
        std::vector<uint64_t> rec_off(1, 0);
        const size_t fb = (size_t)(file_off[g + 1] - file_off[g]);
        std::vector<uint8_t> fetched;
        if (!raw && fb) {
            fetched.resize(fb);
            HIPCHK(ctx, hipMemcpy(fetched.data(), d_raw + file_off[g], fb, hipMemcpyDeviceToHost));
        }
        parse_fastx_strict(raw ? raw + file_off[g] : fetched.data(), fb, &seq, &rec_off, ctx->layout.fastq_skip_bad != 0);
        const uint64_t goff[2] = {0, (uint64_t)rec_off.size() - 1};
        const uint8_t dummy = 0;
        rc = lash_sketch_batch(ctx, prm, seq.empty() ? &dummy : seq.data(), rec_off.data(), rec_off.size() - 1, goff, 1, out_images + (size_t)g * ib);
        if (rc) return rc;
    }
    bad.resize(n_malformed);
    ctx->bad_files = bad;                                          // still reported (the host may want to stop streaming this file)
    // Without LASH_F_ACCUMULATE the corner files have been redone exactly: nothing left to report.  An accumulating call redoes only the
    // malformed files (the registers already in the images are not the library's to replay): its other corner files stay reported
    // (the redo calls had wiped the device flags, and the list was cleared regardless)
    ctx->hll_flags_n = 0;
    ctx->hll_flags_on_host = true;
    ctx->hll_left.clear();
    if (prm->flags & LASH_F_ACCUMULATE)
        for (uint32_t g : corner)
            if (std::find(bad.begin(), bad.end(), g) == bad.end()) ctx->hll_left.push_back(g);
    return LASH_OK;
}

extern "C" {

int lash_synth_genomes_device(lash_ctx *ctx, uint64_t first_genome, uint32_t n_genomes, uint64_t n_bases, uint8_t *d_out)
{
    if (!ctx || (n_genomes && n_bases && !d_out)) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, launch_synth(first_genome, n_genomes, n_bases, d_out, ctx->stream));
    return LASH_OK;
}

}  // extern "C"

// ---- k-mer abundance filter (kmer_filter.hip; `lash sketch --min-count`) ------------------------------------------------------------

// Stages `raw` and packs it into the context's scratch batch; synchronizes.  Files whose FASTQ structure broke (ctx->bad_files) are packed a
// second time from a copy that lash_fastq_sanitize has cut down to the records needletail's iterator yields, so the counting pass and the
// filtered sketch see exactly the records lash_sketch_files_raw sketches for such a file.
static int filter_pack(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, const uint8_t *file_fmt, uint32_t n_files)
{
    int rc;
    const uint64_t bytes = file_off[n_files];
    if ((rc = reserve(ctx, ctx->st_seq, bytes + 64))) return rc;
    const uint8_t *d_raw = static_cast<const uint8_t *>(ctx->st_seq.ptr);
    std::vector<uint8_t> clean;
    std::vector<uint32_t> bad;
    for (int pass = 0; pass < 2; ++pass) {
        const uint8_t *src = pass ? clean.data() : raw;
        if (bytes) HIPCHK(ctx, hipMemcpyAsync(ctx->st_seq.ptr, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = pack_into(ctx, &ctx->scratch, ctx->stream, nullptr, d_raw, d_raw + bytes, nullptr, 0, nullptr, file_off, n_files, file_fmt))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = check_pack_flag(ctx, &ctx->scratch))) return rc;
        ctx->raw_files_pending = n_files;
        if ((rc = read_format_errors(ctx))) return rc;
        if (pass || ctx->bad_files.empty()) break;
        bad = ctx->bad_files;
        clean.assign(raw, raw + bytes);
        for (uint32_t g : bad)
            lash_fastq_sanitize(clean.data() + file_off[g], file_off[g + 1] - file_off[g], ctx->layout.fastq_skip_bad);
    }
    if (!bad.empty()) ctx->bad_files = bad;                          // still reported (lash_ctx_format_errors)
    return LASH_OK;
}

static KmerFilterArgs filter_args(const lash_ctx *ctx, const lash_params *prm, const lash_kmer_filter *f)
{
    const lash_packed &pk = ctx->scratch;
    KmerFilterArgs a{};
    a.words = static_cast<const uint32_t *>(pk.words.ptr);
    a.brk = static_cast<const uint32_t *>(pk.brk.ptr);
    a.genomes = pk.d_descs;
    a.nvalid = pk.d_nvalid;
    a.cell_word = f->d_cell_word;
    a.log2_cells = f->d_log2;
    a.cells = static_cast<uint32_t *>(f->cells.ptr);
    a.comp_mask = layout_dev(ctx->layout, prm->algo).comp_mask;
    a.n_genomes = pk.n_genomes;
    a.k = prm->k;
    return a;
}

static uint64_t longest_file(const uint64_t *file_off, uint32_t n_files)
{
    uint64_t m = 0;
    for (uint32_t g = 0; g < n_files; ++g) m = std::max(m, file_off[g + 1] - file_off[g]);
    return m;
}

static int filter_call_check(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off, const uint8_t *file_fmt,
                             uint32_t n_files, const lash_kmer_filter *f)
{
    if (!ctx || !f || !file_off || (n_files && !file_fmt)) return LASH_EINVAL;
    const int rc = lash_params_check(prm);
    if (rc) return rc;
    if ((prm->flags & LASH_F_AMINO) || n_files != f->n_files || f->device != ctx->device) return LASH_EINVAL;
    if (file_off[n_files] && !raw) return LASH_EINVAL;
    return LASH_OK;
}

extern "C" {

int lash_kmer_filter_create(lash_ctx *ctx, uint32_t n_files, const uint8_t *log2_cells, lash_kmer_filter **out)
{
    if (!ctx || !out || (n_files && !log2_cells)) return LASH_EINVAL;
    *out = nullptr;
    for (uint32_t g = 0; g < n_files; ++g)
        if (log2_cells[g] < 10 || log2_cells[g] > 36) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    lash_kmer_filter *f = new (std::nothrow) lash_kmer_filter();
    if (!f) return LASH_ENOMEM;
    f->device = ctx->device;
    f->n_files = n_files;
    f->log2_cells.assign(log2_cells, log2_cells + n_files);
    f->cell_word.assign((size_t)n_files + 1, 0);
    for (uint32_t g = 0; g < n_files; ++g) f->cell_word[g + 1] = f->cell_word[g] + (1ull << (log2_cells[g] - 2));
    auto run = [&]() -> int {
        int rc;
        if ((rc = reserve(ctx, f->cells, (size_t)f->cell_word[n_files] * 4))) return rc;
        if (f->cell_word[n_files]) HIPCHK(ctx, hipMemsetAsync(f->cells.ptr, 0, (size_t)f->cell_word[n_files] * 4, ctx->stream));
        std::vector<Section> sec = {{f->cell_word.data(), f->cell_word.size() * 8, 0}, {f->log2_cells.data(), f->log2_cells.size(), 0}};
        const size_t total = layout_sections(sec);
        if ((rc = reserve(ctx, f->tables, total))) return rc;
        if ((rc = upload_sections(ctx, f->tables.ptr, sec, total, ctx->stream))) return rc;
        f->d_cell_word = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(f->tables.ptr) + sec[0].off);
        f->d_log2 = static_cast<const uint8_t *>(f->tables.ptr) + sec[1].off;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return LASH_OK;
    };
    const int rc = run();
    if (rc) {
        (void)hipGetLastError();
        lash_kmer_filter_free(ctx, f);
        return rc;                                                   // (tables that do not fit: LASH_ENOMEM, from hipMalloc)
    }
    *out = f;
    return LASH_OK;
}

void lash_kmer_filter_free(lash_ctx *ctx, lash_kmer_filter *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    release(f->cells);
    release(f->tables);
    delete f;
}

int lash_kmer_filter_count_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off, const uint8_t *file_fmt,
                               uint32_t n_files, lash_kmer_filter *f)
{
    int rc = filter_call_check(ctx, prm, raw, file_off, file_fmt, n_files, f);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    ctx->bad_files.clear();
    if (n_files == 0) return LASH_OK;
    if ((rc = filter_pack(ctx, raw, file_off, file_fmt, n_files))) return rc;
    HIPCHK(ctx, launch_kmer_count(filter_args(ctx, prm, f), longest_file(file_off, n_files), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

int lash_kmer_filter_counts(lash_ctx *ctx, const lash_kmer_filter *f, uint32_t file, uint8_t *out)
{
    if (!ctx || !f || !out || file >= f->n_files || f->device != ctx->device) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // cell i is byte i & 3 of word i >> 2: on the (little-endian) host the words ARE the cells in order
    HIPCHK(ctx, hipMemcpy(out, static_cast<const uint32_t *>(f->cells.ptr) + f->cell_word[file], (size_t)1 << f->log2_cells[file], hipMemcpyDeviceToHost));
    return LASH_OK;
}

int lash_sketch_files_raw_filtered(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off, const uint8_t *file_fmt,
                                   uint32_t n_files, const lash_kmer_filter *f, uint32_t min_count, uint8_t *out_images)
{
    int rc = filter_call_check(ctx, prm, raw, file_off, file_fmt, n_files, f);
    if (rc) return rc;
    if (min_count < 1 || min_count > 255 || (n_files && !out_images)) return LASH_EINVAL;
    // the filtered launch exists for plans with a plain register table in LDS (hmh; hll p <= 15, ull p <= 14 by default)
    if (!sketch_plan_keeps(make_sketch_plan(prm->algo, prm->k, prm->p, rule_variant(ctx->layout, prm->algo, prm->flags)))) {
        ctx->err = "lash_sketch_files_raw_filtered: this sketch type / precision has no filtered launch (hmh, hll p <= 15, ull p <= 14)";
        return LASH_EINVAL;
    }
    (void)hipSetDevice(ctx->device);
    ctx->bad_files.clear();
    ctx->last_packed.clear();
    ctx->last_sole_only = false;
    ctx->last.calls += 1;
    if (n_files == 0) return LASH_OK;
    if ((rc = filter_pack(ctx, raw, file_off, file_fmt, n_files))) return rc;
    const std::vector<uint32_t> bad = ctx->bad_files;                // (sketch_from leaves them alone; kept across the launches anyway)
    const size_t img_bytes = (size_t)n_files * image_bytes(ctx->layout, prm->algo, prm->p);
    if ((rc = reserve(ctx, ctx->st_img, img_bytes + 64))) return rc;
    if ((rc = reserve(ctx, ctx->kf_keep, (size_t)ctx->scratch.total_brk * 4))) return rc;
    if ((prm->flags & LASH_F_ACCUMULATE) && img_bytes)
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_img.ptr, out_images, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    KmerFilterArgs ka = filter_args(ctx, prm, f);
    ka.keep = static_cast<uint32_t *>(ctx->kf_keep.ptr);
    ka.min_count = min_count;
    HIPCHK(ctx, launch_kmer_keep(ka, longest_file(file_off, n_files), ctx->stream));
    if ((rc = timing_begin(ctx))) return rc;
    lash_params fp = *prm;
    fp.flags |= LASH_F_NO_DIRECT | LASH_F_NO_SOLE;                   // always the pack-first route, every file on the sliced kernel
    rc = sketch_from(ctx, &fp, &ctx->scratch, static_cast<uint8_t *>(ctx->st_img.ptr), ctx->cur_ev, true, ka.keep);
    ctx->cur_ev = nullptr;
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (img_bytes) HIPCHK(ctx, hipMemcpy(out_images, ctx->st_img.ptr, img_bytes, hipMemcpyDeviceToHost));
    ctx->bad_files = bad;
    return LASH_OK;
}

}  // extern "C"
