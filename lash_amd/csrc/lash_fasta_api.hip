// lash_fasta_api.hip — the per-record entries of liblash_gfx950.so (include/lash_gfx950.h): lash_fasta_index[_device] and its accessors, the
// device-side record index of raw multi-FASTA bytes (fasta_index.hip), and lash_sketch_records_raw, which hands a range of that index
// to the raw-file route with records where it has files (`lash sketch --per-record`); lash_fasta_windows[_device], which rewrites the records
// of an index as fixed-length windows (fasta_windows.hip), and lash_sketch_windows_raw, which hands a range of those to the same route
// (`lash sketch --window`); lash_fasta_translate[_device], which writes the six reading frames of the records of an index as residues cut into
// segments (fasta_translate.hip), and lash_sketch_translated, which hands groups of those records to the amino-acid route (`lash sketch
// --translate`).  The windows and the translation both start from the sequence coordinates of fasta_coords.hip, kept in ctx->fc_scratch.
#include "lash_ctx.h"
#include "lash_internal.h"
#include "text_tiles.h"

struct lash_rec_index {
    int device = 0;
    uint32_t n = 0, n_files = 0;
    uint64_t total = 0;                          // bytes indexed == file_off[n_files]
    DevBuf start, id_len, file;                  // [n + 1] u64, [n] u32, [n] u32
    DevBuf raw;                                  // lash_fasta_index (host bytes): the device copy the index was made from, kept so that
    const uint8_t *h_raw = nullptr;              // lash_sketch_records_raw on the same host buffer does not send the bytes again
    mutable std::vector<uint64_t> h_start;       // host copy of start[], fetched by the first lash_sketch_records_raw
};

struct lash_win_index {
    int device = 0;
    uint64_t n = 0, window = 0, bytes = 0;       // windows; their length; size of buf == off[n]
    DevBuf record, begin, length, off;           // [n] u64 each, off [n + 1]: where every window's one-record FASTA file starts in buf
    DevBuf buf;                                  // the windows, each as ">\n" + its bases + "\n"
    mutable std::vector<uint64_t> h_off;         // host copy of off[], fetched by the first lash_sketch_windows_raw
};

struct lash_tr_index {
    int device = 0;
    uint32_t n = 0;                              // records of the index it was made from
    uint64_t bytes = 0, n_seg = 0;               // size of buf == out_base[n] == seg_off[n_seg]; segments == break bytes
    DevBuf buf;                                  // the frames of every record: residues, 'X', '*'
    DevBuf seg_off, rec_seg, out_base;           // [n_seg + 1], [n + 1], [n + 1] u64
    std::vector<uint64_t> h_rec_seg, h_out_base; // host copies: the groups of lash_sketch_translated are planned from them
};

// ---- what the entries below share ----------------------------------------------------------------------------------------------------
namespace {

int chk(lash_ctx *ctx, hipError_t e, const char *what)
{
    return e == hipSuccess ? LASH_OK : fail(ctx, e == hipErrorOutOfMemory ? LASH_ENOMEM : LASH_EHIP, what, e);
}

// memory that the result of a call owns (the context's own buffers grow through reserve())
int room(lash_ctx *ctx, DevBuf &b, size_t bytes)
{
    const int rc = chk(ctx, hipMalloc(&b.ptr, bytes), "hipMalloc");
    if (rc == LASH_OK) b.cap = bytes;
    return rc;
}

// the free path of the three indexes: kernels queued on the stream may still use the buffers, so it is drained before they go
void free_buffers(lash_ctx *ctx, std::initializer_list<DevBuf *> bufs)
{
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    }
    for (DevBuf *b : bufs) release(*b);
}

// one table of an index (made on `device`) to the host.  null_if_empty: a table of no bytes may go to a null pointer (the rule of the window
// accessors; the record and translate accessors refuse a null pointer whatever the size)
int copy_out(lash_ctx *ctx, int device, const DevBuf &b, void *dst, size_t bytes, bool null_if_empty)
{
    if (!ctx || ctx->device != device || (!dst && !(null_if_empty && bytes == 0))) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) HIPCHK(ctx, hipMemcpy(dst, b.ptr, bytes, hipMemcpyDeviceToHost));
    return LASH_OK;
}

// the index belongs to this context and was made from this buffer.  whole: the call reads all of the buffer, so raw may be null only if
// there is nothing to read
int index_guard(const lash_ctx *ctx, const lash_rec_index *ix, const void *raw, const uint64_t *file_off, uint32_t n_files, bool whole)
{
    if (!ctx || !ix || !file_off) return LASH_EINVAL;
    if (ix->device != ctx->device || n_files != ix->n_files || file_off[n_files] != ix->total) return LASH_EINVAL;   // another context or buffer
    return whole && ix->total && !raw ? LASH_EINVAL : LASH_OK;
}

// the bytes the index was made from, on the device: the index's own copy when raw is the host buffer it was made from, else raw staged into
// ctx->st_seq (*staged).  The staging buffer is the context's: this relies on the caller draining the stream before it returns, so that the
// next call may reuse the buffer.  lash_fasta_windows does so explicitly; lash_fasta_translate_device has drained the stream on every exit.
int index_device_bytes(lash_ctx *ctx, const lash_rec_index *ix, const uint8_t *raw, const uint8_t **d_raw, bool *staged)
{
    *staged = !(ix->raw.ptr && ix->h_raw == raw);
    *d_raw = static_cast<const uint8_t *>(ix->raw.ptr);
    if (!*staged) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    const int rc = reserve(ctx, ctx->st_seq, ix->total + 64);
    if (rc) return rc;
    *d_raw = static_cast<const uint8_t *>(ctx->st_seq.ptr);
    return ix->total ? chk(ctx, hipMemcpyAsync(ctx->st_seq.ptr, raw, ix->total, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") : LASH_OK;
}

uint32_t tiles_of(uint64_t bytes) { return (uint32_t)((bytes + TEXT_TILE - 1) / TEXT_TILE); }

}  // namespace

// Errors after work has been queued: the three _device entries below leave through a done() of their own, which drains the stream before the
// half-built index and the call's other memory are released.  A plain return stands only where nothing is queued: before the first launch and
// right after a drain.

extern "C" {

void lash_rec_index_free(lash_ctx *ctx, lash_rec_index *ix)
{
    if (!ix) return;
    free_buffers(ctx, {&ix->start, &ix->id_len, &ix->file, &ix->raw});
    delete ix;
}

int lash_fasta_index_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, lash_rec_index **out)
{
    if (!ctx || !out || !file_off || file_off[0] != 0) return LASH_EINVAL;
    *out = nullptr;
    for (uint32_t g = 0; g < n_files; ++g)
        if (file_off[g + 1] < file_off[g]) return LASH_EINVAL;
    const uint64_t total = file_off[n_files];
    if (total && !d_raw) return LASH_EINVAL;
    if (total >= (1ull << 33)) return LASH_ELIMIT;                 // record numbers are 32 bits wide
    (void)hipSetDevice(ctx->device);
    const uint32_t n_tiles = tiles_of(total);
    int rc;
    if ((rc = reserve(ctx, ctx->fa_off, (size_t)(n_files + 1) * 8))) return rc;
    if ((rc = reserve(ctx, ctx->fa_scratch, fasta_index_scratch_bytes(n_tiles)))) return rc;
    if ((rc = upload(ctx, ctx->fa_off.ptr, file_off, (size_t)(n_files + 1) * 8))) return rc;
    const uint64_t *d_off = static_cast<const uint64_t *>(ctx->fa_off.ptr);
    uint8_t *scratch = static_cast<uint8_t *>(ctx->fa_scratch.ptr);
    lash_rec_index *ix = nullptr;
    auto done = [&](int code) -> int {
        if (code != LASH_OK) { (void)hipStreamSynchronize(ctx->stream); lash_rec_index_free(ctx, ix); }
        return code;
    };
    const uint32_t *d_two = nullptr;
    uint32_t two[2] = {0, 0};
    if ((rc = chk(ctx, launch_fasta_mark(d_raw, total, d_off, n_files, n_tiles, scratch, &d_two, ctx->stream), "launch_fasta_mark")) ||
        (rc = chk(ctx, hipMemcpyAsync(two, d_two, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")))
        return done(rc);
    if (two[1]) { ctx->err = "lash_fasta_index: a file does not begin with '>' (FASTA only)"; return LASH_EINVAL; }
    if (!(ix = new (std::nothrow) lash_rec_index())) return LASH_ENOMEM;
    ix->device = ctx->device;
    ix->n = two[0];
    ix->n_files = n_files;
    ix->total = total;
    if ((rc = room(ctx, ix->start, ((size_t)ix->n + 1) * 8)) || (rc = room(ctx, ix->id_len, ((size_t)ix->n + 1) * 4)) ||
        (rc = room(ctx, ix->file, ((size_t)ix->n + 1) * 4)) ||
        (rc = chk(ctx, launch_fasta_write(d_raw, total, d_off, n_files, n_tiles, scratch, ix->n, static_cast<uint64_t *>(ix->start.ptr),
                                          static_cast<uint32_t *>(ix->file.ptr), static_cast<uint32_t *>(ix->id_len.ptr), ctx->stream),
                  "launch_fasta_write")))
        return done(rc);
    *out = ix;
    return LASH_OK;
}

int lash_fasta_index(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, lash_rec_index **out)
{
    if (!ctx || !out || !file_off) return LASH_EINVAL;
    *out = nullptr;
    const uint64_t total = file_off[n_files];
    if (total && !raw) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    DevBuf d{};                                                   // owned by the index from here on: one copy of the bytes per batch, not two
    int rc = room(ctx, d, total + 64);
    if (rc) return rc;
    if (total) rc = chk(ctx, hipMemcpyAsync(d.ptr, raw, total, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    if (rc == LASH_OK) rc = lash_fasta_index_device(ctx, static_cast<const uint8_t *>(d.ptr), file_off, n_files, out);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); release(d); return rc; }
    (*out)->raw = d;
    (*out)->h_raw = raw;
    return LASH_OK;
}

uint64_t lash_rec_index_n_records(const lash_rec_index *ix) { return ix ? ix->n : 0; }
int lash_rec_index_start(lash_ctx *ctx, const lash_rec_index *ix, uint64_t *out) { return ix ? copy_out(ctx, ix->device, ix->start, out, ((size_t)ix->n + 1) * 8, false) : LASH_EINVAL; }
int lash_rec_index_id_len(lash_ctx *ctx, const lash_rec_index *ix, uint32_t *out) { return ix ? copy_out(ctx, ix->device, ix->id_len, out, (size_t)ix->n * 4, false) : LASH_EINVAL; }
int lash_rec_index_file(lash_ctx *ctx, const lash_rec_index *ix, uint32_t *out) { return ix ? copy_out(ctx, ix->device, ix->file, out, (size_t)ix->n * 4, false) : LASH_EINVAL; }

int lash_sketch_records_raw(lash_ctx *ctx, const lash_params *prm, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files,
                            const lash_rec_index *ix, uint64_t r0, uint64_t r1, uint8_t *out_images)
{
    int rc = index_guard(ctx, ix, raw, file_off, n_files, false);
    if (rc) return rc;
    if (r0 > r1 || r1 > ix->n || (r1 > r0 && (!raw || !out_images))) return LASH_EINVAL;
    if ((rc = lash_params_check(prm))) return rc;
    if (prm->flags & LASH_F_AMINO) return LASH_EINVAL;
    if (ix->h_start.empty()) {
        ix->h_start.resize((size_t)ix->n + 1);
        if ((rc = lash_rec_index_start(ctx, ix, ix->h_start.data()))) { ix->h_start.clear(); return rc; }
    }
    // records [r0, r1) as the files of one raw call: a FASTA record is a well-formed FASTA file, and consecutive records are contiguous
    // (a file ends where the next one's first record starts)
    const uint32_t n = (uint32_t)(r1 - r0);
    const std::vector<uint8_t> fmt(n, (uint8_t)LASH_FMT_FASTA);
    if (ix->raw.ptr && ix->h_raw == raw)                           // the index holds these bytes on the device: offsets as they are
        return files_raw_staged(ctx, prm, raw, static_cast<const uint8_t *>(ix->raw.ptr), ix->h_start.data() + r0, fmt.data(), n, out_images);
    std::vector<uint64_t> off((size_t)n + 1);
    for (uint32_t i = 0; i <= n; ++i) off[i] = ix->h_start[r0 + i] - ix->h_start[r0];
    return lash_sketch_files_raw(ctx, prm, raw + ix->h_start[r0], off.data(), fmt.data(), n, out_images);
}

void lash_win_index_free(lash_ctx *ctx, lash_win_index *wi)
{
    if (!wi) return;
    free_buffers(ctx, {&wi->record, &wi->begin, &wi->length, &wi->off, &wi->buf});
    delete wi;
}

int lash_fasta_windows_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *ix,
                              uint64_t window, lash_win_index **out)
{
    if (!out || window == 0) return LASH_EINVAL;
    *out = nullptr;
    int rc = index_guard(ctx, ix, d_raw, file_off, n_files, true);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    const uint32_t n_tiles = tiles_of(ix->total);
    if ((rc = reserve(ctx, ctx->fc_scratch, fasta_windows_scratch_bytes(n_tiles, ix->n)))) return rc;
    uint8_t *scratch = static_cast<uint8_t *>(ctx->fc_scratch.ptr);
    const uint64_t *d_start = static_cast<const uint64_t *>(ix->start.ptr), *d_s = nullptr, *d_n = nullptr;
    lash_win_index *wi = nullptr;
    auto done = [&](int code) -> int {
        if (code != LASH_OK) { (void)hipStreamSynchronize(ctx->stream); lash_win_index_free(ctx, wi); }
        return code;
    };
    uint64_t seq_bytes = 0, n_win = 0;
    if ((rc = chk(ctx, launch_fasta_windows_count(d_raw, ix->total, d_start, ix->n, n_tiles, window, scratch, &d_s, &d_n, ctx->stream),
                  "launch_fasta_windows_count")) ||
        (rc = chk(ctx, hipMemcpyAsync(&seq_bytes, d_s, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipMemcpyAsync(&n_win, d_n, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")))
        return done(rc);
    if (n_win > 0xFFFFFFFFull) return LASH_ELIMIT;                 // window numbers are the raw-file route's file numbers: 32 bits
    if (!(wi = new (std::nothrow) lash_win_index())) return LASH_ENOMEM;
    wi->device = ctx->device;
    wi->n = n_win;
    wi->window = window;
    wi->bytes = seq_bytes + 3 * n_win;
    const size_t tab = ((size_t)n_win + 1) * 8;
    if ((rc = room(ctx, wi->record, tab)) || (rc = room(ctx, wi->begin, tab)) || (rc = room(ctx, wi->length, tab)) || (rc = room(ctx, wi->off, tab)) ||
        (rc = room(ctx, wi->buf, (size_t)wi->bytes + 64)) ||
        (rc = chk(ctx, launch_fasta_windows_write(d_raw, ix->total, d_start, ix->n, n_tiles, window, scratch, n_win,
                                                  static_cast<uint64_t *>(wi->record.ptr), static_cast<uint64_t *>(wi->begin.ptr),
                                                  static_cast<uint64_t *>(wi->length.ptr), static_cast<uint64_t *>(wi->off.ptr),
                                                  static_cast<uint8_t *>(wi->buf.ptr), ctx->stream), "launch_fasta_windows_write")))
        return done(rc);
    *out = wi;
    return LASH_OK;
}

int lash_fasta_windows(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *ix,
                       uint64_t window, lash_win_index **out)
{
    if (!out || window == 0) return LASH_EINVAL;
    *out = nullptr;
    int rc = index_guard(ctx, ix, raw, file_off, n_files, true);
    if (rc) return rc;
    const uint8_t *d_raw = nullptr;
    bool staged = false;
    if ((rc = index_device_bytes(ctx, ix, raw, &d_raw, &staged))) return rc;
    rc = lash_fasta_windows_device(ctx, d_raw, file_off, n_files, ix, window, out);
    // the staging buffer is the context's: done with it before anyone reuses it.  A stream that fails here leaves no index behind
    if (rc == LASH_OK && staged && (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) {
        lash_win_index_free(ctx, *out);
        *out = nullptr;
    }
    return rc;
}

uint64_t lash_win_index_n_windows(const lash_win_index *wi) { return wi ? wi->n : 0; }
uint64_t lash_win_index_bytes(const lash_win_index *wi) { return wi ? wi->bytes : 0; }
const uint8_t *lash_win_index_buffer_device(const lash_win_index *wi) { return wi ? static_cast<const uint8_t *>(wi->buf.ptr) : nullptr; }
int lash_win_index_record(lash_ctx *ctx, const lash_win_index *wi, uint64_t *out) { return wi ? copy_out(ctx, wi->device, wi->record, out, (size_t)wi->n * 8, true) : LASH_EINVAL; }
int lash_win_index_begin(lash_ctx *ctx, const lash_win_index *wi, uint64_t *out) { return wi ? copy_out(ctx, wi->device, wi->begin, out, (size_t)wi->n * 8, true) : LASH_EINVAL; }
int lash_win_index_length(lash_ctx *ctx, const lash_win_index *wi, uint64_t *out) { return wi ? copy_out(ctx, wi->device, wi->length, out, (size_t)wi->n * 8, true) : LASH_EINVAL; }
int lash_win_index_offset(lash_ctx *ctx, const lash_win_index *wi, uint64_t *out) { return wi ? copy_out(ctx, wi->device, wi->off, out, ((size_t)wi->n + 1) * 8, true) : LASH_EINVAL; }

int lash_sketch_windows_raw(lash_ctx *ctx, const lash_params *prm, const lash_win_index *wi, uint64_t w0, uint64_t w1, uint8_t *out_images)
{
    if (!ctx || !wi || w0 > w1 || w1 > wi->n || (w1 > w0 && !out_images) || wi->device != ctx->device) return LASH_EINVAL;
    int rc = lash_params_check(prm);
    if (rc) return rc;
    if (prm->flags & LASH_F_AMINO) return LASH_EINVAL;
    if (wi->h_off.empty()) {
        wi->h_off.resize((size_t)wi->n + 1);
        if ((rc = lash_win_index_offset(ctx, wi, wi->h_off.data()))) { wi->h_off.clear(); return rc; }
    }
    // windows [w0, w1) as the files of one raw call: each is a well-formed one-record FASTA file, and they lie back to back in buf
    const uint32_t n = (uint32_t)(w1 - w0);
    const std::vector<uint8_t> fmt(n, (uint8_t)LASH_FMT_FASTA);
    return files_raw_staged(ctx, prm, nullptr, static_cast<const uint8_t *>(wi->buf.ptr), wi->h_off.data() + w0, fmt.data(), n, out_images);
}

void lash_tr_index_free(lash_ctx *ctx, lash_tr_index *ti)
{
    if (!ti) return;
    free_buffers(ctx, {&ti->buf, &ti->seg_off, &ti->rec_seg, &ti->out_base});
    delete ti;
}

int lash_fasta_translate_device(lash_ctx *ctx, const uint8_t *d_raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *ix,
                                lash_tr_index **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    int rc = index_guard(ctx, ix, d_raw, file_off, n_files, true);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    const uint32_t n_tiles = tiles_of(ix->total);
    if ((rc = reserve(ctx, ctx->fc_scratch, fasta_coords_scratch_bytes(n_tiles, ix->n)))) return rc;
    uint8_t *scratch = static_cast<uint8_t *>(ctx->fc_scratch.ptr);
    const uint64_t *d_start = static_cast<const uint64_t *>(ix->start.ptr);
    lash_tr_index *ti = new (std::nothrow) lash_tr_index();
    if (!ti) return LASH_ENOMEM;
    ti->device = ctx->device;
    ti->n = ix->n;
    DevBuf tile_cnt{};
    // (a call that succeeds has drained the stream too: its last step reads rec_seg back)
    auto done = [&](int code) -> int {
        if (code != LASH_OK) { (void)hipStreamSynchronize(ctx->stream); lash_tr_index_free(ctx, ti); }
        release(tile_cnt);
        return code;
    };
    const size_t tab = ((size_t)ix->n + 1) * 8;
    if ((rc = room(ctx, ti->out_base, tab)) || (rc = room(ctx, ti->rec_seg, tab))) return done(rc);
    uint64_t *d_out_base = static_cast<uint64_t *>(ti->out_base.ptr);
    ti->h_out_base.resize((size_t)ix->n + 1);
    if ((rc = chk(ctx, launch_fasta_translate_sizes(d_raw, ix->total, d_start, ix->n, n_tiles, scratch, d_out_base, ctx->stream),
                  "launch_fasta_translate_sizes")) ||
        (rc = chk(ctx, hipMemcpyAsync(ti->h_out_base.data(), d_out_base, tab, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")))
        return done(rc);
    ti->bytes = ti->h_out_base[ix->n];
    const size_t n_out_tiles = tiles_of(ti->bytes);
    if ((rc = room(ctx, ti->buf, (size_t)ti->bytes + 64)) || (rc = room(ctx, tile_cnt, (n_out_tiles + 2) * 8))) return done(rc);
    uint8_t *d_buf = static_cast<uint8_t *>(ti->buf.ptr);
    uint64_t *d_tile = static_cast<uint64_t *>(tile_cnt.ptr);
    if ((rc = chk(ctx, hipMemsetAsync(d_buf + ti->bytes, 0, 64, ctx->stream), "hipMemsetAsync")) ||     // (the slack lanes of the sketch kernel may load)
        (rc = chk(ctx, launch_fasta_translate_write(d_raw, ix->total, d_start, ix->n, n_tiles, scratch, d_out_base, ti->bytes, d_buf, d_tile, ctx->stream),
                  "launch_fasta_translate_write")) ||
        (rc = chk(ctx, hipMemcpyAsync(&ti->n_seg, d_tile + n_out_tiles, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")))
        return done(rc);
    if ((rc = room(ctx, ti->seg_off, ((size_t)ti->n_seg + 1) * 8))) return done(rc);
    ti->h_rec_seg.resize((size_t)ix->n + 1);
    if ((rc = chk(ctx, launch_fasta_translate_segments(d_buf, ti->bytes, d_tile, d_out_base, ix->n, ti->n_seg, static_cast<uint64_t *>(ti->seg_off.ptr),
                                                       static_cast<uint64_t *>(ti->rec_seg.ptr), ctx->stream), "launch_fasta_translate_segments")) ||
        (rc = chk(ctx, hipMemcpyAsync(ti->h_rec_seg.data(), ti->rec_seg.ptr, tab, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) ||
        (rc = chk(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")))
        return done(rc);
    *out = ti;
    return done(LASH_OK);
}

int lash_fasta_translate(lash_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, uint32_t n_files, const lash_rec_index *ix, lash_tr_index **out)
{
    if (!out) return LASH_EINVAL;
    *out = nullptr;
    int rc = index_guard(ctx, ix, raw, file_off, n_files, true);
    if (rc) return rc;
    const uint8_t *d_raw = nullptr;
    bool staged = false;
    if ((rc = index_device_bytes(ctx, ix, raw, &d_raw, &staged))) return rc;
    return lash_fasta_translate_device(ctx, d_raw, file_off, n_files, ix, out);      // (it drains the stream: the staging buffer is free again)
}

uint64_t lash_tr_index_n_segments(const lash_tr_index *ti) { return ti ? ti->n_seg : 0; }
uint64_t lash_tr_index_bytes(const lash_tr_index *ti) { return ti ? ti->bytes : 0; }
const uint8_t *lash_tr_index_buffer_device(const lash_tr_index *ti) { return ti ? static_cast<const uint8_t *>(ti->buf.ptr) : nullptr; }
int lash_tr_index_seg_off(lash_ctx *ctx, const lash_tr_index *ti, uint64_t *out) { return ti ? copy_out(ctx, ti->device, ti->seg_off, out, ((size_t)ti->n_seg + 1) * 8, false) : LASH_EINVAL; }
int lash_tr_index_rec_seg(lash_ctx *ctx, const lash_tr_index *ti, uint64_t *out) { return ti ? copy_out(ctx, ti->device, ti->rec_seg, out, ((size_t)ti->n + 1) * 8, false) : LASH_EINVAL; }

int lash_sketch_translated(lash_ctx *ctx, const lash_params *prm, const lash_tr_index *ti, const uint64_t *group_rec_off, uint32_t n_groups,
                           uint8_t *out_images)
{
    if (!ctx || !prm || !ti || !group_rec_off || (n_groups && !out_images) || ti->device != ctx->device) return LASH_EINVAL;
    lash_params p = *prm;
    p.flags |= LASH_F_AMINO;
    int rc = lash_params_check(&p);                                // k 1..12 among the rest
    if (rc) return rc;
    // group g = records [group_rec_off[g], group_rec_off[g + 1]): its segments and bytes are contiguous, a record starts at a segment boundary
    std::vector<uint64_t> gseg((size_t)n_groups + 1), gbyte((size_t)n_groups + 1);
    for (uint32_t g = 0; g <= n_groups; ++g) {
        if (group_rec_off[g] > ti->n || (g && group_rec_off[g] < group_rec_off[g - 1])) return LASH_EINVAL;
        gseg[g] = ti->h_rec_seg[group_rec_off[g]];
        gbyte[g] = ti->h_out_base[group_rec_off[g]];
        if (g && gseg[g] - gseg[g - 1] > 0xFFFFFFFFull) return LASH_ELIMIT;
    }
    if (n_groups == 0) return LASH_OK;
    (void)hipSetDevice(ctx->device);
    const size_t img_bytes = (size_t)n_groups * image_bytes(ctx->layout, p.algo, p.p);
    if ((rc = reserve(ctx, ctx->st_img, img_bytes + 64))) return rc;
    if (p.flags & LASH_F_ACCUMULATE) HIPCHK(ctx, hipMemcpyAsync(ctx->st_img.ptr, out_images, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = lash_sketch_batch_device(ctx, &p, static_cast<const uint8_t *>(ti->buf.ptr), static_cast<const uint64_t *>(ti->seg_off.ptr), ti->n_seg, gseg.data(),
                                  gbyte.data(), n_groups, static_cast<uint8_t *>(ctx->st_img.ptr));
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_images, ctx->st_img.ptr, img_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LASH_OK;
}

}  // extern "C"
