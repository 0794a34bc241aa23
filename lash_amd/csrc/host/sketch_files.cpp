#include "sketch_files.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../../../include/lash_gfx950.h"
#include "batch_queue.hpp"
#include "chunk_reader.hpp"
#include "fastx.hpp"
#include "json_out.hpp"
#include "zstd_dl.hpp"

namespace lashhost {

std::string layout_from_option(const std::string &spec, lash_layout &out)
{
    const char *env = getenv("LASH_LAYOUT");
    const std::string text = !spec.empty() ? spec : (env ? env : "");
    if (lash_layout_parse(text.c_str(), &out) != LASH_OK)
        return "bad layout '" + text + "' (codes=ACGT,kmer=msb|lsb,hmh_x=high|low,hmh_reg=le|be,hll_bucket=low|high,fastq_err=stop|skip,"
               "hmh_hdr=,hll_hdr=azspl,ull_hdr=l)";
    return "";
}

std::string read_list_file(const std::string &path, std::vector<std::string> &files)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) return "cannot open list file " + path;
    std::string line;
    files.clear();
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();       // BufRead::lines strips "\r\n" too
        bool blank = true;
        for (unsigned char c : line)
            if (!(c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r')) { blank = false; break; }
        if (!blank) files.push_back(line);                                // kept verbatim (main.rs:204-206)
    }
    return "";
}

std::string write_parameters_json(const std::string &output_name, const std::string &algorithm, int k, int precision,
                                  uint64_t seed, bool amino)
{
    std::map<std::string, std::string> kv;
    kv["k"] = std::to_string(k);
    kv["algorithm"] = algorithm;
    kv["seed"] = std::to_string(seed);
    kv["molecule"] = amino ? "amino_acid" : "nucleotide";                 // main.rs:248-252 (the reference hard-wires aa = false, main.rs:198)
    if (algorithm == "ull" || algorithm == "hll") kv["precision"] = std::to_string(precision);
    std::ofstream out(output_name + "_parameters.json", std::ios::binary);
    if (!out) return "cannot create " + output_name + "_parameters.json";
    out << json_pretty_string_object(kv);
    return out.good() ? "" : "write failed";
}

namespace {

struct FileSlot {
    bool compressed = false, sized = false, big = false;
    uint64_t size = 0;
    std::vector<uint8_t> inflated;        // compressed inputs only, until placed
    std::string err;
};

// --per-record: bytes of images one sub-call may produce, and a batch may hold unwritten (8 192 HyperMinHash images)
constexpr size_t kRecordImageCap = 256u << 20;

std::unique_ptr<PinnedBuf> new_pinned() { return std::unique_ptr<PinnedBuf>(new PinnedBuf(lash_host_alloc_pinned, lash_host_free_pinned)); }

std::string gpu_error(lash_ctx *ctx, int rc) { return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx); }

// A HyperLogLog register above 53 - p: the image's `sum` field is the exact sum, the reference's incrementally rounded one may differ
// in its last bits (include/lash_gfx950.h: lash_ctx_hll_inexact_sums).  `what` names the file, record or window; `why` what failed.
void hll_note(const std::string &what, const std::string &why = "")
{
    fprintf(stderr, "note: %s: a HyperLogLog register exceeds 53 - p%s; the header's sum field is the exact sum and may differ from lash's "
                    "incrementally rounded value in its last bits\n", what.c_str(), why.c_str());
}

// that note for every sketch of the last call (n of them) that the library could not replay; what(i) names sketch i
void hll_notes_of_last_call(lash_ctx *ctx, uint32_t n, const std::function<std::string(uint32_t)> &what)
{
    std::vector<uint32_t> idx(n);
    const uint32_t nc = lash_ctx_hll_inexact_sums(ctx, idx.data(), n);
    for (uint32_t i = 0; i < nc && i < n; ++i) hll_note(what(idx[i]));
}

// simple worker pool
class Pool {
public:
    explicit Pool(int n)
    {
        for (int i = 0; i < n; ++i)
            th_.emplace_back([this] {
                for (;;) {
                    std::function<void()> f;
                    {
                        std::unique_lock<std::mutex> lk(mu_);
                        cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                        if (q_.empty()) return;
                        f = std::move(q_.front());
                        q_.pop_front();
                    }
                    f();
                }
            });
    }
    void submit(std::function<void()> f)
    {
        std::lock_guard<std::mutex> lk(mu_);
        q_.push_back(std::move(f));
        cv_.notify_one();
    }
    ~Pool()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
private:
    std::vector<std::thread> th_;
    std::deque<std::function<void()>> q_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool stop_ = false;
};

bool peek_compressed(const std::string &path, uint64_t &size, std::string &err)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) { err = "Invalid input file: cannot open " + path; return false; }
    size = (uint64_t)st.st_size;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { err = "Invalid input file: cannot open " + path; return false; }
    unsigned char m[6] = {0, 0, 0, 0, 0, 0};
    size_t got = fread(m, 1, 6, f);
    fclose(f);
    if (got >= 2 && m[0] == 0x1f && m[1] == 0x8b) return true;
    if (got >= 4 && m[0] == 0x28 && m[1] == 0xb5 && m[2] == 0x2f && m[3] == 0xfd) return true;
    if (got >= 3 && m[0] == 'B' && m[1] == 'Z' && m[2] == 'h') return true;
    if (got >= 6 && m[0] == 0xfd && m[1] == '7' && m[2] == 'z' && m[3] == 'X' && m[4] == 'Z' && m[5] == 0) return true;
    return false;
}

std::string read_exact(const std::string &path, uint8_t *dst, uint64_t size)
{
    int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return "Invalid input file: cannot open " + path;
    uint64_t done = 0;
    while (done < size) {
        ssize_t n = pread(fd, dst + done, (size_t)std::min<uint64_t>(size - done, 1u << 30), (off_t)done);
        if (n <= 0) { close(fd); return "Invalid input file: short read on " + path; }
        done += (uint64_t)n;
    }
    close(fd);
    return "";
}

// Two pinned chunk buffers: this thread fills chunk n+1 (inflate wait + copy out of the members + finding the cut)
// while a second thread has the library sketch chunk n (H2D copy + kernels; the only user of `ctx` meanwhile).
std::string stream_big_file(lash_ctx *ctx, const lash_params &prm0, const std::string &path, uint64_t chunk_bytes,
                            PinnedBuf &buf0, PinnedBuf &buf1, uint8_t *image, uint64_t &bytes_seen, int threads)
{
    // (--aa: a protein record is never cut, the carried line is made of bases; threads: a multi-member .gz inflates in parallel, pgzip.hpp)
    ChunkReader rd(path, chunk_bytes, threads, (prm0.flags & LASH_F_AMINO) ? CutRule::between_records : CutRule::carry,
                   "a protein record larger than a --stream-mb chunk: " + path);
    std::string err = rd.open();
    if (!err.empty()) return err;
    if (!buf0.reserve(chunk_bytes + 64) || !buf1.reserve(chunk_bytes + 64)) return "out of pinned host memory";
    PinnedBuf *bufs[2] = {&buf0, &buf1};

    // ---- the sketching side ----
    struct Job { int b; size_t cut; int fmt; };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> jobs;
    bool busy[2] = {false, false}, no_more = false, halt = false, corner_noted = false;
    // HyperLogLog: the image before each chunk and the carried incremental `sum` (lash_hll_replay_streamed_chunk, round 5: a streamed
    // file's header then equals the reference's, which reads the whole file into one sketch in order, utils.rs:457-505)
    std::vector<uint8_t> image_before;
    double hll_carry[2] = {0.0, 0.0};
    int hll_have_carry = 0;
    lash_layout lay0;
    (void)lash_ctx_get_layout(ctx, &lay0);
    const bool skip_bad = lay0.fastq_skip_bad != 0;           // layout switch U6: malformed records are dropped, the reading goes on
    std::string gpu_err;
    uint64_t calls = 0;
    double t_gpu = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); };
    std::thread sketcher([&]() {
        for (;;) {
            Job jb;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !jobs.empty() || no_more; });
                if (jobs.empty()) return;
                jb = jobs.front();
                jobs.pop_front();
            }
            bool stop = false, skip;
            std::string e;
            { std::lock_guard<std::mutex> lk(mu); skip = halt; }
            if (!skip && jb.cut) {
                const auto t0 = now();
                lash_params prm = prm0;
                if (calls) prm.flags |= LASH_F_ACCUMULATE;
                const uint64_t off[2] = {0, (uint64_t)jb.cut};
                const uint8_t f = (uint8_t)jb.fmt;
                const bool hll_nt = prm.algo == LASH_HLL && !(prm.flags & LASH_F_AMINO);
                if (hll_nt) {                                     // (the first chunk starts from the empty sketch: every register 0)
                    image_before.assign(lash_layout_image_bytes(&lay0, LASH_HLL, prm.p), 0);
                    if (calls) memcpy(image_before.data(), image, image_before.size());
                }
                const int rc = lash_sketch_files_raw(ctx, &prm, bufs[jb.b]->p, off, &f, 1, image);
                if (rc != LASH_OK) e = gpu_error(ctx, rc);
                else {
                    ++calls;
                    if (hll_nt) {
                        // a register above 53 - p: this chunk's part of the incremental sum is replayed, later chunks carry it on
                        const int rr = lash_hll_replay_streamed_chunk(ctx, &prm0, bufs[jb.b]->p, (uint64_t)jb.cut, jb.fmt, image_before.data(), image,
                                                                      hll_carry, &hll_have_carry);
                        if (rr != LASH_OK && !corner_noted) hll_note(path, std::string(" and the replay of the streamed chunk failed (") + lash_strerror(rr) + ")");
                        if (rr != LASH_OK) corner_noted = true;
                    }
                    // a malformed FASTQ record ends needletail's iteration (utils.rs:457): the library kept this chunk's
                    // records before it; nothing after it belongs to the sketch
                    if (lash_ctx_format_errors(ctx, nullptr, 0) != 0 && !skip_bad) stop = true;
                }
                t_gpu += since(t0);
            }
            std::lock_guard<std::mutex> lk(mu);
            if (!e.empty() && gpu_err.empty()) gpu_err = e;
            if (stop || !e.empty()) halt = true;
            busy[jb.b] = false;
            cv.notify_all();
        }
    });

    // ---- the reading side ----
    int cur = 0;
    size_t have = 0;                                      // bytes at the front of the current buffer carried from the previous chunk
    // LASH_CLI_TIMING: where a streamed file's wall time goes (read = inflate wait + copy out of the members; check; waiting
    // for the sketching side; its own time runs concurrently)
    const bool timing = getenv("LASH_CLI_TIMING") != nullptr;
    double t_read = 0, t_check = 0, t_wait = 0;
    std::string result;
    while (!rd.eof()) {
        uint8_t *b = bufs[cur]->p;
        auto t0 = now();
        if (!(result = rd.fill(b, have)).empty()) break;
        t_read += since(t0);
        if (!(result = rd.classify(b)).empty()) break;
        // FASTQ: the chunk starts and ends at record boundaries and goes to the library as it is.  Malformed records — line
        // structure AND quality-line lengths — are found on the device (pack_kernels.hip, fastq_check.hip); the library then
        // re-does the chunk with needletail's rule and reports it (round 3: no host pass over every byte any more).
        t0 = now();
        if (!(result = rd.cut(b)).empty()) break;
        t_check += since(t0);
        // what follows the cut moves to the front of the other buffer — once the sketching side has let go of it
        t0 = now();
        const int other = cur ^ 1;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !busy[other]; });
            if (halt) break;                              // an error, or the library found the record structure broken: nothing more to add
        }
        t_wait += since(t0);
        have = rd.move_rest(b, bufs[other]->p);           // cut > have / 2, carry <= 33 bytes: the buffer always drains
        {
            std::lock_guard<std::mutex> lk(mu);
            busy[cur] = true;
            jobs.push_back(Job{cur, rd.cut_at(), rd.fmt()});
        }
        cv.notify_all();
        cur = other;
    }
    bytes_seen += rd.bytes_read();
    { std::lock_guard<std::mutex> lk(mu); no_more = true; }
    cv.notify_all();
    sketcher.join();
    if (result.empty()) result = gpu_err;
    if (timing)
        fprintf(stderr, "[lash cli] streamed %s: read %.2f s, check %.2f s, waited for the sketching side %.2f s (its calls: %.2f s, concurrent)\n",
                path.c_str(), t_read, t_check, t_wait, t_gpu);
    return result;
}

// --min-count: cells of a file's count table, from its (uncompressed) size alone
int count_cells_log2_for(uint64_t bytes, int forced)
{
    if (forced) return forced;
    int l2 = 16;
    while (l2 < 36 && (1ull << l2) < 8 * std::min<uint64_t>(bytes, 1ull << 40)) ++l2;
    return l2;
}

// --min-count for a file above --stream-mb: the file is read twice (a compressed one a third time before, for its size: the table's size
// depends on the input only) — every chunk through lash_kmer_filter_count_raw, then every chunk again through the filtered call with
// LASH_F_ACCUMULATE.  Chunks are cut between records, so the cells and the image equal those of the file in one piece; a record longer
// than a chunk would repeat k-mers at the cut (find_cut's carried bases) and is refused.  One buffer, no overlap of reading and sketching.
std::string stream_big_file_filtered(lash_ctx *ctx, const lash_params &prm0, const std::string &path, uint64_t chunk_bytes, PinnedBuf &buf,
                                     uint8_t *image, uint64_t &bytes_seen, int threads, uint32_t min_count, int forced_log2, int &log2_used)
{
    if (!buf.reserve(chunk_bytes + 64)) return "out of pinned host memory";
    lash_layout lay0;
    (void)lash_ctx_get_layout(ctx, &lay0);
    const bool skip_bad = lay0.fastq_skip_bad != 0;
    uint64_t total = 0;
    // chunk(p, n, fmt) per chunk, in order; it returns false to end the pass (and sets err when that is a failure).  Without `chunk`
    // the pass only sizes the file.
    auto pass = [&](const std::function<bool(const uint8_t *, size_t, int, std::string &)> &chunk) -> std::string {
        ChunkReader rd(path, chunk_bytes, threads, chunk ? CutRule::between_records : CutRule::none,
                       "--min-count: a record of " + path + " is larger than a --stream-mb chunk and cannot be counted in pieces; raise --stream-mb");
        std::string err = rd.open();
        size_t have = 0;
        while (err.empty() && !rd.eof()) {
            err = rd.fill(buf.p, have);
            if (err.empty() && chunk) err = rd.classify(buf.p);
            if (err.empty()) err = rd.cut(buf.p);
            if (err.empty() && chunk && !chunk(buf.p, rd.cut_at(), rd.fmt(), err)) break;
            if (err.empty()) have = rd.move_rest(buf.p, buf.p);
        }
        total = rd.bytes_read();
        return err;
    };
    std::string err, perr;
    uint64_t size = 0;
    struct stat st;
    if (peek_compressed(path, size, perr)) {
        if (!(err = pass(nullptr)).empty()) return err;
        size = total;
    } else if (!perr.empty()) return perr;
    else if (stat(path.c_str(), &st) == 0) size = (uint64_t)st.st_size;
    log2_used = count_cells_log2_for(size, forced_log2);
    const uint8_t l2 = (uint8_t)log2_used;
    lash_kmer_filter *flt = nullptr;
    int rc = lash_kmer_filter_create(ctx, 1, &l2, &flt);
    if (rc != LASH_OK) return std::string("--min-count: a count table of 2^") + std::to_string(log2_used) + " cells: " + lash_strerror(rc);
    // counting, then sketching with LASH_F_ACCUMULATE from the second chunk on.  A malformed FASTQ record ends needletail's iteration
    // (utils.rs:457): the library keeps the chunk's records before it, later chunks add nothing
    uint64_t calls = 0;
    for (int sketching = 0; sketching < 2 && err.empty(); ++sketching)
        err = pass([&](const uint8_t *p, size_t n, int fmt, std::string &e) {
            lash_params prm = prm0;
            if (calls) prm.flags |= LASH_F_ACCUMULATE;
            const uint64_t off[2] = {0, (uint64_t)n};
            const uint8_t f = (uint8_t)fmt;
            const int r = sketching ? lash_sketch_files_raw_filtered(ctx, &prm, p, off, &f, 1, flt, min_count, image)
                                    : lash_kmer_filter_count_raw(ctx, &prm0, p, off, &f, 1, flt);
            if (r != LASH_OK) { e = gpu_error(ctx, r); return false; }
            calls += sketching;
            return lash_ctx_format_errors(ctx, nullptr, 0) == 0 || skip_bad;
        });
    lash_kmer_filter_free(ctx, flt);
    bytes_seen += total;
    return err;
}

// --translate needs about five times a batch in device memory (the input, the coordinates, two residues per base, the segment table)
std::string translate_error(lash_ctx *ctx, int rc)
{
    return gpu_error(ctx, rc) + (rc == LASH_ENOMEM ? " (--translate takes about 5 x the batch in device memory: lower --batch-mb / --stream-mb)" : "");
}

// --translate for a file above --stream-mb, one sketch: chunks of whole records (a k-mer never spans two records, so the union of the
// chunks' images is the file's), each indexed, translated and sketched into the one image, with LASH_F_ACCUMULATE from the second on.
// One buffer, no overlap of reading and sketching.
std::string stream_big_file_translated(lash_ctx *ctx, const lash_params &prm0, const std::string &path, uint64_t chunk_bytes, PinnedBuf &buf,
                                       uint8_t *image, uint64_t &bytes_seen, int threads)
{
    if (!buf.reserve(chunk_bytes + 64)) return "out of pinned host memory";
    ChunkReader rd(path, chunk_bytes, threads, CutRule::whole_records, "--translate");
    std::string err = rd.open();
    size_t have = 0;
    uint64_t calls = 0;
    while (err.empty() && !rd.eof()) {
        err = rd.fill(buf.p, have);
        if (err.empty()) err = rd.classify(buf.p);
        if (err.empty()) err = rd.cut(buf.p);
        if (!err.empty()) break;
        lash_params prm = prm0;
        if (calls) prm.flags |= LASH_F_ACCUMULATE;
        const uint64_t off[2] = {0, (uint64_t)rd.cut_at()};
        lash_rec_index *ix = nullptr;
        lash_tr_index *ti = nullptr;
        int rc = lash_fasta_index(ctx, buf.p, off, 1, &ix);
        if (rc == LASH_OK) rc = lash_fasta_translate(ctx, buf.p, off, 1, ix, &ti);
        const uint64_t goff[2] = {0, lash_rec_index_n_records(ix)};
        if (rc == LASH_OK) rc = lash_sketch_translated(ctx, &prm, ti, goff, 1, image);
        if (rc != LASH_OK) err = translate_error(ctx, rc);
        lash_tr_index_free(ctx, ti);
        lash_rec_index_free(ctx, ix);
        ++calls;
        if (err.empty()) have = rd.move_rest(buf.p, buf.p);
    }
    bytes_seen += rd.bytes_read();
    return err;
}

// what the routes of one `lash sketch` run share
struct Run {
    const std::chrono::steady_clock::time_point t_start;
    const SketchOptions &opt;
    const std::vector<std::string> &files;
    const lash_params prm;
    const size_t ib;                                       // bytes of one image
    // --window splits at records as --per-record does, then cuts every record into windows: the same batches, parts and hand-off
    const bool by_record;
    const std::string split_flag;                          // "--window", "--translate" or "--per-record", for messages
    BatchQueue q;
    uint64_t n_bytes = 0, n_batches = 0;                   // the planner's: input bytes seen, batches planned
    const bool timing = getenv("LASH_CLI_TIMING") != nullptr;
    std::string werr;                                      // the writer's: its error, and under by_record the ids in output order
    std::vector<std::string> names;
    std::mutex tmu, l2mu;
    int l2_lo = 99, l2_hi = 0;                             // --min-count: the table sizes this run chose (guarded by l2mu)

    static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    // LASH_CLI_TIMING=1: pipeline marks on stderr (seconds since sketch_files() started)
    void mark(const char *what, uint64_t a = 0, double dur = -1.0)
    {
        if (!timing) return;
        const double t = since(t_start);
        std::lock_guard<std::mutex> lk(tmu);
        if (dur >= 0) fprintf(stderr, "[lash cli] %7.3f s  %s %llu (%.3f s)\n", t, what, (unsigned long long)a, dur);
        else fprintf(stderr, "[lash cli] %7.3f s  %s %llu\n", t, what, (unsigned long long)a);
    }
    void note_log2(int l2) { std::lock_guard<std::mutex> lk(l2mu); l2_lo = std::min(l2_lo, l2); l2_hi = std::max(l2_hi, l2); }
};

// --per-record / --window: index the batch on the device, then sketch its records (or their windows) in sub-calls of at most
// kRecordImageCap bytes of images; each sub-call's images go to the writer as one part, and BatchQueue::add_part holds this worker back
// while the batch has a cap's worth of them unwritten.
std::string sketch_records(Run &run, lash_ctx *ctx, Batch &b)
{
    const uint32_t nf = (uint32_t)(b.f1 - b.f0);
    const char *raw = reinterpret_cast<const char *>(b.buf->p);
    lash_rec_index *ix = nullptr;
    lash_win_index *wi = nullptr;
    lash_tr_index *ti = nullptr;
    int rc = lash_fasta_index(ctx, b.buf->p, b.file_off.data(), nf, &ix);
    if (rc != LASH_OK) return gpu_error(ctx, rc);
    uint64_t n = lash_rec_index_n_records(ix);             // the items to sketch: records, or their windows
    std::vector<uint64_t> start(n + 1);
    std::vector<uint32_t> id_len(n);
    if ((rc = lash_rec_index_start(ctx, ix, start.data())) == LASH_OK) rc = lash_rec_index_id_len(ctx, ix, id_len.data());
    if (rc == LASH_OK && run.opt.window) {
        // --window: the records cut into windows on the device (lash_fasta_windows), named ID:B-E (1-based, inclusive)
        rc = lash_fasta_windows(ctx, b.buf->p, b.file_off.data(), nf, ix, run.opt.window, &wi);
        n = rc == LASH_OK ? lash_win_index_n_windows(wi) : 0;
        std::vector<uint64_t> wrec(n), wbeg(n), wlen(n);
        if (rc == LASH_OK) rc = lash_win_index_record(ctx, wi, wrec.data());
        if (rc == LASH_OK) rc = lash_win_index_begin(ctx, wi, wbeg.data());
        if (rc == LASH_OK) rc = lash_win_index_length(ctx, wi, wlen.data());
        if (rc == LASH_OK) b.names.reserve(n);
        for (uint64_t w = 0; w < n && rc == LASH_OK; ++w)
            b.names.push_back(std::string(raw + start[wrec[w]] + 1, id_len[wrec[w]]) + ":" + std::to_string(wbeg[w] + 1) + "-" + std::to_string(wbeg[w] + wlen[w]));
    } else if (rc == LASH_OK) {
        b.names.reserve(n);
        for (uint64_t r = 0; r < n; ++r) b.names.emplace_back(raw + start[r] + 1, id_len[r]);
        // --translate: the six frames of every record as residues (lash_fasta_translate); a record is then a group of one
        if (run.opt.translate) rc = lash_fasta_translate(ctx, b.buf->p, b.file_off.data(), nf, ix, &ti);
    }
    const std::string item = run.opt.window ? "window '" : "record '";
    const uint64_t step = std::max<uint64_t>(1, kRecordImageCap / std::max<size_t>(run.ib, 1));
    for (uint64_t i0 = 0; i0 < n && rc == LASH_OK; i0 += step) {
        const uint64_t i1 = std::min(n, i0 + step);
        std::vector<uint8_t> part((size_t)(i1 - i0) * run.ib, 0);
        if (ti) {
            std::vector<uint64_t> goff((size_t)(i1 - i0) + 1);
            for (uint64_t i = i0; i <= i1; ++i) goff[i - i0] = i;
            rc = lash_sketch_translated(ctx, &run.prm, ti, goff.data(), (uint32_t)(i1 - i0), part.data());
        } else
            rc = wi ? lash_sketch_windows_raw(ctx, &run.prm, wi, i0, i1, part.data())
                    : lash_sketch_records_raw(ctx, &run.prm, b.buf->p, b.file_off.data(), nf, ix, i0, i1, part.data());
        if (rc != LASH_OK) break;
        // (no note is expected: a call that does not accumulate re-does such records exactly)
        if (run.prm.algo == LASH_HLL)
            hll_notes_of_last_call(ctx, (uint32_t)(i1 - i0), [&](uint32_t i) { return item + b.names[i0 + i] + "' of " + run.files[b.f0]; });
        run.q.add_part(b, std::move(part), kRecordImageCap);
    }
    const std::string e = rc == LASH_OK ? "" : run.opt.translate ? translate_error(ctx, rc) : gpu_error(ctx, rc);
    lash_tr_index_free(ctx, ti);
    lash_win_index_free(ctx, wi);
    lash_rec_index_free(ctx, ix);
    return e;
}

// --min-count: a batch's files are counted, then sketched with the keep rule, by the same worker (lash_kmer_filter_*)
int sketch_filtered(Run &run, lash_ctx *ctx, Batch &b)
{
    const uint32_t ng = (uint32_t)(b.f1 - b.f0);
    std::vector<uint8_t> l2(ng);
    for (uint32_t g = 0; g < ng; ++g) {
        l2[g] = (uint8_t)count_cells_log2_for(b.file_off[g + 1] - b.file_off[g], run.opt.count_cells_log2);
        run.note_log2(l2[g]);
    }
    lash_kmer_filter *flt = nullptr;
    int rc = lash_kmer_filter_create(ctx, ng, l2.data(), &flt);
    if (rc == LASH_OK) rc = lash_kmer_filter_count_raw(ctx, &run.prm, b.buf->p, b.file_off.data(), b.fmt.data(), ng, flt);
    if (rc == LASH_OK) rc = lash_sketch_files_raw_filtered(ctx, &run.prm, b.buf->p, b.file_off.data(), b.fmt.data(), ng, flt, run.opt.min_count, b.images.data());
    lash_kmer_filter_free(ctx, flt);
    return rc;
}

// --translate, one image per file: the batch's records are found and translated on the device, a file is the group of its records
std::string sketch_translated_batch(Run &run, lash_ctx *ctx, Batch &b)
{
    const uint32_t ng = (uint32_t)(b.f1 - b.f0);
    lash_rec_index *ix = nullptr;
    lash_tr_index *ti = nullptr;
    int rc = lash_fasta_index(ctx, b.buf->p, b.file_off.data(), ng, &ix);
    if (rc != LASH_OK) return gpu_error(ctx, rc);
    const uint64_t n = lash_rec_index_n_records(ix);
    std::vector<uint32_t> file(n);
    std::vector<uint64_t> goff((size_t)ng + 1, 0);
    if ((rc = lash_rec_index_file(ctx, ix, file.data())) == LASH_OK) {
        for (uint64_t r = 0; r < n; ++r) ++goff[file[r] + 1];              // records come in file order
        for (uint32_t g = 0; g < ng; ++g) goff[g + 1] += goff[g];
        rc = lash_fasta_translate(ctx, b.buf->p, b.file_off.data(), ng, ix, &ti);
    }
    if (rc == LASH_OK) rc = lash_sketch_translated(ctx, &run.prm, ti, goff.data(), ng, b.images.data());
    const std::string e = rc == LASH_OK ? "" : translate_error(ctx, rc);
    lash_tr_index_free(ctx, ti);
    lash_rec_index_free(ctx, ix);
    return e;
}

// one image per file of the batch; the FASTA/FASTQ parse runs on the GPU (lash_sketch_files_raw)
std::string sketch_batch(Run &run, lash_ctx *ctx, Batch &b)
{
    if (run.opt.translate) return sketch_translated_batch(run, ctx, b);
    const uint32_t ng = (uint32_t)(b.f1 - b.f0);
    const int rc = run.opt.min_count ? sketch_filtered(run, ctx, b)
                                     : lash_sketch_files_raw(ctx, &run.prm, b.buf->p, b.file_off.data(), b.fmt.data(), ng, b.images.data());
    if (rc != LASH_OK) return gpu_error(ctx, rc);
    if (run.prm.algo == LASH_HLL) hll_notes_of_last_call(ctx, ng, [&](uint32_t i) { return run.files[b.f0 + i]; });
    return "";
}

// one per device, each with its own context
void gpu_worker(Run &run, int device)
{
    lash_ctx *ctx = nullptr;
    int rc = lash_ctx_create(&ctx, device);
    if (rc == LASH_OK) rc = lash_ctx_set_layout(ctx, &run.opt.layout);
    run.mark("context ready on device", (uint64_t)device);
    while (BatchQueue::Ptr b = run.q.next(run.by_record)) {
        if (b->err.empty() && rc != LASH_OK) b->err = lash_strerror(rc);
        if (b->err.empty()) {
            if (!run.by_record) b->images.assign((b->f1 - b->f0) * run.ib, 0);
            const auto g0 = std::chrono::steady_clock::now();
            b->err = run.by_record ? sketch_records(run, ctx, *b) : sketch_batch(run, ctx, *b);
            run.mark("GPU done, batch", b->index, Run::since(g0));
        }
        run.q.finish(b);
    }
    if (ctx) lash_ctx_destroy(ctx);
}

// the writer: images in batch (== file) order into one zstd stream (utils.rs:567-574; frames: zstd_dl.hpp)
void write_images(Run &run, const std::string &path)
{
    std::string &err = run.werr;
    ZstdWriter zw;
    err = zw.open(path, 3, run.opt.threads);           // Encoder::new(w, 3) + multithread(threads)
    while (BatchQueue::Ptr b = run.q.writer_next()) {
        for (;;) {                                         // --per-record: the batch's parts, as they come, until it is finished
            std::vector<uint8_t> part;
            if (!run.q.writer_next_part(*b, part)) break;
            if (err.empty()) err = zw.write(part.data(), part.size());
        }
        run.q.writer_done();
        if (err.empty() && !b->err.empty()) err = b->err;
        if (err.empty() && !b->images.empty()) err = zw.write(b->images.data(), b->images.size());
        if (run.by_record) run.names.insert(run.names.end(), b->names.begin(), b->names.end());
    }
    if (err.empty()) err = zw.finish();
}

// Size and kind of every file, on the pool's threads in ranges of 512 (a collection of 100 000 viral genomes spent 0.25 s in this loop
// on one thread — as long as the GPU needs for all of them a hundred times over); the first error in FILE order is the one reported.
std::string size_files(Pool &pool, const std::vector<std::string> &files, uint64_t stream_bytes, std::vector<FileSlot> &slots)
{
    const size_t n_files = files.size(), R = 512, n_ranges = (n_files + R - 1) / R;
    std::vector<std::string> range_err(n_ranges);
    std::mutex pmu;
    std::condition_variable pcv;
    size_t pending = n_ranges;
    for (size_t r = 0; r < n_ranges; ++r) {
        pool.submit([&, r]() {
            for (size_t i = r * R; i < std::min(n_files, (r + 1) * R); ++i) {
                std::string e;
                uint64_t sz = 0;
                const bool comp = peek_compressed(files[i], sz, e);
                if (!e.empty()) { range_err[r] = e; break; }
                slots[i].compressed = comp;
                slots[i].big = comp ? sz > stream_bytes / 3 : sz > stream_bytes;
                if (slots[i].big) { slots[i].compressed = false; slots[i].size = 0; slots[i].sized = true; }   // handled by the planner itself
                else if (!comp) { slots[i].size = sz; slots[i].sized = true; }
            }
            std::lock_guard<std::mutex> lk(pmu);
            if (--pending == 0) pcv.notify_all();
        });
    }
    std::unique_lock<std::mutex> lk(pmu);
    pcv.wait(lk, [&] { return pending == 0; });
    for (const std::string &e : range_err)
        if (!e.empty()) return e;
    return "";
}

// --per-record / --window, a file above --stream-mb: it goes to the GPU workers as a sequence of batches, each a chunk of at most
// --stream-mb that ends before the last record start in it; a record is never split.  A chunk pins up to --stream-mb (1 GiB by default)
// where a batch pins --batch-mb, and pinning is the slowest thing the host does (~0.18 s per GB): `chunk_cap` allows no more chunks in
// flight than keep every worker busy while one is being read, and their buffers are recycled from chunk to chunk.  The chunks are read
// here, one after another, on the planner's thread (a .gz inflates on ByteStream's threads); the previous chunk's buffer has gone to a
// worker, so the bytes after its cut wait in `tail`.
std::string plan_record_chunks(Run &run, size_t i, uint64_t stream_bytes, size_t chunk_cap)
{
    ChunkReader rd(run.files[i], stream_bytes, run.opt.threads, CutRule::whole_records, run.split_flag);
    std::string e = rd.open();
    std::vector<uint8_t> tail;
    while (e.empty() && !rd.eof()) {
        auto b = std::make_shared<Batch>();
        b->f0 = i;
        b->f1 = i + 1;
        b->buf = run.q.take_slot(chunk_cap);
        if (!b->buf) b->buf = new_pinned();
        if (!b->buf->reserve(stream_bytes + 64)) e = "out of pinned host memory";
        else {
            uint8_t *p = b->buf->p;
            if (!tail.empty()) memcpy(p, tail.data(), tail.size());
            e = rd.fill(p, tail.size());
            if (e.empty()) e = rd.classify(p);
            if (e.empty()) e = rd.cut(p);
            if (e.empty()) { tail.resize(rd.rest()); rd.move_rest(p, tail.data()); }
        }
        b->err = e;
        b->file_off = {0, e.empty() ? (uint64_t)rd.cut_at() : 0};
        b->fmt.assign(1, (uint8_t)LASH_FMT_FASTA);
        b->index = run.n_batches++;
        run.q.push(b);
    }
    run.n_bytes += rd.bytes_read();
    return e;
}

// the planner's own context on the first device and its chunk buffers, kept across files (pinning costs 0.2 s per GiB)
struct Streamer {
    lash_ctx *ctx = nullptr;
    PinnedBuf buf{lash_host_alloc_pinned, lash_host_free_pinned}, buf2{lash_host_alloc_pinned, lash_host_free_pinned};
    ~Streamer() { if (ctx) lash_ctx_destroy(ctx); }
};

// A file above --stream-mb, one sketch: it is its own "batch", streamed here, on the planner's thread and in file order, into one
// accumulated image.  Returns an error that ends the run; one of the file's own travels with its batch.
std::string plan_streamed_file(Run &run, Streamer &st, size_t i, uint64_t stream_bytes, int device)
{
    auto b = std::make_shared<Batch>();
    b->f0 = i;
    b->f1 = i + 1;
    b->images.assign(run.ib, 0);
    if (!st.ctx) {
        int rc = lash_ctx_create(&st.ctx, device);
        if (rc == LASH_OK) rc = lash_ctx_set_layout(st.ctx, &run.opt.layout);
        if (rc != LASH_OK) return lash_strerror(rc);
    }
    if (run.opt.translate)
        b->err = stream_big_file_translated(st.ctx, run.prm, run.files[i], stream_bytes, st.buf, b->images.data(), run.n_bytes, run.opt.threads);
    else if (run.opt.min_count) {
        int l2 = 0;
        b->err = stream_big_file_filtered(st.ctx, run.prm, run.files[i], stream_bytes, st.buf, b->images.data(), run.n_bytes, run.opt.threads,
                                          run.opt.min_count, run.opt.count_cells_log2, l2);
        if (l2) run.note_log2(l2);
    } else
        b->err = stream_big_file(st.ctx, run.prm, run.files[i], stream_bytes, st.buf, st.buf2, b->images.data(), run.n_bytes, run.opt.threads);
    b->index = run.n_batches++;
    run.q.publish(b);
    return "";
}

}  // namespace

// test hook (host_hooks.cpp): the chunk-cut rule of the large-file streamer
size_t stream_find_cut(const uint8_t *b, size_t n, int fmt, std::vector<uint8_t> &carry) { return find_cut(b, n, fmt, carry); }

std::string sketch_files(const SketchOptions &opt, const std::vector<std::string> &files, const std::string &output_name,
                         SketchStats *stats)
{
    // ---- options ----
    const auto t_start = std::chrono::steady_clock::now();
    lash_params prm{opt.algo, opt.k, opt.precision, opt.flags, opt.seed};
    if (lash_params_check(&prm) != LASH_OK) return lash_strerror(LASH_EINVAL);
    const std::vector<int> devices = opt.devices.empty() ? std::vector<int>{0} : opt.devices;
    const int n_dev_avail = lash_device_count();
    if (n_dev_avail <= 0) return lash_strerror(LASH_ENODEV);
    for (int d : devices)
        if (d < 0 || d >= n_dev_avail) return "device index out of range";
    const size_t n_files = files.size();
    Run run{t_start, opt, files, prm, lash_layout_image_bytes(&opt.layout, opt.algo, opt.precision), opt.per_record || opt.window != 0,
            opt.window ? "--window" : opt.translate ? "--translate" : "--per-record"};
    // Enough batches to keep every device fed and to read ahead while the HIP contexts come up (~0.3 s), but not more
    // page-locked memory than ~512 MiB: pinning costs ~0.18 s per GB and is the slowest thing the host does here.
    const size_t in_flight_cap = std::max<size_t>(2 * devices.size() + 1, (size_t)((512ull << 20) / std::max<uint64_t>(opt.batch_bytes, 1)));
    const uint64_t stream_bytes = std::min<uint64_t>(std::max<uint64_t>(opt.stream_bytes, 1u << 16), 0xF0000000ull);

    // ---- GPU workers (one context per device) and the in-order writer ----
    std::vector<std::thread> workers;
    for (int d : devices) workers.emplace_back(gpu_worker, std::ref(run), d);
    std::thread writer(write_images, std::ref(run), output_name + "_sketches.bin");

    // ---- readers: inflate compressed inputs ahead of the planner; place every file's bytes into its batch ----
    std::vector<FileSlot> slots(n_files);
    std::mutex smu;
    std::condition_variable cv_sized, cv_window;
    uint64_t inflated_held = 0;                            // bytes of inflated-but-unplaced data (guarded by smu)
    const uint64_t inflate_window = std::max<uint64_t>(2 * opt.batch_bytes, 1ull << 28);
    std::string err;
    {
        Pool pool(std::max(1, opt.threads));
        size_t next_inflate = 0;
        auto pump_inflates = [&]() {                       // called with smu held
            while (next_inflate < n_files) {
                FileSlot &s = slots[next_inflate];
                if (!s.compressed) { ++next_inflate; continue; }
                if (inflated_held >= inflate_window) break;
                const size_t i = next_inflate++;
                inflated_held += 1;                        // placeholder so that at least progress is bounded per file
                pool.submit([&, i]() {
                    std::vector<uint8_t> data;
                    std::string e = slurp_maybe_compressed(files[i], data);
                    std::lock_guard<std::mutex> lk(smu);
                    slots[i].err = e;
                    slots[i].size = data.size();
                    inflated_held += data.size();
                    slots[i].inflated.swap(data);
                    slots[i].sized = true;
                    cv_sized.notify_all();
                });
            }
        };
        err = size_files(pool, files, stream_bytes, slots);
        Streamer streamer;
        std::shared_ptr<Batch> cur;
        auto finalize = [&]() {
            if (!cur || cur->f1 == cur->f0) return;
            cur->buf = run.q.take_slot(in_flight_cap);     // bounded number of batches planned / queued / running / unwritten
            if (!cur->buf) cur->buf = new_pinned();
            const auto p0 = std::chrono::steady_clock::now();
            if (!cur->buf->reserve(cur->file_off.back() + 64)) { cur->err = "out of pinned host memory"; }
            cur->index = run.n_batches++;
            run.mark("batch planned (pinned buffer ready)", cur->index, Run::since(p0));
            cur->fmt.assign(cur->f1 - cur->f0, 0);
            cur->remaining = cur->f1 - cur->f0;
            std::shared_ptr<Batch> b = cur;
            // one task per run of files of about 1 MiB (at most 256 files): a task per 10 kB file is 2 us of work behind a queue that
            // sixteen threads share — 6 250 files of a batch took 32 ms to read, 80 us per file and thread
            for (size_t g0 = b->f0; g0 < b->f1;) {
                size_t g1 = g0 + 1;
                uint64_t run_bytes = slots[g0].size;
                while (g1 < b->f1 && g1 - g0 < 256 && run_bytes + slots[g1].size <= (1u << 20)) run_bytes += slots[g1++].size;
                pool.submit([&, b, g0, g1]() {
                  for (size_t i = g0; i < g1; ++i) {
                    FileSlot &s = slots[i];
                    uint8_t *dst = b->buf->p ? b->buf->p + b->file_off[i - b->f0] : nullptr;
                    std::string e = s.err;
                    if (e.empty() && dst) {
                        if (s.compressed) {
                            if (s.size) memcpy(dst, s.inflated.data(), s.size);
                            std::vector<uint8_t>().swap(s.inflated);
                            std::lock_guard<std::mutex> lk(smu);
                            inflated_held -= std::min<uint64_t>(inflated_held, s.size + 1);
                            cv_window.notify_all();
                        } else {
                            e = read_exact(files[i], dst, s.size);
                        }
                        if (e.empty()) {
                            const int f = sniff_format(dst, s.size);
                            if (!f) e = error_not_fastx(files[i]);
                            else if ((run.by_record || opt.translate) && f != LASH_FMT_FASTA) e = error_not_fasta(run.split_flag, files[i]);
                            b->fmt[i - b->f0] = (uint8_t)(f ? f : LASH_FMT_FASTA);
                            // (malformed FASTQ records: found on the device, the file is then re-done by the library with
                            // needletail's rule — utils.rs:457 — or, under layout fastq_err=skip, without the bad records)
                        }
                    }
                    if (!e.empty()) { std::lock_guard<std::mutex> lk(b->emu); if (b->err.empty()) b->err = e; }
                    if (b->remaining.fetch_sub(1) == 1) {
                        run.mark("batch read into memory", b->index);
                        run.q.push(b);
                    }
                  }
                });
                g0 = g1;
            }
            cur.reset();
        };

        // ---- the plan: files in order into batches; a file above --stream-mb goes its own way ----
        for (size_t i = 0; i < n_files && err.empty(); ++i) {
            {
                std::unique_lock<std::mutex> lk(smu);
                pump_inflates();
                while (!slots[i].sized) {
                    cv_sized.wait_for(lk, std::chrono::milliseconds(50));
                    pump_inflates();
                }
            }
            if (slots[i].big) {
                finalize();
                err = run.by_record ? plan_record_chunks(run, i, stream_bytes, std::min(in_flight_cap, devices.size() + 1))
                                    : plan_streamed_file(run, streamer, i, stream_bytes, devices[0]);
                continue;
            }
            if (!cur) { cur = std::make_shared<Batch>(); cur->f0 = cur->f1 = i; }
            cur->file_off.push_back(cur->file_off.back() + slots[i].size);
            cur->f1 = i + 1;
            run.n_bytes += slots[i].size;
            if (cur->file_off.back() >= opt.batch_bytes) finalize();
        }
        if (err.empty()) finalize();
    }   // Pool joins here: every placement task has run

    // ---- join ----
    run.q.close(run.n_batches);
    for (auto &t : workers) t.join();
    writer.join();
    run.mark("writer done", 0);
    if (err.empty()) err = run.werr;
    if (!err.empty()) {
        if (run.by_record) (void)remove((output_name + "_sketches.bin").c_str());   // a refused --per-record run leaves no output
        return err;
    }

    // ---- names (utils.rs:577-580) and stats ----
    {
        std::ofstream out(output_name + "_files.json", std::ios::binary);
        if (!out) return "cannot create " + output_name + "_files.json";
        out << json_pretty_string_array(run.by_record ? run.names : files);
        if (!out.good()) return "write failed";
    }
    if (opt.min_count && run.l2_hi)
        fprintf(stderr, "--min-count %u: count tables of 2^%d%s cells per file\n", opt.min_count, run.l2_lo,
                run.l2_lo == run.l2_hi ? "" : (" to 2^" + std::to_string(run.l2_hi)).c_str());
    if (stats) {
        stats->files = n_files;
        stats->records = run.names.size();
        stats->bytes = run.n_bytes;
        stats->batches = run.n_batches;
        stats->seconds = Run::since(t_start);
    }
    return "";
}

}  // namespace lashhost
