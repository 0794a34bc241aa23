// dist.cpp — `lash dist` for the gfx950 build.
//
// Mirrors /root/reference/src/main.rs:280-617 (file discovery, parameter checks, output formats, distance formula)
// and utils.rs:84-373 (hmh_distance, ull_distance, hll_distance).  The O(N_ref * N_qry * registers) scans run on the GPU(s);
// what is O(sketches) or O(pairs) runs on `-t` host threads.  Every estimator is restated from the published algorithm the
// crate ports [PARITY UNPINNED, like every crate-internal rule; tools/ref_probe pins them through `<case>.dist.tsv`]:
//   hmh  C / N pair counts (lash_hmh_pair_counts) + LogLog-beta cardinalities + expected-collision correction of
//        axiomhq/hyperminhash (crate hyperminhash 0.1.4);
//   hll  union zero / sum per pair (lash_hll_pair_union_stats) + streaming_algorithms' HLL++ `len()`: linear counting below
//        the published per-precision threshold, else alpha*m^2/sum.  Its third regime (estimate <= 5m: subtract a
//        k-nearest-neighbour bias read from the HLL++ empirical tables) needs data that is not in this image; a sketch
//        or union that falls there is refused with a message instead of being estimated differently, unless the tables come
//        from --hll-bias FILE or are simulated on the GPU at start-up (--hll-bias-sim: lash_hll_bias_simulate, regenerated
//        measurements, not the crate's numbers);
//   ull  union estimate per pair on the GPU (lash_ull_pair_union_estimates: merged-register histogram + FGRA or ML,
//        ull_estimators.h), per-sketch estimates with lash_ull_estimate; similarity by inclusion-exclusion (utils.rs:272).
// Order: the reference keeps its sketches in hashbrown maps seeded with XXH3(93) and takes the column order, the
// same-files triangle and (under rayon: up to scheduling) the row order from `.keys()`; name_order.hpp
// restates that order, so rows, columns and the (Reference, Query) orientation of each triangle pair come out as the
// reference's `-t 1` run writes them.  --file-order keeps list-file order instead.
// Several GPUs (--devices 0,1,..): blocks of reference rows are handed to one worker per device and written in order.
// --max-dist D (not upstream): a block's pairs are filtered on the device (lash_sketch_set_pair_block_within) and only the rows with
// d <= D are formatted — the same rows in the same order as without the option, minus the others.
// --top K (not upstream): a block's pairs go through a selection on the device (lash_sketch_set_pair_block_top) and the survivors into
// per-name lists on the host (lash_top_*, one per worker, merged at the end); N_K of a name is complete only after the last block, so the
// kept rows are written once, at the end, in (row, col) order — the same rows in the same order as without the option, minus the others.
// --cluster D (not upstream; same files only): single-linkage clusters, two names being linked iff --max-dist D prints their pair.  A
// block's pairs are joined in a label array on the device (lash_sketch_set_pair_block_cluster, one lash_cluster per worker, merged at the
// end); no pair text at all, the N lines "representative<TAB>member" are written once, at the end.
// --containment query|reference (not upstream): the distance of the containment fraction s/(1+s) * (a_r + a_q) / a_q (or / a_r) instead of
// 2s/(1+s) (csrc/dist_pair.h).  Directional, so the run is always the rectangle: same files print the full square, both orientations; every
// rectangular route (all pairs, --max-dist, --top) takes it, the measure going down to the device's filters.
// --derep D (not upstream; same files only): greedy representatives in row order, "within D" meaning that --max-dist D prints the pair.
// A row is decided from the representatives among the rows before it (lash_sketch_set_pair_block_derep, one lash_derep), so the blocks
// run in row order on one worker; the N lines are written once, at the end.
// --tree / --linkage L (not upstream; same files only): agglomerative clustering of the whole matrix of printed distances.  A block's pair
// statistics come back as for the unfiltered run, -t threads turn them into the exact doubles (dist_block_values: the numbers the list
// form prints, before rounding to six decimals) and the block's triangle rows go into the run's one N x N matrix on the first device
// (lash_tree_set_rows; other devices' workers hand theirs over through the host).  After the last block lash_tree_build merges on the
// device; --tree writes the Newick text, --cluster D --linkage average|complete the clusters of the cut at D (newick.hpp).  --tree --nj
// fills the same matrix and lets lash_tree_build_nj join it: the neighbour-joining tree, unrooted, no heights to cut.
// --pcoa K (not upstream; same files only) fills the same matrix too and lets lash_tree_build_pcoa centre it and solve its K algebraically
// largest eigenpairs on the device; K eigenvalues and N x K coordinates come back and go out as one table (dist_format: pcoa_text).
#include "dist.hpp"

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <condition_variable>
#include <map>
#include <mutex>
#include <sstream>
#include <numeric>
#include <thread>
#include <vector>

#include "../../../include/lash_gfx950.h"
#include "dist_format.hpp"
#include "json_out.hpp"
#include "name_order.hpp"
#include "newick.hpp"
#include "zstd_dl.hpp"

namespace lashhost {
namespace {

// main.rs:284-337
std::string find_files(const std::string &prefix, std::map<std::string, std::string> &out)
{
    std::string norm = prefix;
    size_t slash = norm.find_last_of('/');
    if (slash != std::string::npos) norm = norm.substr(slash + 1);
    if (norm.rfind("./", 0) == 0) norm = norm.substr(2);
    DIR *d = opendir("./");
    if (!d) return "cannot read the current directory";
    out.clear();
    while (dirent *e = readdir(d)) {
        std::string name = e->d_name;
        struct stat st;
        if (stat(name.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) continue;
        if (name.rfind(norm, 0) != 0) continue;
        auto ends = [&](const char *suf) { size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
        if (ends("parameters.json")) out["params"] = name;
        else if (ends("files.json")) out["files"] = name;
        else if (ends(".bin")) out["sketches"] = name;
    }
    closedir(d);
    if (out.size() != 3) {
        std::ostringstream m;
        m << "There should be 3 files starting with " << norm << " but " << out.size() << " were found instead";
        return m.str();
    }
    return "";
}

std::string slurp(const std::string &path, std::string &out)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) return "cannot open " + path;
    std::ostringstream ss;
    ss << in.rdbuf();
    out = ss.str();
    return "";
}

const char *const BIAS_MSG = ": cardinality estimate <= 5 * 2^p needs the HLL++ bias tables of streaming_algorithms, which are "
                             "not built in (pass --hll-bias-sim to simulate them, --hll-bias <file from lash hll-bias or tools/ref_probe/extract_hll_bias.py>, or sketch with a smaller -p)";

// One precision's simulated table on an open context; `line` = its provenance ("p 14: 200 points, 2048 trials, seed 42")
std::string simulate_bias(lash_ctx *ctx, int p, uint32_t points, uint32_t trials, uint64_t seed, std::vector<double> &raw, std::vector<double> &bias,
                          std::string &line)
{
    const uint32_t all = 5u * (1u << p) + 1u;
    const uint32_t n = points ? std::min(points, all) : lash_hll_bias_default_points(p);
    raw.assign(n, 0.0);
    bias.assign(n, 0.0);
    const int rc = lash_hll_bias_simulate(ctx, p, n, trials, seed, nullptr, raw.data(), bias.data());
    if (rc != LASH_OK) return std::string("cannot simulate the HLL++ bias table: ") + lash_strerror(rc) + " " + lash_ctx_last_error(ctx);
    char buf[160];
    snprintf(buf, sizeof buf, "p %d: %u points, %u trials, seed %llu", p, n, trials ? trials : 2048u, (unsigned long long)seed);
    line = buf;
    return "";
}

const char *const SIM_NOTE = "HLL++ bias table simulated on the GPU (regenerated measurements, not streaming_algorithms' tables)";

// LASH_CLI_TIMING: where the wall time of a run goes
struct Timing {
    const bool on = getenv("LASH_CLI_TIMING") != nullptr;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    void mark(const char *what) const { if (on) fprintf(stderr, "[lash dist] %7.3f s  %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), what); }
};

// what a run reads from its two sketch-file sets, checked
struct DistInput {
    int k = 0, algo_id = 0, prec = 0, ull_est = LASH_ULL_FGRA;
    bool same_files = false, same_sketches = false;                  // the triangle: the same name file (main.rs:404) and no --containment; one sketch file, read once
    bool same_order = false;                                         // the same name file, whatever is printed
    std::vector<std::string> rnames, qnames;                         // the name files
    std::vector<uint32_t> rorder, qorder;                            // the maps' key order: the rows / columns, as indices into the name files
    std::vector<uint8_t> rimg_store, qimg_store;
    uint32_t nr = 0, nq = 0;
    std::vector<std::string> row_name, col_name, col_tab;
    std::vector<uint32_t> row_id, col_id;                            // "q_name == r_name prints 0" (main.rs:452-453) as an integer compare per pair
    std::vector<uint32_t> same_col;                                  // --max-dist / --top: the column carrying each row's name, or NO_COLUMN
    const std::vector<uint8_t> &rimg() const { return rimg_store; }
    const std::vector<uint8_t> &qimg() const { return same_sketches ? rimg_store : qimg_store; }
    bool one_set() const { return same_sketches && same_order; }     // the same images in the same order: one set is both sides
};

std::string load_input(const DistOptions &opt, const Timing &timing, DistInput &in)
{
    std::map<std::string, std::string> rf, qf;
    std::string err = find_files(opt.ref_prefix, rf);
    if (err.empty()) err = find_files(opt.query_prefix, qf);
    if (!err.empty()) return err;
    std::string txt;
    std::map<std::string, std::string> rp, qp;
    if (!(err = slurp(rf["params"], txt)).empty() || !json_parse_string_object(txt, rp)) return err.empty() ? "bad parameters JSON " + rf["params"] : err;
    if (!(err = slurp(qf["params"], txt)).empty() || !json_parse_string_object(txt, qp)) return err.empty() ? "bad parameters JSON " + qf["params"] : err;
    if (rp["k"] != qp["k"]) return "Genomes were not sketched with the same k";                       // main.rs:368-370
    if (rp["algorithm"] != qp["algorithm"]) return "Algorithms do not match in query and sketch genomes";
    const std::string algo = rp["algorithm"];
    if ((algo == "ull" || algo == "hll") && rp["precision"] != qp["precision"])
        return algo + " was not sketched with same precision btwn genomes";
    in.k = atoi(rp["k"].c_str());
    if (opt.model != 0 && opt.model != 1) return "model needs to be 0 or 1";
    const bool hll = algo == "hll", ull = algo == "ull";
    if (!hll && !ull && algo != "hmh") return "Algorithm must be either hmh, ull, or hll";
    if (ull) {                                                                                        // utils.rs:213-217
        if (opt.estimator == "ml") in.ull_est = LASH_ULL_ML;
        else if (opt.estimator != "fgra") return "estimator needs to be either fgra or ml";
    }
    if (!(err = slurp(rf["files"], txt)).empty() || !json_parse_string_array(txt, in.rnames)) return err.empty() ? "bad names JSON " + rf["files"] : err;
    if (!(err = slurp(qf["files"], txt)).empty() || !json_parse_string_array(txt, in.qnames)) return err.empty() ? "bad names JSON " + qf["files"] : err;
    in.same_order = qf["files"] == rf["files"];                                                       // main.rs:404
    in.same_files = in.same_order && opt.measure == LASH_MEASURE_JACCARD;                             // (a containment is a rectangle)
    in.same_sketches = rf["sketches"] == qf["sketches"];                                              // all-vs-all: one file, read once
    if (opt.has_cluster && !(in.same_files && in.same_sketches))
        return "--cluster needs an all-vs-all run: -q and -r must name the same sketch files";
    if (opt.tree && !(in.same_files && in.same_sketches))
        return "--tree needs an all-vs-all run: -q and -r must name the same sketch files";
    if (opt.pcoa && !(in.same_files && in.same_sketches))
        return "--pcoa needs an all-vs-all run: -q and -r must name the same sketch files";
    if (opt.has_derep && !(in.same_files && in.same_sketches))
        return "--derep needs an all-vs-all run: -q and -r must name the same sketch files";
    // utils.rs:111-127: the maps' key order (a repeated name is one entry carrying its last sketch)
    if (opt.file_order) {
        in.rorder.resize(in.rnames.size()); std::iota(in.rorder.begin(), in.rorder.end(), 0u);
        in.qorder.resize(in.qnames.size()); std::iota(in.qorder.begin(), in.qorder.end(), 0u);
    } else {
        in.rorder = hashbrown_key_order(in.rnames);
        in.qorder = in.same_order ? in.rorder : hashbrown_key_order(in.qnames);
    }

    if (!(err = zstd_decompress_file(rf["sketches"], in.rimg_store)).empty()) return err;
    if (!in.same_sketches && !(err = zstd_decompress_file(qf["sketches"], in.qimg_store)).empty()) return err;
    timing.mark("sketch files read and inflated");
    in.algo_id = hll ? LASH_HLL : ull ? LASH_ULL : LASH_HMH;
    in.prec = (hll || ull) ? atoi(rp["precision"].c_str()) : 0;
    if (hll && (in.prec < 4 || in.prec > 16)) return "bad precision in " + rf["params"];
    if (ull && (in.prec < 3 || in.prec > 26)) return "bad precision in " + rf["params"];
    const size_t ib = lash_layout_image_bytes(&opt.layout, in.algo_id, in.prec);
    if (!ib) return "bad layout";
    if (in.rimg().size() < in.rnames.size() * ib) return "Error with reading from " + rf["sketches"];
    if (in.qimg().size() < in.qnames.size() * ib) return "Error with reading from " + qf["sketches"];
    // rows / columns: the ENTRIES of the two maps in key order (a repeated name is one entry carrying its last sketch,
    // utils.rs:111-127) — everything below is indexed by position in rorder / qorder, never by name-file index
    const uint32_t nr = in.nr = (uint32_t)in.rorder.size(), nq = in.nq = (uint32_t)in.qorder.size();
    in.row_name.resize(nr); in.col_name.resize(nq);
    for (uint32_t i = 0; i < nr; ++i) in.row_name[i] = in.rnames[in.rorder[i]];
    for (uint32_t j = 0; j < nq; ++j) in.col_name[j] = in.qnames[in.qorder[j]];
    name_ids(in.row_name, in.col_name, in.row_id, in.col_id);
    if (!opt.matrix) in.col_tab = tabbed_names(in.col_name);
    // a name is one entry per side, so at most one column carries a row's name; found once — those pairs print 0
    if (opt.has_max_dist || opt.top) {
        std::vector<uint32_t> col_of(in.row_name.size() + in.col_name.size(), NO_COLUMN);
        for (uint32_t j = 0; j < nq; ++j) col_of[in.col_id[j]] = j;
        in.same_col.resize(nr);
        for (uint32_t i = 0; i < nr; ++i) in.same_col[i] = col_of[in.row_id[i]];
    }
    return "";
}

// The sketches go to every device ONCE (lash_sketch_set: images + what the pair kernels derive from them), in map order; per-sketch
// cardinalities (utils.rs:101-103, 213-217, 314-315) come from register histograms made on the GPU.
struct DevSets { int device = 0; lash_ctx *ctx = nullptr; lash_sketch_set *ref = nullptr, *qry = nullptr; };
struct DeviceSets {
    std::vector<DevSets> sets;
    std::vector<double> rcard, qcard;                                // (one set: qcard is a copy of rcard)
    ~DeviceSets()
    {
        for (DevSets &d : sets) {
            if (d.qry && d.qry != d.ref) lash_sketch_set_free(d.ctx, d.qry);
            if (d.ref) lash_sketch_set_free(d.ctx, d.ref);
            if (d.ctx) lash_ctx_destroy(d.ctx);
        }
    }
    const DevSets *on(int device) const { for (const DevSets &d : sets) if (d.device == device) return &d; return nullptr; }
};

std::string make_device_sets(const DistOptions &opt, const DistInput &in, const std::vector<int> &devices, const lash_hll_bias *bias, DeviceSets &dev)
{
    const bool one_set = in.one_set();
    dev.rcard.resize(in.nr);
    for (int dv : devices) {
        if (dev.on(dv)) continue;
        dev.sets.emplace_back();
        DevSets &d = dev.sets.back();
        d.device = dv;
        int rc = lash_ctx_create(&d.ctx, dv);
        if (rc == LASH_OK) rc = lash_ctx_set_layout(d.ctx, &opt.layout);
        if (rc == LASH_OK)
            rc = lash_sketch_set_create(d.ctx, in.algo_id, in.prec, in.rimg().data(), (uint32_t)in.rnames.size(), in.rorder.data(), in.nr, &d.ref);
        if (rc == LASH_OK) {
            if (one_set) d.qry = d.ref;
            else rc = lash_sketch_set_create(d.ctx, in.algo_id, in.prec, in.qimg().data(), (uint32_t)in.qnames.size(), in.qorder.data(), in.nq, &d.qry);
        }
        // (every device computes its sets' cardinalities: the sets keep them for the expected-collision vectors)
        uint32_t bad = 0;
        if (rc == LASH_OK) {
            rc = lash_sketch_set_cardinalities(d.ctx, d.ref, in.ull_est, bias, dev.rcard.data(), &bad);
            if (rc == LASH_ERANGE) return in.row_name[bad] + BIAS_MSG;
        }
        if (rc == LASH_OK && !one_set) {
            dev.qcard.resize(in.nq);
            rc = lash_sketch_set_cardinalities(d.ctx, d.qry, in.ull_est, bias, dev.qcard.data(), &bad);
            if (rc == LASH_ERANGE) return in.col_name[bad] + BIAS_MSG;
        }
        if (rc == LASH_OK) rc = lash_sketch_set_prepare(d.ctx, d.ref, d.qry);
        if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(d.ctx);
    }
    if (one_set) dev.qcard = dev.rcard;
    return "";
}

// Blocks of reference rows [begin[b], begin[b + 1]): bounded pair tables (all-vs-all on 10^5 sketches is 5 * 10^9 printed pairs), about
// the same number of PRINTED pairs each — with same files row i prints i + 1 columns, so late blocks hold fewer rows.
std::vector<uint32_t> plan_blocks(const DistOptions &opt, const DistInput &in)
{
    const uint32_t nr = in.nr, nq = in.nq;
    std::vector<uint32_t> begin{0};
    const uint64_t total = in.same_files ? (uint64_t)nr * (nr + 1) / 2 : (uint64_t)nr * nq;
    const uint64_t want = opt.block_rows ? 0 : std::max<uint64_t>(std::min<uint64_t>(32ull << 20, total / 16 + 1), 4096);   // pairs per block, >= ~16 blocks
    uint64_t acc = 0;
    for (uint32_t i = 0; i < nr; ++i) {
        acc += in.same_files ? i + 1 : nq;
        const bool cut = opt.block_rows ? (i + 1 - begin.back()) >= opt.block_rows : acc >= want;
        if (cut && i + 1 < nr) { begin.push_back(i + 1); acc = 0; }
    }
    if (nr) begin.push_back(nr);
    return begin;
}

// what the workers of a run share
struct Run {
    const DistOptions &opt;
    const DistInput &in;
    const DeviceSets &dev;
    const lash_hll_bias *bias;
    const Timing &timing;
    std::vector<int> devices;                                    // one worker each
    std::vector<uint32_t> block_begin;
    bool gpu_ec = false;
    int fmt_threads = 1;
    FILE *out = nullptr;
    std::atomic<uint32_t> next_block{0};
    std::mutex wmu;
    std::condition_variable wcv;
    uint32_t next_to_write = 0;
    std::string fail;                                            // guarded by wmu
    // --top: per worker, the lists of the K nearest of every name (the columns; in a triangle run the set) from the blocks it ran
    std::vector<lash_top *> tops;
    std::atomic<uint64_t> top_candidates{0};                     // (LASH_CLI_TIMING: what the device passed to the host)
    // --cluster: per worker, the clusters joined by the blocks it ran (created by the worker: the labels live on its device)
    std::vector<lash_cluster *> clusters;
    std::atomic<uint64_t> cl_pairs{0}, cl_pruned{0}, cl_joined{0}, cl_sent{0};   // (LASH_CLI_TIMING)
    // --derep: the one worker's accumulator (created by it: rep[] lives on its device)
    lash_derep *derep = nullptr;
    lash_derep_stats dr{};                                       // (LASH_CLI_TIMING: summed over the blocks; representatives: the last block's)
    // --tree / --linkage: the run's one matrix, on the first device, with a context of its own; workers take tree_mu to hand rows over
    lash_ctx *tree_ctx = nullptr;
    lash_tree *tree = nullptr;
    std::mutex tree_mu;
    ~Run()
    {
        for (lash_top *p : tops) lash_top_free(p);
        for (lash_cluster *p : clusters) lash_cluster_free(p);
        lash_derep_free(derep);
        lash_tree_free(tree_ctx, tree);
        if (tree_ctx) lash_ctx_destroy(tree_ctx);
        if (out) fclose(out);
    }
};

struct Block { uint32_t i0, i1, n_cols; };

// one worker: its own context (stream and staging; the sets are shared, read-only) and the buffers it reuses from block to block
struct Worker {
    Run &run;
    const DistOptions &opt;
    const DistInput &in;
    const size_t wi;
    const DevSets *ds;
    lash_ctx *ctx = nullptr;
    // the unfiltered run's pair tables in page-locked memory (the copy back runs at the link rate): hmh C / N; hll zero + sum; ull the union estimate
    uint32_t *C = nullptr, *N = nullptr;
    double *U = nullptr, *EC = nullptr;
    size_t cap = 0, ec_cap = 0;
    RowText row_text;                                            // the block's text
    std::vector<uint32_t> w_row, w_col;                          // --max-dist / --top: the block's survivors
    std::vector<double> w_dist;
    std::vector<lash_top_key> col_bound, row_bound;              // --top: this worker's K-th key per name, for the next block
    std::vector<double> tree_rows;                               // --tree: the block's distances on their way into the matrix
    Worker(Run &r, size_t i) : run(r), opt(r.opt), in(r.in), wi(i), ds(r.dev.on(r.devices[i])) {}
    ~Worker() { lash_host_free_pinned(C); lash_host_free_pinned(N); lash_host_free_pinned(U); lash_host_free_pinned(EC); if (ctx) lash_ctx_destroy(ctx); }

    // The failure text of a block whose library call returned rc; `bad`: the refused pair's place in the block (LASH_ERANGE).
    std::string block_failure(const Block &b, int rc, uint64_t bad = 0) const
    {
        if (rc == LASH_OK) return "";
        if (rc == LASH_ERANGE) return "union of " + in.row_name[b.i0 + bad / b.n_cols] + " and " + in.col_name[bad % b.n_cols] + BIAS_MSG;
        return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);
    }

    // --max-dist / --top: entry(cap) fills the survivor buffers and sets *kept to the full count; again with larger ones until all rows fit
    template <class Entry>
    int kept_rows(uint64_t *kept, Entry entry)
    {
        if (w_row.empty()) { w_row.resize(1u << 16); w_col.resize(1u << 16); w_dist.resize(1u << 16); }
        for (;;) {
            const int rc = entry(w_row.size());
            if (rc != LASH_OK || *kept <= w_row.size()) return rc;
            w_row.resize(*kept + *kept / 4); w_col.resize(w_row.size()); w_dist.resize(w_row.size());
        }
    }

    // --top: pair statistics, expected collisions and the selection on the device; the survivors go to this worker's lists
    std::string block_top(const Block &b)
    {
        lash_top *top = run.tops[wi];
        uint64_t kept = 0, bad = 0, cand = 0;
        col_bound.resize(b.n_cols);
        row_bound.resize(b.i1 - b.i0);
        lash_top_key *rb = in.same_files ? row_bound.data() : nullptr;
        lash_top_bounds(top, b.i0, b.i1, b.n_cols, col_bound.data(), rb);
        int rc = kept_rows(&kept, [&](uint64_t cap) {
            return lash_sketch_set_pair_block_top_measure(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, in.same_files ? 1 : 0, in.k, opt.model, opt.fp32 ? 1 : 0,
                                                          in.ull_est, run.bias, opt.measure, opt.top, opt.has_max_dist ? opt.max_dist : NAN,
                                                          in.same_col.data() + b.i0, col_bound.data(), rb, w_row.data(), w_col.data(), w_dist.data(), cap,
                                                          &kept, &bad, &cand);
        });
        run.top_candidates += cand;
        if (rc == LASH_OK) rc = lash_top_add(top, w_row.data(), w_col.data(), w_dist.data(), kept);
        return block_failure(b, rc, bad);
    }

    // --cluster: pair statistics, expected collisions and the joins on the device; the library links the pairs it could not decide
    std::string block_cluster(const Block &b)
    {
        uint64_t bad = 0;
        lash_cluster_stats cs;
        const int rc = lash_sketch_set_pair_block_cluster(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, in.k, opt.model, opt.fp32 ? 1 : 0, in.ull_est, run.bias,
                                                          opt.cluster_dist, run.clusters[wi], &cs, &bad);
        if (rc == LASH_OK) { run.cl_pairs += cs.pairs; run.cl_pruned += cs.pruned; run.cl_joined += cs.joined_on_device; run.cl_sent += cs.sent_to_host; }
        return block_failure(b, rc, bad);
    }

    // --derep: pair statistics, expected collisions, mark and trim on the device; the library walks what comes back.  One worker, so
    // the blocks arrive in row order
    std::string block_derep(const Block &b)
    {
        uint64_t bad = 0;
        lash_derep_stats st;
        const int rc = lash_sketch_set_pair_block_derep(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, in.k, opt.model, opt.fp32 ? 1 : 0, in.ull_est, run.bias,
                                                        opt.derep_dist, run.derep, &st, &bad);
        if (rc == LASH_OK) {
            run.dr.pairs += st.pairs; run.dr.pruned_not_rep += st.pruned_not_rep; run.dr.pruned_after_hit += st.pruned_after_hit;
            run.dr.sent_to_host += st.sent_to_host; run.dr.evaluated += st.evaluated; run.dr.representatives = st.representatives;
        }
        return block_failure(b, rc, bad);
    }

    // --max-dist: pair statistics, expected collisions and the cutoff on the device; only the survivors come back
    std::string block_within(const Block &b)
    {
        uint64_t kept = 0, bad = 0;
        const int rc = kept_rows(&kept, [&](uint64_t cap) {
            return lash_sketch_set_pair_block_within_measure(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, in.same_files ? 1 : 0, in.k, opt.model,
                                                             opt.fp32 ? 1 : 0, in.ull_est, run.bias, opt.measure, opt.max_dist, w_row.data(), w_col.data(),
                                                             w_dist.data(), cap, &kept, &bad, nullptr);
        });
        if (rc == LASH_OK)
            format_block_within(b.i0, b.i1, in.same_files, in.nq, opt.max_dist, w_row.data(), w_col.data(), w_dist.data(), kept, in.same_col.data(),
                                in.row_name, in.col_tab, row_text);
        return block_failure(b, rc, bad);
    }

    // the unfiltered block's pair tables (and small pairs' expected collisions), copied back
    std::string pair_tables(const Block &b, BlockTables &bt)
    {
        const bool hll = in.algo_id == LASH_HLL, ull = in.algo_id == LASH_ULL;
        const size_t np = (size_t)(b.i1 - b.i0) * b.n_cols;
        if (np > cap) {
            lash_host_free_pinned(C); lash_host_free_pinned(N); lash_host_free_pinned(U);
            C = N = nullptr; U = nullptr;
            cap = np + np / 8;
            if (!ull) C = static_cast<uint32_t *>(lash_host_alloc_pinned(cap * 4));
            if (!hll && !ull) N = static_cast<uint32_t *>(lash_host_alloc_pinned(cap * 4));
            if (hll || ull) U = static_cast<double *>(lash_host_alloc_pinned(cap * 8));
            if (!((ull || C) && (hll || ull || N) && (!(hll || ull) || U))) return "out of page-locked host memory";
        }
        int rc = lash_sketch_set_pair_block(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, in.same_files ? 1 : 0, in.ull_est, C, N, U);
        bool have_ec = false;
        if (rc == LASH_OK && run.gpu_ec) {
            // hyperminhash's expected_collisions below 2^19 distinct k-mers on both sides is a 65 536-cell sum — on the host
            // 4 ms to 0.2 s per pair; the library does the block's small pairs as one matrix product on the GPU
            if (np > ec_cap) { lash_host_free_pinned(EC); ec_cap = np + np / 8; EC = static_cast<double *>(lash_host_alloc_pinned(ec_cap * 8)); }
            uint64_t n_small = 0;
            rc = EC ? lash_sketch_set_hmh_expected_collisions(ctx, ds->ref, b.i0, b.i1, ds->qry, b.n_cols, EC, &n_small) : LASH_ENOMEM;
            have_ec = n_small != 0;
        }
        if (rc != LASH_OK) return block_failure(b, rc);
        bt.c_or_zero = C; bt.n_counts = N; bt.sum_or_union = U; bt.hmh_ec = have_ec ? EC : nullptr; bt.ld = b.n_cols;
        return "";
    }

    // every pair: the pair tables come back and -t threads format them
    std::string block_all(const Block &b)
    {
        BlockTables bt;
        const std::string f = pair_tables(b, bt);
        if (!f.empty()) return f;
        return dist_block_rows(in.algo_id, in.prec, in.k, opt.model, opt.fp32, run.bias, b.i0, b.i1, in.same_files, in.nq, run.dev.rcard.data(), run.dev.qcard.data(),
                               bt, in.row_name, in.col_name, in.col_tab, in.row_id.data(), in.col_id.data(), opt.matrix, run.fmt_threads, row_text, opt.measure);
    }

    // --tree: the pair tables come back, -t threads make the exact distances of the block's triangle rows, and those go into the matrix
    std::string block_tree(const Block &b)
    {
        BlockTables bt;
        std::string f = pair_tables(b, bt);
        if (!f.empty()) return f;
        tree_rows.resize((size_t)(b.i1 - b.i0) * b.i1);
        f = dist_block_values(in.algo_id, in.prec, in.k, opt.model, opt.fp32, run.bias, b.i0, b.i1, run.dev.rcard.data(), bt, in.row_name, in.row_id.data(),
                              run.fmt_threads, tree_rows.data());
        if (!f.empty()) return f;
        std::lock_guard<std::mutex> lk(run.tree_mu);
        const int rc = lash_tree_set_rows(run.tree_ctx, run.tree, b.i0, b.i1, tree_rows.data());
        return rc == LASH_OK ? "" : std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(run.tree_ctx);
    }

    // Blocks in turn, each through its mode's step, written in block order whatever order the workers finish in.
    void work()
    {
        int rc = lash_ctx_create(&ctx, run.devices[wi]);
        if (rc == LASH_OK) rc = lash_ctx_set_layout(ctx, &opt.layout);
        if (rc == LASH_OK && opt.has_cluster && !opt.use_tree()) rc = lash_cluster_create(ctx, in.nr, &run.clusters[wi]);
        if (rc == LASH_OK && opt.has_derep) rc = lash_derep_create(ctx, in.nr, &run.derep);
        std::string my_fail = rc == LASH_OK ? "" : std::string(lash_strerror(rc));
        const uint32_t n_blocks = (uint32_t)run.block_begin.size() - 1;
        for (;;) {
            const uint32_t blk = run.next_block.fetch_add(1);
            if (blk >= n_blocks) break;
            const uint32_t i0 = run.block_begin[blk], i1 = run.block_begin[blk + 1];
            const Block b{i0, i1, in.same_files ? std::min(i1, in.nq) : in.nq};   // the triangle: no row of the block prints beyond its own column
            bool skip;
            { std::lock_guard<std::mutex> lk(run.wmu); skip = !run.fail.empty(); }
            row_text.off.clear(); row_text.len.clear();
            if (my_fail.empty() && !skip)
                my_fail = opt.use_tree() ? block_tree(b) : opt.top ? block_top(b) : opt.has_cluster ? block_cluster(b) : opt.has_derep ? block_derep(b)
                          : opt.has_max_dist ? block_within(b) : block_all(b);
            std::unique_lock<std::mutex> lk(run.wmu);
            run.wcv.wait(lk, [&] { return run.next_to_write == blk; });
            if (!my_fail.empty() && run.fail.empty()) run.fail = my_fail;
            if (run.fail.empty())
                for (size_t r = 0; r < row_text.rows(); ++r) fwrite(row_text.data(r), 1, row_text.size(r), run.out);
            ++run.next_to_write;
            lk.unlock();
            run.wcv.notify_all();
        }
    }
};

// --top: the workers' lists merged, the kept pairs in (row, col) order through the --max-dist formatter (every pair passes; same-name
// pairs are in the lists with d = 0 when they are among the K nearest)
std::string finish_top(Run &run)
{
    const DistInput &in = run.in;
    for (size_t w = 1; w < run.tops.size(); ++w)
        if (lash_top_merge(run.tops[0], run.tops[w]) != LASH_OK) return "cannot merge the --top lists";
    uint64_t n = 0;
    std::vector<uint32_t> t_row, t_col;
    std::vector<double> t_dist;
    if (lash_top_result(run.tops[0], nullptr, nullptr, nullptr, 0, &n) == LASH_OK) {
        t_row.resize(n); t_col.resize(n); t_dist.resize(n);
        if (lash_top_result(run.tops[0], t_row.data(), t_col.data(), t_dist.data(), n, &n) != LASH_OK) return "cannot read the --top lists";
    }
    RowText text;
    const std::vector<uint32_t> no_same(in.nr, NO_COLUMN);
    format_block_within(0, in.nr, in.same_files, in.nq, HUGE_VAL, t_row.data(), t_col.data(), t_dist.data(), n, no_same.data(), in.row_name, in.col_tab, text);
    for (size_t r = 0; r < text.rows(); ++r) fwrite(text.data(r), 1, text.size(r), run.out);
    if (run.timing.on) fprintf(stderr, "[lash dist] --top: %llu candidates from the device, %llu rows kept\n",
                               (unsigned long long)run.top_candidates.load(), (unsigned long long)n);
    run.timing.mark("--top: the kept rows written");
    return "";
}

// every name under label[name], the first name of its cluster in row order: the --cluster text after the header
void write_clusters(Run &run, const std::vector<uint32_t> &label, uint64_t *n_clusters)
{
    const DistInput &in = run.in;
    std::vector<uint32_t> by_rep(in.nr);
    std::iota(by_rep.begin(), by_rep.end(), 0u);
    std::stable_sort(by_rep.begin(), by_rep.end(), [&](uint32_t x, uint32_t y) { return label[x] < label[y]; });
    std::string text;
    *n_clusters = 0;
    for (uint32_t i : by_rep) {
        *n_clusters += label[i] == i;
        text.append(in.row_name[label[i]]).push_back('\t');
        text.append(in.row_name[i]).push_back('\n');
        if (text.size() >= (1u << 20)) { fwrite(text.data(), 1, text.size(), run.out); text.clear(); }
    }
    fwrite(text.data(), 1, text.size(), run.out);
}

// --cluster: the workers' clusters merged; every name under its cluster's first name, in row order
std::string finish_cluster(Run &run)
{
    const DistInput &in = run.in;
    const std::vector<lash_cluster *> &cl = run.clusters;
    for (size_t w = 1; w < cl.size(); ++w)
        if (!cl[0] || !cl[w] || lash_cluster_merge(cl[0], cl[w]) != LASH_OK) return "cannot merge the --cluster labels";
    std::vector<uint32_t> label(in.nr);
    if (in.nr && (!cl[0] || lash_cluster_labels(cl[0], label.data()) != LASH_OK)) return "cannot read the --cluster labels";
    uint64_t n_clusters = 0;
    write_clusters(run, label, &n_clusters);
    if (run.timing.on) fprintf(stderr, "[lash dist] --cluster: %llu pairs looked at, %llu pruned as already joined, %llu joined on the device, "
                               "%llu sent to the host, %llu clusters\n", (unsigned long long)run.cl_pairs.load(), (unsigned long long)run.cl_pruned.load(),
                               (unsigned long long)run.cl_joined.load(), (unsigned long long)run.cl_sent.load(), (unsigned long long)n_clusters);
    run.timing.mark("--cluster: the clusters written");
    return "";
}

// --tree / --linkage: the merges on the device, then the Newick text or the clusters of the cut
std::string finish_tree(Run &run)
{
    const DistInput &in = run.in;
    const DistOptions &opt = run.opt;
    if (opt.pcoa) {
        const uint32_t k = opt.pcoa;
        std::vector<double> eig(k), coords((size_t)in.nr * k);
        lash_pcoa_stats st{};
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = lash_tree_build_pcoa(run.tree_ctx, run.tree, k, 0.0, 0, eig.data(), coords.data(), &st);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != LASH_OK) return std::string("--pcoa: ") + lash_strerror(rc) + " " + lash_ctx_last_error(run.tree_ctx);
        if (run.timing.on) fprintf(stderr, "[lash dist] --pcoa: %u names, %llu iterations, %llu products, %llu matrix bytes, shift %.6g, worst residual "
                                           "%.3g, build %.3f ms\n", in.nr, (unsigned long long)st.iterations, (unsigned long long)st.products,
                                   (unsigned long long)st.bytes, st.shift, st.worst_residual, ms);
        const std::string text = pcoa_text(in.row_name, k, eig.data(), coords.data(), st.trace);
        fwrite(text.data(), 1, text.size(), run.out);
        run.timing.mark("--pcoa: the coordinates written");
        return "";
    }
    if (opt.nj) {
        std::vector<lash_nj_join> joins(in.nr > 1 ? in.nr - 1 : 0);
        lash_tree_stats st{};
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = lash_tree_build_nj(run.tree_ctx, run.tree, joins.data(), &st);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != LASH_OK) return std::string("--tree --nj: ") + lash_strerror(rc) + " " + lash_ctx_last_error(run.tree_ctx);
        if (run.timing.on) fprintf(stderr, "[lash dist] --tree --nj: %u names, %llu steps, %llu matrix bytes, build %.3f ms\n", in.nr,
                                   (unsigned long long)st.steps, (unsigned long long)st.bytes, ms);
        std::string err;
        const std::string text = newick_text_nj(in.row_name, joins.data(), err) + "\n";
        if (!err.empty()) return "--tree --nj: " + err;
        fwrite(text.data(), 1, text.size(), run.out);
        run.timing.mark("--tree --nj: the tree written");
        return "";
    }
    const int linkage = opt.linkage < 0 ? LASH_LINKAGE_AVERAGE : opt.linkage;
    std::vector<lash_tree_merge> merges(in.nr > 1 ? in.nr - 1 : 0);
    lash_tree_stats st{};
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = lash_tree_build(run.tree_ctx, run.tree, linkage, merges.data(), &st);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != LASH_OK) return std::string("--tree: ") + lash_strerror(rc) + " " + lash_ctx_last_error(run.tree_ctx);
    if (run.timing.on) fprintf(stderr, "[lash dist] --tree: %u names, %llu steps, %llu rescanned rows, %llu matrix bytes, build %.3f ms\n", in.nr,
                               (unsigned long long)st.steps, (unsigned long long)st.rescanned_rows, (unsigned long long)st.bytes, ms);
    if (opt.tree) {
        std::string err;
        const std::string text = newick_text(in.row_name, merges.data(), err) + "\n";
        if (!err.empty()) return "--tree: " + err;
        fwrite(text.data(), 1, text.size(), run.out);
        run.timing.mark("--tree: the tree written");
        return "";
    }
    std::vector<uint32_t> label;
    if (!tree_cut_labels(in.nr, merges.data(), opt.cluster_dist, label)) return "--linkage: the merge list is not a tree";
    uint64_t n_clusters = 0;
    write_clusters(run, label, &n_clusters);
    if (run.timing.on) fprintf(stderr, "[lash dist] --cluster --linkage: %llu clusters\n", (unsigned long long)n_clusters);
    run.timing.mark("--cluster: the clusters written");
    return "";
}

// --derep: every name under its representative, in row order of the representative, then of the member (a representative is below
// every member of its own, so it comes first)
std::string finish_derep(Run &run)
{
    const DistInput &in = run.in;
    std::vector<uint32_t> rep(in.nr);
    if (in.nr && (!run.derep || lash_derep_result(run.derep, rep.data()) != LASH_OK)) return "cannot read the --derep representatives";
    std::vector<uint32_t> by_rep(in.nr);
    std::iota(by_rep.begin(), by_rep.end(), 0u);
    std::stable_sort(by_rep.begin(), by_rep.end(), [&](uint32_t x, uint32_t y) { return rep[x] < rep[y]; });
    std::string text;
    for (uint32_t i : by_rep) {
        text.append(in.row_name[rep[i]]).push_back('\t');
        text.append(in.row_name[i]).push_back('\n');
        if (text.size() >= (1u << 20)) { fwrite(text.data(), 1, text.size(), run.out); text.clear(); }
    }
    fwrite(text.data(), 1, text.size(), run.out);
    if (run.timing.on) fprintf(stderr, "[lash dist] --derep: %llu pairs looked at, %llu pruned as not a representative, %llu pruned after a sure hit, "
                               "%llu sent to the host, %llu evaluated, %llu representatives\n", (unsigned long long)run.dr.pairs,
                               (unsigned long long)run.dr.pruned_not_rep, (unsigned long long)run.dr.pruned_after_hit,
                               (unsigned long long)run.dr.sent_to_host, (unsigned long long)run.dr.evaluated, (unsigned long long)run.dr.representatives);
    run.timing.mark("--derep: the representatives written");
    return "";
}

}  // namespace

std::string run_dist(const DistOptions &opt)
{
    const Timing timing{};
    DistInput in;
    std::string err = load_input(opt, timing, in);
    if (!err.empty()) return err;
    if (opt.pcoa && in.nr < 2) return "--pcoa needs at least 2 names: " + std::to_string(in.nr) + " cannot be ordinated";
    const bool hll = in.algo_id == LASH_HLL, hmh = in.algo_id == LASH_HMH;
    lash_hll_bias *bias = nullptr;
    if (hll && !opt.hll_bias_file.empty()) {
        const int brc = lash_hll_bias_load(opt.hll_bias_file.c_str(), &bias);
        if (brc != LASH_OK) return "cannot read HLL++ bias tables from " + opt.hll_bias_file + ": " + lash_strerror(brc);
    }
    if (hll && opt.hll_bias_sim) {                                   // once, on the first device, before the cardinalities
        lash_ctx *ctx = nullptr;
        const int dv = opt.devices.empty() ? opt.device : opt.devices[0];
        int rc = lash_ctx_create(&ctx, dv);
        if (rc != LASH_OK) return std::string("--hll-bias-sim: ") + lash_strerror(rc);
        std::vector<double> raw, b;
        std::string line;
        err = simulate_bias(ctx, in.prec, 0, 0, 42, raw, b, line);
        lash_ctx_destroy(ctx);
        if (!err.empty()) return err;
        if (lash_hll_bias_from_arrays(&bias, in.prec, raw.data(), b.data(), (uint32_t)raw.size()) != LASH_OK) return "--hll-bias-sim: bad table";
        fprintf(stderr, "[lash dist] --hll-bias-sim: %s, %s\n", SIM_NOTE, line.c_str());
        timing.mark("--hll-bias-sim: the table simulated");
    }
    struct BiasGuard { lash_hll_bias *b; ~BiasGuard() { lash_hll_bias_free(b); } } bias_guard{bias};

    // Without --devices, two workers share the GPU: while one formats and writes its block the other has the next block's
    // pair statistics computed (a block is GPU work, then -t threads of formatting, then an ordered write).
    DeviceSets dev;
    Run run{opt, in, dev, bias, timing};
    run.devices = opt.devices.empty() ? std::vector<int>{opt.device, opt.device} : opt.devices;
    if (opt.has_derep) {                                                                              // blocks depend on each other in row order
        if (opt.devices.size() > 1) return "--derep runs its blocks in row order on one worker: --devices must name one device";
        run.devices.resize(1);
    }
    if (!(err = make_device_sets(opt, in, run.devices, bias, dev)).empty()) return err;
    timing.mark("sketches resident on the device(s), cardinalities, pair-kernel operands");
    // hyperminhash's expected collisions need the GPU only when some pair has both sketches at or below 2^19 distinct k-mers
    bool small_ref = false, small_qry = false;
    if (hmh) {
        for (double c : dev.rcard) small_ref = small_ref || !(c > 524288.0);
        for (double c : dev.qcard) small_qry = small_qry || !(c > 524288.0);
    }
    run.gpu_ec = small_ref && small_qry;
    run.out = fopen(opt.output_file.c_str(), "w");
    if (!run.out) return "cannot create " + opt.output_file;
    if (opt.tree || opt.pcoa) {}                                                                     // (the tree, or the table of coordinates, is the whole output)
    else if (opt.has_cluster || opt.has_derep) fprintf(run.out, "Representative\tMember\n");
    else if (!opt.matrix) fprintf(run.out, "Reference\tQuery\tDistance\n");                          // main.rs:409-412
    else for (uint32_t j = 0; j < in.nq; ++j) fprintf(run.out, "\t%s", in.col_name[j].c_str());      // main.rs:439-441
    run.block_begin = plan_blocks(opt, in);
    const uint32_t n_blocks = (uint32_t)run.block_begin.size() - 1;
    if (run.devices.size() > n_blocks) run.devices.resize(std::max<uint32_t>(n_blocks, 1));
    run.fmt_threads = std::max(1, opt.threads / (int)run.devices.size());
    run.tops.assign(run.devices.size(), nullptr);
    run.clusters.assign(run.devices.size(), nullptr);
    if (opt.use_tree()) {
        int rc = lash_ctx_create(&run.tree_ctx, run.devices[0]);
        if (rc != LASH_OK) return std::string("--tree: ") + lash_strerror(rc);
        if ((rc = lash_tree_create(run.tree_ctx, in.nr, &run.tree)) != LASH_OK)
            return std::string("--tree: ") + lash_strerror(rc) + " " + lash_ctx_last_error(run.tree_ctx);
    }
    if (opt.top)
        for (lash_top *&t : run.tops)
            if (lash_top_create(in.same_files ? in.nr : in.nq, opt.top, in.same_files ? 1 : 0, &t) != LASH_OK) return "cannot create the --top lists";
    {
        std::vector<std::thread> pool;
        for (size_t d = 1; d < run.devices.size(); ++d) pool.emplace_back([&run, d] { Worker(run, d).work(); });
        Worker(run, 0).work();
        for (auto &t : pool) t.join();
    }
    if (run.fail.empty() && opt.top) run.fail = finish_top(run);
    if (run.fail.empty() && opt.use_tree()) run.fail = finish_tree(run);
    else if (run.fail.empty() && opt.has_cluster) run.fail = finish_cluster(run);
    if (run.fail.empty() && opt.has_derep) run.fail = finish_derep(run);
    fclose(run.out);
    run.out = nullptr;
    timing.mark("all rows written");
    return run.fail;
}

std::string run_hll_bias(const HllBiasOptions &opt)
{
    lash_ctx *ctx = nullptr;
    const int rc = lash_ctx_create(&ctx, opt.device);
    if (rc != LASH_OK) return lash_strerror(rc);
    struct CtxGuard { lash_ctx *c; ~CtxGuard() { lash_ctx_destroy(c); } } guard{ctx};
    std::string text = std::string("# ") + SIM_NOTE + ", written by `lash hll-bias`\n"
                       "# format: \"p <p> <n>\" then n lines \"<raw estimate> <bias>\" (lash dist --hll-bias)\n";
    for (int p : opt.ps) {
        std::vector<double> raw, bias;
        std::string line;
        const std::string err = simulate_bias(ctx, p, opt.points, opt.trials, opt.seed, raw, bias, line);
        if (!err.empty()) return err;
        char buf[96];
        text += "# " + line + "\n";
        snprintf(buf, sizeof buf, "p %d %zu\n", p, raw.size());
        text += buf;
        for (size_t j = 0; j < raw.size(); ++j) {
            snprintf(buf, sizeof buf, "%.17g %.17g\n", raw[j], bias[j]);          // 17 digits: the same doubles when read back
            text += buf;
        }
        fprintf(stderr, "[lash hll-bias] %s, %s\n", SIM_NOTE, line.c_str());
    }
    FILE *f = fopen(opt.output.c_str(), "w");
    if (!f) return "cannot create " + opt.output;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return "cannot write " + opt.output;
    return "";
}

std::string load_dist_side(const DistOptions &opt, DistSide &out)
{
    DistOptions one = opt;
    one.query_prefix = opt.ref_prefix;
    one.matrix = true;                                               // (no tabbed column names: nothing is printed from here)
    const Timing timing{false};                                      // (the caller reports its own times)
    DistInput in;
    const std::string err = load_input(one, timing, in);
    if (!err.empty()) return err;
    out.algo_id = in.algo_id;
    out.prec = in.prec;
    out.ull_est = in.ull_est;
    out.k = in.k;
    out.names = std::move(in.rnames);
    out.order = std::move(in.rorder);
    out.images = std::move(in.rimg_store);
    std::map<std::string, std::string> found;
    if (find_files(opt.ref_prefix, found).empty()) out.params_file = found["params"];
    return "";
}

std::string load_hll_bias(const DistOptions &opt, int algo_id, int prec, const char *tag, lash_hll_bias **out)
{
    *out = nullptr;
    if (algo_id != LASH_HLL) return "";
    if (!opt.hll_bias_file.empty()) {
        const int brc = lash_hll_bias_load(opt.hll_bias_file.c_str(), out);
        if (brc != LASH_OK) return "cannot read HLL++ bias tables from " + opt.hll_bias_file + ": " + lash_strerror(brc);
    }
    if (opt.hll_bias_sim) {
        lash_ctx *ctx = nullptr;
        const int rc = lash_ctx_create(&ctx, opt.device);
        if (rc != LASH_OK) return std::string("--hll-bias-sim: ") + lash_strerror(rc);
        std::vector<double> raw, b;
        std::string line;
        const std::string err = simulate_bias(ctx, prec, 0, 0, 42, raw, b, line);
        lash_ctx_destroy(ctx);
        if (!err.empty()) return err;
        if (lash_hll_bias_from_arrays(out, prec, raw.data(), b.data(), (uint32_t)raw.size()) != LASH_OK) return "--hll-bias-sim: bad table";
        fprintf(stderr, "[%s] --hll-bias-sim: %s, %s\n", tag, SIM_NOTE, line.c_str());
    }
    return "";
}

}  // namespace lashhost
