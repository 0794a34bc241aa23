// dist.hpp — `lash dist` (/root/reference/src/main.rs:280-617, utils.rs:84-373): the consumer of the sketch files.
// SURVEY.md §8(f) row f2 ("next"): not part of the round-1 hot path.
#pragma once
#include <string>
#include <vector>

#include "../../../include/lash_gfx950.h"

namespace lashhost {

struct DistOptions {
    std::string query_prefix, ref_prefix, output_file = "dist", estimator = "fgra";
    int model = 1;          // 1 = Poisson: min(-ln(f)/k, 1); 0 = binomial: 1 - f^(1/k)   (main.rs:415-423)
    int threads = 1;
    bool fp32 = false, matrix = false;
    bool file_order = false;   // rows / columns / triangle in list-file order instead of the reference's map order (name_order.hpp)
    int device = 0;
    std::vector<int> devices;  // --devices 0,1,...: one worker per entry, blocks of reference rows in turn; empty = {device}
    uint32_t block_rows = 0;   // reference rows per GPU call; 0 = as many as keep the pair tables under ~0.5 GB
    bool has_max_dist = false; // --max-dist D: print only the rows whose distance d passes d <= D (list form only)
    double max_dist = 0.0;
    uint32_t top = 0;          // --top K (1..LASH_TOP_MAX): print only the rows in some name's K nearest (list form only); 0 = off
    bool has_cluster = false;  // --cluster D: single-linkage clusters of a triangle run instead of pairs; names are linked iff --max-dist D prints them
    double cluster_dist = 0.0;
    bool tree = false;         // --tree: one Newick tree of all names of a triangle run instead of pairs (agglomerative, merged on the device)
    bool nj = false;           // --nj (with --tree): the neighbour-joining tree instead of a linkage tree (lash_tree_build_nj)
    int linkage = -1;          // --linkage average|single|complete: LASH_LINKAGE_*; -1 = not given (--tree: average; --cluster: single, the
                               // union-find route, which an explicit single takes too; average / complete cut the tree at D)
    uint32_t pcoa = 0;         // --pcoa K (1..16): the K principal coordinates of all names of a triangle run instead of pairs, from the same
                               // matrix on the device (lash_tree_build_pcoa); 0 = off
    bool use_tree() const { return tree || pcoa || (has_cluster && (linkage == LASH_LINKAGE_AVERAGE || linkage == LASH_LINKAGE_COMPLETE)); }
    bool has_derep = false;    // --derep D: greedy representatives of a triangle run in row order; "within D" iff --max-dist D prints the pair
    double derep_dist = 0.0;
    int measure = LASH_MEASURE_JACCARD;   // --containment query|reference: LASH_MEASURE_CONTAIN_*; directional, so the run is a rectangle even
                               // when -q and -r name the same files (list form only; not with --cluster / --derep)
    std::string hll_bias_file; // --hll-bias / $LASH_HLL_BIAS: HLL++ bias tables (lash_hll_bias_load); empty = that regime is refused
    bool hll_bias_sim = false; // --hll-bias-sim: for hll sketches, simulate the table of their p on the first device (lash_hll_bias_simulate,
                               // defaults) and go on as if it had come from --hll-bias; nothing at all for hmh / ull
    lash_layout layout;        // --layout / $LASH_LAYOUT (include/lash_gfx950.h)
    DistOptions() { lash_layout_default(&layout); }
};

std::string run_dist(const DistOptions &opt);

// `lash hll-bias`: the HLL++ bias tables of the precisions `ps`, simulated on `device`, as the text file lash_hll_bias_load reads
struct HllBiasOptions {
    std::string output;
    std::vector<int> ps;       // each 4..18
    uint32_t points = 0, trials = 0;   // 0 = the defaults of lash_hll_bias_simulate; points above 5 * 2^p + 1 are cut to that for a small p
    uint64_t seed = 42;
    int device = 0;
};
std::string run_hll_bias(const HllBiasOptions &opt);

// One collection as `dist` reads a side of a run ({prefix}_sketches.bin, {prefix}_files.json, {prefix}_parameters.json), for the
// commands that take a single collection (growth.cpp): opt.ref_prefix names it; estimator, file_order and layout are honoured.
struct DistSide {
    int algo_id = 0, prec = 0, ull_est = 0, k = 0;
    std::vector<std::string> names;      // the name file
    std::vector<uint32_t> order;         // the rows, as indices into names: the reference's key order, or list order under file_order
    std::vector<uint8_t> images;         // the sketch file, inflated: one image per name
    std::string params_file;             // the collection's parameters JSON, as found (merge.cpp copies it)
};
std::string load_dist_side(const DistOptions &opt, DistSide &out);
// The HLL++ tables of a run, as `dist` gets them (--hll-bias FILE / --hll-bias-sim on opt.device): *out stays NULL for hmh / ull sketches
// and when no tables were asked for.  tag names the command in the provenance line.  The caller frees *out (lash_hll_bias_free).
std::string load_hll_bias(const DistOptions &opt, int algo_id, int prec, const char *tag, lash_hll_bias **out);

}  // namespace lashhost
