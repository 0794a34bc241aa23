// main.cpp — the `lash` command line of the gfx950 build, on top of liblash_gfx950.so.  One function per command:
//   sketch    FASTA/FASTQ files to sketches: the reference's flags (its src/main.rs:30-96, 180-279) and the GPU-side extras
//   dist      distances between two sets of sketches (main.rs:107-176, 280-617) and the output forms built on them
//   growth    union cardinality of a collection along orderings                           (not upstream)
//   merge     one sketch per group of a collection's sketches                             (not upstream)
//   spectrum  how the k-mers of each group's union are shared among its members, hmh      (not upstream)
//   screen    winner-takes-all containment of samples against a database, hmh             (not upstream)
//   hll-bias  the HLL++ bias tables `dist --hll-bias` reads, simulated                    (not upstream)
// Every option is described once, in usage() below; --layout SPEC (or $LASH_LAYOUT) in include/lash_gfx950.h (`lash_layout`).
// Each cmd_* is its option table, the checks that are its own, the assignments into its options struct, and the run; parsing,
// the typed values and the checks several commands share are in cli_args.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/lash_gfx950.h"
#include "cli_args.hpp"
#include "dist.hpp"
#include "growth.hpp"
#include "merge.hpp"
#include "screen.hpp"
#include "sketch_files.hpp"
#include "spectrum.hpp"

using namespace lashhost;

namespace {

const char *VERSION = "0.1.4";      // main.rs:27 (hard-coded there although the crate is 0.1.6)

void usage()
{
    fprintf(stderr,
            "Fast and Memory Efficient (Meta)genome Sketching via HyperLogLog, HyperMinhash and UltraLogLog (MI355X build)\n\n"
            "Usage: lash <COMMAND>\n\nCommands:\n"
            "  sketch  Sketches genomes and serializes them, sketches are compressed\n"
            "  dist    Computes distance between sketches\n"
            "  growth  Union cardinality of a collection along orderings: how much each further genome adds\n"
            "  merge   One sketch per group of a collection's sketches (clusters, the files of a sample), united on the GPU\n"
            "  spectrum  How the k-mers of each group's union are shared among its members: core, shell and cloud (hmh sketches)\n"
            "  screen  What is in a sample: references scored by containment, every shared k-mer credited to its best reference only (hmh sketches)\n"
            "  hll-bias  Simulates the HLL++ bias tables on the GPU and writes the file dist --hll-bias reads\n\n"
            "sketch options:\n"
            "  -f, --file <file>            One file containing list of FASTA/FASTQ files (.gz/.zstd supported), one per line\n"
            "  -o, --output <output>        Input a prefix/name for your output files [default: sketch]\n"
            "  -k, --kmer <kmer_length>     Length of the kmer [default: 16]\n"
            "  -t, --threads <threads>      Number of threads to use, default to all logical cores\n"
            "  -a, --algorithm <algorithm>  HyperMinHash (hmh), UltraLogLog (ull), or HyperLogLog (hll) [default: hmh]\n"
            "  -p, --precision <precision>  Specifiy precision, for ull and hll only. [default: 10]\n"
            "  -s, --seed <seed>            Random seed [default: 42]\n"
            "      --aa                     Amino acid sketching (k 1-12); the reference carries this flag commented out\n"
            "      --per-record             One sketch per FASTA record instead of one per file (multi-FASTA collections; like Mash -i);\n"
            "                               {output}_files.json then holds the record ids.  FASTA only, not with --aa\n"
            "      --window <W>             One sketch per W-base window of every FASTA record (W >= k; the windows are cut on the GPU, do not\n"
            "                               overlap and never span two records; a record's last, shorter window is kept).  {output}_files.json\n"
            "                               then holds ID:B-E, the record id and the 1-based inclusive range.  FASTA only, not with --aa or\n"
            "                               --min-count; --per-record changes nothing\n"
            "      --translate              Protein sketches of nucleotide FASTA: every record is translated on the GPU in all six reading frames\n"
            "                               (standard code; ACGT in either case, any other byte makes its codon ambiguous) and sketched like --aa,\n"
            "                               no k-mer spanning a stop, an ambiguous codon, two frames or two records.  Needs -k 1..12 (the default\n"
            "                               16 is refused).  One sketch per file, or per record with --per-record; the output reads like --aa\n"
            "                               output (molecule: amino_acid).  FASTA only; takes about 5 x --batch-mb of device memory; not with\n"
            "                               --aa, --min-count or --window\n"
            "      --min-count <M>          Keep only the k-mers a file holds at least M times (1-255; read sets: a sequencing error makes\n"
            "                               k-mers seen once; like Mash -m).  Counted per file on the GPU in 2^L saturating cells, two cells\n"
            "                               per k-mer; a rarer k-mer gets in only when collisions fill both.  Files are read twice.  hmh,\n"
            "                               hll -p <= 15, ull -p <= 14; not with --aa or --per-record\n"
            "      --count-cells-log2 <L>   with --min-count: cells per file, 10-36 [default: ceil(log2(8 x file bytes)), within 16-36]\n"
            "      --gpus <n> | --device <d> | --devices <d,d,...>  GPUs to use, one worker each [default: device 0]\n"
            "dist options:\n"
            "  -q, --query <prefix>  -r, --reference <prefix>  -o, --output_file <name> [default: dist]\n"
            "  -t, --threads <n>  -e, --estimator <fgra|ml>  -m, --model <1|0>  --fp32  --dm\n"
            "      --file-order   rows and columns in list-file order (default: the reference's hash-map key order)\n"
            "      --max-dist <D> print only the pairs whose distance is <= D (same rows, same order; not with --dm)\n"
            "      --top <K>      print only each query's K nearest (triangle runs: a pair in either name's K nearest; the\n"
            "                     name itself counts, so use K+1 for K others), K 1-1024; same rows, same order; not with --dm\n"
            "      --cluster <D>  all-vs-all only (-q and -r the same sketch files): single-linkage clusters instead of pairs; two\n"
            "                     names are linked iff --max-dist D prints their pair.  Output: Representative<TAB>Member, one line\n"
            "                     per name, the representative being the cluster's first name in row order; not with --dm,\n"
            "                     --top or --max-dist\n"
            "      --derep <D>    all-vs-all only: greedy dereplication instead of pairs.  Names are walked in row order; a name is a\n"
            "                     Representative iff no earlier representative is within D of it (--max-dist D prints their pair),\n"
            "                     else a member of the first such representative.  Row order is the priority: pass --file-order to\n"
            "                     set it with the list file.  Output: Representative<TAB>Member, one line per name; not with --dm,\n"
            "                     --top, --max-dist, --cluster or more than one entry in --devices\n"
            "      --tree         all-vs-all only: one Newick tree of all names instead of pairs, followed by a newline.  Agglomerative\n"
            "                     clustering of the printed distances, merged on the GPU (8 x N^2 bytes of device memory); --linkage\n"
            "                     says how [default: average, UPGMA].  Branch lengths are half the difference of the merge heights; a\n"
            "                     name with any of ()[]':;, or white space is quoted.  Not with --dm, --top, --max-dist, --cluster,\n"
            "                     --derep or --containment\n"
            "      --linkage <average|single|complete>  with --tree or --cluster: the distance of two clusters is the mean, the\n"
            "                     smallest or the largest distance of their members.  --cluster D --linkage average|complete cuts\n"
            "                     that tree at height D (same output form); single [the default of --cluster] is --cluster as above\n"
            "      --nj           with --tree: the neighbour-joining tree (Saitou & Nei; the rule of PHYLIP neighbor, QuickTree, rapidNJ,\n"
            "                     mashtree) instead of a linkage tree, joined on the GPU from the same matrix.  It assumes no clock, so\n"
            "                     it is the one to read as a phylogeny; it is unrooted (the root prints as a trifurcation) and a branch\n"
            "                     length may be negative.  Not with --linkage or --cluster: an NJ tree has no heights to cut\n"
            "      --pcoa <K>     all-vs-all only: principal coordinates (PCoA, classical MDS; skbio pcoa, ape::pcoa, cmdscale) of all names\n"
            "                     instead of pairs, K 1-16.  The matrix of printed distances is Gower-centred and its K algebraically largest\n"
            "                     eigenpairs are solved on the GPU (8 x N^2 bytes of device memory).  Output, tab-separated, numbers as\n"
            "                     %%.10g: #Eigenvalue and K values; #Explained and K values, eigenvalue / trace (they can sum past 1: sketch\n"
            "                     distances are not Euclidean and the trace counts the negative eigenvalues); Name PC1 .. PCK; one line per\n"
            "                     name in row order.  An axis whose eigenvalue is <= 0, or beyond N - 1, is all zeros; where eigenvalues\n"
            "                     coincide the axes are one valid basis of their space.  Not with --dm, --top, --max-dist, --cluster, --derep,\n"
            "                     --containment, --tree, --nj or --linkage\n"
            "      --containment <query|reference>  the distance of the containment fraction instead of the Jaccard-derived one, for sides\n"
            "                     of different size (a genome against a metagenome, a plasmid against its host): query = how much of the\n"
            "                     query is in the reference, reference = how much of the reference is in the query.  Directional, so\n"
            "                     always the rectangle: -q and -r on the same files print the full square, both orientations.  Works\n"
            "                     with --max-dist and --top (per query); not with --dm, --cluster or --derep\n"
            "      --hll-bias <file>  HLL++ bias tables (lash hll-bias, or tools/ref_probe/extract_hll_bias.py) [default: $LASH_HLL_BIAS];\n"
            "                     without them hll estimates <= 5 * 2^p are refused\n"
            "      --hll-bias-sim hll sketches only: simulate the bias table of their precision on the GPU at start-up (as lash hll-bias\n"
            "                     does with its defaults) and use it; regenerated measurements, not the reference crate's numbers.\n"
            "                     Not with --hll-bias; $LASH_HLL_BIAS is ignored\n"
            "growth options:\n"
            "  -r, --reference <prefix>     The collection: {prefix}_sketches.bin, _files.json and _parameters.json, read as dist reads a side\n"
            "  -o, --output_file <name>     Where the table goes [default: growth]: Order<TAB>Step<TAB>Name<TAB>Union<TAB>New, one line per\n"
            "                               (order, step), steps from 1.  Union = the estimated distinct k-mers of the order's first Step names\n"
            "                               (the number dist's cardinalities give for the merged sketch), New = Union minus the line before\n"
            "                               (an estimate can go down by a hair: New may be negative); both with three decimals\n"
            "      --orders <P>             Orderings to walk [default: 1].  Order 0 is the row order: the reference's hash-map key order, or\n"
            "                               list-file order with --file-order.  Orders 1 .. P-1 are Fisher-Yates shuffles of it, drawn from\n"
            "                               splitmix64 seeded with --seed: the same options give the same file\n"
            "      --seed <S>               Seed of the shuffles [default: 42]\n"
            "      --file-order             order 0 in list-file order\n"
            "  -e, --estimator <fgra|ml>  -t, --threads <n> (formatting only; the bytes do not depend on it)  --device <D>\n"
            "      --hll-bias <file> | --hll-bias-sim   as for dist: without tables an hll union with an estimate <= 5 * 2^p is refused\n"
            "                               All orders are folded on the GPU in one pass per chunk of orders; hmh, hll, and ull up to -p 16\n"
            "merge options:\n"
            "  -r, --reference <prefix>     The collection, read as dist reads a side\n"
            "  -o, --output <prefix>        Where the merged collection goes: {prefix}_sketches.bin, _files.json (the group names) and\n"
            "                               _parameters.json (the input's, copied): dist, growth and merge read it like any other\n"
            "      --groups <file>          Lines of group<TAB>member, a member being a name of the collection: what dist --cluster and\n"
            "                               --derep write, heading line included.  One sketch per group, the union of its members, in order\n"
            "                               of first appearance.  A member may be in several groups; a name several sketches carry selects\n"
            "                               all of them.  Blank lines are skipped; a line without exactly one tab, an empty name or an\n"
            "                               unknown member is refused with its line number\n"
            "      --all <name>             One group of every sketch instead, called <name>; not with --groups or --keep-others\n"
            "      --keep-others            Sketches in no group follow the groups under their own names, in row order (the reference's\n"
            "                               key order, where a repeated name is one row; list order with --file-order) [default: dropped,\n"
            "                               and counted on stderr]\n"
            "      --file-order  --device <D>  -t, --threads <n> (compression only; the bytes of the sketches do not depend on it)\n"
            "spectrum options:\n"
            "  -r, --reference <prefix>     The collection, read as dist reads a side; HyperMinHash sketches only (an hll or ull register\n"
            "                               does not identify a k-mer: such a collection is refused)\n"
            "  -o, --output <prefix>        Where the tables go.  {prefix}_spectrum.tsv: Group<TAB>Members<TAB>Count<TAB>Buckets<TAB>Kmers, one line per\n"
            "                               group and count c >= 1 that has buckets: Buckets of the occupied buckets hold a k-mer that exactly c\n"
            "                               members have, Kmers = Buckets / occupied x the union's distinct k-mers.  {prefix}_groups.tsv:\n"
            "                               Group<TAB>Members<TAB>Occupied<TAB>Union<TAB>Core<TAB>Shell<TAB>Cloud, one line per group; floats with three decimals\n"
            "      --groups <file>          Lines of group<TAB>member as for merge (what dist --cluster and --derep write).  A sketch counts once\n"
            "                               per group however often its name is listed; two sketches that carry one name count as two\n"
            "      --all <name>             One group of every sketch, called <name> [the default, called all]; not with --groups\n"
            "      --core <F>               A count c of a group of n members is core iff c >= F x n [default: 0.95] ...\n"
            "      --cloud <F>              ... cloud iff c < F x n [default: 0.15], else shell.  Both in (0, 1], cloud <= core\n"
            "      --curves                 Also {prefix}_curves.tsv: Group<TAB>Genomes<TAB>Pan<TAB>Core, one line per group and m = 1 .. n: the expected\n"
            "                               distinct k-mers of the union (Pan) and of the intersection (Core) of m members, exactly, over all\n"
            "                               subsets of m members (growth --orders P samples orderings instead)\n"
            "      --file-order  --device <D>  --layout <SPEC>  -t, --threads <n> (accepted as for merge; the tables do not depend on them)\n"
            "screen options:\n"
            "  -r, --reference <prefix>     The database, read as dist reads a side; HyperMinHash sketches only (an hll or ull collection is refused)\n"
            "  -q, --query <prefix>         The samples (metagenomes, read sets), sketched with the same -k; HyperMinHash too\n"
            "  -o, --output <file>          Where the table goes: Query<TAB>Reference<TAB>Shared<TAB>Won<TAB>Buckets<TAB>Distance<TAB>WtaDistance, queries in\n"
            "                               row order (the reference's key order, or list order with --file-order), a query's references best\n"
            "                               first.  Distance = what dist --containment reference prints for the pair (the same name prints its\n"
            "                               own distance, not 0).  Shared = the buckets whose sampled k-mer of the query is one of the\n"
            "                               reference's; Won = those of them no better reference of the query holds (winner takes all, like mash\n"
            "                               screen -w); Buckets = the buckets either sketch occupies.  WtaDistance = Distance recomputed with\n"
            "                               Won in the place of Shared.  Better: Distance ascending, then the larger reference, then its row\n"
            "      --max-dist <D>           The candidates of a query are the references with Distance <= D, and a row is printed iff its\n"
            "                               WtaDistance <= D too, D in [0, 1] [default: every reference whose collision-corrected similarity is\n"
            "                               positive: Distance < 1]\n"
            "      --keep-losers            Print every candidate, also those whose WtaDistance no longer passes\n"
            "  -m, --model <1|0>  --file-order  --block-rows <N>  --device <D>  --layout <SPEC>  -t, --threads <n> (the bytes do not depend on\n"
            "                               --block-rows or -t)\n"
            "                               A 5 Mbp genome in a 5 Gbp sample rests on about 16 of the 16384 buckets: winner takes all removes\n"
            "                               redundancy, it does not add resolution\n"
            "hll-bias options:\n"
            "  -o, --output <file>          Where the tables go (text: \"p <p> <n>\" then n lines \"<raw estimate> <bias>\")\n"
            "  -p, --precision <p[,p...]>   Precisions to simulate, each 4-18 [default: 4,5,...,18]\n"
            "      --points <N>             Cardinalities per table, evenly spaced over 0..5*2^p: 6 to 5*2^p+1 (more is cut to that)\n"
            "                               [default: 200]\n"
            "      --trials <T>             Random sets per table [default: 2048]\n"
            "      --seed <S>               Seed of the sets; the same options give the same file [default: 42]\n"
            "      --device <D>             GPU to use [default: 0]\n");
}

// sketch, dist and hll-bias take an unknown --name (and its value) in silence, as they always have: candidates to close separately
const Command SKETCH = {{{"file", 'f', true}, {"output", 'o', true}, {"kmer", 'k', true}, {"threads", 't', true}, {"algorithm", 'a', true},
                         {"precision", 'p', true}, {"seed", 's', true}, {"aa", 0, false}, {"per-record", 0, false}, {"window", 0, true},
                         {"translate", 0, false}, {"min-count", 0, true}, {"count-cells-log2", 0, true}, {"gpus", 0, true}, {"device", 0, true},
                         {"devices", 0, true}, {"batch-mb", 0, true}, {"stream-mb", 0, true}, {"hmh-x-low", 0, false}, {"layout", 0, true}}, false};
const Command DIST = {{{"query", 'q', true}, {"reference", 'r', true}, {"output_file", 'o', true}, {"threads", 't', true}, {"estimator", 'e', true},
                       {"model", 'm', true}, {"fp32", 0, false}, {"dm", 0, false}, {"file-order", 0, false}, {"max-dist", 0, true}, {"top", 0, true},
                       {"cluster", 0, true}, {"derep", 0, true}, {"tree", 0, false}, {"linkage", 0, true}, {"nj", 0, false}, {"pcoa", 0, true},
                       {"containment", 0, true}, {"hll-bias", 0, true}, {"hll-bias-sim", 0, false}, {"device", 0, true}, {"devices", 0, true},
                       {"block-rows", 0, true}, {"layout", 0, true}}, false};
const Command HLL_BIAS = {{{"output", 'o', true}, {"precision", 'p', true}, {"points", 0, true}, {"trials", 0, true}, {"seed", 0, true},
                           {"device", 0, true}}, false};
// one collection, one table: whatever else `dist` takes (-q, --dm, --top, ...) is not an option of these commands
const Command GROWTH = {{{"reference", 'r', true}, {"output_file", 'o', true}, {"threads", 't', true}, {"estimator", 'e', true}, {"orders", 0, true},
                         {"seed", 0, true}, {"file-order", 0, false}, {"hll-bias", 0, true}, {"hll-bias-sim", 0, false}, {"device", 0, true},
                         {"layout", 0, true}}, true};
const Command MERGE = {{{"reference", 'r', true}, {"output", 'o', true}, {"threads", 't', true}, {"groups", 0, true}, {"all", 0, true},
                        {"keep-others", 0, false}, {"file-order", 0, false}, {"device", 0, true}, {"layout", 0, true}}, true};
const Command SPECTRUM = {{{"reference", 'r', true}, {"output", 'o', true}, {"threads", 't', true}, {"groups", 0, true}, {"all", 0, true},
                           {"core", 0, true}, {"cloud", 0, true}, {"curves", 0, false}, {"file-order", 0, false}, {"device", 0, true},
                           {"layout", 0, true}}, true};
const Command SCREEN = {{{"reference", 'r', true}, {"query", 'q', true}, {"output", 'o', true}, {"threads", 't', true}, {"model", 'm', true},
                         {"max-dist", 0, true}, {"keep-losers", 0, false}, {"file-order", 0, false}, {"block-rows", 0, true}, {"device", 0, true},
                         {"layout", 0, true}}, true};

int panic(const char *what)                     // where the reference panics: its message, exit code 101
{
    fprintf(stderr, "%s\n", what);
    return 101;
}

int cmd_sketch(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, SKETCH)) return 2;
    if (a.has("help")) { usage(); return 0; }
    if (!a.require({{"file", "file"}})) return 2;
    SketchOptions opt;
    const std::string output = a.str("output", "sketch"), alg = a.str("algorithm", "hmh");
    uint64_t k = 16, p = 10, seed = 42, threads = std::thread::hardware_concurrency(), gpus = 0, dev = 0, batch_mb = 64, stream_mb = 1024,
             w = 0, m = 0, l2 = 0;
    if (!a.u64("kmer", k) || !a.u64("precision", p) || !a.u64("seed", seed) || !a.u64("threads", threads) || !a.u64("gpus", gpus) ||
        !a.u64("device", dev) || !a.u64("batch-mb", batch_mb) || !a.u64("stream-mb", stream_mb))
        return 2;
    static_assert(LASH_HMH == 0 && LASH_HLL == 1 && LASH_ULL == 2, "the place in the word list is the algorithm");
    if (!a.choice("algorithm", {"hmh", "hll", "ull"}, opt.algo, nullptr)) return panic("Algorithm must be either hmh, ull, or hll");   // main.rs:245
    if (k < 1 || k > 32) return panic("k-mer length must be 1-32");                                                                      // utils.rs:501
    const char *amino_k = "k-mer length for amino acid must be 1\xe2\x80\x93" "12";                                                      // utils.rs:554
    const bool amino = a.has("aa");                                                            // main.rs:97-104 (commented out there)
    opt.per_record = a.has("per-record");
    opt.translate = a.has("translate");
    if (!a.allowed("translate", {{"aa", "--translate takes nucleotide input and makes the proteins itself"},
                                 {"min-count", "k-mers are counted for nucleotide sketches only"},
                                 {"window", "windows of translated records are not supported"}}))
        return 2;
    if (!a.u64("window", w, 1, UINT64_MAX, "a positive integer is required") ||
        !a.allowed("window", {{"aa", "windows are cut for nucleotide FASTA only"},
                              {nullptr, std::to_string(w) + " is shorter than -k " + std::to_string(k) + ": no window would hold a k-mer", w < k},
                              {"min-count", "k-mers are counted per file"}}))
        return 2;
    if (opt.translate && k > 12) return panic(amino_k);                                        // the --aa message
    if (!a.allowed("per-record", {{"aa", "records are split for nucleotide FASTA only"}})) return 2;
    if (amino && k > 12) return panic(amino_k);
    if (!a.allowed("count-cells-log2", {{nullptr, "needs --min-count", !a.has("min-count")}})) return 2;
    // the filtered launch exists where the sketch's registers are a plain table in LDS (include/lash_gfx950.h)
    const uint64_t max_p = opt.algo == LASH_HLL ? 15 : 14;
    if (!a.u64("min-count", m, 1, 255, "an integer from 1 to 255 is required") ||
        !a.u64("count-cells-log2", l2, 10, 36, "an integer from 10 to 36 is required") ||
        !a.allowed("min-count", {{"aa", "k-mers are counted for nucleotide input only"},
                                 {"per-record", "k-mers are counted per file"},
                                 {nullptr, "supports -a " + alg + " up to -p " + std::to_string(max_p) + " (and -a hmh); -p " + std::to_string(p) +
                                           " is not supported", opt.algo != LASH_HMH && p > max_p}}))
        return 2;
    opt.window = w;
    opt.min_count = (uint32_t)m;
    opt.count_cells_log2 = (int)l2;
    opt.k = (int)k;
    opt.precision = (int)p;
    opt.seed = seed;
    opt.threads = (int)std::max<uint64_t>(1, threads);
    opt.batch_bytes = std::max<uint64_t>(1, batch_mb) << 20;
    opt.stream_bytes = std::max<uint64_t>(1, stream_mb) << 20;
    opt.flags = (a.has("hmh-x-low") ? LASH_F_HMH_X_LOW : 0) | (amino || opt.translate ? LASH_F_AMINO : 0);
    if (!layout_option(a, opt.layout) || !devices_option(a, opt.devices)) return 2;   // --devices: the workers, e.g. 0,1,2,3 (0,0 = two on GPU 0)
    if (!a.has("devices")) {
        if (gpus > 0) for (uint64_t d = 0; d < gpus; ++d) opt.devices.push_back((int)d);
        else opt.devices.push_back((int)dev);
    }

    std::vector<std::string> files;
    std::string err = read_list_file(a.str("file"), files);
    if (!err.empty()) return finish(err, "");
    SketchStats st;
    err = sketch_files(opt, files, output, &st);
    if (opt.window && err.rfind("--window takes FASTA input", 0) == 0) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }   // a refusal of the flag
    if (err.empty()) err = write_parameters_json(output, alg, opt.k, opt.precision, opt.seed, amino || opt.translate);
    if (!err.empty()) return finish(err, "");
    if (opt.window)
        fprintf(stderr, "sketched %llu windows of %llu files (%.3f GB of FASTA text) in %.2f s on %zu GPU(s), %llu batches\n",
                (unsigned long long)st.records, (unsigned long long)st.files, st.bytes / 1e9, st.seconds, opt.devices.size(),
                (unsigned long long)st.batches);
    else if (opt.per_record)
        fprintf(stderr, "sketched %llu records of %llu files (%.3f GB of FASTA text) in %.2f s on %zu GPU(s), %llu batches\n",
                (unsigned long long)st.records, (unsigned long long)st.files, st.bytes / 1e9, st.seconds, opt.devices.size(),
                (unsigned long long)st.batches);
    else
        fprintf(stderr, "sketched %llu files (%.3f GB of FASTA/FASTQ text) in %.2f s on %zu GPU(s), %llu batches\n",
                (unsigned long long)st.files, st.bytes / 1e9, st.seconds, opt.devices.size(), (unsigned long long)st.batches);
    return 0;
}

// what `dist` looks a prefix's three files up by (dist.cpp find_files): the part after the last '/', without a leading "./"
std::string prefix_stem(const std::string &prefix)
{
    const size_t slash = prefix.find_last_of('/');
    std::string stem = slash == std::string::npos ? prefix : prefix.substr(slash + 1);
    if (stem.rfind("./", 0) == 0) stem = stem.substr(2);
    return stem;
}

// The output forms of dist stand in the order they were added; each names the earlier ones it cannot go with, so a new form is one
// more block at the end: its value, its rules (the first that hits is the refusal), its field of DistOptions.
int cmd_dist(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, DIST)) return 2;
    if (a.has("help")) { usage(); return 0; }
    if (!a.require({{"query", "query"}, {"reference", "reference"}}, true)) return 2;
    DistOptions opt;
    opt.query_prefix = a.str("query");
    opt.ref_prefix = a.str("reference");
    opt.output_file = a.str("output_file", "dist");
    opt.estimator = a.str("estimator", "fgra");
    uint64_t model = 1, block_rows = 0, top = 0, pcoa = 0;
    int contain = 0;
    if (!a.u64("block-rows", block_rows) || !a.u64("model", model) || !threads_device_order(a, opt) || !bias_source(a, opt) ||
        !devices_option(a, opt.devices))
        return 2;
    opt.block_rows = (uint32_t)std::min<uint64_t>(block_rows, 0xFFFFFFFFull);
    opt.model = (int)model;
    opt.fp32 = a.has("fp32");
    opt.matrix = a.has("dm");
    const Rule all_vs_all = {nullptr, "needs an all-vs-all run: -q and -r must name the same sketch files",
                             prefix_stem(opt.query_prefix) != prefix_stem(opt.ref_prefix)};
    if (!a.real("max-dist", opt.max_dist) || !a.allowed("max-dist", {{"dm", "a square matrix cannot drop cells"}})) return 2;
    if (!a.u64("top", top, 1, LASH_TOP_MAX, "an integer from 1 to " + std::to_string(LASH_TOP_MAX) + " is required") ||
        !a.allowed("top", {{"dm", "a square matrix cannot drop cells"}}))
        return 2;
    if (!a.real("cluster", opt.cluster_dist) ||
        !a.allowed("cluster", {{"dm", "clusters are not a matrix"},
                               {"top", "it prints clusters, not pairs"},
                               {"max-dist", "--cluster D is its own cutoff"}}))
        return 2;
    if (!a.real("derep", opt.derep_dist) ||
        !a.allowed("derep", {{"dm", "representatives are not a matrix"},
                             {"top", "it prints representatives, not pairs"},
                             {"max-dist", "--derep D is its own cutoff"},
                             {"cluster", "greedy representatives or single-linkage clusters, not both"},
                             {nullptr, "cannot be used with more than one entry in --devices: a block of rows is decided from the "
                                       "representatives of the blocks before it, so the blocks run in row order on one worker", opt.devices.size() > 1}}))
        return 2;
    if (!a.choice("containment", {"query", "reference"}, contain, "query or reference is required") ||
        !a.allowed("containment", {{"dm", "list form only"},
                                   {"cluster", "clusters need a symmetric distance"},
                                   {"derep", "representatives need a symmetric distance"}}))
        return 2;
    if (!a.allowed("tree", {{"dm", "a tree is not a matrix"},
                            {"top", "a tree needs every pair"},
                            {"max-dist", "a tree needs every pair"},
                            {"cluster", "the whole tree or its cut at D, not both"},
                            {"derep", "a tree or greedy representatives, not both"},
                            {"containment", "a tree needs a symmetric distance"},
                            all_vs_all}))
        return 2;
    static_assert(LASH_LINKAGE_AVERAGE == 0 && LASH_LINKAGE_SINGLE == 1 && LASH_LINKAGE_COMPLETE == 2, "the place in the word list is the linkage");
    if (!a.choice("linkage", {"average", "single", "complete"}, opt.linkage, "average, single or complete is required") ||
        !a.allowed("linkage", {{nullptr, "needs --tree or --cluster (it says how their clusters are merged)", !a.has("tree") && !a.has("cluster")}}))
        return 2;
    if (!a.allowed("nj", {{"cluster", "a neighbour-joining tree has no heights to cut"},
                          {"linkage", "neighbour joining is a rule of its own, not a linkage"},
                          {nullptr, "needs --tree (it says which tree --tree writes)", !a.has("tree")}}))
        return 2;
    if (!a.u64("pcoa", pcoa, 1, 16, "an integer from 1 to 16 is required") ||
        !a.allowed("pcoa", {{"dm", "coordinates are not a matrix of distances"},
                            {"top", "principal coordinates need every pair"},
                            {"max-dist", "principal coordinates need every pair"},
                            {"cluster", "coordinates or clusters, not both"},
                            {"derep", "coordinates or greedy representatives, not both"},
                            {"containment", "principal coordinates need a symmetric distance"},
                            {"tree", "coordinates or a tree, not both"},
                            {"nj", "coordinates or a tree, not both"},
                            {"linkage", "principal coordinates merge no clusters"},
                            all_vs_all}))
        return 2;
    opt.has_max_dist = a.has("max-dist");
    opt.top = (uint32_t)top;
    opt.has_cluster = a.has("cluster");
    opt.has_derep = a.has("derep");
    if (a.has("containment")) opt.measure = contain == 0 ? LASH_MEASURE_CONTAIN_QUERY : LASH_MEASURE_CONTAIN_REFERENCE;
    opt.tree = a.has("tree");
    opt.nj = a.has("nj");
    opt.pcoa = (uint32_t)pcoa;
    if (!layout_option(a, opt.layout)) return 2;
    return finish(run_dist(opt), "Distances computed.\n");                                    // main.rs:615
}

int cmd_growth(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, GROWTH)) return 2;
    if (a.has("help")) { usage(); return 0; }
    if (!a.require({{"reference", "reference"}})) return 2;
    GrowthOptions opt;
    opt.side.ref_prefix = opt.side.query_prefix = a.str("reference");
    opt.output_file = a.str("output_file", "growth");
    opt.side.estimator = a.str("estimator", "fgra");
    uint64_t orders = 1;
    int estimator = 0;
    if (!a.choice("estimator", {"fgra", "ml"}, estimator, "fgra or ml is required") ||
        !a.u64("orders", orders, 1, 0xFFFFFFFFull, "a positive integer is required") || !a.u64("seed", opt.seed) ||
        !threads_device_order(a, opt.side) || !bias_source(a, opt.side) || !layout_option(a, opt.side.layout))
        return 2;
    opt.orders = (uint32_t)orders;
    return finish(run_growth(opt), "Growth table written.\n");
}

int cmd_merge(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, MERGE)) return 2;
    if (a.has("help")) { usage(); return 0; }
    MergeOptions opt;
    if (!a.require({{"reference", "prefix"}, {"output", "prefix"}}) || !groups_or_all(a, true, opt.groups_file, opt.all_name) ||
        !threads_device_order(a, opt.side) || !layout_option(a, opt.side.layout))
        return 2;
    opt.side.ref_prefix = opt.side.query_prefix = a.str("reference");
    opt.output = a.str("output");
    opt.keep_others = a.has("keep-others");
    return finish(run_merge(opt), "Merged sketches written.\n");
}

int cmd_spectrum(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, SPECTRUM)) return 2;
    if (a.has("help")) { usage(); return 0; }
    SpectrumOptions opt;
    const auto fraction = [](double f) { return f > 0.0 && f <= 1.0; };
    if (!a.require({{"reference", "prefix"}, {"output", "prefix"}}) || !groups_or_all(a, false, opt.groups_file, opt.all_name) ||
        !a.real("core", opt.core, fraction, "a number in (0, 1] is required") || !a.real("cloud", opt.cloud, fraction, "a number in (0, 1] is required"))
        return 2;
    const std::string err = check_fractions(opt.core, opt.cloud);
    if (!err.empty()) { fprintf(stderr, "error: %s (--core %g, --cloud %g)\n", err.c_str(), opt.core, opt.cloud); return 2; }
    if (!threads_device_order(a, opt.side) || !layout_option(a, opt.side.layout)) return 2;
    opt.side.ref_prefix = opt.side.query_prefix = a.str("reference");
    opt.output = a.str("output");
    opt.curves = a.has("curves");
    return finish(run_spectrum(opt), "Spectrum tables written.\n");
}

int cmd_screen(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, SCREEN)) return 2;
    if (a.has("help")) { usage(); return 0; }
    ScreenOptions opt;
    uint64_t model = 1, block_rows = 0;
    if (!a.require({{"reference", "prefix"}, {"query", "prefix"}, {"output", "file"}}) ||
        !a.real("max-dist", opt.max_dist, [](double d) { return check_screen_max_dist(d).empty(); }, check_screen_max_dist(NAN)) ||
        !a.u64("model", model, 0, 1, "0 or 1 is required") || !a.u64("block-rows", block_rows) || !threads_device_order(a, opt.side) ||
        !layout_option(a, opt.side.layout))
        return 2;
    opt.has_max_dist = a.has("max-dist");
    opt.side.ref_prefix = a.str("reference");
    opt.side.query_prefix = a.str("query");
    opt.output = a.str("output");
    opt.keep_losers = a.has("keep-losers");
    opt.side.model = (int)model;
    opt.side.block_rows = (uint32_t)std::min<uint64_t>(block_rows, 0xFFFFFFFFull);
    return finish(run_screen(opt), "Screen table written.\n");
}

int cmd_hll_bias(int argc, char **argv)
{
    Args a;
    if (!a.parse(argc, argv, HLL_BIAS)) return 2;
    if (a.has("help")) { usage(); return 0; }
    if (!a.require({{"output", "file"}})) return 2;
    HllBiasOptions opt;
    opt.output = a.str("output");
    uint64_t points = 0, trials = 0, dev = 0;
    std::vector<uint64_t> ps;
    const bool all_in_range = a.u64_list("precision", ps, 4, 18);      // (ps holds the items before the first that is not)
    for (size_t i = 0; i < ps.size(); ++i)
        if (std::find(ps.begin(), ps.begin() + i, ps[i]) != ps.begin() + i) { a.invalid("precision", std::to_string(ps[i]) + " is named twice"); return 2; }
    if (!all_in_range) { a.invalid("precision", "a list of integers from 4 to 18 is required"); return 2; }
    if (!a.has("precision")) for (int p = 4; p <= 18; ++p) opt.ps.push_back(p);
    for (uint64_t p : ps) opt.ps.push_back((int)p);
    if (!a.u64("points", points, 6, 0xFFFFFFFFull, "an integer of at least 6 is required (the bias is read from the 6 nearest)") ||
        !a.u64("trials", trials, 1, 1u << 20, "an integer from 1 to 1048576 is required") || !a.u64("seed", opt.seed) || !a.u64("device", dev))
        return 2;
    opt.points = (uint32_t)points;
    opt.trials = (uint32_t)trials;
    opt.device = (int)dev;
    return finish(run_hll_bias(opt), "HLL++ bias tables written.\n");
}

}  // namespace

static void epoch_mark(const char *what)
{
    if (!getenv("LASH_CLI_TIMING")) return;
    const double t = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    fprintf(stderr, "[lash cli] epoch %.3f  %s\n", t, what);
}

int main(int argc, char **argv)
{
    epoch_mark("main entered");
    printf("\n ************** initializing logger *****************\n\n");                   // main.rs:23
    fflush(stdout);
    if (argc < 2) { usage(); return 2; }
    const std::string cmd = argv[1];
    if (cmd == "sketch") { const int rc = cmd_sketch(argc, argv); epoch_mark("main returning"); return rc; }
    if (cmd == "dist") return cmd_dist(argc, argv);
    if (cmd == "hll-bias") return cmd_hll_bias(argc, argv);
    if (cmd == "growth") return cmd_growth(argc, argv);
    if (cmd == "merge") return cmd_merge(argc, argv);
    if (cmd == "spectrum") return cmd_spectrum(argc, argv);
    if (cmd == "screen") return cmd_screen(argc, argv);
    if (cmd == "--version" || cmd == "-V") { printf("Genome Sketching via HyperLogLog, HyperMinhash and UltraLogLog %s\n", VERSION); return 0; }
    usage();
    return cmd == "--help" || cmd == "-h" || cmd == "help" ? 0 : 2;
}
