// main.cpp — `lash` command line for the gfx950 build: the flag surface of the reference's clap definition
// (/root/reference/src/main.rs:26-177) on top of liblash_gfx950.so.
//   lash sketch -f LIST [-o sketch] [-k 16] [-t N] [-a hmh|hll|ull] [-p 10] [-s 42]        (main.rs:30-96, 180-279)
//   lash dist   -q PREFIX -r PREFIX [-o dist] [-t N] [-e fgra|ml] [-m 1|0] [--fp32] [--dm]   (main.rs:107-176, 280-617)
//   lash growth -r PREFIX [-o growth] [--orders P] [--seed S] [--file-order] [-e fgra|ml] [-t N]   (not upstream: union cardinality along orderings)
//   lash merge  -r PREFIX -o OUT (--groups FILE | --all NAME) [--keep-others] [--file-order] [-t N]   (not upstream: one sketch per group of sketches)
//   lash spectrum -r PREFIX -o OUT [--groups FILE | --all NAME] [--core F] [--cloud F] [--curves] [--file-order] [-t N]   (not upstream: k-mer sharing spectrum of groups, hmh)
//   lash screen -r DB -q SAMPLE -o FILE [--max-dist D] [--keep-losers] [-m 1|0] [--file-order] [--block-rows N] [-t N]   (not upstream: winner-takes-all containment of samples against a database, hmh)
//   lash hll-bias -o FILE [-p P[,P...]] [--points N] [--trials T] [--seed S] [--device D]    (not upstream: HLL++ bias tables, simulated)
// Extras that do not exist upstream: --gpus N / --device D / --devices LIST (which GPUs to use, one worker each), --batch-mb M, --stream-mb M (files
// larger than M MiB are streamed in chunks with on-device accumulation), --hmh-x-low, --min-count M [--count-cells-log2 L] (drop the k-mers a
// file holds fewer than M times, counted on the GPU), --window (one sketch per W-base window of every record), --translate (six-frame protein sketches of nucleotide FASTA, translated on the GPU), --per-record (one sketch per FASTA record, the records
// found on the GPU); dist: --device D, --block-rows N, --hll-bias FILE / --hll-bias-sim (HLL++ bias tables from a file / simulated on the GPU),
// --file-order (rows / columns in list-file order instead of the reference's seeded hash-map order), --max-dist D (print only
// the pairs with distance <= D), --top K (only each name's K nearest), --cluster D (single-linkage clusters of an all-vs-all instead
// of pairs), --derep D (greedy representatives of an all-vs-all in row order), --containment query|reference (the distance of the
// containment fraction instead of the Jaccard-derived one; always a rectangle), --tree / --linkage average|single|complete (one Newick
// tree of an all-vs-all, merged on the GPU; with --cluster D, that tree cut at D), --tree --nj (the neighbour-joining tree instead, joined on the GPU), --pcoa K (principal coordinates of an all-vs-all, solved on the GPU) (reference rows per GPU call); both: --layout SPEC (or $LASH_LAYOUT): the crate-internal rules as data, see `lash_layout`
// in include/lash_gfx950.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/lash_gfx950.h"
#include "dist.hpp"
#include "growth.hpp"
#include "merge.hpp"
#include "screen.hpp"
#include "sketch_files.hpp"
#include "spectrum.hpp"

using namespace lashhost;

namespace {

const char *VERSION = "0.1.4";      // main.rs:27 (hard-coded there although the crate is 0.1.6)

struct Args {
    std::map<std::string, std::string> kv;
    std::map<std::string, bool> flags;
};

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

bool parse(int argc, char **argv, int first, const std::map<std::string, std::string> &alias,
           const std::vector<std::string> &bool_flags, Args &out, std::string &err)
{
    for (int i = first; i < argc; ++i) {
        std::string a = argv[i];
        std::string key, val;
        bool has_val = false;
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            key = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            if (eq != std::string::npos) { val = a.substr(eq + 1); has_val = true; }
        } else if (a.size() >= 2 && a[0] == '-') {
            auto it = alias.find(a.substr(1, 1));
            if (it == alias.end()) { err = "unexpected argument '" + a + "'"; return false; }
            key = it->second;
            if (a.size() > 2) { val = a.substr(2); has_val = true; }
        } else { err = "unexpected argument '" + a + "'"; return false; }
        bool is_flag = false;
        for (auto &f : bool_flags) if (f == key) is_flag = true;
        if (is_flag) { out.flags[key] = true; continue; }
        if (!has_val) {
            if (i + 1 >= argc) { err = "a value is required for '--" + key + "'"; return false; }
            val = argv[++i];
        }
        out.kv[key] = val;
    }
    return true;
}

bool to_u64(const std::string &s, uint64_t &v)
{
    if (s.empty()) return false;
    char *e = nullptr;
    v = strtoull(s.c_str(), &e, 10);
    return e && *e == 0 && s[0] != '-';
}

int cmd_sketch(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"f", "file"}, {"o", "output"}, {"k", "kmer"}, {"t", "threads"},
                                                      {"a", "algorithm"}, {"p", "precision"}, {"s", "seed"}};
    if (!parse(argc, argv, 2, alias, {"hmh-x-low", "aa", "per-record", "translate", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("file")) { fprintf(stderr, "error: the following required arguments were not provided:\n  --file <file>\n"); return 2; }
    SketchOptions opt;
    const std::string output = a.kv.count("output") ? a.kv["output"] : "sketch";
    const std::string alg = a.kv.count("algorithm") ? a.kv["algorithm"] : "hmh";
    uint64_t k = 16, p = 10, seed = 42, threads = std::thread::hardware_concurrency(), gpus = 0, dev = 0, batch_mb = 64,
             stream_mb = 1024;
    if (a.kv.count("kmer") && !to_u64(a.kv["kmer"], k)) { fprintf(stderr, "error: invalid value for --kmer\n"); return 2; }
    if (a.kv.count("precision") && !to_u64(a.kv["precision"], p)) { fprintf(stderr, "error: invalid value for --precision\n"); return 2; }
    if (a.kv.count("seed") && !to_u64(a.kv["seed"], seed)) { fprintf(stderr, "error: invalid value for --seed\n"); return 2; }
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("gpus") && !to_u64(a.kv["gpus"], gpus)) { fprintf(stderr, "error: invalid value for --gpus\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    if (a.kv.count("batch-mb") && !to_u64(a.kv["batch-mb"], batch_mb)) { fprintf(stderr, "error: invalid value for --batch-mb\n"); return 2; }
    if (a.kv.count("stream-mb") && !to_u64(a.kv["stream-mb"], stream_mb)) { fprintf(stderr, "error: invalid value for --stream-mb\n"); return 2; }
    if (alg == "hmh") opt.algo = LASH_HMH;
    else if (alg == "hll") opt.algo = LASH_HLL;
    else if (alg == "ull") opt.algo = LASH_ULL;
    else { fprintf(stderr, "Algorithm must be either hmh, ull, or hll\n"); return 101; }      // main.rs:245 panic
    if (k < 1 || k > 32) { fprintf(stderr, "k-mer length must be 1-32\n"); return 101; }       // utils.rs:501 panic
    const bool amino = a.flags.count("aa") != 0;                                               // main.rs:97-104 (commented out there)
    opt.per_record = a.flags.count("per-record") != 0;
    opt.translate = a.flags.count("translate") != 0;
    if (opt.translate && amino) { fprintf(stderr, "error: --translate cannot be used with --aa (--translate takes nucleotide input and makes the proteins itself)\n"); return 2; }
    if (opt.translate && a.kv.count("min-count")) { fprintf(stderr, "error: --translate cannot be used with --min-count (k-mers are counted for nucleotide sketches only)\n"); return 2; }
    if (opt.translate && a.kv.count("window")) { fprintf(stderr, "error: --translate cannot be used with --window (windows of translated records are not supported)\n"); return 2; }
    if (a.kv.count("window")) {
        uint64_t w = 0;
        if (!to_u64(a.kv["window"], w) || w < 1) {
            fprintf(stderr, "error: invalid value '%s' for --window: a positive integer is required\n", a.kv["window"].c_str());
            return 2;
        }
        if (amino) { fprintf(stderr, "error: --window cannot be used with --aa (windows are cut for nucleotide FASTA only)\n"); return 2; }
        if (w < k) { fprintf(stderr, "error: --window %llu is shorter than -k %llu: no window would hold a k-mer\n", (unsigned long long)w, (unsigned long long)k); return 2; }
        if (a.kv.count("min-count")) { fprintf(stderr, "error: --window cannot be used with --min-count (k-mers are counted per file)\n"); return 2; }
        opt.window = w;
    }
    if (opt.translate && k > 12) { fprintf(stderr, "k-mer length for amino acid must be 1\xe2\x80\x93" "12\n"); return 101; }   // the --aa message
    if (opt.per_record && amino) { fprintf(stderr, "error: --per-record cannot be used with --aa (records are split for nucleotide FASTA only)\n"); return 2; }
    if (amino && k > 12) { fprintf(stderr, "k-mer length for amino acid must be 1\xe2\x80\x93" "12\n"); return 101; }   // utils.rs:554 panic
    if (a.kv.count("count-cells-log2") && !a.kv.count("min-count")) { fprintf(stderr, "error: --count-cells-log2 needs --min-count\n"); return 2; }
    if (a.kv.count("min-count")) {
        uint64_t m = 0, l2 = 0;
        if (!to_u64(a.kv["min-count"], m) || m < 1 || m > 255) {
            fprintf(stderr, "error: invalid value '%s' for --min-count: an integer from 1 to 255 is required\n", a.kv["min-count"].c_str());
            return 2;
        }
        if (a.kv.count("count-cells-log2") && (!to_u64(a.kv["count-cells-log2"], l2) || l2 < 10 || l2 > 36)) {
            fprintf(stderr, "error: invalid value '%s' for --count-cells-log2: an integer from 10 to 36 is required\n", a.kv["count-cells-log2"].c_str());
            return 2;
        }
        if (amino) { fprintf(stderr, "error: --min-count cannot be used with --aa (k-mers are counted for nucleotide input only)\n"); return 2; }
        if (opt.per_record) { fprintf(stderr, "error: --min-count cannot be used with --per-record (k-mers are counted per file)\n"); return 2; }
        // the filtered launch exists where the sketch's registers are a plain table in LDS (include/lash_gfx950.h)
        const uint64_t max_p = opt.algo == LASH_HLL ? 15 : 14;
        if (opt.algo != LASH_HMH && p > max_p) {
            fprintf(stderr, "error: --min-count supports -a %s up to -p %llu (and -a hmh); -p %llu is not supported\n", alg.c_str(),
                    (unsigned long long)max_p, (unsigned long long)p);
            return 2;
        }
        opt.min_count = (uint32_t)m;
        opt.count_cells_log2 = (int)l2;
    }
    opt.k = (int)k;
    opt.precision = (int)p;
    opt.seed = seed;
    opt.threads = (int)std::max<uint64_t>(1, threads);
    opt.batch_bytes = std::max<uint64_t>(1, batch_mb) << 20;
    opt.stream_bytes = std::max<uint64_t>(1, stream_mb) << 20;
    opt.flags = (a.flags.count("hmh-x-low") ? LASH_F_HMH_X_LOW : 0) | (amino || opt.translate ? LASH_F_AMINO : 0);
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.kv.count("devices")) {                              // explicit worker list, e.g. 0,1,2,3 (repeats allowed: 0,0 = two workers on GPU 0)
        const std::string &l = a.kv["devices"];
        size_t at = 0;
        while (at <= l.size()) {
            const size_t c = l.find(',', at);
            uint64_t d = 0;
            if (!to_u64(l.substr(at, c == std::string::npos ? std::string::npos : c - at), d)) { fprintf(stderr, "error: invalid value for --devices\n"); return 2; }
            opt.devices.push_back((int)d);
            if (c == std::string::npos) break;
            at = c + 1;
        }
    } else if (gpus > 0) for (uint64_t d = 0; d < gpus; ++d) opt.devices.push_back((int)d);
    else opt.devices.push_back((int)dev);

    std::vector<std::string> files;
    err = read_list_file(a.kv["file"], files);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    SketchStats st;
    err = sketch_files(opt, files, output, &st);
    if (opt.window && err.rfind("--window takes FASTA input", 0) == 0) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }   // a refusal of the flag
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    err = write_parameters_json(output, alg, opt.k, opt.precision, opt.seed, amino || opt.translate);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
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

int cmd_dist(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"q", "query"}, {"r", "reference"}, {"o", "output_file"}, {"t", "threads"},
                                                      {"e", "estimator"}, {"m", "model"}};
    if (!parse(argc, argv, 2, alias, {"fp32", "dm", "file-order", "hll-bias-sim", "tree", "nj", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("query") || !a.kv.count("reference")) {
        fprintf(stderr, "error: the following required arguments were not provided:\n  --query <query>\n  --reference <reference>\n");
        return 2;
    }
    DistOptions opt;
    opt.query_prefix = a.kv["query"];
    opt.ref_prefix = a.kv["reference"];
    opt.output_file = a.kv.count("output_file") ? a.kv["output_file"] : "dist";
    opt.estimator = a.kv.count("estimator") ? a.kv["estimator"] : "fgra";
    uint64_t model = 1, threads = std::thread::hardware_concurrency(), dev = 0, block_rows = 0;
    if (a.kv.count("block-rows") && !to_u64(a.kv["block-rows"], block_rows)) { fprintf(stderr, "error: invalid value for --block-rows\n"); return 2; }
    opt.block_rows = (uint32_t)std::min<uint64_t>(block_rows, 0xFFFFFFFFull);
    if (a.kv.count("model") && !to_u64(a.kv["model"], model)) { fprintf(stderr, "error: invalid value for --model\n"); return 2; }
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.model = (int)model;
    opt.threads = (int)std::max<uint64_t>(1, threads);
    opt.fp32 = a.flags.count("fp32") != 0;
    opt.matrix = a.flags.count("dm") != 0;
    opt.file_order = a.flags.count("file-order") != 0;
    opt.hll_bias_sim = a.flags.count("hll-bias-sim") != 0;
    if (opt.hll_bias_sim && a.kv.count("hll-bias")) {
        fprintf(stderr, "error: --hll-bias-sim cannot be used with --hll-bias (simulate the tables or read them from a file, not both)\n");
        return 2;
    }
    if (a.kv.count("hll-bias")) opt.hll_bias_file = a.kv["hll-bias"];
    else if (const char *e = opt.hll_bias_sim ? nullptr : getenv("LASH_HLL_BIAS")) opt.hll_bias_file = e;
    opt.device = (int)dev;
    if (a.kv.count("devices")) {
        const std::string &l = a.kv["devices"];
        size_t at = 0;
        while (at <= l.size()) {
            const size_t c = l.find(',', at);
            uint64_t d = 0;
            if (!to_u64(l.substr(at, c == std::string::npos ? std::string::npos : c - at), d)) { fprintf(stderr, "error: invalid value for --devices\n"); return 2; }
            opt.devices.push_back((int)d);
            if (c == std::string::npos) break;
            at = c + 1;
        }
    }
    if (a.kv.count("max-dist")) {
        const std::string &v = a.kv["max-dist"];
        char *e = nullptr;
        const double d = v.empty() ? NAN : strtod(v.c_str(), &e);
        if (!e || *e != 0 || !std::isfinite(d)) { fprintf(stderr, "error: invalid value '%s' for --max-dist: a finite number is required\n", v.c_str()); return 2; }
        if (opt.matrix) { fprintf(stderr, "error: --max-dist cannot be used with --dm (a square matrix cannot drop cells)\n"); return 2; }
        opt.has_max_dist = true;
        opt.max_dist = d;
    }
    if (a.kv.count("top")) {
        const std::string &v = a.kv["top"];
        uint64_t n = 0;
        if (!to_u64(v, n) || n < 1 || n > LASH_TOP_MAX) {
            fprintf(stderr, "error: invalid value '%s' for --top: an integer from 1 to %u is required\n", v.c_str(), LASH_TOP_MAX);
            return 2;
        }
        if (opt.matrix) { fprintf(stderr, "error: --top cannot be used with --dm (a square matrix cannot drop cells)\n"); return 2; }
        opt.top = (uint32_t)n;
    }
    if (a.kv.count("cluster")) {
        const std::string &v = a.kv["cluster"];
        char *e = nullptr;
        const double d = v.empty() ? NAN : strtod(v.c_str(), &e);
        if (!e || *e != 0 || !std::isfinite(d)) { fprintf(stderr, "error: invalid value '%s' for --cluster: a finite number is required\n", v.c_str()); return 2; }
        if (opt.matrix) { fprintf(stderr, "error: --cluster cannot be used with --dm (clusters are not a matrix)\n"); return 2; }
        if (opt.top) { fprintf(stderr, "error: --cluster cannot be used with --top (it prints clusters, not pairs)\n"); return 2; }
        if (opt.has_max_dist) { fprintf(stderr, "error: --cluster cannot be used with --max-dist (--cluster D is its own cutoff)\n"); return 2; }
        opt.has_cluster = true;
        opt.cluster_dist = d;
    }
    if (a.kv.count("derep")) {
        const std::string &v = a.kv["derep"];
        char *e = nullptr;
        const double d = v.empty() ? NAN : strtod(v.c_str(), &e);
        if (!e || *e != 0 || !std::isfinite(d)) { fprintf(stderr, "error: invalid value '%s' for --derep: a finite number is required\n", v.c_str()); return 2; }
        if (opt.matrix) { fprintf(stderr, "error: --derep cannot be used with --dm (representatives are not a matrix)\n"); return 2; }
        if (opt.top) { fprintf(stderr, "error: --derep cannot be used with --top (it prints representatives, not pairs)\n"); return 2; }
        if (opt.has_max_dist) { fprintf(stderr, "error: --derep cannot be used with --max-dist (--derep D is its own cutoff)\n"); return 2; }
        if (opt.has_cluster) { fprintf(stderr, "error: --derep cannot be used with --cluster (greedy representatives or single-linkage clusters, not both)\n"); return 2; }
        if (opt.devices.size() > 1) {
            fprintf(stderr, "error: --derep cannot be used with more than one entry in --devices: a block of rows is decided from the "
                            "representatives of the blocks before it, so the blocks run in row order on one worker\n");
            return 2;
        }
        opt.has_derep = true;
        opt.derep_dist = d;
    }
    if (a.kv.count("containment")) {
        const std::string &v = a.kv["containment"];
        if (v == "query") opt.measure = LASH_MEASURE_CONTAIN_QUERY;
        else if (v == "reference") opt.measure = LASH_MEASURE_CONTAIN_REFERENCE;
        else { fprintf(stderr, "error: invalid value '%s' for --containment: query or reference is required\n", v.c_str()); return 2; }
        if (opt.matrix) { fprintf(stderr, "error: --containment cannot be used with --dm (list form only)\n"); return 2; }
        if (opt.has_cluster) { fprintf(stderr, "error: --containment cannot be used with --cluster (clusters need a symmetric distance)\n"); return 2; }
        if (opt.has_derep) { fprintf(stderr, "error: --containment cannot be used with --derep (representatives need a symmetric distance)\n"); return 2; }
    }
    if (a.flags.count("tree")) {
        if (opt.matrix) { fprintf(stderr, "error: --tree cannot be used with --dm (a tree is not a matrix)\n"); return 2; }
        if (opt.top) { fprintf(stderr, "error: --tree cannot be used with --top (a tree needs every pair)\n"); return 2; }
        if (opt.has_max_dist) { fprintf(stderr, "error: --tree cannot be used with --max-dist (a tree needs every pair)\n"); return 2; }
        if (opt.has_cluster) { fprintf(stderr, "error: --tree cannot be used with --cluster (the whole tree or its cut at D, not both)\n"); return 2; }
        if (opt.has_derep) { fprintf(stderr, "error: --tree cannot be used with --derep (a tree or greedy representatives, not both)\n"); return 2; }
        if (opt.measure != LASH_MEASURE_JACCARD) { fprintf(stderr, "error: --tree cannot be used with --containment (a tree needs a symmetric distance)\n"); return 2; }
        if (prefix_stem(opt.query_prefix) != prefix_stem(opt.ref_prefix)) {
            fprintf(stderr, "error: --tree needs an all-vs-all run: -q and -r must name the same sketch files\n");
            return 2;
        }
        opt.tree = true;
    }
    if (a.kv.count("linkage")) {
        const std::string &v = a.kv["linkage"];
        if (v == "average") opt.linkage = LASH_LINKAGE_AVERAGE;
        else if (v == "single") opt.linkage = LASH_LINKAGE_SINGLE;
        else if (v == "complete") opt.linkage = LASH_LINKAGE_COMPLETE;
        else { fprintf(stderr, "error: invalid value '%s' for --linkage: average, single or complete is required\n", v.c_str()); return 2; }
        if (!opt.tree && !opt.has_cluster) { fprintf(stderr, "error: --linkage needs --tree or --cluster (it says how their clusters are merged)\n"); return 2; }
    }
    if (a.flags.count("nj")) {
        if (opt.has_cluster) { fprintf(stderr, "error: --nj cannot be used with --cluster (a neighbour-joining tree has no heights to cut)\n"); return 2; }
        if (opt.linkage >= 0) { fprintf(stderr, "error: --nj cannot be used with --linkage (neighbour joining is a rule of its own, not a linkage)\n"); return 2; }
        if (!opt.tree) { fprintf(stderr, "error: --nj needs --tree (it says which tree --tree writes)\n"); return 2; }
        opt.nj = true;
    }
    if (a.kv.count("pcoa")) {
        const std::string &v = a.kv["pcoa"];
        uint64_t n = 0;
        if (!to_u64(v, n) || n < 1 || n > 16) { fprintf(stderr, "error: invalid value '%s' for --pcoa: an integer from 1 to 16 is required\n", v.c_str()); return 2; }
        if (opt.matrix) { fprintf(stderr, "error: --pcoa cannot be used with --dm (coordinates are not a matrix of distances)\n"); return 2; }
        if (opt.top) { fprintf(stderr, "error: --pcoa cannot be used with --top (principal coordinates need every pair)\n"); return 2; }
        if (opt.has_max_dist) { fprintf(stderr, "error: --pcoa cannot be used with --max-dist (principal coordinates need every pair)\n"); return 2; }
        if (opt.has_cluster) { fprintf(stderr, "error: --pcoa cannot be used with --cluster (coordinates or clusters, not both)\n"); return 2; }
        if (opt.has_derep) { fprintf(stderr, "error: --pcoa cannot be used with --derep (coordinates or greedy representatives, not both)\n"); return 2; }
        if (opt.measure != LASH_MEASURE_JACCARD) { fprintf(stderr, "error: --pcoa cannot be used with --containment (principal coordinates need a symmetric distance)\n"); return 2; }
        if (opt.tree) { fprintf(stderr, "error: --pcoa cannot be used with --tree (coordinates or a tree, not both)\n"); return 2; }
        if (opt.nj) { fprintf(stderr, "error: --pcoa cannot be used with --nj (coordinates or a tree, not both)\n"); return 2; }
        if (opt.linkage >= 0) { fprintf(stderr, "error: --pcoa cannot be used with --linkage (principal coordinates merge no clusters)\n"); return 2; }
        if (prefix_stem(opt.query_prefix) != prefix_stem(opt.ref_prefix)) {
            fprintf(stderr, "error: --pcoa needs an all-vs-all run: -q and -r must name the same sketch files\n");
            return 2;
        }
        opt.pcoa = (uint32_t)n;
    }
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    err = run_dist(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("Distances computed.\n");                                                          // main.rs:615
    return 0;
}

// lash growth -r PREFIX [-o growth] [--orders P] [--seed S] [--file-order] [-e fgra|ml] [-t N] [--hll-bias FILE | --hll-bias-sim] [--device D]
int cmd_growth(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"r", "reference"}, {"o", "output_file"}, {"t", "threads"}, {"e", "estimator"}};
    // one collection, one table: whatever else `dist` takes (-q, --dm, --top, ...) is not an option of this command
    const std::vector<std::string> known = {"reference", "output_file", "threads", "estimator", "orders", "seed", "file-order", "hll-bias",
                                            "hll-bias-sim", "device", "layout", "help"};
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--", 0) != 0) continue;
        const std::string key = s.substr(2, s.find('=') == std::string::npos ? std::string::npos : s.find('=') - 2);
        if (std::find(known.begin(), known.end(), key) == known.end()) { fprintf(stderr, "error: unexpected argument '--%s'\n", key.c_str()); return 2; }
    }
    if (!parse(argc, argv, 2, alias, {"file-order", "hll-bias-sim", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("reference")) { fprintf(stderr, "error: the following required arguments were not provided:\n  --reference <reference>\n"); return 2; }
    GrowthOptions opt;
    opt.side.ref_prefix = opt.side.query_prefix = a.kv["reference"];
    opt.output_file = a.kv.count("output_file") ? a.kv["output_file"] : "growth";
    opt.side.estimator = a.kv.count("estimator") ? a.kv["estimator"] : "fgra";
    if (opt.side.estimator != "fgra" && opt.side.estimator != "ml") {
        fprintf(stderr, "error: invalid value '%s' for --estimator: fgra or ml is required\n", opt.side.estimator.c_str());
        return 2;
    }
    uint64_t orders = 1, threads = std::thread::hardware_concurrency(), dev = 0;
    if (a.kv.count("orders") && (!to_u64(a.kv["orders"], orders) || orders < 1 || orders > 0xFFFFFFFFull)) {
        fprintf(stderr, "error: invalid value '%s' for --orders: a positive integer is required\n", a.kv["orders"].c_str());
        return 2;
    }
    if (a.kv.count("seed") && !to_u64(a.kv["seed"], opt.seed)) { fprintf(stderr, "error: invalid value for --seed\n"); return 2; }
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.orders = (uint32_t)orders;
    opt.side.threads = (int)std::max<uint64_t>(1, threads);
    opt.side.device = (int)dev;
    opt.side.file_order = a.flags.count("file-order") != 0;
    opt.side.hll_bias_sim = a.flags.count("hll-bias-sim") != 0;
    if (opt.side.hll_bias_sim && a.kv.count("hll-bias")) {
        fprintf(stderr, "error: --hll-bias-sim cannot be used with --hll-bias (simulate the tables or read them from a file, not both)\n");
        return 2;
    }
    if (a.kv.count("hll-bias")) opt.side.hll_bias_file = a.kv["hll-bias"];
    else if (const char *e = opt.side.hll_bias_sim ? nullptr : getenv("LASH_HLL_BIAS")) opt.side.hll_bias_file = e;
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.side.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    err = run_growth(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("Growth table written.\n");
    return 0;
}

// lash merge -r PREFIX -o OUT (--groups FILE | --all NAME) [--keep-others] [--file-order] [--device D] [--layout SPEC] [-t N]
int cmd_merge(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"r", "reference"}, {"o", "output"}, {"t", "threads"}};
    const std::vector<std::string> known = {"reference", "output", "threads", "groups", "all", "keep-others", "file-order", "device", "layout", "help"};
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--", 0) != 0) continue;
        const std::string key = s.substr(2, s.find('=') == std::string::npos ? std::string::npos : s.find('=') - 2);
        if (std::find(known.begin(), known.end(), key) == known.end()) { fprintf(stderr, "error: unexpected argument '--%s'\n", key.c_str()); return 2; }
    }
    if (!parse(argc, argv, 2, alias, {"keep-others", "file-order", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("reference") || !a.kv.count("output")) {
        fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", a.kv.count("reference") ? "" : "  --reference <prefix>\n",
                a.kv.count("output") ? "" : "  --output <prefix>\n");
        return 2;
    }
    if (a.kv.count("groups") && a.kv.count("all")) { fprintf(stderr, "error: --groups cannot be used with --all (a list of groups or one group of everything, not both)\n"); return 2; }
    if (!a.kv.count("groups") && !a.kv.count("all")) { fprintf(stderr, "error: one of --groups <file> and --all <name> is required\n"); return 2; }
    if (a.kv.count("all") && a.flags.count("keep-others")) { fprintf(stderr, "error: --keep-others cannot be used with --all (--all leaves no others)\n"); return 2; }
    if (a.kv.count("all") && a.kv["all"].empty()) { fprintf(stderr, "error: invalid value '' for --all: a name is required\n"); return 2; }
    MergeOptions opt;
    opt.side.ref_prefix = opt.side.query_prefix = a.kv["reference"];
    opt.output = a.kv["output"];
    if (a.kv.count("groups")) opt.groups_file = a.kv["groups"];
    if (a.kv.count("all")) opt.all_name = a.kv["all"];
    opt.keep_others = a.flags.count("keep-others") != 0;
    opt.side.file_order = a.flags.count("file-order") != 0;
    uint64_t threads = std::thread::hardware_concurrency(), dev = 0;
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.side.threads = (int)std::max<uint64_t>(1, threads);
    opt.side.device = (int)dev;
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.side.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    err = run_merge(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("Merged sketches written.\n");
    return 0;
}

// lash spectrum -r PREFIX -o OUT [--groups FILE | --all NAME] [--core F] [--cloud F] [--curves] [--file-order] [--device D] [--layout SPEC] [-t N]
int cmd_spectrum(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"r", "reference"}, {"o", "output"}, {"t", "threads"}};
    const std::vector<std::string> known = {"reference", "output", "threads", "groups", "all", "core", "cloud", "curves", "file-order", "device", "layout", "help"};
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--", 0) != 0) continue;
        const std::string key = s.substr(2, s.find('=') == std::string::npos ? std::string::npos : s.find('=') - 2);
        if (std::find(known.begin(), known.end(), key) == known.end()) { fprintf(stderr, "error: unexpected argument '--%s'\n", key.c_str()); return 2; }
    }
    if (!parse(argc, argv, 2, alias, {"curves", "file-order", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("reference") || !a.kv.count("output")) {
        fprintf(stderr, "error: the following required arguments were not provided:\n%s%s", a.kv.count("reference") ? "" : "  --reference <prefix>\n",
                a.kv.count("output") ? "" : "  --output <prefix>\n");
        return 2;
    }
    if (a.kv.count("groups") && a.kv.count("all")) { fprintf(stderr, "error: --groups cannot be used with --all (a list of groups or one group of everything, not both)\n"); return 2; }
    if (a.kv.count("all") && a.kv["all"].empty()) { fprintf(stderr, "error: invalid value '' for --all: a name is required\n"); return 2; }
    SpectrumOptions opt;
    for (const char *key : {"core", "cloud"}) {
        if (!a.kv.count(key)) continue;
        const std::string &v = a.kv[key];
        char *e = nullptr;
        const double f = v.empty() ? NAN : strtod(v.c_str(), &e);
        if (!e || *e != 0 || !(f > 0.0 && f <= 1.0)) { fprintf(stderr, "error: invalid value '%s' for --%s: a number in (0, 1] is required\n", v.c_str(), key); return 2; }
        (std::string(key) == "core" ? opt.core : opt.cloud) = f;
    }
    err = check_fractions(opt.core, opt.cloud);
    if (!err.empty()) { fprintf(stderr, "error: %s (--core %g, --cloud %g)\n", err.c_str(), opt.core, opt.cloud); return 2; }
    opt.side.ref_prefix = opt.side.query_prefix = a.kv["reference"];
    opt.output = a.kv["output"];
    if (a.kv.count("groups")) opt.groups_file = a.kv["groups"];
    if (a.kv.count("all")) opt.all_name = a.kv["all"];
    opt.curves = a.flags.count("curves") != 0;
    opt.side.file_order = a.flags.count("file-order") != 0;
    uint64_t threads = std::thread::hardware_concurrency(), dev = 0;
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.side.threads = (int)std::max<uint64_t>(1, threads);
    opt.side.device = (int)dev;
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.side.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    err = run_spectrum(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("Spectrum tables written.\n");
    return 0;
}

// lash screen -r DB_PREFIX -q SAMPLE_PREFIX -o FILE [--max-dist D] [--keep-losers] [-m 0|1] [--file-order] [--block-rows N] [--device D] [--layout SPEC] [-t N]
int cmd_screen(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"r", "reference"}, {"q", "query"}, {"o", "output"}, {"t", "threads"}, {"m", "model"}};
    const std::vector<std::string> known = {"reference", "query", "output", "threads", "model", "max-dist", "keep-losers", "file-order", "block-rows",
                                            "device", "layout", "help"};
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--", 0) != 0) continue;
        const std::string key = s.substr(2, s.find('=') == std::string::npos ? std::string::npos : s.find('=') - 2);
        if (std::find(known.begin(), known.end(), key) == known.end()) { fprintf(stderr, "error: unexpected argument '--%s'\n", key.c_str()); return 2; }
    }
    if (!parse(argc, argv, 2, alias, {"keep-losers", "file-order", "help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("reference") || !a.kv.count("query") || !a.kv.count("output")) {
        fprintf(stderr, "error: the following required arguments were not provided:\n%s%s%s", a.kv.count("reference") ? "" : "  --reference <prefix>\n",
                a.kv.count("query") ? "" : "  --query <prefix>\n", a.kv.count("output") ? "" : "  --output <file>\n");
        return 2;
    }
    ScreenOptions opt;
    if (a.kv.count("max-dist")) {
        const std::string &v = a.kv["max-dist"];
        char *e = nullptr;
        const double d = v.empty() ? NAN : strtod(v.c_str(), &e);
        if (!e || *e != 0 || !check_screen_max_dist(d).empty()) {
            fprintf(stderr, "error: invalid value '%s' for --max-dist: %s\n", v.c_str(), check_screen_max_dist(NAN).c_str());
            return 2;
        }
        opt.has_max_dist = true;
        opt.max_dist = d;
    }
    uint64_t model = 1, threads = std::thread::hardware_concurrency(), dev = 0, block_rows = 0;
    if (a.kv.count("model") && (!to_u64(a.kv["model"], model) || model > 1)) {
        fprintf(stderr, "error: invalid value '%s' for --model: 0 or 1 is required\n", a.kv["model"].c_str());
        return 2;
    }
    if (a.kv.count("block-rows") && !to_u64(a.kv["block-rows"], block_rows)) { fprintf(stderr, "error: invalid value for --block-rows\n"); return 2; }
    if (a.kv.count("threads") && !to_u64(a.kv["threads"], threads)) { fprintf(stderr, "error: invalid value for --threads\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.side.ref_prefix = a.kv["reference"];
    opt.side.query_prefix = a.kv["query"];
    opt.output = a.kv["output"];
    opt.keep_losers = a.flags.count("keep-losers") != 0;
    opt.side.model = (int)model;
    opt.side.block_rows = (uint32_t)std::min<uint64_t>(block_rows, 0xFFFFFFFFull);
    opt.side.threads = (int)std::max<uint64_t>(1, threads);
    opt.side.device = (int)dev;
    opt.side.file_order = a.flags.count("file-order") != 0;
    err = layout_from_option(a.kv.count("layout") ? a.kv["layout"] : "", opt.side.layout);
    if (!err.empty()) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    err = run_screen(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("Screen table written.\n");
    return 0;
}

int cmd_hll_bias(int argc, char **argv)
{
    Args a;
    std::string err;
    const std::map<std::string, std::string> alias = {{"o", "output"}, {"p", "precision"}};
    if (!parse(argc, argv, 2, alias, {"help"}, a, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (a.flags.count("help")) { usage(); return 0; }
    if (!a.kv.count("output")) { fprintf(stderr, "error: the following required arguments were not provided:\n  --output <file>\n"); return 2; }
    HllBiasOptions opt;
    opt.output = a.kv["output"];
    uint64_t points = 0, trials = 0, dev = 0;
    if (a.kv.count("precision")) {
        const std::string &l = a.kv["precision"];
        size_t at = 0;
        while (at <= l.size()) {
            const size_t c = l.find(',', at);
            uint64_t p = 0;
            if (!to_u64(l.substr(at, c == std::string::npos ? std::string::npos : c - at), p) || p < 4 || p > 18) {
                fprintf(stderr, "error: invalid value '%s' for --precision: a list of integers from 4 to 18 is required\n", l.c_str());
                return 2;
            }
            for (int q : opt.ps)
                if (q == (int)p) { fprintf(stderr, "error: invalid value '%s' for --precision: %d is named twice\n", l.c_str(), q); return 2; }
            opt.ps.push_back((int)p);
            if (c == std::string::npos) break;
            at = c + 1;
        }
    } else for (int p = 4; p <= 18; ++p) opt.ps.push_back(p);
    if (a.kv.count("points") && (!to_u64(a.kv["points"], points) || points < 6 || points > 0xFFFFFFFFull)) {
        fprintf(stderr, "error: invalid value '%s' for --points: an integer of at least 6 is required (the bias is read from the 6 nearest)\n",
                a.kv["points"].c_str());
        return 2;
    }
    if (a.kv.count("trials") && (!to_u64(a.kv["trials"], trials) || trials < 1 || trials > (1u << 20))) {
        fprintf(stderr, "error: invalid value '%s' for --trials: an integer from 1 to 1048576 is required\n", a.kv["trials"].c_str());
        return 2;
    }
    if (a.kv.count("seed") && !to_u64(a.kv["seed"], opt.seed)) { fprintf(stderr, "error: invalid value for --seed\n"); return 2; }
    if (a.kv.count("device") && !to_u64(a.kv["device"], dev)) { fprintf(stderr, "error: invalid value for --device\n"); return 2; }
    opt.points = (uint32_t)points;
    opt.trials = (uint32_t)trials;
    opt.device = (int)dev;
    err = run_hll_bias(opt);
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("HLL++ bias tables written.\n");
    return 0;
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
