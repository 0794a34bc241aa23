// spectrum.hpp — `lash spectrum` (not upstream): how the k-mers of a group's union are shared among its members — in all of them (core),
// in some (shell), in few (cloud) — read off the HyperMinHash sketches of one collection on the GPU (lash_sketch_set_group_spectrum),
// with the expected core and pan-genome curves over all subsets that follow from the counts.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "dist.hpp"

namespace lashhost {

struct SpectrumOptions {
    DistOptions side;          // ref_prefix, threads, file_order, device, layout: as `dist` reads a side
    std::string output;        // prefix of {output}_spectrum.tsv, _groups.tsv and, with curves, _curves.tsv
    std::string groups_file;   // --groups FILE: lines of group<TAB>member (merge.hpp: parse_groups) ...
    std::string all_name;      // ... or --all NAME: one group of everything; neither: that group, called "all"
    double core = 0.95;        // a count c of a group of n is core iff c >= core * n ...
    double cloud = 0.15;       // ... cloud iff c < cloud * n, else shell
    bool curves = false;
};

// "" or why the two fractions are refused: each in (0, 1], cloud <= core
std::string check_fractions(double core, double cloud);

// The numbers of one group from its bins (hist[0 .. n], n members; hist[0] = the empty buckets) and its union's cardinality U.
// K(c) = (double)hist[c] / (double)occupied * U; the class sums add K(c) in ascending c; an occupied count of 0 gives zeros.
struct SpectrumClasses { double core = 0.0, shell = 0.0, cloud = 0.0; };
SpectrumClasses spectrum_classes(const uint32_t *hist, uint32_t n, double U, double core, double cloud);
// the exact expectations over all m-subsets of the members, m = 1 .. n: pan[m - 1], core[m - 1]
void spectrum_curves(const uint32_t *hist, uint32_t n, double U, std::vector<double> &pan, std::vector<double> &core);

std::string run_spectrum(const SpectrumOptions &opt);

}  // namespace lashhost
