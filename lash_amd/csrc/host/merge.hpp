// merge.hpp — `lash merge` (not upstream): one sketch per group of names of one sketch collection — clusters into pangenomes, the
// files of a sample into one sketch, contigs into bins — united on the GPU (lash_sketch_set_group_union) and written as a collection
// that `dist`, `growth` and `merge` read like any other.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "dist.hpp"

namespace lashhost {

struct MergeOptions {
    DistOptions side;          // ref_prefix, threads, file_order, device, layout: as `dist` reads a side
    std::string output;        // prefix of the three files written
    std::string groups_file;   // --groups FILE: lines of group<TAB>member ...
    std::string all_name;      // ... or --all NAME: one group of everything
    bool keep_others = false;  // names in no group follow the groups as singletons under their own names
};

// groups as a CSR list over name-file indices
struct GroupList {
    std::vector<std::string> names;      // in order of first appearance
    std::vector<uint64_t> off;           // [names.size() + 1]
    std::vector<uint32_t> members;
};

// The text of a groups file against the collection's names: lines of group<TAB>member, what `dist --cluster` and `--derep` write
// (their heading line Representative<TAB>Member, if it is the first line, is skipped; so are blank lines; a trailing CR is dropped).
// A member is a whole name; a name several sketches carry selects all of them.  Returns "" or the refusal, which names the line.
std::string parse_groups(const std::string &text, const std::vector<std::string> &names, GroupList &out);

std::string run_merge(const MergeOptions &opt);

}  // namespace lashhost
