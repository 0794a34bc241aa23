// newick.hpp — what `lash dist --tree` and `--cluster D --linkage average|complete` make of a merge list (lash_tree_build,
// include/lash_gfx950.h): the Newick text of the whole tree, and the flat clusters of a cut at one height.  Shared by the command line
// (dist.cpp) and, through liblash_host.so, by the tests.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/lash_gfx950.h"

namespace lashhost {

// A name as a Newick label: bare, or in single quotes with embedded quotes doubled when it holds any of ()[]':;, or white space.
std::string newick_label(const std::string &name);

// The tree of names.size() = n leaves and n - 1 merges (scipy node ids: leaves 0..n-1, the node of merge s is n + s; merge s joins
// two earlier nodes, each node joined once).  A leaf prints its label, the node of a merge "(" child a "," child b ")"; every child is
// followed by ":" and its branch length h_parent / 2 - h_child / 2 as %.10g (a leaf's h is 0); the root by ";".  n = 1: "name;",
// n = 0: ";".  No trailing newline.  Returns "" and sets err when the merge list is not a tree over these leaves.
std::string newick_text(const std::vector<std::string> &names, const lash_tree_merge *merges, std::string &err);

// The cut at max_height: exactly the merges with height <= max_height applied (NaN applies none); label[i] = the smallest leaf of i's
// component, for all n leaves.  false when the merge list is not a tree over n leaves.
bool tree_cut_labels(uint32_t n, const lash_tree_merge *merges, double max_height, std::vector<uint32_t> &label);

}  // namespace lashhost
