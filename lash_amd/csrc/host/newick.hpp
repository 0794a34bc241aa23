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

// The neighbour-joining tree of names.size() = n leaves and n - 1 records (lash_tree_build_nj: n - 2 joins, the node of join s being
// n + s, then the closing record (x, y, L) of the last two nodes).  The node of a join prints as "(" a ":" len_a "," b ":" len_b ")",
// lengths as %.10g.  The tree is unrooted: the root is a trifurcation at whichever of x, y is node 2n - 3, its two children in record
// order, then the other node with length L: "(A:la,B:lb,C:L);".  n = 2: "(A:h,B:h);" with h = L * 0.5.  n = 1: "name;", n = 0: ";".
// No trailing newline.  Returns "" and sets err when the list is not such a tree: a child at or above its join's node, a node joined
// twice, a closing record that does not hold node 2n - 3.
std::string newick_text_nj(const std::vector<std::string> &names, const lash_nj_join *joins, std::string &err);

// The cut at max_height: exactly the merges with height <= max_height applied (NaN applies none); label[i] = the smallest leaf of i's
// component, for all n leaves.  false when the merge list is not a tree over n leaves.
bool tree_cut_labels(uint32_t n, const lash_tree_merge *merges, double max_height, std::vector<uint32_t> &label);

}  // namespace lashhost
