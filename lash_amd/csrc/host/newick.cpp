// newick.cpp — see newick.hpp.
#include "newick.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace lashhost {

std::string newick_label(const std::string &name)
{
    bool quote = false;
    for (const char ch : name)
        if ((ch != 0 && strchr("()[]':;,", ch)) || ch == ' ' || (ch >= '\t' && ch <= '\r')) { quote = true; break; }
    if (!quote) return name;
    std::string out = "'";
    for (const char ch : name) {
        if (ch == '\'') out += '\'';
        out += ch;
    }
    out += '\'';
    return out;
}

namespace {

// every child below 2n - 1 and below its own merge's node, each node a child at most once
bool merges_are_a_tree(uint32_t n, const lash_tree_merge *m)
{
    if (n < 2) return true;
    std::vector<uint8_t> used((size_t)2 * n - 1, 0);
    for (uint32_t s = 0; s + 1 < n; ++s)
        for (const uint32_t c : {m[s].a, m[s].b}) {
            if (c >= n + s || used[c]) return false;
            used[c] = 1;
        }
    return true;
}

}  // namespace

std::string newick_text(const std::vector<std::string> &names, const lash_tree_merge *merges, std::string &err)
{
    const uint32_t n = (uint32_t)names.size();
    err.clear();
    if (n == 0) return ";";
    if (n == 1) return newick_label(names[0]) + ";";
    if (!merges_are_a_tree(n, merges)) { err = "the merge list is not a tree"; return ""; }
    auto height = [&](uint32_t node) { return node < n ? 0.0 : merges[node - n].height; };
    std::string out;
    // depth first without recursion (a chain of 10^5 merges is 10^5 deep): a frame is a node and how many of its children are written
    struct Frame { uint32_t node, parent, done; };
    std::vector<Frame> stack{{2 * n - 2, 0xFFFFFFFFu, 0}};
    char buf[48];
    while (!stack.empty()) {
        Frame &f = stack.back();
        const bool leaf = f.node < n;
        if (!leaf && f.done < 2) {
            out += f.done == 0 ? '(' : ',';
            const uint32_t child = f.done == 0 ? merges[f.node - n].a : merges[f.node - n].b;
            ++f.done;
            const uint32_t parent = f.node;
            stack.push_back({child, parent, 0});                                     // (f is dead from here on)
            continue;
        }
        if (leaf) out += newick_label(names[f.node]);
        else out += ')';
        if (f.parent == 0xFFFFFFFFu) out += ';';
        else {
            snprintf(buf, sizeof buf, ":%.10g", height(f.parent) / 2 - height(f.node) / 2);
            out += buf;
        }
        stack.pop_back();
    }
    return out;
}

std::string newick_text_nj(const std::vector<std::string> &names, const lash_nj_join *joins, std::string &err)
{
    const uint32_t n = (uint32_t)names.size();
    err.clear();
    if (n == 0) return ";";
    if (n == 1) return newick_label(names[0]) + ";";
    char buf[48];
    const lash_nj_join &last = joins[n - 2];
    if (n == 2) {
        if (!((last.a == 0 && last.b == 1) || (last.a == 1 && last.b == 0))) { err = "the join list is not a tree"; return ""; }
        snprintf(buf, sizeof buf, ":%.10g", last.len_a * 0.5);
        return "(" + newick_label(names[last.a]) + buf + "," + newick_label(names[last.b]) + buf + ");";
    }
    // nodes 0 .. 2n - 3; every one a child exactly once, the closing record's two included
    const uint32_t root = 2 * n - 3;
    std::vector<uint8_t> used((size_t)2 * n - 2, 0);
    std::vector<double> len((size_t)2 * n - 2, 0.0);                                 // the branch above every node
    for (uint32_t s = 0; s + 2 < n; ++s) {
        const uint32_t c[2] = {joins[s].a, joins[s].b};
        const double l[2] = {joins[s].len_a, joins[s].len_b};
        for (int e = 0; e < 2; ++e) {
            if (c[e] >= n + s || used[c[e]]) { err = "the join list is not a tree"; return ""; }
            used[c[e]] = 1;
            len[c[e]] = l[e];
        }
    }
    if (last.a > root || last.b > root || last.a == last.b || used[last.a] || used[last.b] || (last.a != root && last.b != root)) {
        err = "the join list is not a tree: its closing record does not hold the last two nodes";
        return "";
    }
    const uint32_t other = last.a == root ? last.b : last.a;
    len[other] = last.len_a;
    std::string out;
    // depth first without recursion, as newick_text; the root has a third child
    struct Frame { uint32_t node, done; };
    std::vector<Frame> stack{{root, 0}};
    while (!stack.empty()) {
        Frame &f = stack.back();
        const bool leaf = f.node < n;
        const uint32_t n_children = leaf ? 0 : f.node == root ? 3 : 2;
        if (f.done < n_children) {
            out += f.done == 0 ? '(' : ',';
            const uint32_t child = f.done == 0 ? joins[f.node - n].a : f.done == 1 ? joins[f.node - n].b : other;
            ++f.done;
            stack.push_back({child, 0});                                             // (f is dead from here on)
            continue;
        }
        if (leaf) out += newick_label(names[f.node]);
        else out += ')';
        if (f.node == root) out += ';';
        else {
            snprintf(buf, sizeof buf, ":%.10g", len[f.node]);
            out += buf;
        }
        stack.pop_back();
    }
    return out;
}

bool tree_cut_labels(uint32_t n, const lash_tree_merge *merges, double max_height, std::vector<uint32_t> &label)
{
    label.resize(n);
    std::iota(label.begin(), label.end(), 0u);
    if (n < 2) return true;
    if (!merges_are_a_tree(n, merges)) return false;
    std::vector<uint32_t> leaf_of((size_t)2 * n - 1);                                // a leaf below every node
    std::iota(leaf_of.begin(), leaf_of.begin() + n, 0u);
    auto find = [&](uint32_t x) {
        while (label[x] != x) { label[x] = label[label[x]]; x = label[x]; }
        return x;
    };
    for (uint32_t s = 0; s + 1 < n; ++s) {
        const uint32_t a = leaf_of[merges[s].a], b = leaf_of[merges[s].b];
        leaf_of[n + s] = a;
        if (!(merges[s].height <= max_height)) continue;
        const uint32_t ra = find(a), rb = find(b);
        if (ra != rb) label[ra > rb ? ra : rb] = ra > rb ? rb : ra;                  // the smaller index is the root
    }
    for (uint32_t i = 0; i < n; ++i) label[i] = find(i);
    return true;
}

}  // namespace lashhost

extern "C" {

// The functions above for callers outside C++ (tests through liblash_host.so).  newick: n NUL-terminated names; returns the
// malloc'd text (free with lash_host_free) or NULL when the merge list is not a tree.  cut: 0, or -1 for such a list.
char *lash_host_newick(const char *const *names, uint32_t n, const lash_tree_merge *merges)
{
    std::vector<std::string> v(names, names + n);
    std::string err;
    const std::string text = lashhost::newick_text(v, merges, err);
    if (!err.empty()) return nullptr;
    char *p = static_cast<char *>(malloc(text.size() + 1));
    if (p) memcpy(p, text.c_str(), text.size() + 1);
    return p;
}

// newick_text_nj likewise: n - 1 records; NULL when the list is not such a tree
char *lash_host_newick_nj(const char *const *names, uint32_t n, const lash_nj_join *joins)
{
    std::vector<std::string> v(names, names + n);
    std::string err;
    const std::string text = lashhost::newick_text_nj(v, joins, err);
    if (!err.empty()) return nullptr;
    char *p = static_cast<char *>(malloc(text.size() + 1));
    if (p) memcpy(p, text.c_str(), text.size() + 1);
    return p;
}

int lash_host_tree_cut(uint32_t n, const lash_tree_merge *merges, double max_height, uint32_t *label)
{
    std::vector<uint32_t> lab;
    if (!lashhost::tree_cut_labels(n, merges, max_height, lab)) return -1;
    if (n) memcpy(label, lab.data(), (size_t)n * 4);
    return 0;
}

}  // extern "C"
