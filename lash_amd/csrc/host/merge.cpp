// merge.cpp — `lash merge` for the gfx950 build (not upstream).
//
// The union of sketches is bit for bit the sketch of the inputs together, so a cluster's pangenome sketch, the sketch of a sample
// sequenced in several files or a bin's sketch needs no second pass over the sequences: the collection goes to the device once
// (one sketch set, in name-file order) and lash_sketch_set_group_union folds every group there (csrc/group_union.hip).  Groups are
// done in batches whose images stay under about 1 GiB and written in order through the zstd writer of `lash sketch`; the names file
// holds the group names and the parameters file is the input's, byte for byte, so the result reads like any sketched collection.
#include "merge.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <unordered_map>

#include "json_out.hpp"
#include "zstd_dl.hpp"

namespace lashhost {

std::string parse_groups(const std::string &text, const std::vector<std::string> &names, GroupList &out)
{
    std::unordered_map<std::string, std::vector<uint32_t>> by_name;
    for (size_t i = 0; i < names.size(); ++i) by_name[names[i]].push_back((uint32_t)i);
    std::unordered_map<std::string, size_t> group_of;
    std::vector<std::vector<uint32_t>> lists;
    out = GroupList();
    size_t at = 0, line_no = 0;
    while (at < text.size()) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(at, end - at);
        at = end + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line_no == 1 && line == "Representative\tMember") continue;
        const std::string where = "line " + std::to_string(line_no) + ": ";
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) return where + "no tab (group<TAB>member is required)";
        if (line.find('\t', tab + 1) != std::string::npos) return where + "more than one tab (group<TAB>member is required)";
        const std::string group = line.substr(0, tab), member = line.substr(tab + 1);
        if (group.empty()) return where + "empty group name";
        if (member.empty()) return where + "empty member name";
        const auto hit = by_name.find(member);
        if (hit == by_name.end()) return where + "'" + member + "' is not a name of the collection";
        auto g = group_of.find(group);
        if (g == group_of.end()) {
            g = group_of.emplace(group, lists.size()).first;
            out.names.push_back(group);
            lists.emplace_back();
        }
        lists[g->second].insert(lists[g->second].end(), hit->second.begin(), hit->second.end());
    }
    if (lists.empty()) return "no group in the file";
    out.off.push_back(0);
    for (const std::vector<uint32_t> &l : lists) {
        out.members.insert(out.members.end(), l.begin(), l.end());
        out.off.push_back(out.members.size());
    }
    return "";
}

std::string run_merge(const MergeOptions &opt)
{
    DistSide in;
    std::string err = load_dist_side(opt.side, in);
    if (!err.empty()) return err;
    const uint32_t n = (uint32_t)in.names.size();

    GroupList gl;
    if (!opt.all_name.empty()) {
        gl.names.push_back(opt.all_name);
        gl.members.resize(n);
        for (uint32_t i = 0; i < n; ++i) gl.members[i] = i;
        gl.off = {0, n};
    } else {
        std::ifstream f(opt.groups_file, std::ios::binary);
        if (!f) return "cannot open " + opt.groups_file;
        std::ostringstream ss;
        ss << f.rdbuf();
        err = parse_groups(ss.str(), in.names, gl);
        if (!err.empty()) return opt.groups_file + ": " + err;
    }
    // the names in no group: dropped, or singletons behind the groups in row order (the reference's key order, or list order)
    std::vector<bool> listed(n, false);
    for (uint32_t m : gl.members) listed[m] = true;
    uint64_t unlisted = 0;
    for (uint32_t i : in.order)
        if (!listed[i]) {
            ++unlisted;
            if (!opt.keep_others) continue;
            gl.names.push_back(in.names[i]);
            gl.members.push_back(i);
            gl.off.push_back(gl.members.size());
        }
    if (unlisted && !opt.keep_others) fprintf(stderr, "%llu sketches are in no group and were dropped (--keep-others keeps them)\n", (unsigned long long)unlisted);
    const size_t n_groups = gl.names.size();
    if (n_groups > 0xFFFFFFFFull) return "too many groups";

    const size_t ib = lash_layout_image_bytes(&opt.side.layout, in.algo_id, in.prec);
    lash_ctx *ctx = nullptr;
    lash_sketch_set *set = nullptr;
    struct Guard { lash_ctx *&c; lash_sketch_set *&s; ~Guard() { if (s) lash_sketch_set_free(c, s); if (c) lash_ctx_destroy(c); } } guard{ctx, set};
    int rc = lash_ctx_create(&ctx, opt.side.device);
    if (rc != LASH_OK) return lash_strerror(rc);
    if (rc == LASH_OK) rc = lash_ctx_set_layout(ctx, &opt.side.layout);
    if (rc == LASH_OK) rc = lash_sketch_set_create(ctx, in.algo_id, in.prec, in.images.data(), n, nullptr, n, &set);
    if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);

    lash_group_union_opts plan{0, 0, 0};
    rc = lash_sketch_set_group_union_plan(ctx, set, gl.off.data(), (uint32_t)n_groups, nullptr, &plan);
    if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);

    const lash_group_union_opts run{plan.segment, plan.slices, 0};      // every batch as planned for the whole list
    ZstdWriter zw;
    const std::string bin = opt.output + "_sketches.bin";
    err = zw.open(bin, 3, opt.side.threads);
    if (!err.empty()) return err;
    const size_t per_batch = std::max<size_t>(1, ((size_t)1 << 30) / ib);
    std::vector<uint8_t> images;
    std::vector<uint64_t> off;
    double fold_ms = 0.0;
    for (size_t g0 = 0; g0 < n_groups && err.empty(); g0 += per_batch) {
        const size_t g1 = std::min(n_groups, g0 + per_batch);
        off.assign(gl.off.begin() + g0, gl.off.begin() + g1 + 1);
        for (uint64_t &o : off) o -= gl.off[g0];
        images.resize((g1 - g0) * ib);
        uint64_t bad = 0;
        const auto t0 = std::chrono::steady_clock::now();
        rc = lash_sketch_set_group_union(ctx, set, off.data(), gl.members.data() + gl.off[g0], (uint32_t)(g1 - g0), &run, images.data(), &bad);
        fold_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != LASH_OK) err = std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);
        else err = zw.write(images.data(), images.size());
    }
    if (err.empty()) err = zw.finish();
    if (!err.empty()) { (void)remove(bin.c_str()); return err; }
    {
        std::ofstream out(opt.output + "_files.json", std::ios::binary);
        if (!out) return "cannot create " + opt.output + "_files.json";
        out << json_pretty_string_array(gl.names);
        if (!out.good()) return "write failed";
    }
    {
        std::ifstream src(in.params_file, std::ios::binary);
        if (!src) return "cannot open " + in.params_file;
        std::ofstream out(opt.output + "_parameters.json", std::ios::binary);
        if (!out) return "cannot create " + opt.output + "_parameters.json";
        std::ostringstream ss;
        ss << src.rdbuf();
        const std::string bytes = ss.str();
        out.write(bytes.data(), (std::streamsize)bytes.size());
        if (!out.good()) return "write failed";
    }
    if (getenv("LASH_CLI_TIMING")) {
        fprintf(stderr, "[lash merge] %u names, %zu groups, %zu members, segment %u, fold %.3f ms\n", n, n_groups, gl.members.size(), plan.segment,
                fold_ms);
    }
    return "";
}

}  // namespace lashhost
