// spectrum.cpp — `lash spectrum` for the gfx950 build (not upstream).
//
// A bucket's union register belongs to one k-mer of the group's union, drawn uniformly from the bucket's distinct k-mers, and the
// members whose register equals it are the members that hold that k-mer: over the occupied buckets, the histogram of that number is
// a uniform sample of the union's multiplicity spectrum.  The collection goes to the device once (one sketch set,
// in name-file order); lash_sketch_set_group_spectrum returns every group's bins and union image; the union's cardinality — the number
// `lash merge` followed by the cardinality path gives — scales the bins to k-mers.  HyperMinHash collections only.
#include "spectrum.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "merge.hpp"

namespace lashhost {

std::string check_fractions(double core, double cloud)
{
    if (!(core > 0.0 && core <= 1.0)) return "--core must lie in (0, 1]";
    if (!(cloud > 0.0 && cloud <= 1.0)) return "--cloud must lie in (0, 1]";
    if (cloud > core) return "--cloud must not be above --core";
    return "";
}

SpectrumClasses spectrum_classes(const uint32_t *hist, uint32_t n, double U, double core, double cloud)
{
    SpectrumClasses k;
    const uint32_t occupied = 16384u - hist[0];
    if (!occupied) return k;
    for (uint32_t c = 1; c <= n; ++c) {
        if (!hist[c]) continue;
        const double kmers = (double)hist[c] / (double)occupied * U;
        if ((double)c >= core * (double)n) k.core += kmers;
        else if ((double)c < cloud * (double)n) k.cloud += kmers;
        else k.shell += kmers;
    }
    return k;
}

void spectrum_curves(const uint32_t *hist, uint32_t n, double U, std::vector<double> &pan, std::vector<double> &core)
{
    pan.assign(n, 0.0);
    core.assign(n, 0.0);
    const uint32_t occupied = 16384u - hist[0];
    if (!occupied) return;
    std::vector<uint32_t> cs;                                               // the counts that have buckets, ascending
    for (uint32_t c = 1; c <= n; ++c)
        if (hist[c]) cs.push_back(c);
    std::vector<double> in_all(cs.size(), 1.0), in_none(cs.size(), 1.0);   // prod_{i<m} (c-i)/(n-i) and prod_{i<m} (n-c-i)/(n-i)
    const double scale = U / (double)occupied;
    for (uint32_t m = 1; m <= n; ++m) {
        const uint32_t i = m - 1;
        double sum_core = 0.0, sum_pan = 0.0;
        for (size_t x = 0; x < cs.size(); ++x) {
            const uint32_t c = cs[x];
            in_all[x] = c > i ? in_all[x] * (double)(c - i) / (double)(n - i) : 0.0;
            in_none[x] = n - c > i ? in_none[x] * (double)(n - c - i) / (double)(n - i) : 0.0;
            sum_core += (double)hist[c] * in_all[x];
            sum_pan += (double)hist[c] * (1.0 - in_none[x]);
        }
        core[i] = scale * sum_core;
        pan[i] = scale * sum_pan;
    }
}

namespace {

bool write_file(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}

}  // namespace

std::string run_spectrum(const SpectrumOptions &opt)
{
    DistSide in;
    std::string err = load_dist_side(opt.side, in);
    if (!err.empty()) return err;
    if (in.algo_id != LASH_HMH)
        return std::string("the collection was sketched with -a ") + (in.algo_id == LASH_HLL ? "hll" : "ull") +
               ": lash spectrum needs HyperMinHash sketches (-a hmh), whose registers identify a k-mer";
    const uint32_t n = (uint32_t)in.names.size();

    GroupList gl;
    if (opt.groups_file.empty()) {
        gl.names.push_back(opt.all_name.empty() ? "all" : opt.all_name);
        gl.members.resize(n);
        for (uint32_t i = 0; i < n; ++i) gl.members[i] = i;
        gl.off = {0, n};
    } else {
        std::ifstream f(opt.groups_file, std::ios::binary);
        if (!f) return "cannot open " + opt.groups_file;
        std::ostringstream ss;
        ss << f.rdbuf();
        GroupList listed;
        err = parse_groups(ss.str(), in.names, listed);
        if (!err.empty()) return opt.groups_file + ": " + err;
        // a sketch counts once per group, however often its name is listed
        gl.names = listed.names;
        gl.off.push_back(0);
        for (size_t g = 0; g < listed.names.size(); ++g) {
            std::vector<uint32_t> m(listed.members.begin() + listed.off[g], listed.members.begin() + listed.off[g + 1]);
            std::sort(m.begin(), m.end());
            m.erase(std::unique(m.begin(), m.end()), m.end());
            gl.members.insert(gl.members.end(), m.begin(), m.end());
            gl.off.push_back(gl.members.size());
        }
    }
    const size_t n_groups = gl.names.size();
    if (n_groups > 0xFFFFFFFFull) return "too many groups";

    const size_t ib = lash_layout_image_bytes(&opt.side.layout, in.algo_id, in.prec), hdr = lash_layout_header_bytes(&opt.side.layout, in.algo_id);
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
    const lash_group_union_opts run{plan.segment, plan.slices, 0};          // every batch as planned for the whole list

    // groups in batches whose union images stay under about 1 GiB; the tables are small and are written when all of them are done
    std::string spectrum = "Group\tMembers\tCount\tBuckets\tKmers\n", groups = "Group\tMembers\tOccupied\tUnion\tCore\tShell\tCloud\n",
                curves = "Group\tGenomes\tPan\tCore\n";
    const size_t per_batch = std::max<size_t>(1, ((size_t)1 << 30) / ib);
    std::vector<uint8_t> images;
    std::vector<uint32_t> hist;
    std::vector<uint64_t> off;
    std::vector<double> pan, core;
    char buf[160];
    for (size_t g0 = 0; g0 < n_groups; g0 += per_batch) {
        const size_t g1 = std::min(n_groups, g0 + per_batch);
        off.assign(gl.off.begin() + g0, gl.off.begin() + g1 + 1);
        for (uint64_t &o : off) o -= gl.off[g0];
        images.resize((g1 - g0) * ib);
        hist.resize(off.back() + (g1 - g0));
        uint64_t bad = 0;
        rc = lash_sketch_set_group_spectrum(ctx, set, off.data(), gl.members.data() + gl.off[g0], (uint32_t)(g1 - g0), &run, hist.data(), images.data(), &bad);
        if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);
        for (size_t g = g0; g < g1; ++g) {
            const uint32_t members = (uint32_t)(off[g - g0 + 1] - off[g - g0]);
            const uint32_t *h = hist.data() + off[g - g0] + (g - g0);
            const uint32_t occupied = 16384u - h[0];
            const double U = lash_hmh_cardinality(images.data() + (g - g0) * ib + hdr, opt.side.layout.hmh_reg_be);
            if (occupied)
                for (uint32_t c = 1; c <= members; ++c) {
                    if (!h[c]) continue;
                    snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%.3f\n", members, c, h[c], (double)h[c] / (double)occupied * U);
                    spectrum += gl.names[g];
                    spectrum += buf;
                }
            const SpectrumClasses k = spectrum_classes(h, members, U, opt.core, opt.cloud);
            snprintf(buf, sizeof buf, "\t%u\t%u\t%.3f\t%.3f\t%.3f\t%.3f\n", members, occupied, U, k.core, k.shell, k.cloud);
            groups += gl.names[g];
            groups += buf;
            if (opt.curves) {
                spectrum_curves(h, members, U, pan, core);
                for (uint32_t m = 1; m <= members; ++m) {
                    snprintf(buf, sizeof buf, "\t%u\t%.10g\t%.10g\n", m, pan[m - 1], core[m - 1]);
                    curves += gl.names[g];
                    curves += buf;
                }
            }
        }
    }
    if (!write_file(opt.output + "_spectrum.tsv", spectrum)) return "cannot write " + opt.output + "_spectrum.tsv";
    if (!write_file(opt.output + "_groups.tsv", groups)) return "cannot write " + opt.output + "_groups.tsv";
    if (opt.curves && !write_file(opt.output + "_curves.tsv", curves)) return "cannot write " + opt.output + "_curves.tsv";
    return "";
}

}  // namespace lashhost
