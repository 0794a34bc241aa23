// screen.cpp — `lash screen` for the gfx950 build (not upstream; the question of Mash's `screen -w`).
//
// Both collections go to the device once, rows in the reference's key order (list order under --file-order).  Candidates: per query the
// references whose `--containment reference` distance d passes d <= D, found block of rows by block of rows as `dist --max-dist` finds
// them (lash_sketch_set_pair_block_within_measure); the same blocks give each pair's N (lash_sketch_set_pair_block) and, for small pairs,
// its expected collisions (lash_sketch_set_hmh_expected_collisions).  Priority within a query: d ascending, then the reference's
// cardinality descending (Mash's tie rule: the larger genome), then the reference row.  One call of lash_sketch_set_screen_wta gives,
// for every candidate, the buckets it shares with the query and the buckets it won; WtaDistance is lash_dist_rows_measure's number for
// the pair with C replaced by the buckets won.  Every number is a pure function of the two collections, so the bytes do not depend on
// --block-rows or -t.
#include "screen.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "dist_format.hpp"

namespace lashhost {

std::string check_screen_max_dist(double d)
{
    if (!(d >= 0.0 && d <= 1.0)) return "a number from 0 to 1 is required";
    return "";
}

namespace {

struct Candidate {
    uint32_t row;      // the reference row
    uint32_t n;        // the pair's N
    double d;          // the containment distance
    double ec;         // the pair's expected collisions where the device computed them (small pairs)
    bool has_ec;
};

std::string refused_algo(const char *which, int algo_id)
{
    return std::string("the ") + which + " collection was sketched with -a " + (algo_id == LASH_HLL ? "hll" : "ull") +
           ": lash screen needs HyperMinHash sketches (-a hmh), whose registers identify a k-mer";
}

}  // namespace

std::string run_screen(const ScreenOptions &opt)
{
    DistSide R, Q;
    std::string err = load_dist_side(opt.side, R);
    if (!err.empty()) return err;
    DistOptions qside = opt.side;
    qside.ref_prefix = opt.side.query_prefix;
    if (!(err = load_dist_side(qside, Q)).empty()) return err;
    if (R.k != Q.k) return "Genomes were not sketched with the same k";
    if (R.algo_id != Q.algo_id) return "Algorithms do not match in query and sketch genomes";
    if (R.algo_id != LASH_HMH) return refused_algo("reference", R.algo_id);
    if (Q.algo_id != LASH_HMH) return refused_algo("query", Q.algo_id);
    const uint32_t nr = (uint32_t)R.order.size(), nq = (uint32_t)Q.order.size();
    const double D = opt.has_max_dist ? opt.max_dist : std::nextafter(1.0, 0.0);
    const int measure = LASH_MEASURE_CONTAIN_REFERENCE;

    lash_ctx *ctx = nullptr;
    lash_sketch_set *ref = nullptr, *qry = nullptr;
    struct Guard {
        lash_ctx *&c; lash_sketch_set *&r; lash_sketch_set *&q;
        ~Guard() { if (q) lash_sketch_set_free(c, q); if (r) lash_sketch_set_free(c, r); if (c) lash_ctx_destroy(c); }
    } guard{ctx, ref, qry};
    auto failed = [&](int rc) { return std::string(lash_strerror(rc)) + " " + (ctx ? lash_ctx_last_error(ctx) : ""); };
    int rc = lash_ctx_create(&ctx, opt.side.device);
    if (rc != LASH_OK) return lash_strerror(rc);
    rc = lash_ctx_set_layout(ctx, &opt.side.layout);
    if (rc == LASH_OK) rc = lash_sketch_set_create(ctx, LASH_HMH, 0, R.images.data(), (uint32_t)R.names.size(), R.order.data(), nr, &ref);
    if (rc == LASH_OK) rc = lash_sketch_set_create(ctx, LASH_HMH, 0, Q.images.data(), (uint32_t)Q.names.size(), Q.order.data(), nq, &qry);
    std::vector<double> rcard(nr), qcard(nq);
    uint32_t bad_card = 0;
    if (rc == LASH_OK) rc = lash_sketch_set_cardinalities(ctx, ref, LASH_ULL_FGRA, nullptr, rcard.data(), &bad_card);
    if (rc == LASH_OK) rc = lash_sketch_set_cardinalities(ctx, qry, LASH_ULL_FGRA, nullptr, qcard.data(), &bad_card);
    if (rc == LASH_OK) rc = lash_sketch_set_prepare(ctx, ref, qry);
    if (rc != LASH_OK) return failed(rc);

    // the candidates, block of reference rows by block
    std::vector<std::vector<Candidate>> cand(nq);
    const uint32_t block = opt.side.block_rows ? opt.side.block_rows : (uint32_t)std::max<uint64_t>(1, (4ull << 20) / std::max(nq, 1u));
    std::vector<uint32_t> C, N, w_row, w_col;
    std::vector<double> EC, w_dist;
    for (uint32_t i0 = 0; i0 < nr && nq; i0 += std::min(block, nr - i0)) {
        const uint32_t i1 = i0 + std::min(block, nr - i0);
        const size_t np = (size_t)(i1 - i0) * nq;
        C.resize(np);
        N.resize(np);
        EC.assign(np, 0.0);
        uint64_t n_small = 0, kept = 0, bad = 0;
        rc = lash_sketch_set_pair_block(ctx, ref, i0, i1, qry, nq, 0, LASH_ULL_FGRA, C.data(), N.data(), nullptr);
        if (rc == LASH_OK) rc = lash_sketch_set_hmh_expected_collisions(ctx, ref, i0, i1, qry, nq, EC.data(), &n_small);
        if (w_row.empty()) { w_row.resize(1u << 12); w_col.resize(1u << 12); w_dist.resize(1u << 12); }
        while (rc == LASH_OK) {
            rc = lash_sketch_set_pair_block_within_measure(ctx, ref, i0, i1, qry, nq, 0, R.k, opt.side.model, 0, LASH_ULL_FGRA, nullptr, measure, D,
                                                           w_row.data(), w_col.data(), w_dist.data(), w_row.size(), &kept, &bad, nullptr);
            if (rc != LASH_OK || kept <= w_row.size()) break;
            w_row.resize(kept + kept / 4); w_col.resize(w_row.size()); w_dist.resize(w_row.size());
        }
        if (rc != LASH_OK) return failed(rc);
        for (uint64_t s = 0; s < kept; ++s) {
            const size_t at = (size_t)(w_row[s] - i0) * nq + w_col[s];
            cand[w_col[s]].push_back(Candidate{w_row[s], N[at], w_dist[s], EC[at], n_small != 0});
        }
    }

    // priority, and the lists as one CSR
    std::vector<uint64_t> off(nq + 1, 0);
    std::vector<uint32_t> rows;
    for (uint32_t j = 0; j < nq; ++j) {
        std::sort(cand[j].begin(), cand[j].end(), [&](const Candidate &a, const Candidate &b) {
            if (a.d != b.d) return a.d < b.d;
            if (rcard[a.row] != rcard[b.row]) return rcard[a.row] > rcard[b.row];
            return a.row < b.row;
        });
        for (const Candidate &c : cand[j]) rows.push_back(c.row);
        off[j + 1] = rows.size();
    }
    std::vector<uint32_t> shared(rows.size()), won(rows.size());
    uint64_t bad_index = 0;
    rc = lash_sketch_set_screen_wta(ctx, ref, qry, off.data(), rows.data(), nullptr, shared.data(), won.data(), &bad_index);
    if (rc != LASH_OK) return failed(rc);

    std::string text = "Query\tReference\tShared\tWon\tBuckets\tDistance\tWtaDistance\n";
    char buf[64];
    for (uint32_t j = 0; j < nq; ++j) {
        const std::string &qname = Q.names[Q.order[j]];
        for (size_t t = 0; t < cand[j].size(); ++t) {
            const Candidate &c = cand[j][t];
            const uint64_t e = off[j] + t;
            double wta = 0.0;
            uint64_t bad_pair = 0;
            rc = lash_dist_rows_measure(LASH_HMH, 0, R.k, opt.side.model, 0, 1, 1, &rcard[c.row], &qcard[j], &won[e], &c.n, nullptr, nullptr,
                                        c.has_ec ? &c.ec : nullptr, measure, &wta, &bad_pair);
            if (rc != LASH_OK) return lash_strerror(rc);
            if (!opt.keep_losers && !(wta <= D)) continue;
            text += qname;
            text += '\t';
            text += R.names[R.order[c.row]];
            snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t", shared[e], won[e], c.n);
            text += buf;
            append_dist(text, c.d);
            text += '\t';
            append_dist(text, wta);
            text += '\n';
        }
    }
    FILE *f = fopen(opt.output.c_str(), "w");
    if (!f) return "cannot create " + opt.output;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return "cannot write " + opt.output;
    return "";
}

}  // namespace lashhost
