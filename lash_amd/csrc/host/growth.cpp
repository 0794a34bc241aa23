// growth.cpp — `lash growth` for the gfx950 build (not upstream).
//
// The pangenome growth (rarefaction) curve of one sketch collection: for each ordering of its names, the distinct k-mers of the
// first t of them, t = 1 .. N, and what name t added.  A union of sketches is the sketch of the union, so the curve is a fold of
// register tables; lash_sketch_set_prefix_union_cardinalities does all orders in one call (one launch per chunk of orders,
// csrc/prefix_union.hip) and returns the numbers the single-sketch estimators give for each prefix's image.
// Input: one side of a `dist` run, read by dist.cpp's loader.  Order 0 is the run's row order (the reference's key order, or list
// order with --file-order: how a user says "in this order"); orders 1 .. P-1 are seeded shuffles of it (growth.hpp), so a run is a
// function of (files, --orders, --seed).  One device.  -t threads format the table; the bytes do not depend on it.
#include "growth.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>

namespace lashhost {

std::vector<uint32_t> growth_order(uint32_t n, uint32_t o, uint64_t seed)
{
    std::vector<uint32_t> a(n);
    std::iota(a.begin(), a.end(), 0u);
    if (o == 0) return a;
    uint64_t state = seed ^ ((uint64_t)o * 0x9E3779B97F4A7C15ull);
    for (uint32_t j = n; j-- > 1;) {
        const uint64_t r = (uint64_t)(((unsigned __int128)splitmix64_next(state) * (uint64_t)(j + 1)) >> 64);
        std::swap(a[j], a[(uint32_t)r]);
    }
    return a;
}

std::string run_growth(const GrowthOptions &opt)
{
    DistSide in;
    std::string err = load_dist_side(opt.side, in);
    if (!err.empty()) return err;
    lash_hll_bias *bias = nullptr;
    err = load_hll_bias(opt.side, in.algo_id, in.prec, "lash growth", &bias);
    struct BiasGuard { lash_hll_bias *&b; ~BiasGuard() { lash_hll_bias_free(b); } } bias_guard{bias};
    if (!err.empty()) return err;

    const uint32_t n = (uint32_t)in.order.size(), P = opt.orders;
    std::vector<uint32_t> orders;
    orders.reserve((size_t)P * n);
    for (uint32_t o = 0; o < P; ++o) {
        const std::vector<uint32_t> a = growth_order(n, o, opt.seed);
        orders.insert(orders.end(), a.begin(), a.end());
    }

    lash_ctx *ctx = nullptr;
    lash_sketch_set *set = nullptr;
    struct Guard { lash_ctx *&c; lash_sketch_set *&s; ~Guard() { if (s) lash_sketch_set_free(c, s); if (c) lash_ctx_destroy(c); } } guard{ctx, set};
    int rc = lash_ctx_create(&ctx, opt.side.device);
    if (rc != LASH_OK) return lash_strerror(rc);
    if (rc == LASH_OK) rc = lash_ctx_set_layout(ctx, &opt.side.layout);
    if (rc == LASH_OK) rc = lash_sketch_set_create(ctx, in.algo_id, in.prec, in.images.data(), (uint32_t)in.names.size(), in.order.data(), n, &set);
    if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);
    std::vector<double> card((size_t)P * n);
    lash_prefix_union_opts plan{0, 0};
    const auto t_build = std::chrono::steady_clock::now();
    if (n) {
        uint64_t bad = 0;
        rc = lash_sketch_set_prefix_union_plan(ctx, set, P, n, nullptr, &plan);
        if (rc == LASH_OK) rc = lash_sketch_set_prefix_union_cardinalities(ctx, set, orders.data(), P, n, in.ull_est, bias, &plan, card.data(), &bad);
        if (rc == LASH_ERANGE) {
            const uint64_t o = bad / n, t = bad % n;
            return "order " + std::to_string(o) + ", step " + std::to_string(t + 1) + " (" + in.names[in.order[orders[bad]]] +
                   "): the union's cardinality estimate is <= 5 * 2^p and needs the HLL++ bias tables of streaming_algorithms, which are not "
                   "built in (pass --hll-bias-sim to simulate them, --hll-bias <file from lash hll-bias>, or sketch with a smaller -p)";
        }
        if (rc != LASH_OK) return std::string(lash_strerror(rc)) + " " + lash_ctx_last_error(ctx);
    }
    const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();

    // the table: P * N lines in (order, step) order, formatted by -t threads in contiguous runs of lines
    const size_t lines = (size_t)P * n;
    const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, opt.side.threads), lines / 4096 + 1));
    std::vector<std::string> part(T);
    auto format = [&](size_t w) {
        const size_t i0 = lines * w / T, i1 = lines * (w + 1) / T;
        std::string &s = part[w];
        char buf[96];
        for (size_t i = i0; i < i1; ++i) {
            const size_t o = i / n, t = i % n;
            const double u = card[i], added = t ? u - card[i - 1] : u;
            s += std::to_string(o);
            s += '\t';
            s += std::to_string(t + 1);
            s += '\t';
            s += in.names[in.order[orders[i]]];
            snprintf(buf, sizeof buf, "\t%.3f\t%.3f\n", u, added);
            s += buf;
        }
    };
    {
        std::vector<std::thread> pool;
        for (size_t w = 1; w < T; ++w) pool.emplace_back(format, w);
        format(0);
        for (auto &t : pool) t.join();
    }
    FILE *f = fopen(opt.output_file.c_str(), "w");
    if (!f) return "cannot create " + opt.output_file;
    bool ok = fputs("Order\tStep\tName\tUnion\tNew\n", f) >= 0;
    for (const std::string &s : part) ok = ok && fwrite(s.data(), 1, s.size(), f) == s.size();
    if (fclose(f) != 0 || !ok) return "cannot write " + opt.output_file;
    if (getenv("LASH_CLI_TIMING")) {
        fprintf(stderr, "[lash growth] %u names, %u orders, %u slices, %llu histogram bytes, build %.3f ms\n", n, P, plan.slices,
                (unsigned long long)plan.hist_budget_bytes, build_ms);
    }
    return "";
}

}  // namespace lashhost
