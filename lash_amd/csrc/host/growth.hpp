// growth.hpp — `lash growth` (not upstream): how much each further genome of a collection adds.  The union cardinality of the
// first t names along one or more orderings of one sketch collection, folded on the GPU (lash_sketch_set_prefix_union_cardinalities).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "dist.hpp"

namespace lashhost {

struct GrowthOptions {
    DistOptions side;          // ref_prefix, estimator, threads, file_order, hll_bias_file / hll_bias_sim, device, layout: as `dist` reads a side
    std::string output_file = "growth";
    uint32_t orders = 1;       // order 0 = the rows as they are; orders 1 .. P-1 = seeded shuffles of it
    uint64_t seed = 42;
};

// splitmix64 as published (Steele, Lea & Flood 2014; Vigna's splitmix64.c): the state advances by the golden gamma, the output is mixed
inline uint64_t splitmix64_next(uint64_t &state)
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Order o of n rows: 0 = identity; else the Fisher–Yates shuffle of the identity driven by splitmix64 from state seed ^ (o * gamma),
// position j = n-1 .. 1 swapped with the high 64 bits of next() * (j + 1)
std::vector<uint32_t> growth_order(uint32_t n, uint32_t o, uint64_t seed);

std::string run_growth(const GrowthOptions &opt);

}  // namespace lashhost
