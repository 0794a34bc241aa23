// dist_tree.h — the lash_tree object (include/lash_gfx950.h: lash_tree_*) as dist_tree.hip (create, set_rows, get_rows, free, the
// linkage build) and dist_nj.hip (the neighbour-joining build) share it.  Internal: not part of the ABI.
#pragma once
#include "lash_ctx.h"

struct lash_tree {
    int device = 0;
    uint32_t n = 0;
    bool built = false;
    double *d_D = nullptr;                        // [n][n]
    double *d_stage = nullptr;                    // set_rows: a piece of the caller's triangle on its way into d_D
    size_t stage_cap = 0;                         // doubles
    std::vector<uint8_t> row_set;                 // host: which rows set_rows has seen
    bool has_nan = false;                         // host: the first NaN cell set_rows has seen, in (row, col) order of arrival
    uint32_t nan_row = 0, nan_col = 0;
    bool has_inf = false;                         // host: the first infinite cell, likewise (lash_tree_build_nj refuses it; the linkage
    uint32_t inf_row = 0, inf_col = 0;            // builds order +-inf like any other number and ignore this)
};

namespace lash {

constexpr uint32_t TREE_NONE = 0xFFFFFFFFu;

// the smaller of two keys (d, a, b), lexicographic; no NaN ever gets here (the builds refuse it)
__device__ inline bool key_less(double d0, uint32_t a0, uint32_t b0, double d1, uint32_t a1, uint32_t b1)
{
    if (d0 != d1) return d0 < d1;
    if (a0 != a1) return a0 < a1;
    return b0 < b1;
}

__device__ inline void wave_min_key(double &d, uint32_t &a, uint32_t &b)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, 64);
        const uint32_t oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64);
        if (key_less(od, oa, ob, d, a, b)) { d = od; a = oa; b = ob; }
    }
}

// The workgroup's minimum key in every thread of wave 0 (the other waves return their own wave's).  WAVES = blockDim.x / 64.
template <uint32_t WAVES>
__device__ inline void block_min_key(double &d, uint32_t &a, uint32_t &b, double *s_d, uint32_t *s_a, uint32_t *s_b)
{
    wave_min_key(d, a, b);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { s_d[wave] = d; s_a[wave] = a; s_b[wave] = b; }
    __syncthreads();
    if (wave == 0) {
        if (lane < WAVES) { d = s_d[lane]; a = s_a[lane]; b = s_b[lane]; }
        else { d = HUGE_VAL; a = TREE_NONE; b = TREE_NONE; }
        wave_min_key(d, a, b);
    }
}

}  // namespace lash
