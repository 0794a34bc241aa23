// hll_bias_sim.hip — HLL++ bias tables by Monte-Carlo on the GPU (lash_hll_bias_simulate, include/lash_gfx950.h; DESIGN.md
// "Simulated HLL++ bias tables").  Heule et al. made their tables by sketching random sets of every cardinality up to 5m and
// recording the mean raw estimate and its bias; the crate's copy of those numbers is not in this tree, so the same
// measurement is run here, from a seed, with every step fixed so that a CPU restatement gives the same bits
// (tests/hllsimref.py):
//   mix(x)            splitmix64's output step on x + 0x9E3779B97F4A7C15 (a bijection: the elements of a trial are distinct)
//   element i of t    h = mix(mix(seed ^ t * 0xD1342543DE82EF95) + i)
//   register rule     bucket = h & (m - 1), w = h >> p, rank = clz64(w) - p + 1 (65 - p for w == 0), reg = max(reg, rank)
//   checkpoint j      n_j = j * 5m / (N - 1); after the elements i < n_j: S = sum_r hist[r] * 2^-r from 0.0 in increasing r,
//                     E = alpha * m * m / S (the expression of pairmath::hll_len_regime)
//   table             raw_j = (sum_t E[t][j]) / T: the exact sum (so trial order, or any order, without a rounding between
//                     the addends) and the exact quotient, rounded ONCE to the nearest double — raw_0 is alpha * m for every T,
//                     which a sum rounded after each addend misses by an ulp from T = 3 on; bias_j = raw_j - n_j
// One workgroup runs one trial with its registers (one dword each: LDS has no byte max) and the 65-entry histogram in LDS.
// The histogram is kept incrementally: the max-atomic returns the old register, an increase moves one count from hist[old]
// to hist[new].  Increases of one register telescope whatever their order, so after the barrier the histogram is a function
// of the register state alone and E does not depend on lane order.  From p = 16 the registers of a trial no longer fit one
// workgroup's LDS (2^15 dwords = 128 KiB of the CU's 160): the trial is split over slices of 2^15 buckets, every slice
// workgroup hashes every element and keeps its own buckets, and the per-slice integer histograms are added (integer atomics:
// exact, so order-free) before a second kernel forms S the same way.  The mean over trials is taken on the host (sim_exact_mean).
#include "dist_pair.h"
#include "lash_ctx.h"

namespace {

constexpr int SIM_SLICE_LOG = 15;            // buckets per workgroup: 2^15 dword registers = 128 KiB of LDS
constexpr uint32_t SIM_RANKS = 65;           // rank 0..64 (rank <= 65 - p <= 61 is reached; 65 as the procedure states it)
constexpr size_t SIM_HIST_BYTES = 64u << 20; // slice path: trials per launch are bounded by this much global histogram

__host__ __device__ inline uint64_t sim_mix(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ inline double sim_estimate(const uint32_t *hist, double alpha, double m)
{
#pragma clang fp contract(off)
    double s = 0.0, w = 1.0;                                             // w = 2^-r exactly
    for (uint32_t r = 0; r < SIM_RANKS; ++r) { s += (double)hist[r] * w; w *= 0.5; }
    return alpha * m * m / s;
}

// grid = trials * slices workgroups; LDS = [slice_m registers | 65 counts | 65 counts (snapshot)] dwords.
// slices == 1: E[(t0 + trial) * n_points + j] is written here.  slices > 1: ghist[(trial * n_points + j) * 65 + r] += counts.
__global__ __launch_bounds__(1024) void hll_bias_sim_kernel(int p, uint32_t n_points, uint32_t t0, uint32_t slice_log, uint64_t seed,
                                                            double alpha, double *E, uint32_t *ghist)
{
    extern __shared__ uint32_t sim_lds[];
    const uint32_t slice_m = 1u << slice_log, slices = (1u << p) >> slice_log;           // slice_log = min(p, 15)
    uint32_t *reg = sim_lds, *hist = sim_lds + slice_m, *snap = hist + SIM_RANKS;
    const uint32_t trial = blockIdx.x / slices, slice = blockIdx.x % slices;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    for (uint32_t i = tid; i < slice_m; i += nthr) reg[i] = 0;
    for (uint32_t r = tid; r < SIM_RANKS; r += nthr) hist[r] = r == 0 ? slice_m : 0;     // (a workgroup may be one wave: 64 lanes, 65 counts)
    __syncthreads();
    const uint64_t m = 1ull << p, five_m = 5 * m;
    const uint64_t base = sim_mix(seed ^ ((uint64_t)(t0 + trial) * 0xD1342543DE82EF95ull));
    uint64_t n_prev = 0;
    for (uint32_t j = 0; j < n_points; ++j) {
        const uint64_t n_j = (uint64_t)j * five_m / (n_points - 1);
        for (uint64_t i = n_prev + tid; i < n_j; i += nthr) {
            const uint64_t h = sim_mix(base + i);
            const uint32_t bucket = (uint32_t)(h & (m - 1));
            if ((bucket >> slice_log) != slice) continue;
            const uint64_t w = h >> p;
            const uint32_t rank = (w ? (uint32_t)__builtin_clzll(w) : 64u) - (uint32_t)p + 1u;
            const uint32_t old = atomicMax(&reg[bucket & (slice_m - 1)], rank);
            if (old < rank) { atomicSub(&hist[old], 1u); atomicAdd(&hist[rank], 1u); }
        }
        n_prev = n_j;
        __syncthreads();                                                 // the registers hold exactly the elements i < n_j
        if (slices == 1) {
            // a snapshot, so that the one lane that sums it does not hold the others back: they go on inserting, and snap is
            // written again only after the next barrier above, which that lane reaches after its sum
            for (uint32_t r = tid; r < SIM_RANKS; r += nthr) snap[r] = hist[r];
            __syncthreads();
            if (tid == 0) E[(uint64_t)(t0 + trial) * n_points + j] = sim_estimate(snap, alpha, (double)m);
        } else {
            for (uint32_t r = tid; r < SIM_RANKS; r += nthr) {
                const uint32_t c = hist[r];
                if (c) atomicAdd(&ghist[((uint64_t)trial * n_points + j) * SIM_RANKS + r], c);
            }
            __syncthreads();                                             // hist is read before the next inserts move it
        }
    }
}

// slice path: one lane per (trial of the launch, checkpoint)
__global__ __launch_bounds__(256) void hll_bias_sim_finish_kernel(int p, uint32_t n_points, uint32_t t0, uint32_t n_trials, double alpha,
                                                                  const uint32_t *ghist, double *E)
{
    const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= (uint64_t)n_trials * n_points) return;
    E[(uint64_t)t0 * n_points + at] = sim_estimate(ghist + at * SIM_RANKS, alpha, (double)(1ull << p));
}

// The mean of n non-negative finite doubles e[0], e[stride], ... as the ONE double nearest to the exact quotient (ties to even):
// every addend goes into a fixed-point accumulator that spans the whole double range (so the sum has no rounding and no order),
// the division by n is a long division, and the only rounding is the last step.  The mean of equal values is that value.
// false: an addend is negative, infinite or NaN.
bool sim_exact_mean(const double *e, size_t stride, uint32_t n, double *out)
{
    constexpr int LIMBS = 36, BIAS = 1190;                               // bit 0 = 2^-1190: 2^-1126 (the lowest mantissa bit of a double) / 2^64
    uint64_t acc[LIMBS] = {0}, q[LIMBS];
    for (uint32_t t = 0; t < n; ++t) {
        const double x = e[(size_t)t * stride];
        if (!(x >= 0.0) || std::isinf(x)) return false;
        if (x == 0.0) continue;
        int ex;
        const uint64_t mant = (uint64_t)std::ldexp(std::frexp(x, &ex), 53);    // x = mant * 2^(ex - 53), exactly
        const int pos = ex - 53 + BIAS;
        const unsigned __int128 v = (unsigned __int128)mant << (pos & 63);
        int l = pos >> 6;
        uint64_t add[2] = {(uint64_t)v, (uint64_t)(v >> 64)};
        unsigned carry = 0;
        for (int i = 0; i < 2 || carry; ++i, ++l) {
            const uint64_t a = i < 2 ? add[i] : 0, before = acc[l];
            acc[l] = before + a + carry;
            carry = (acc[l] < before || (carry && acc[l] == before)) ? 1u : 0u;
        }
    }
    uint64_t rem = 0;
    for (int i = LIMBS - 1; i >= 0; --i) {
        const unsigned __int128 cur = ((unsigned __int128)rem << 64) | acc[i];
        q[i] = (uint64_t)(cur / n);
        rem = (uint64_t)(cur % n);
    }
    int top = LIMBS - 1;
    while (top >= 0 && q[top] == 0) --top;
    if (top < 0) { *out = 0.0; return true; }
    const int hb = 64 * top + 63 - __builtin_clzll(q[top]);
    auto bit = [&](int i) { return i >= 0 && ((q[i >> 6] >> (i & 63)) & 1u); };
    uint64_t mant = 0;
    for (int i = hb; i > hb - 53; --i) mant = (mant << 1) | (bit(i) ? 1u : 0u);
    bool sticky = rem != 0;
    for (int i = hb - 54; i >= 0 && !sticky; --i) sticky = bit(i);
    if (bit(hb - 53) && (sticky || (mant & 1u))) ++mant;
    *out = std::ldexp((double)mant, hb - 52 - BIAS);
    return true;
}

}  // namespace

extern "C" {

uint32_t lash_hll_bias_default_points(int p)
{
    if (p < 4 || p > 18) return 0;
    const uint64_t all = 5 * (1ull << p) + 1;
    return (uint32_t)std::min<uint64_t>(200, all);
}

int lash_hll_bias_simulate(lash_ctx *ctx, int p, uint32_t n_points, uint32_t n_trials, uint64_t seed, uint64_t *out_n, double *out_raw,
                           double *out_bias)
{
    if (!ctx || !out_raw || !out_bias || p < 4 || p > 18) return LASH_EINVAL;
    const uint64_t m = 1ull << p, five_m = 5 * m;
    if (n_points == 0) n_points = lash_hll_bias_default_points(p);
    if (n_trials == 0) n_trials = 2048;
    if (n_points < 6 || n_points > five_m + 1 || n_trials > (1u << 20)) return LASH_EINVAL;
    (void)hipSetDevice(ctx->device);
    const uint32_t slice_log = (uint32_t)std::min(p, SIM_SLICE_LOG), slice_m = 1u << slice_log, slices = (uint32_t)(m >> slice_log);
    const size_t lds = ((size_t)slice_m + 2 * SIM_RANKS) * 4;
    // lanes: about two elements each per checkpoint interval (between two barriers), one wave at least
    uint32_t threads = 64;
    while (threads < 1024 && (uint64_t)threads * 2 < five_m / (n_points - 1)) threads *= 2;
    const double alpha = pairmath::hll_alpha(p);
    const uint64_t cells = (uint64_t)n_trials * n_points;
    // scratch of this call alone (a table is made once per run): E[T][N], and on the slice path the launch's histograms
    struct Scratch { void *p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } } e_buf, h_buf;
    HIPCHK(ctx, hipMalloc(&e_buf.p, cells * 8));
    double *d_E = static_cast<double *>(e_buf.p);
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(hll_bias_sim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (slices == 1) {
        hipLaunchKernelGGL(hll_bias_sim_kernel, dim3(n_trials), dim3(threads), lds, ctx->stream, p, n_points, 0u, slice_log, seed, alpha, d_E,
                           static_cast<uint32_t *>(nullptr));
        HIPCHK(ctx, hipGetLastError());
    } else {
        const size_t per_trial = (size_t)n_points * SIM_RANKS * 4;
        const uint32_t step = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_trials, SIM_HIST_BYTES / per_trial));
        HIPCHK(ctx, hipMalloc(&h_buf.p, step * per_trial));
        uint32_t *d_hist = static_cast<uint32_t *>(h_buf.p);
        for (uint32_t t0 = 0; t0 < n_trials; t0 += step) {
            const uint32_t nt = std::min(step, n_trials - t0);
            HIPCHK(ctx, hipMemsetAsync(d_hist, 0, nt * per_trial, ctx->stream));
            hipLaunchKernelGGL(hll_bias_sim_kernel, dim3(nt * slices), dim3(threads), lds, ctx->stream, p, n_points, t0, slice_log, seed, alpha,
                               static_cast<double *>(nullptr), d_hist);
            HIPCHK(ctx, hipGetLastError());
            const uint64_t lanes = (uint64_t)nt * n_points;
            hipLaunchKernelGGL(hll_bias_sim_finish_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, p, n_points, t0, nt,
                               alpha, d_hist, d_E);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    std::vector<double> E(cells);
    HIPCHK(ctx, hipMemcpyAsync(E.data(), d_E, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t j = 0; j < n_points; ++j) {
        const uint64_t n_j = (uint64_t)j * five_m / (n_points - 1);
        if (!sim_exact_mean(E.data() + j, n_points, n_trials, &out_raw[j])) { ctx->err = "hll_bias_sim: a raw estimate is not finite"; return LASH_EHIP; }
        out_bias[j] = out_raw[j] - (double)n_j;
        if (out_n) out_n[j] = n_j;
    }
    return LASH_OK;
}

}  // extern "C"
