// dist_pcoa.hip — `lash dist --pcoa K`: principal coordinates (classical MDS) of the N x N matrix of printed distances, solved on the GPU
// (include/lash_gfx950.h: lash_tree_build_pcoa).  It works on the lash_tree matrix that dist_tree.hip creates and fills.
//
// The rule.  A = -1/2 D o D; B[i][j] = A[i][j] - (r[i] + r[j]) + g with r the row means of A and g the mean of r (Gower
// centring; r[i] + r[j] is one rounded sum, so B is symmetric bit for bit like D).  The axes are the k' = min(k, n - 1) ALGEBRAICALLY
// largest eigenpairs (theta_a, v_a) of B, theta descending, |v_a| = 1, the component of largest size positive (ties: the lowest row);
// coordinate [i][a] = v_a[i] * sqrt(max(theta_a, 0)).  Sketch distances are not Euclidean: B has negative eigenvalues and one of them
// may exceed theta_k in size, so a plain subspace iteration on B would converge to the wrong vectors.
//
// The solver: subspace iteration on B + sigma I with m = min(n, max(2k, k + 8)) vectors and a Rayleigh-Ritz step per iteration.
//   Y = B Q                      the hot kernel, below
//   H = Q^T Y                    m x m, a fixed tree over rows; goes to the host, which solves it by cyclic Jacobi: H = W Theta W^T
//   V = Q W, U = Y W             the Ritz vectors and B times them; E = U - V Theta, whose column norms are the residuals of B itself
//   stop when |E_a| <= tol * max(theta_1, 0) for every a <= k'
//   sigma = |B|_F / 1000 + 1.1 * sqrt(|B|_F^2 - sum of all m theta_a^2)       (the first three iterations: the first term alone)
//   Q = orth(U + sigma V)        Gram matrix, Cholesky, triangular solve, twice (CholeskyQR2)
// The Ritz values are sorted algebraically, so a large negative eigenvalue whose vector the subspace holds goes to the bottom of the list
// and costs one of the m - k' spare vectors, not a large shift; the three open iterations let the eigenvalues of largest size, of either
// sign, in.  What is under the root is the squared Frobenius norm of B outside the subspace, |B|_F^2 - |Q^T B Q|_F^2: once the subspace
// is invariant it bounds the square of every eigenvalue the subspace does not hold, so each of those has lambda + sigma > 0 and they
// rank algebraically against the wanted ones.  That alone does not make the answer algebraic: when more negative eigenvalues exceed a
// wanted one in size than there are spare vectors, the subspace holds them, the root is small, and the wanted one stays out.  So a
// converged answer is accepted only if theta_k' + sigma >= 0 for the shift of the last filter step: the subspace holds the m eigenvalues
// of largest |lambda + sigma| and theta_k' is one of them, so then every eigenvalue outside has mu + sigma <= theta_k' + sigma.  If
// not, the solve starts again from the start vectors with the textbook shift throughout, 1.1 sqrt(|B|_F^2 - sum of the POSITIVE
// theta_a^2) + |B|_F / 1000 >= -lambda_min(B) (Ritz values interlace: theta_a <= lambda_a), under which B + sigma I is positive
// definite and the order by size is the algebraic one.  That pass is the slow one: a shift of the size
// of a negative eigenvalue alone (the |B|_F bound) would converge at the rate sigma / (theta_k + sigma), which is hopeless when theta_k
// is small beside it.  Where sigma would come within 0.8 .. 1.25 of the size of a negative Ritz value it is raised to 1.25 times that
// size, so that no column of U + sigma V cancels; with the |B|_F / 1000 floor the columns stay within about 1e4 of each other in norm,
// which CholeskyQR2 takes.  sigma may change between iterations: the subspace is filtered by one factor B + sigma_t I at a time.
//
// The product.  B is symmetric bit for bit, so Y[i][c] = sum over k of B[k][i] Q[k][c]: a wave owns 16 output rows i and walks k with
// v_mfma_f64_16x16x4_f64, whose A operand (lane l: row l & 15, k l >> 4) is then one 8-byte load per lane in which a quarter wave reads
// one 128-byte line of row k: B goes from memory into the MFMA without a transpose.  The 8 waves of a workgroup own 128 adjacent rows
// (1 KiB of every row k) and share the Q rows of the walk, staged through LDS 64 rows at a time.  The walk is cut into segments (grid y),
// so that small n still fills the chip; the segments' partial sums are added in segment order by a second kernel.  B is read once.
// Every reduction here is a fixed tree: no atomics, and two builds of the same matrix bits give the same bits.
#include "dist_tree.h"

#pragma clang fp contract(off)

namespace lash {

typedef double pcoa_v4f64 __attribute__((ext_vector_type(4)));

__device__ inline uint64_t pcoa_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The workgroup's sum in every thread: a butterfly inside each wave, then the waves' sums in wave order.  s holds WAVES doubles.
template <uint32_t WAVES>
__device__ inline double pcoa_block_sum(double v, double *s)
{
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (uint32_t w = 0; w < WAVES; ++w) t = t + s[w];
    __syncthreads();
    return t;
}

// ---- centring ---------------------------------------------------------------------------------------------------------------------
// D -> A = -1/2 D o D in place, rmean[i] = mean of row i of A; one workgroup per row, columns strided in a fixed order
__global__ void __launch_bounds__(256) pcoa_square_kernel(double *__restrict__ D, uint32_t n, double *__restrict__ rmean)
{
    __shared__ double s[4];
    double *row = D + (size_t)blockIdx.x * n;
    double sum = 0.0;
    for (uint32_t c = threadIdx.x; c < n; c += 256u) {
        const double d = row[c];
        const double a = -0.5 * (d * d);
        row[c] = a;
        sum = sum + a;
    }
    sum = pcoa_block_sum<4>(sum, s);
    if (threadIdx.x == 0) rmean[blockIdx.x] = sum / (double)n;
}

// *out = (sum of x[0..n)) * scale; one workgroup
__global__ void __launch_bounds__(256) pcoa_sum_kernel(const double *__restrict__ x, uint32_t n, double scale, double *__restrict__ out)
{
    __shared__ double s[4];
    double sum = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) sum = sum + x[i];
    sum = pcoa_block_sum<4>(sum, s);
    if (threadIdx.x == 0) *out = sum * scale;
}

// A -> B in place; rowsq[i] = sum of squares of row i of B, diag[i] = B[i][i]
__global__ void __launch_bounds__(256) pcoa_centre_kernel(double *__restrict__ A, uint32_t n, const double *__restrict__ rmean,
                                                          const double *__restrict__ g, double *__restrict__ rowsq, double *__restrict__ diag)
{
    __shared__ double s[4];
    const uint32_t i = blockIdx.x;
    double *row = A + (size_t)i * n;
    const double ri = rmean[i], gm = *g;
    double sq = 0.0;
    for (uint32_t c = threadIdx.x; c < n; c += 256u) {
        const double both = ri + rmean[c];
        const double b = (row[c] - both) + gm;
        row[c] = b;
        sq = sq + b * b;
        if (c == i) diag[i] = b;
    }
    sq = pcoa_block_sum<4>(sq, s);
    if (threadIdx.x == 0) rowsq[i] = sq;
}

// ---- panels: row-major [n][LD], LD = 16 or 32, columns >= m zero ------------------------------------------------------------------
// start vectors: uniform in (-1, 1) from splitmix64 of (seed, row, column)
__global__ void __launch_bounds__(256) pcoa_init_kernel(double *__restrict__ Q, uint32_t n, uint32_t ld, uint32_t m)
{
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)n * ld) return;
    const uint32_t r = (uint32_t)(at / ld), c = (uint32_t)(at % ld);
    double v = 0.0;
    if (c < m) {
        const uint64_t z = pcoa_splitmix64(0x70636F61ull + ((uint64_t)r << 6) + c);
        v = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    Q[at] = v;
}

// Y = B Q, or the partial sums of it: see the head of the file.  grid (ceil(n / 128), segments); part is [segments][n][16 * MT].
constexpr uint32_t PCOA_WAVES = 8;
constexpr uint32_t PCOA_ROWS = 16 * PCOA_WAVES;   // output rows of a workgroup
constexpr uint32_t PCOA_KC = 64;                  // rows of Q per LDS stage

template <int MT>
__global__ void __launch_bounds__(64 * PCOA_WAVES) pcoa_product_kernel(const double *__restrict__ B, const double *__restrict__ Q,
                                                                      double *__restrict__ part, uint32_t n, uint32_t seg_len)
{
    constexpr uint32_t LD = 16u * MT;
    constexpr uint32_t STEPS = PCOA_KC / 4;
    __shared__ double Qs[PCOA_KC][LD];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15u, kq = lane >> 4;
    const uint32_t i = blockIdx.x * PCOA_ROWS + wave * 16u + col;                               // the output row this lane loads B for
    const bool i_ok = i < n;
    const uint32_t k_begin = blockIdx.y * seg_len;
    const uint32_t k_end = n - k_begin < seg_len ? n : k_begin + seg_len;                        // (k_begin < n: the grid has no empty segment)
    pcoa_v4f64 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = pcoa_v4f64{0.0, 0.0, 0.0, 0.0};
    double a_cur[STEPS], a_next[STEPS];
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) a_next[s] = 0.0;
    auto fetch = [&](uint32_t kc, double *a) {
#pragma unroll
        for (uint32_t s = 0; s < STEPS; ++s) {
            const uint32_t k = kc + 4u * s + kq;
            a[s] = (i_ok && k < k_end) ? B[(size_t)k * n + i] : 0.0;                            // (k < n and i < n: never out of bounds)
        }
    };
    fetch(k_begin, a_cur);
    for (uint32_t kc = k_begin; kc < k_end; kc += PCOA_KC) {
        __syncthreads();                                                                        // the stage before has been read
        for (uint32_t e = threadIdx.x; e < PCOA_KC * LD; e += 64u * PCOA_WAVES) {
            const uint32_t k = kc + e / LD;
            Qs[e / LD][e % LD] = k < k_end ? Q[(size_t)k * LD + e % LD] : 0.0;
        }
        __syncthreads();
        if (kc + PCOA_KC < k_end) fetch(kc + PCOA_KC, a_next);
#pragma unroll
        for (uint32_t s = 0; s < STEPS; ++s) {
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[s], Qs[4u * s + kq][16u * t + col], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (uint32_t s = 0; s < STEPS; ++s) a_cur[s] = a_next[s];
    }
    // D register j of lane l = [row (l >> 4) + 4 j][column l & 15]
    double *out = part + (size_t)blockIdx.y * n * LD;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = blockIdx.x * PCOA_ROWS + wave * 16u + kq + 4u * j;
            if (r < n) out[(size_t)r * LD + 16u * t + col] = acc[t][j];
        }
}

// Y[e] = part[0][e] + part[1][e] + ... in that order
__global__ void __launch_bounds__(256) pcoa_partsum_kernel(const double *__restrict__ part, uint32_t segments, size_t count, double *__restrict__ Y)
{
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= count) return;
    double sum = part[e];
    for (uint32_t s = 1; s < segments; ++s) sum = sum + part[(size_t)s * count + e];
    Y[e] = sum;
}

// partial[p][a][b] = sum over the rows r of chunk p, ascending, of X[r][a] * Z[r][b]; 32 x 32 whatever LD (the rest zero)
constexpr uint32_t PCOA_GRAM_ROWS = 64;
template <uint32_t LD>
__global__ void __launch_bounds__(256) pcoa_gram_kernel(const double *__restrict__ X, const double *__restrict__ Z, uint32_t n, double *__restrict__ partial)
{
    __shared__ double xs[PCOA_GRAM_ROWS][32], zs[PCOA_GRAM_ROWS][32];
    const uint32_t r0 = blockIdx.x * PCOA_GRAM_ROWS;
    for (uint32_t e = threadIdx.x; e < PCOA_GRAM_ROWS * 32u; e += 256u) {
        const uint32_t r = r0 + e / 32u, c = e % 32u;
        const bool ok = r < n && c < LD;
        xs[e / 32u][c] = ok ? X[(size_t)r * LD + c] : 0.0;
        zs[e / 32u][c] = ok ? Z[(size_t)r * LD + c] : 0.0;
    }
    __syncthreads();
    const uint32_t a = threadIdx.x >> 3, b0 = (threadIdx.x & 7u) * 4u;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t r = 0; r < PCOA_GRAM_ROWS; ++r) {
        const double x = xs[r][a];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + x * zs[r][b0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) partial[(size_t)blockIdx.x * 1024u + a * 32u + b0 + j] = acc[j];
}

// G[e] = partial[0][e] + partial[1][e] + ..., e < 1024
__global__ void __launch_bounds__(256) pcoa_gram_reduce_kernel(const double *__restrict__ partial, uint32_t chunks, double *__restrict__ G)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    double sum = 0.0;
    for (uint32_t p = 0; p < chunks; ++p) sum = sum + partial[(size_t)p * 1024u + e];
    G[e] = sum;
}

// G = R^T R, R upper triangular, for the leading m x m of G[32][32]; one wave, lane j owns column j.  A pivot that is not positive
// raises *flag (the build then fails) and is replaced by 1 so that nothing after it divides by zero.
__global__ void __launch_bounds__(64) pcoa_chol_kernel(const double *__restrict__ G, uint32_t m, double *__restrict__ R, uint32_t *__restrict__ flag)
{
    __shared__ double g[32][33];
    const uint32_t j = threadIdx.x;
    if (j < 32u)
        for (uint32_t i = 0; i < 32u; ++i) g[i][j] = G[i * 32u + j];
    __syncthreads();
    for (uint32_t k = 0; k < m; ++k) {
        double d = g[k][k];
        if (!(d > 0.0) || !(d < HUGE_VAL)) { if (j == 0) *flag = 1u; d = 1.0; }
        const double p = sqrt(d);
        __syncthreads();
        if (j >= k && j < m) g[k][j] = g[k][j] / p;
        __syncthreads();
        for (uint32_t i = k + 1; i < m; ++i)
            if (j >= i && j < m) g[i][j] = g[i][j] - g[k][i] * g[k][j];
        __syncthreads();
    }
    if (j < 32u)
        for (uint32_t i = 0; i < 32u; ++i) R[i * 32u + j] = (i <= j && j < m) ? g[i][j] : 0.0;
}

// Z <- Z R^-1 (a row x solves x R = z by forward substitution); one thread per row
template <uint32_t LD>
__global__ void __launch_bounds__(256) pcoa_trsolve_kernel(double *__restrict__ Z, uint32_t n, uint32_t m, const double *__restrict__ R)
{
    __shared__ double rs[32][33];
    for (uint32_t e = threadIdx.x; e < 1024u; e += 256u) rs[e / 32u][e % 32u] = R[e];
    __syncthreads();
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    double x[LD];
#pragma unroll
    for (uint32_t c = 0; c < LD; ++c) x[c] = Z[(size_t)r * LD + c];
#pragma unroll
    for (uint32_t c = 0; c < LD; ++c) {
        if (c < m) {
            double s = x[c];
#pragma unroll
            for (uint32_t i = 0; i < c; ++i) s = s - x[i] * rs[i][c];
            x[c] = s / rs[c][c];
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < LD; ++c) Z[(size_t)r * LD + c] = x[c];
}

// V = Q W, U = Y W, Z = U + sigma V, E = U - V diag(theta); W is [32][32] with zeros beyond m; one thread per row
template <uint32_t LD>
__global__ void __launch_bounds__(256) pcoa_rotate_kernel(const double *__restrict__ Q, const double *__restrict__ Y, const double *__restrict__ W,
                                                          const double *__restrict__ theta, double sigma, double *__restrict__ V,
                                                          double *__restrict__ Z, double *__restrict__ E, uint32_t n)
{
    __shared__ double ws[32][32];
    __shared__ double th[32];
    for (uint32_t e = threadIdx.x; e < 1024u; e += 256u) ws[e / 32u][e % 32u] = W[e];
    if (threadIdx.x < 32u) th[threadIdx.x] = theta[threadIdx.x];
    __syncthreads();
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    double q[LD], y[LD];
#pragma unroll
    for (uint32_t c = 0; c < LD; ++c) { q[c] = Q[(size_t)r * LD + c]; y[c] = Y[(size_t)r * LD + c]; }
    for (uint32_t a = 0; a < LD; ++a) {
        double v = 0.0, u = 0.0;
#pragma unroll
        for (uint32_t c = 0; c < LD; ++c) { const double w = ws[c][a]; v = v + q[c] * w; u = u + y[c] * w; }
        V[(size_t)r * LD + a] = v;
        Z[(size_t)r * LD + a] = u + sigma * v;
        E[(size_t)r * LD + a] = u - th[a] * v;
    }
}

uint32_t pcoa_product_segments(uint32_t n, uint32_t *seg_len)
{
    const uint32_t row_blocks = (n + PCOA_ROWS - 1) / PCOA_ROWS, stages = (n + PCOA_KC - 1) / PCOA_KC;
    const uint32_t want = std::max(1u, std::min((512u + row_blocks - 1) / row_blocks, stages));
    const uint32_t len = ((n + want - 1) / want + PCOA_KC - 1) / PCOA_KC * PCOA_KC;
    *seg_len = len;
    return (n + len - 1) / len;
}

hipError_t launch_pcoa_centre(double *d_D, uint32_t n, double *d_rmean, double *d_rowsq, double *d_diag, double *d_scal, hipStream_t st)
{
    hipLaunchKernelGGL(pcoa_square_kernel, dim3(n), dim3(256), 0, st, d_D, n, d_rmean);
    hipLaunchKernelGGL(pcoa_sum_kernel, dim3(1), dim3(256), 0, st, d_rmean, n, 1.0 / (double)n, d_scal);
    hipLaunchKernelGGL(pcoa_centre_kernel, dim3(n), dim3(256), 0, st, d_D, n, d_rmean, d_scal, d_rowsq, d_diag);
    hipLaunchKernelGGL(pcoa_sum_kernel, dim3(1), dim3(256), 0, st, d_rowsq, n, 1.0, d_scal + 1);
    hipLaunchKernelGGL(pcoa_sum_kernel, dim3(1), dim3(256), 0, st, d_diag, n, 1.0, d_scal + 2);
    return hipGetLastError();
}

hipError_t launch_pcoa_init(double *d_Q, uint32_t n, uint32_t ld, uint32_t m, hipStream_t st)
{
    const size_t count = (size_t)n * ld;
    hipLaunchKernelGGL(pcoa_init_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, st, d_Q, n, ld, m);
    return hipGetLastError();
}

hipError_t launch_pcoa_product(const double *d_B, uint32_t n, const double *d_Q, uint32_t ld, double *d_Y, double *d_part, hipStream_t st)
{
    uint32_t seg_len = 0;
    const uint32_t segments = pcoa_product_segments(n, &seg_len);
    const dim3 grid((n + PCOA_ROWS - 1) / PCOA_ROWS, segments);
    double *dst = segments == 1 ? d_Y : d_part;
    if (ld == 16) hipLaunchKernelGGL(pcoa_product_kernel<1>, grid, dim3(64 * PCOA_WAVES), 0, st, d_B, d_Q, dst, n, seg_len);
    else hipLaunchKernelGGL(pcoa_product_kernel<2>, grid, dim3(64 * PCOA_WAVES), 0, st, d_B, d_Q, dst, n, seg_len);
    if (segments > 1) {
        const size_t count = (size_t)n * ld;
        hipLaunchKernelGGL(pcoa_partsum_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, st, d_part, segments, count, d_Y);
    }
    return hipGetLastError();
}

hipError_t launch_pcoa_gram(const double *d_X, const double *d_Z, uint32_t n, uint32_t ld, double *d_partial, double *d_G, hipStream_t st)
{
    const uint32_t chunks = (n + PCOA_GRAM_ROWS - 1) / PCOA_GRAM_ROWS;
    if (ld == 16) hipLaunchKernelGGL(pcoa_gram_kernel<16>, dim3(chunks), dim3(256), 0, st, d_X, d_Z, n, d_partial);
    else hipLaunchKernelGGL(pcoa_gram_kernel<32>, dim3(chunks), dim3(256), 0, st, d_X, d_Z, n, d_partial);
    hipLaunchKernelGGL(pcoa_gram_reduce_kernel, dim3(4), dim3(256), 0, st, d_partial, chunks, d_G);
    return hipGetLastError();
}

hipError_t launch_pcoa_orthonormalise(double *d_Z, uint32_t n, uint32_t ld, uint32_t m, double *d_partial, double *d_G, double *d_R, uint32_t *d_flag,
                                      hipStream_t st)
{
    for (int pass = 0; pass < 2; ++pass) {
        const hipError_t e = launch_pcoa_gram(d_Z, d_Z, n, ld, d_partial, d_G, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pcoa_chol_kernel, dim3(1), dim3(64), 0, st, d_G, m, d_R, d_flag);
        if (ld == 16) hipLaunchKernelGGL(pcoa_trsolve_kernel<16>, dim3((n + 255) / 256), dim3(256), 0, st, d_Z, n, m, d_R);
        else hipLaunchKernelGGL(pcoa_trsolve_kernel<32>, dim3((n + 255) / 256), dim3(256), 0, st, d_Z, n, m, d_R);
    }
    return hipGetLastError();
}

hipError_t launch_pcoa_rotate(const double *d_Q, const double *d_Y, const double *d_W, const double *d_theta, double sigma, double *d_V, double *d_Z,
                              double *d_E, uint32_t n, uint32_t ld, hipStream_t st)
{
    if (ld == 16) hipLaunchKernelGGL(pcoa_rotate_kernel<16>, dim3((n + 255) / 256), dim3(256), 0, st, d_Q, d_Y, d_W, d_theta, sigma, d_V, d_Z, d_E, n);
    else hipLaunchKernelGGL(pcoa_rotate_kernel<32>, dim3((n + 255) / 256), dim3(256), 0, st, d_Q, d_Y, d_W, d_theta, sigma, d_V, d_Z, d_E, n);
    return hipGetLastError();
}

}  // namespace lash

namespace {

constexpr uint32_t PCOA_OPEN_ITERATIONS = 3;      // iterations that take the floor of the shift alone

// H (m x m, symmetric, row-major ld 32) = W diag(theta) W^T by cyclic Jacobi; theta descending, W's columns the vectors
void jacobi_eigen(const double *H, uint32_t m, double *theta, double *W)
{
    std::vector<double> a((size_t)m * m), v((size_t)m * m, 0.0);
    for (uint32_t i = 0; i < m; ++i) {
        for (uint32_t j = 0; j < m; ++j) a[(size_t)i * m + j] = 0.5 * (H[i * 32u + j] + H[j * 32u + i]);
        v[(size_t)i * m + i] = 1.0;
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < m; ++j) (i == j ? diag : off) += a[(size_t)i * m + j] * a[(size_t)i * m + j];
        if (off <= 1e-32 * diag || off == 0.0) break;                                           // (sums of squares: 1e-16 in norm)
        for (uint32_t p = 0; p + 1 < m; ++p)
            for (uint32_t q = p + 1; q < m; ++q) {
                const double apq = a[(size_t)p * m + q];
                if (apq == 0.0) continue;
                const double app = a[(size_t)p * m + p], aqq = a[(size_t)q * m + q];
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (uint32_t k = 0; k < m; ++k) {
                    const double akp = a[(size_t)k * m + p], akq = a[(size_t)k * m + q];
                    a[(size_t)k * m + p] = c * akp - s * akq;
                    a[(size_t)k * m + q] = s * akp + c * akq;
                }
                for (uint32_t k = 0; k < m; ++k) {
                    const double apk = a[(size_t)p * m + k], aqk = a[(size_t)q * m + k];
                    a[(size_t)p * m + k] = c * apk - s * aqk;
                    a[(size_t)q * m + k] = s * apk + c * aqk;
                }
                for (uint32_t k = 0; k < m; ++k) {
                    const double vkp = v[(size_t)k * m + p], vkq = v[(size_t)k * m + q];
                    v[(size_t)k * m + p] = c * vkp - s * vkq;
                    v[(size_t)k * m + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<uint32_t> order(m);
    for (uint32_t i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return a[(size_t)x * m + x] > a[(size_t)y * m + y]; });
    for (uint32_t e = 0; e < 1024u; ++e) W[e] = 0.0;
    for (uint32_t c = 0; c < 32u; ++c) theta[c] = 0.0;
    for (uint32_t c = 0; c < m; ++c) {
        theta[c] = a[(size_t)order[c] * m + order[c]];
        for (uint32_t k = 0; k < m; ++k) W[k * 32u + c] = v[(size_t)k * m + order[c]];
    }
}

// The shift of the next iterate (the head of the file): theta holds the m Ritz values, descending.  safe: the textbook shift, an upper
// bound of -lambda_min(B): Ritz values interlace (theta_a <= lambda_a), so |B|_F^2 less the squares of the positive ones bounds the
// square of every eigenvalue they do not account for, every negative one among them.
double pcoa_shift(const double *theta, uint32_t m, double frob2, uint32_t iter, bool safe)
{
    double held = 0.0;
    for (uint32_t a = 0; a < m; ++a)
        if (!safe || theta[a] > 0.0) held += theta[a] * theta[a];
    double sigma = 1e-3 * std::sqrt(frob2);
    if (safe || iter > PCOA_OPEN_ITERATIONS) sigma += 1.1 * std::sqrt(std::max(0.0, frob2 - held));
    if (safe) return sigma;
    for (uint32_t a = m; a-- > 0;) {                                                            // negative Ritz values, the smallest in size first
        if (!(theta[a] < 0.0)) continue;
        const double x = -theta[a];
        if (0.8 * x < sigma && sigma < 1.25 * x) sigma = 1.25 * x;
    }
    return sigma;
}

}  // namespace

extern "C" int lash_tree_build_pcoa(lash_ctx *ctx, lash_tree *t, uint32_t k, double tol, uint32_t max_iter, double *out_eigenvalues, double *out_coords,
                                    lash_pcoa_stats *stats)
{
    using namespace lash;
    if (stats) *stats = lash_pcoa_stats{};
    if (!ctx || !t || t->device != ctx->device) return LASH_EINVAL;
    const uint32_t n = t->n;
    char buf[200];
    auto refuse = [&]() { ctx->err = buf; return LASH_EINVAL; };
    if (k < 1 || k > 16) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: k must be 1 to 16, not %u", k); return refuse(); }
    if (t->built) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: the tree has been built (the build consumes the matrix)"); return refuse(); }
    if (n < 2) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: principal coordinates need at least 2 rows, not %u", n); return refuse(); }
    if (!out_eigenvalues || !out_coords) return LASH_EINVAL;
    for (uint32_t r = 0; r < n; ++r)
        if (!t->row_set[r]) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: row %u has not been set", r); return refuse(); }
    if (t->has_nan) {
        snprintf(buf, sizeof buf, "lash_tree_build_pcoa: the distance of row %u and col %u is NaN: the coordinates are undefined", t->nan_row, t->nan_col);
        return refuse();
    }
    if (t->has_inf) {
        snprintf(buf, sizeof buf, "lash_tree_build_pcoa: the distance of row %u and col %u is not finite: centring would subtract infinities",
                 t->inf_row, t->inf_col);
        return refuse();
    }
    if (!(tol > 0.0)) tol = 1e-10;
    if (max_iter == 0) max_iter = 2000;
    (void)hipSetDevice(t->device);

    const uint32_t kk = std::min(k, n - 1);
    const uint32_t m = std::min(n, std::max(2 * k, k + 8));
    const uint32_t ld = m <= 16 ? 16u : 32u;
    uint32_t seg_len = 0;
    const uint32_t segments = pcoa_product_segments(n, &seg_len);
    const uint32_t chunks = (n + PCOA_GRAM_ROWS - 1) / PCOA_GRAM_ROWS;
    const size_t panel = (size_t)n * ld;

    size_t at = 0;
    auto take = [&](size_t doubles) { const size_t o = at; at += (doubles + 31) & ~size_t(31); return o; };
    const size_t o_Q = take(panel), o_Y = take(panel), o_V = take(panel), o_Z = take(panel), o_E = take(panel),
                 o_part = take(segments > 1 ? panel * segments : 0), o_partial = take((size_t)chunks * 1024), o_G = take(1024), o_R = take(1024),
                 o_W = take(1024), o_theta = take(32), o_rmean = take(n), o_rowsq = take(n), o_diag = take(n), o_scal = take(4), o_flag = take(1);
    double *base = nullptr;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&base), at * sizeof(double)));
    struct Guard { double *p; ~Guard() { (void)hipFree(p); } } guard{base};
    t->built = true;                                                                            // from here on the matrix is consumed
    if (stats) stats->bytes = (uint64_t)n * n * sizeof(double);
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(base, 0, at * sizeof(double), st));
    double *Q = base + o_Q, *Y = base + o_Y, *V = base + o_V, *Z = base + o_Z, *E = base + o_E, *part = base + o_part, *partial = base + o_partial,
           *G = base + o_G, *R = base + o_R, *W = base + o_W, *theta = base + o_theta, *scal = base + o_scal;
    uint32_t *flag = reinterpret_cast<uint32_t *>(base + o_flag);

    // centring, in place; g, |B|_F^2 and the trace come back once
    HIPCHK(ctx, launch_pcoa_centre(t->d_D, n, base + o_rmean, base + o_rowsq, base + o_diag, scal, st));
    HIPCHK(ctx, launch_pcoa_init(Q, n, ld, m, st));
    HIPCHK(ctx, launch_pcoa_orthonormalise(Q, n, ld, m, partial, G, R, flag, st));
    double h_scal[3] = {0.0, 0.0, 0.0};
    HIPCHK(ctx, hipMemcpyAsync(h_scal, scal, sizeof h_scal, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const double frob2 = h_scal[1], trace = h_scal[2];
    if (!std::isfinite(frob2)) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: the squared distances overflow a double"); return refuse(); }
    if (stats) stats->trace = trace;

    std::vector<double> h_H(1024), h_W(1024), h_theta(32), h_E(1024);
    uint32_t h_flag = 0, iter = 0;
    double worst = 0.0, sigma = 0.0;
    bool done = false;
    // Pass 0 runs the fast shift.  Its answer is accepted only if theta_k' + sigma >= 0 for the shift the last filter step used (or the
    // subspace is the whole space): the subspace holds the m eigenvalues of largest |lambda + sigma|, theta_k' is held, so then every
    // eigenvalue outside has |mu + sigma| <= theta_k' + sigma, that is mu <= theta_k'.  Otherwise held negative eigenvalues may have kept
    // a wanted one out, and pass 1 starts again from the start vectors with the textbook shift, under which B + sigma I is positive
    // definite and the order by size is the algebraic one.  max_iter counts the iterations of both passes together.
    for (int pass = 0; pass < 2 && !done && iter < max_iter; ++pass) {
        const bool safe = pass == 1;
        double used = 0.0;                                                                      // the shift behind the current Q
        bool rejected = false;
        if (safe) {
            HIPCHK(ctx, launch_pcoa_init(Q, n, ld, m, st));
            HIPCHK(ctx, launch_pcoa_orthonormalise(Q, n, ld, m, partial, G, R, flag, st));
        }
        while (iter < max_iter) {
            ++iter;
            HIPCHK(ctx, launch_pcoa_product(t->d_D, n, Q, ld, Y, part, st));
            if (stats) ++stats->products;
            HIPCHK(ctx, launch_pcoa_gram(Q, Y, n, ld, partial, G, st));
            HIPCHK(ctx, hipMemcpyAsync(h_H.data(), G, 1024 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(&h_flag, flag, sizeof h_flag, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
            if (h_flag) { snprintf(buf, sizeof buf, "lash_tree_build_pcoa: the iterate lost rank at iteration %u (internal error)", iter); return refuse(); }
            jacobi_eigen(h_H.data(), m, h_theta.data(), h_W.data());
            sigma = pcoa_shift(h_theta.data(), m, frob2, iter, safe);
            HIPCHK(ctx, hipMemcpyAsync(W, h_W.data(), 1024 * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(theta, h_theta.data(), 32 * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, launch_pcoa_rotate(Q, Y, W, theta, sigma, V, Z, E, n, ld, st));
            HIPCHK(ctx, launch_pcoa_gram(E, E, n, ld, partial, G, st));
            HIPCHK(ctx, hipMemcpyAsync(h_E.data(), G, 1024 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
            const double scale = std::max(h_theta[0], 0.0);
            worst = 0.0;
            bool small = true;
            for (uint32_t a = 0; a < kk; ++a) {
                const double r = std::sqrt(std::max(h_E[a * 32u + a], 0.0));
                if (!(r <= tol * scale)) small = false;
                const double rel = r == 0.0 ? 0.0 : scale > 0.0 ? r / scale : HUGE_VAL;
                if (!(rel <= worst)) worst = rel;
            }
            if (small) {
                if (safe || m == n || h_theta[kk - 1] + used >= 0.0) done = true;
                else rejected = true;
                break;
            }
            if (iter == max_iter) break;
            HIPCHK(ctx, launch_pcoa_orthonormalise(Z, n, ld, m, partial, G, R, flag, st));
            std::swap(Q, Z);
            used = sigma;
        }
        if (!rejected) break;
    }
    if (stats) { stats->iterations = iter; stats->worst_residual = worst; stats->shift = sigma; }
    if (!done) {
        snprintf(buf, sizeof buf, "lash_tree_build_pcoa: no convergence after %u iterations: the worst relative residual is %.3g, above tol %.3g",
                 iter, worst, tol);
        return refuse();
    }
    std::vector<double> h_V(panel);
    HIPCHK(ctx, hipMemcpyAsync(h_V.data(), V, panel * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (uint32_t a = 0; a < k; ++a) out_eigenvalues[a] = a < kk ? h_theta[a] : 0.0;
    for (size_t e = 0; e < (size_t)n * k; ++e) out_coords[e] = 0.0;
    for (uint32_t a = 0; a < kk; ++a) {
        if (!(h_theta[a] > 0.0)) continue;
        double big = 0.0, sign = 1.0, norm2 = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double v = h_V[(size_t)i * ld + a];
            norm2 += v * v;
            if (std::fabs(v) > big) { big = std::fabs(v); sign = v < 0.0 ? -1.0 : 1.0; }
        }
        const double s = sign * std::sqrt(h_theta[a]) / std::sqrt(norm2);
        for (uint32_t i = 0; i < n; ++i) out_coords[(size_t)i * k + a] = h_V[(size_t)i * ld + a] * s + 0.0;
    }
    return LASH_OK;
}
