// init.h -- the dense pieces of the truncated SVD behind the 'svd2' initialiser (reference R/bayesian.R:150-159, irlba;
// SURVEY.md section 8f-3; included once, by svd.hip): the standard normal block of the range finder (philox.h), the Gram
// matrix of a tall [N][R] block, Cholesky factor / Jacobi eigen-decomposition of the k x k result, and the product of the
// tall block with a k x k matrix -- so that the subspace stays on the device between the sparse products (k_spmm) and
// nothing crosses PCIe inside the iteration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace vbnmf {

// standard normal block for the range finder of the truncated SVD: g[major][k], k < r
__global__ __launch_bounds__(256) void k_normal_init(double *__restrict__ g, int64_t nmaj, int r, int R, uint32_t k0, uint32_t k1)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nmaj * R) return;
    const int64_t M = i / R;
    const int k = (int)(i - M * R);
    double v = 0.0;
    if (k < r) {
        uint32_t q[4];
        const uint64_t el = (uint64_t)M * (uint64_t)r + (uint64_t)k;
        philox4x32((uint32_t)el, (uint32_t)(el >> 32), 7u, 0u, k0, k1, q);
        v = sqrt(-2.0 * log(u53(q[0], q[1]))) * cos(6.283185307179586476925 * u53(q[2], q[3]));
    }
    g[i] = v;
}

// ---------------------------------------------------------------- dense pieces of the truncated SVD
constexpr int kGramBlocks = 256;
// Block partials of G = t(A) A for a tall A[N][R]: gp[block][R*R].  Thread (i, j) of a 32 x 32 block owns the elements
// (i + 32 a, j + 32 b) of G, a, b < ceil(R / 32): one element up to R = 32, four at the padded ranks 40..64.
template <int R>
__global__ __launch_bounds__(1024) void k_gram(const double *__restrict__ A, int64_t N, double *__restrict__ gp)
{
    constexpr int T = (R + 31) / 32;
    __shared__ double tile[32][R];
    const int i = threadIdx.x / 32, j = threadIdx.x % 32;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t n0 = (int64_t)blockIdx.x * per, n1 = min(N, n0 + per);
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; a++)
#pragma unroll
        for (int b = 0; b < T; b++) acc[a][b] = 0.0;
    for (int64_t b0 = n0; b0 < n1; b0 += 32) {
        const int rows = (int)min((int64_t)32, n1 - b0);
        __syncthreads();
        for (int t = threadIdx.x; t < rows * R; t += 1024) tile[t / R][t % R] = A[(size_t)b0 * R + t];
        __syncthreads();
#pragma unroll
        for (int a = 0; a < T; a++)
#pragma unroll
            for (int b = 0; b < T; b++) {
                const int ii = i + 32 * a, jj = j + 32 * b;
                if (ii < R && jj < R)
                    for (int q = 0; q < rows; q++) acc[a][b] = fma(tile[q][ii], tile[q][jj], acc[a][b]);
            }
    }
#pragma unroll
    for (int a = 0; a < T; a++)
#pragma unroll
        for (int b = 0; b < T; b++) {
            const int ii = i + 32 * a, jj = j + 32 * b;
            if (ii < R && jj < R) gp[(size_t)blockIdx.x * R * R + ii * R + jj] = acc[a][b];
        }
}

// One block.  G = sum of the block partials (fixed order), then, by `mode`:
//   0: Cholesky G = t(U) U (upper), S = inverse of U (so that A S is orthonormal); diag(U) goes to `vals`
//   1: Jacobi eigen-decomposition G = V diag(lambda) t(V), eigenvalues DESCENDING in `vals`, S = V and, when S2 is
//      given, S2 = V diag(1 / sqrt(lambda)) (right singular vectors: rows of P V / sigma)
// k = columns in use (<= R); columns k..R-1 of S are 0.  status[0] is SET to 1 when G is not positive definite (mode 0).
// vals_host (optional): a pinned, device-visible copy of vals (+ vals_host[R] = seq, written last) for the host's
// convergence test -- no memcpy.
template <int R>
__global__ __launch_bounds__(1024) void k_small(const double *__restrict__ gp, int nb, int k, int mode, double *__restrict__ S,
                                                double *__restrict__ S2, double *__restrict__ vals, double *__restrict__ vals_host,
                                                double seq, int32_t *__restrict__ status)
{
    __shared__ double G[R][R + 1], V[R][R + 1];
    const int i = threadIdx.x / 32, j = threadIdx.x % 32;
    // thread (i, j) of the 32 x 32 block owns the elements (i + 32 a, j + 32 b) of the R x R matrices (R up to 64)
    for (int ii = i; ii < R; ii += 32)
        for (int jj = j; jj < R; jj += 32) {
            double s = 0.0;
            for (int b = 0; b < nb; b++) s += gp[(size_t)b * R * R + ii * R + jj];
            G[ii][jj] = (ii < k && jj < k) ? s : (ii == jj ? 1.0 : 0.0);
            V[ii][jj] = ii == jj ? 1.0 : 0.0;
        }
    __syncthreads();
    if (mode == 0) {
        // Cholesky (upper) by thread 0 of each column step; k <= 64, sequential dependencies: one thread is enough
        if (threadIdx.x == 0) {
            int bad = 0;
            for (int c = 0; c < k; c++) {
                double dsum = G[c][c];
                for (int q = 0; q < c; q++) dsum -= V[q][c] * V[q][c];
                if (!(dsum > 0.0)) { bad = 1; break; }
                const double dd = sqrt(dsum);
                V[c][c] = dd;
                for (int t = c + 1; t < k; t++) {
                    double s2 = G[c][t];
                    for (int q = 0; q < c; q++) s2 -= V[q][c] * V[q][t];
                    V[c][t] = s2 / dd;
                }
                for (int t = 0; t < c; t++) V[c][t] = 0.0;
            }
            if (bad) status[0] = 1;                           // sticky: the caller clears it before a run
            // inverse of the upper factor into G (back substitution, column by column)
            for (int c = 0; c < R; c++) for (int t = 0; t < R; t++) G[c][t] = 0.0;
            if (!bad)
                for (int c = 0; c < k; c++) {
                    G[c][c] = 1.0 / V[c][c];
                    for (int t = c - 1; t >= 0; t--) {
                        double s2 = 0.0;
                        for (int q = t + 1; q <= c; q++) s2 += V[t][q] * G[q][c];
                        G[t][c] = -s2 / V[t][t];
                    }
                }
            for (int c = 0; c < k; c++) { vals[c] = V[c][c]; if (vals_host) vals_host[c] = V[c][c]; }
        }
        __syncthreads();
        for (int ii = i; ii < R; ii += 32)
            for (int jj = j; jj < R; jj += 32) S[ii * R + jj] = G[ii][jj];
        return;
    }
    // cyclic Jacobi on the k x k symmetric G; rotations applied by the 32 lanes of row 0 of the block (lane j: columns j, j + 32)
    // Stopping rule: sum over p < q of G[p][q]^2 <= 1e-30 tr^2, tr = sum |G[p][p]|, on G 2^-ex, ex = the binary exponent
    // of the largest |G[p][p]|.  Scaling by a power of two is exact, so the test is the same for G and for any power-of-two
    // multiple of G whose entries are finite normal numbers, bit for bit -- neither the squares nor the sum of the diagonal
    // can overflow, and what vanishes is below 1e-30 tr^2 anyway.  (The squares of the unscaled entries overflow or vanish
    // from |G| ~ 1e+-154 on, and the rule then held before the first sweep.)
    __shared__ int done;
    for (int sweep = 0; sweep < 30; sweep++) {
        __syncthreads();
        if (threadIdx.x == 0) {
            double dmax = 0.0;
            for (int p = 0; p < k; p++) dmax = fmax(dmax, fabs(G[p][p]));
            int ex = 0;
            (void)frexp(dmax, &ex);                           // (0 for dmax = 0)
            double tr = 0.0, o = 0.0;
            for (int p = 0; p < k; p++) tr += ldexp(fabs(G[p][p]), -ex);
            for (int p = 0; p < k; p++)
                for (int q = p + 1; q < k; q++) { const double rel = ldexp(G[p][q], -ex); o += rel * rel; }
            done = o <= 1e-30 * tr * tr;
        }
        __syncthreads();
        if (done) break;
        for (int p = 0; p < k - 1; p++)
            for (int q = p + 1; q < k; q++) {
                const double apq = G[p][q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double tau = (G[q][q] - G[p][p]) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t); s = t * c;
                }
                __syncthreads();
                if (i == 0)
                    for (int jj = j; jj < k; jj += 32) {         // columns p, q of G and V: G <- G J, V <- V J
                        const double gp_ = G[jj][p], gq_ = G[jj][q];
                        G[jj][p] = c * gp_ - s * gq_; G[jj][q] = s * gp_ + c * gq_;
                        const double vp = V[jj][p], vq = V[jj][q];
                        V[jj][p] = c * vp - s * vq; V[jj][q] = s * vp + c * vq;
                    }
                __syncthreads();
                if (i == 0)
                    for (int jj = j; jj < k; jj += 32) {         // rows p, q of G: G <- t(J) G
                        const double gp_ = G[p][jj], gq_ = G[q][jj];
                        G[p][jj] = c * gp_ - s * gq_; G[q][jj] = s * gp_ + c * gq_;
                    }
                __syncthreads();
            }
    }
    __syncthreads();
    // order the eigenvalues descending (thread 0: selection sort of k <= 64 columns)
    __shared__ int perm[R];
    if (threadIdx.x == 0) {
        for (int c = 0; c < R; c++) perm[c] = c;
        for (int a = 0; a < k; a++) {
            int best = a;
            for (int b = a + 1; b < k; b++) if (G[perm[b]][perm[b]] > G[perm[best]][perm[best]]) best = b;
            const int t = perm[a]; perm[a] = perm[best]; perm[best] = t;
        }
        for (int c = 0; c < k; c++) { vals[c] = G[perm[c]][perm[c]]; if (vals_host) vals_host[c] = vals[c]; }
        if (vals_host) { __threadfence_system(); vals_host[R] = seq; }       // sequence number: the host sees a complete set
    }
    __syncthreads();
    for (int ii = i; ii < R; ii += 32)
        for (int jj = j; jj < R; jj += 32) {
            const double v = (ii < k && jj < k) ? V[ii][perm[jj]] : 0.0;
            S[ii * R + jj] = v;
            if (S2) { const double lam = jj < k ? G[perm[jj]][perm[jj]] : 0.0; S2[ii * R + jj] = lam > 0.0 ? v / sqrt(lam) : 0.0; }
        }
}

// B[N][R] = A[N][R] S (S: R x R row-major); in place allowed (a thread owns a whole row).
template <int R>
__global__ __launch_bounds__(256) void k_apply(const double *__restrict__ A, const double *__restrict__ S, int64_t N, double *__restrict__ B)
{
    __shared__ double sS[R * R];
    for (int t = threadIdx.x; t < R * R; t += 256) sS[t] = S[t];
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    double a[R], o[R];
#pragma unroll
    for (int q = 0; q < R; q++) { a[q] = A[(size_t)row * R + q]; o[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < R; q++)
#pragma unroll
        for (int c = 0; c < R; c++) o[c] = fma(a[q], sS[q * R + c], o[c]);
#pragma unroll
    for (int c = 0; c < R; c++) B[(size_t)row * R + c] = o[c];
}

}  // namespace vbnmf
