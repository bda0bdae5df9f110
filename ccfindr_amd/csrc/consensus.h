// consensus.h -- device kernels of the consensus accumulator (vbnmf_consensus_*, include/vbnmf.h; included once, by
// labels.hip).  factorize() reports, per rank, the dispersion and the cophenetic correlation of the consensus matrix
// C_ij = share of the R runs in which cells i and j carry the same arg-max label (reference R/factorize.R:51-78,
// :218-230).  The reference forms the O(m^2) pair vector; its sums follow from the label vectors alone:
//   sum_{i<j} C_ij   = S1 / R,    S1 = sum_a sum_k pairs(n_k(a))
//   sum_{i<j} C_ij^2 = S2 / R^2,  S2 = sum_{a,b} sum_{k,l} pairs(n_kl(a, b))
// n_kl(a, b) = the contingency table of runs a and b, pairs(c) = c (c - 1) / 2; the term a = b of S2 is run a's term of
// S1.  A new run t therefore adds  pairs(table(t, t))  to S1 and  pairs(table(t, t)) + 2 sum_{a<t} pairs(table(a, t))
// to S2.  Integers throughout: the sums do not depend on the grid, the chunking or the order of the atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vbnmf {

constexpr int kCoinThreads = 256;
constexpr int kCoinChunk = 8192;            // cells per workgroup of k_label_coincidence

// which.max(h[, j])[1] (k_argmax's rule, mlnmf.h: first maximum, NaN never wins, a column of NaNs gives 0) as one row of
// the accumulator's label matrix.  perm: the engine's internal order of the cells (position -> caller's column); the
// row is stored in the caller's order, so engines with different layouts add comparable rows.
__global__ __launch_bounds__(256) void k_argmax_row(const double *__restrict__ h, int64_t m, int r, int R, const int32_t *__restrict__ perm,
                                                    uint8_t *__restrict__ row, int32_t *__restrict__ unlabelled)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double *hr = h + (size_t)j * R;
    int best = 0;
    double bv = 0.0;
    for (int k = 0; k < r; k++) {
        const double v = hr[k];
        if (v == v && (best == 0 || v > bv)) { best = k + 1; bv = v; }
    }
    row[perm ? (int64_t)perm[j] : j] = (uint8_t)best;
    if (best == 0) atomicOr(unlabelled, 1);
}

// Contingency tables of the new label row against every stored row, itself included.  Grid: (cell chunks, stored rows);
// workgroup (c, a) counts the cells of chunk c into a (r+1)^2 table of uint32 in LDS (dynamic: 66.6 KB at rank 128, within
// the CU's 160 KB) with integer LDS atomics, then adds its non-zero bins to run a's global uint64 table.
//   labels: [max_runs][m] uint8, 0 = no label;  t = the new row;  tables: [t + 1][(r+1)^2], zeroed by the caller.
__global__ __launch_bounds__(kCoinThreads) void k_label_coincidence(const uint8_t *__restrict__ labels, int64_t m, int r, int t,
                                                                    unsigned long long *__restrict__ tables)
{
    extern __shared__ uint32_t s_tab[];
    const int q = r + 1, bins = q * q;
    const int a = blockIdx.y;
    for (int b = threadIdx.x; b < bins; b += kCoinThreads) s_tab[b] = 0u;
    __syncthreads();
    const uint8_t *__restrict__ la = labels + (size_t)a * m;
    const uint8_t *__restrict__ lt = labels + (size_t)t * m;
    const int64_t j0 = (int64_t)blockIdx.x * kCoinChunk;
    const int64_t j1 = j0 + kCoinChunk < m ? j0 + kCoinChunk : m;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kCoinThreads) {
        const int ka = la[j], kt = lt[j];
        if (ka < q && kt < q) atomicAdd(&s_tab[ka * q + kt], 1u);
    }
    __syncthreads();
    unsigned long long *__restrict__ g = tables + (size_t)a * bins;
    for (int b = threadIdx.x; b < bins; b += kCoinThreads) {
        const uint32_t c = s_tab[b];
        if (c) atomicAdd(&g[b], (unsigned long long)c);
    }
}

// One workgroup per table: sum of pairs(n) over its bins (strided partial sums, then a fixed-shape tree in LDS), added
// to S2 -- twice for a < t, the pair (a, t) stands for (t, a) too -- and, for the table of the new row with itself, to S1.
//   sums: [0] = S1, [1] = S2.
__global__ __launch_bounds__(kCoinThreads) void k_coincidence_pairs(const unsigned long long *__restrict__ tables, int r, int t,
                                                                    unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long s_part[kCoinThreads];
    const int q = r + 1, bins = q * q;
    const int a = blockIdx.x;
    const unsigned long long *__restrict__ g = tables + (size_t)a * bins;
    unsigned long long s = 0;
    for (int b = threadIdx.x; b < bins; b += kCoinThreads) {
        const unsigned long long c = g[b];
        s += c * (c - (c > 0 ? 1ull : 0ull)) / 2ull;
    }
    s_part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kCoinThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_part[threadIdx.x] += s_part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long v = s_part[0];
        if (a == t) { atomicAdd(&sums[0], v); atomicAdd(&sums[1], v); }
        else atomicAdd(&sums[1], 2ull * v);
    }
}

}  // namespace vbnmf
