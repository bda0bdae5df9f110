// cophenet.h -- the grouped cophenetic correlation (reference R/factorize.R:69-78; host form: consensus.cpp) on the
// device, for more groups than the host form serves (included once, by cophenet.hip).  Two steps:
//   k_coph_setup_*  W[i][j] = distance of groups i, j (the host's expression, so the host's bits) and the weighted
//                   sums S[i][j] = size_i size_j dist(i, j); per row i, the sums over j > i the correlation needs.
//   k_coph_chain    the whole nearest-neighbour chain in ONE workgroup: ~3G dependent row arg-mins and G row / column
//                   updates, no grid barrier and no wait on another workgroup.  It follows consensus.cpp's rule step by
//                   step (chain from the lowest active group; the tip's neighbour is the group the chain came from unless
//                   another is strictly nearer, then the lowest-numbered minimum; the merged cluster keeps the lower
//                   number; the host's update expression in double), so W carries the host's bits after every merge and
//                   the dendrogram is the host's whatever ties the distances hold.
// The correlation's sums need no member lists: a merge of clusters x, y at height h adds h Wx Wy to sum c, h^2 Wx Wy
// to sum c^2 and h S[x][y] to sum d c, S[x][y] = sum_{i in x, j in y} size_i size_j d_ij being additive under merging
// (S[keep][k] += S[drop][k]).  One lane accumulates the G - 1 terms of each in a compensated (two-sum) double.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace vbnmf {

constexpr int kCophSetupThreads = 256;
constexpr int kCophChainThreads = 1024;
constexpr int kCophChainWaves = kCophChainThreads / 64;
constexpr int kCophScanAhead = 4;            // row entries a lane of the chain kernel loads before it compares them
static_assert(kCophMaxGroups <= 32768, "k_coph_chain keeps one activity byte per group in 32 KB of LDS");

// Fixed-shape tree over the workgroup's kCophSetupThreads values (the same shape on every run: the same bits).
template <class T, class Op>
__device__ inline T coph_block_reduce(T v, T *s_part, Op op)
{
    s_part[threadIdx.x] = v;
    __syncthreads();
    for (int w = kCophSetupThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_part[threadIdx.x] = op(s_part[threadIdx.x], s_part[threadIdx.x + w]);
        __syncthreads();
    }
    const T r = s_part[0];
    __syncthreads();
    return r;
}

// One workgroup per group i: row i of W and S from the label tuples, and over j > i
//   isum[i] = { sum size_j ham, sum size_j ham^2 }   (integers: below 2^59 under the entry's limits)
//   mm[i]   = { min ham / R, max ham / R }           (+-HUGE_VAL for the last row)
// The host multiplies by size_i and adds the rows up.  weight[i] = size_i starts the chain's cluster weights.
__global__ __launch_bounds__(kCophSetupThreads) void k_coph_setup_tuples(const uint8_t *__restrict__ tuples, const int64_t *__restrict__ sizes, int G, int R,
                                                                         double *__restrict__ W, double *__restrict__ S, double *__restrict__ weight,
                                                                         unsigned long long *__restrict__ isum, double *__restrict__ mm)
{
    __shared__ unsigned long long s_u[kCophSetupThreads];
    __shared__ int s_i[kCophSetupThreads];
    const int i = blockIdx.x;
    const uint8_t *__restrict__ ti = tuples + (size_t)i * R;
    const double si = (double)sizes[i], runs = (double)R;
    unsigned long long a1 = 0, a2 = 0;
    int kmin = 0x7fffffff, kmax = -1;
    for (int j = threadIdx.x; j < G; j += kCophSetupThreads) {
        const uint8_t *__restrict__ tj = tuples + (size_t)j * R;
        int k = 0;
        for (int a = 0; a < R; a++) k += ti[a] != tj[a];
        const unsigned long long sj = (unsigned long long)sizes[j];
        W[(size_t)i * G + j] = j == i ? 0.0 : (double)k / runs;
        S[(size_t)i * G + j] = si * (double)sj * (double)k;
        if (j > i) {
            a1 += sj * (unsigned long long)k;
            a2 += sj * (unsigned long long)k * (unsigned long long)k;
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
    }
    auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    a1 = coph_block_reduce(a1, s_u, add);
    a2 = coph_block_reduce(a2, s_u, add);
    kmin = coph_block_reduce(kmin, s_i, [](int x, int y) { return x < y ? x : y; });
    kmax = coph_block_reduce(kmax, s_i, [](int x, int y) { return x > y ? x : y; });
    if (threadIdx.x == 0) {
        isum[2 * (size_t)i] = a1; isum[2 * (size_t)i + 1] = a2;
        mm[2 * (size_t)i] = kmax < 0 ? HUGE_VAL : (double)kmin / runs;
        mm[2 * (size_t)i + 1] = kmax < 0 ? -HUGE_VAL : (double)kmax / runs;
        weight[i] = si;
    }
}

// The same from real-valued distances (the test hook): W[i][j] = dist[min][max] as the host mirrors its upper triangle,
//   fsum[i] = { sum size_j d, sum size_j d^2 } over j > i, each lane's terms in ascending j, then the fixed tree.
__global__ __launch_bounds__(kCophSetupThreads) void k_coph_setup_dist(const double *__restrict__ dist, const int64_t *__restrict__ sizes, int G,
                                                                       double *__restrict__ W, double *__restrict__ S, double *__restrict__ weight,
                                                                       double *__restrict__ fsum, double *__restrict__ mm)
{
    __shared__ double s_d[kCophSetupThreads];
    const int i = blockIdx.x;
    const double si = (double)sizes[i];
    double a1 = 0.0, a2 = 0.0, dmin = HUGE_VAL, dmax = -HUGE_VAL;
    for (int j = threadIdx.x; j < G; j += kCophSetupThreads) {
        const double sj = (double)sizes[j];
        const double d = j == i ? 0.0 : (j > i ? dist[(size_t)i * G + j] : dist[(size_t)j * G + i]);
        W[(size_t)i * G + j] = d;
        S[(size_t)i * G + j] = si * sj * d;
        if (j > i) {
            a1 += sj * d;
            a2 += sj * d * d;
            dmin = d < dmin ? d : dmin;
            dmax = d > dmax ? d : dmax;
        }
    }
    auto add = [](double x, double y) { return x + y; };
    a1 = coph_block_reduce(a1, s_d, add);
    a2 = coph_block_reduce(a2, s_d, add);
    dmin = coph_block_reduce(dmin, s_d, [](double x, double y) { return x < y ? x : y; });
    dmax = coph_block_reduce(dmax, s_d, [](double x, double y) { return x > y ? x : y; });
    if (threadIdx.x == 0) {
        fsum[2 * (size_t)i] = a1; fsum[2 * (size_t)i + 1] = a2;
        mm[2 * (size_t)i] = dmin; mm[2 * (size_t)i + 1] = dmax;
        weight[i] = si;
    }
}

// hi + lo += v, the rounding error of the addition kept in lo (two-sum; contraction is off)
__device__ inline void coph_two_sum(double &hi, double &lo, double v)
{
    const double s = hi + v;
    const double b = s - hi;
    lo += (hi - (s - b)) + (v - b);
    hi = s;
}

// lexicographic (value, index) minimum
__device__ inline void coph_lex_min(double &v, int &j, double ov, int oj)
{
    if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
}

// The agglomeration: ONE workgroup of kCophChainThreads.  link: 0 average, 1 single, 2 complete (consensus.cpp's Link).
//   W, S: [G][G], updated in place;  weight: [G] cluster weights;  chain: [G] the chain's stack
//   merges: [G-1][2] (kept, dropped) per merge;  heights: [G-1]
//   out: CophChainOut -- [0..5] sum c, sum c^2, sum S h as (hi, lo) pairs, [6] min c, [7] max c, [8] status, [9] merges done
// Every value that steers the loop (x, prev, y, the stack depth) is computed by all lanes from the same LDS words, so
// the barriers are reached together.  Bounded by construction: G - 1 merges, at most 2 G pushes; past a bound, or when a
// tip has no neighbour at a finite distance, the status word says so and the kernel returns.
__global__ __launch_bounds__(kCophChainThreads) void k_coph_chain(double *W, double *S, double *weight, int *chain, int G, int link,
                                                                  long long *__restrict__ merges, double *__restrict__ heights, double *__restrict__ out)
{
    __shared__ uint8_t s_active[kCophMaxGroups];
    __shared__ double s_val[2][kCophChainWaves];
    __shared__ int s_idx[2][kCophChainWaves];
    __shared__ int s_lowest;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < G; j += kCophChainThreads) s_active[j] = 1;
    if (tid == 0) s_lowest = 0;
    __syncthreads();
    double sc = 0, sc_lo = 0, scc = 0, scc_lo = 0, sdc = 0, sdc_lo = 0, cmin = HUGE_VAL, cmax = -HUGE_VAL;   // lane 0's
    int len = 0, x = -1, prev = -1, status = kCophOk, done = 0;
    long long pushes = 0;
    unsigned turn = 0;
    for (int left = G; left > 1 && status == kCophOk; left--) {
        const int lowest = s_lowest;
        if (len == 0) {
            x = lowest; prev = -1; len = 1;
            if (tid == 0) chain[0] = x;
            pushes++;
        }
        int y = -1;
        for (;;) {
            // nearest active neighbour of x: each lane the lowest-numbered minimum of its stride, then (value, index) minima
            const double *row = W + (size_t)x * G;
            double bv = HUGE_VAL;
            int bj = 0x7fffffff;
            for (int j0 = lowest + tid; j0 < G; j0 += kCophScanAhead * kCophChainThreads) {
                double v[kCophScanAhead];         // the loads of a few trips in flight together; compared in ascending j
#pragma unroll
                for (int u = 0; u < kCophScanAhead; u++) {
                    const int j = j0 + u * kCophChainThreads;
                    v[u] = j < G ? row[j] : HUGE_VAL;
                }
#pragma unroll
                for (int u = 0; u < kCophScanAhead; u++) {
                    const int j = j0 + u * kCophChainThreads;
                    if (j < G && s_active[j] && j != x && v[u] < bv) { bv = v[u]; bj = j; }
                }
            }
            for (int off = 32; off > 0; off >>= 1) coph_lex_min(bv, bj, __shfl_xor(bv, off, 64), __shfl_xor(bj, off, 64));
            const int buf = turn & 1;
            turn++;
            if (lane == 0) { s_val[buf][wave] = bv; s_idx[buf][wave] = bj; }
            __syncthreads();
            bv = s_val[buf][0]; bj = s_idx[buf][0];
            for (int w = 1; w < kCophChainWaves; w++) coph_lex_min(bv, bj, s_val[buf][w], s_idx[buf][w]);
            // the host's rule: stay with prev unless something is strictly nearer
            y = prev;
            if (bj != 0x7fffffff && (prev < 0 || bv < row[prev])) y = bj;
            if (y < 0) { status = kCophNotFinite; break; }
            if (y == prev) break;
            if (++pushes > 2 * (long long)G || len >= G) { status = kCophBound; break; }
            if (tid == 0) chain[len] = y;
            len++;
            prev = x; x = y;
        }
        if (status != kCophOk) break;
        // merge x and y at h = W[x][y]
        const int keep = x < y ? x : y, drop = x < y ? y : x;
        const double h = W[(size_t)x * G + y], sxy = S[(size_t)x * G + y];
        const double wk = weight[keep], wd = weight[drop];
        double *rk = W + (size_t)keep * G;
        const double *rd = W + (size_t)drop * G;
        double *sk = S + (size_t)keep * G;
        const double *sd = S + (size_t)drop * G;
        for (int k = lowest + tid; k < G; k += kCophChainThreads) {
            if (!s_active[k] || k == keep || k == drop) continue;
            const double a = rk[k], b = rd[k];
            double v;
            if (link == 1) v = a < b ? a : b;                  // std::min(a, b)
            else if (link == 2) v = a < b ? b : a;             // std::max(a, b)
            else v = (wk * a + wd * b) / (wk + wd);
            rk[k] = v; W[(size_t)k * G + keep] = v;
            const double s = sk[k] + sd[k];
            sk[k] = s; S[(size_t)k * G + keep] = s;
        }
        __syncthreads();                                       // every read of the weights and the flags is done
        if (tid == 0) {
            const double ww = wk * wd;
            coph_two_sum(sc, sc_lo, h * ww);
            coph_two_sum(scc, scc_lo, h * h * ww);
            coph_two_sum(sdc, sdc_lo, h * sxy);
            cmin = h < cmin ? h : cmin;
            cmax = h > cmax ? h : cmax;
            merges[2 * (size_t)done] = keep; merges[2 * (size_t)done + 1] = drop;
            heights[done] = h;
            weight[keep] = wk + wd;
            s_active[drop] = 0;
            int lo = lowest;
            while (lo < G && !s_active[lo]) lo++;
            s_lowest = lo;
        }
        done++;
        len -= 2;
        __syncthreads();
        if (len >= 1) x = chain[len - 1];
        prev = len >= 2 ? chain[len - 2] : -1;
    }
    if (tid == 0) {
        out[0] = sc; out[1] = sc_lo; out[2] = scc; out[3] = scc_lo; out[4] = sdc; out[5] = sdc_lo;
        out[6] = cmin; out[7] = cmax; out[8] = (double)status; out[9] = (double)done;
    }
}

}  // namespace vbnmf
