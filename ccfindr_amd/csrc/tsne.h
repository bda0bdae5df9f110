// tsne.h -- gfx950 kernels behind visualize_clusters: the exact (theta = 0) t-SNE map of the cells (included once, by tsne.hip).
//
// Reference: visualize_clusters() (R/utils.R:692-712) hands t(h) to Rtsne (:700), a CPU package.  What is computed here is the
// t-SNE authors' published algorithm in its exact O(n^2) form, stated in DESIGN.md 5k; Rtsne itself is not pinned.
//   X: n points x d doubles (on the device as xt[d][n], so a wave's loads of one coordinate are contiguous).
//   D_ij = sum_k (x_ik - x_jk)^2, added in the order k = 0 .. d-1 (symmetric in i, j bit for bit).
//   affinities: per point i a bisection on beta_i until the entropy of p_{.|i} is ln(perplexity)       -> k_tsne_affinity
//   P_ij = (exp(-beta_i D_ij) / S_i + exp(-beta_j D_ij) / S_j) / (2n), never stored: recomputed per pair  -> k_tsne_force
//   w_ij = 1 / (1 + |y_i - y_j|^2);  A_i = sum_j P_ij w_ij (y_i - y_j);  R_i = sum_j w_ij^2 (y_i - y_j);  z_i = sum_j w_ij
//   Z = sum_i z_i;  dY = e A - R / Z;  gains, uY, Y, column means                                        -> k_tsne_update
//   C_i = sum_j P_ij ln P_ij - sum_j P_ij ln w_ij + ln Z sum_j P_ij;  C = sum_i C_i                       -> k_tsne_update
//
// Every sum follows a fixed tree: a thread adds its own terms in ascending order, a wave adds its 64 lanes in an xor butterfly
// (commutative at every level, so all lanes hold the same bits), the waves' values are added in wave order.  No floating-point
// atomics and nothing that depends on the grid's timing: the same input gives the same bits on every call.
// Every loop is bounded by n, d, the tile or kTsneMaxTrips; every index is formed from n and d, which the host checked.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/vbnmf.h"

namespace vbnmf {

constexpr int kTsneWave = 64;
constexpr int kTsneThreads = 256;                    // affinity and force kernels
constexpr int kTsneWaves = kTsneThreads / kTsneWave;
constexpr int kTsneLdsRow = 2048;                    // distances of one row the affinity kernel keeps in LDS: 16 KB, so the registers (94) and not the LDS bound the workgroups of a CU
constexpr int kTsneMaxTrips = 200;
constexpr int kTsneIBlock = 64;                      // points i of one force workgroup: one per lane, the four waves share the j
constexpr int kTsneJTile = 32;                       // points j of one LDS tile: 8 per wave
constexpr int kTsneTileHead = 4;                     // y0, y1, beta, 1/S in front of a tile row's d coordinates
constexpr int kTsneForceSums = 8;                    // A0 A1 R0 R1 z and the three cost sums
constexpr int kTsneUpdThreads = 1024;                // the update kernel: ONE workgroup, so Z and the column means need no second launch
constexpr int kTsneUpdWaves = kTsneUpdThreads / kTsneWave;
static_assert(kTsneJTile % kTsneWaves == 0 && kTsneIBlock == kTsneWave, "a lane is a point i; a wave takes a whole share of a tile");
static_assert((size_t)kTsneJTile * (VBNMF_MAX_RANK + kTsneTileHead) * 8 <= 65536, "the widest tile fits the LDS of a plain launch");

__device__ inline double tsne_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- what the dense and the neighbour path (tsne_knn.h) share ---------------------------------------------------------------
// Stages x_i into s_xi and writes the row D_i. into `row`, k ascending; thread t writes (and later reads) the entries
// j = t, t + 256, .. only, so a row in global memory needs no fence.
__device__ __forceinline__ void tsne_distance_row(const double *xt, int n, int d, int i, double *s_xi, double *row)
{
    const int t = threadIdx.x;
    __syncthreads();                                                           // the last point's reads of the shared arrays are done
    if (t < d) s_xi[t] = xt[(int64_t)t * n + i];
    __syncthreads();
    for (int j = t; j < n; j += kTsneThreads) {
        double D = 0.0;
        for (int k = 0; k < d; k++) {
            const double df = s_xi[k] - xt[(int64_t)k * n + j];
            D += df * df;
        }
        row[j] = D;
    }
}

struct TsneBisection { double beta, S; int trips; };                          // (trips: thread 0's)

// The bisection on beta of one point, by the whole workgroup, over the `count` distances dist(q), the term q == skip left out
// (-1: none).  A trip evaluates S = sum exp(-beta D) + DBL_MIN and sum D exp(-beta D) in the fixed tree: thread t adds the terms
// t, t + 256, .. in ascending order, a wave its 64 lanes in the xor butterfly, the waves are added in wave order.  Thread 0
// alone takes the branch from them and publishes beta and the state through s_ctl, every thread follows.
// A point that converges keeps the beta and S of that trip.  A point that uses up its kTsneMaxTrips keeps the beta of the last
// update and S is evaluated once more at it, so exp(-beta D) / S sums to 1 in either case.
template <class Dist>
__device__ __forceinline__ TsneBisection tsne_bisect(int count, int skip, Dist dist, double log_u, double *s_red, double *s_ctl)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double beta = 1.0, lo = -DBL_MAX, hi = DBL_MAX, S = 0.0;                   // lo, hi, trips: thread 0's
    int trips = 0, state = 0;                                                  // 0 bisecting, 1 converged, 2 out of trips
    for (;;) {
        double sp = 0.0, sdp = 0.0;
        for (int q = t; q < count; q += kTsneThreads) {
            if (q == skip) continue;
            const double D = dist(q);
            const double p = exp(-beta * D);
            sp += p;
            sdp += D * p;
        }
        sp = tsne_wave_sum(sp);
        sdp = tsne_wave_sum(sdp);
        __syncthreads();                                                       // s_red and s_ctl are free
        if (lane == 0) { s_red[wave] = sp; s_red[kTsneWaves + wave] = sdp; }
        __syncthreads();
        sp = s_red[0]; sdp = s_red[kTsneWaves];
#pragma unroll
        for (int w = 1; w < kTsneWaves; w++) { sp += s_red[w]; sdp += s_red[kTsneWaves + w]; }
        S = sp + DBL_MIN;
        if (state == 2) break;
        if (t == 0) {
            const double H = beta * sdp / S + log(S);
            const double delta = H - log_u;
            trips++;
            if (fabs(delta) < 1e-5) state = 1;
            else {
                if (delta > 0.0) { lo = beta; beta = hi == DBL_MAX ? beta * 2.0 : (beta + hi) / 2.0; }
                else { hi = beta; beta = lo == -DBL_MAX ? beta / 2.0 : (beta + lo) / 2.0; }
                if (trips == kTsneMaxTrips) state = 2;
            }
            s_ctl[0] = beta;
            s_ctl[1] = (double)state;
        }
        __syncthreads();
        beta = s_ctl[0];
        state = (int)s_ctl[1];
        if (state == 1) break;
    }
    return {beta, S, trips};
}

// The point of a lane in a kernel whose workgroup owns kTsneIBlock points, one per lane, the four waves sharing the j.
struct TsneLanePoint { int i, ii; bool valid; };                              // ii: a lane past the end loads the last point and writes nothing
__device__ __forceinline__ TsneLanePoint tsne_lane_point(int n, int lane)
{
    const int i = blockIdx.x * kTsneIBlock + lane;
    return {i, i < n ? i : n - 1, i < n};
}

// Joins the four waves' partial sums of such a kernel: a lane's NS sums go to s_part[wave][s][lane] (the kernel's tile, which
// is free after the barrier), and lane i of wave 0 writes (w0 + w1) + (w2 + w3) to the rows row0 .. row0 + NS - 1 of `sums`.
// lane, wave: the kernel's own (formed here again from threadIdx.x they add 12 to 25 instructions to k_tsne_force).
template <int NS>
__device__ __forceinline__ void tsne_merge_waves(const double (&mine)[NS], double *s_part, double *sums, int row0, int n, TsneLanePoint p,
                                                 int lane, int wave)
{
    __syncthreads();                                                           // the tile is free: the waves' partial sums go there
#pragma unroll
    for (int s = 0; s < NS; s++) s_part[(wave * NS + s) * kTsneWave + lane] = mine[s];
    __syncthreads();
    if (wave == 0 && p.valid) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const double p0 = s_part[(0 * NS + s) * kTsneWave + lane], p1 = s_part[(1 * NS + s) * kTsneWave + lane];
            const double p2 = s_part[(2 * NS + s) * kTsneWave + lane], p3 = s_part[(3 * NS + s) * kTsneWave + lane];
            sums[(int64_t)(row0 + s) * n + p.i] = (p0 + p1) + (p2 + p3);
        }
    }
}

// w_ij of one pair with d = y_i - y_j.  The division is IEEE: the tests' 6u on w rests on it.
__device__ __forceinline__ double tsne_pair_w(double d0, double d1) { return 1.0 / (1.0 + d0 * d0 + d1 * d1); }

// ---- affinities ------------------------------------------------------------------------------------------------------------
struct TsneAffArgs {
    int32_t n, d;
    const double *xt;              // [d][n]
    double *scratch;               // [grid][n] rows of D for n > kTsneLdsRow; NULL otherwise
    double log_u;                  // ln(perplexity)
    double *beta, *sum_p, *inv_s;  // [n] beta_i, S_i, 1 / S_i
    int32_t *trips;                // [n]
};

// One workgroup per point i, in grid strides.  The row D_i. is computed once (tsne_distance_row): into LDS while
// n <= kTsneLdsRow, else into the workgroup's own row of `scratch`.  The bisection (tsne_bisect) runs over all j != i.
__global__ __launch_bounds__(kTsneThreads) void k_tsne_affinity(const TsneAffArgs A)
{
    __shared__ double s_row[kTsneLdsRow];
    __shared__ double s_xi[VBNMF_MAX_RANK];
    __shared__ double s_red[2 * kTsneWaves];
    __shared__ double s_ctl[2];
    const int n = A.n;
    double *row = n <= kTsneLdsRow ? s_row : A.scratch + (int64_t)blockIdx.x * n;

    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        tsne_distance_row(A.xt, n, A.d, i, s_xi, row);
        const TsneBisection b = tsne_bisect(n, i, [row](int j) { return row[j]; }, A.log_u, s_red, s_ctl);
        if (threadIdx.x == 0) {
            A.beta[i] = b.beta;
            A.sum_p[i] = b.S;
            A.inv_s[i] = 1.0 / b.S;
            A.trips[i] = b.trips;
        }
    }
}

// ---- forces ----------------------------------------------------------------------------------------------------------------
struct TsneForceArgs {
    int32_t n, d;
    int32_t cost;                  // also form the three cost sums
    const double *xt, *beta, *inv_s, *y0, *y1;
    double inv_2n;
    double *sums;                  // [kTsneForceSums][n]: A0 A1 R0 R1 z, sum P ln P, sum P ln w, sum P
};

// A workgroup owns the kTsneIBlock points i = blockIdx.x * 64 + lane and streams all j through LDS in tiles of kTsneJTile rows
// (y_j0, y_j1, beta_j, 1/S_j, x_j0 .. x_j,d-1).  Wave w takes the rows w * 8 .. w * 8 + 7 of every tile, so a point's terms are
// split over the four waves by j alone; each wave adds its terms in ascending j, and tsne_merge_waves joins the four partial
// sums and writes the point's sums once.
// DR > 0: x_i sits in DR registers (d <= DR), the tile's rows are DR wide and both are zero past d, so the loop over k has no
// bound to test and D_ij keeps its bits.  DR = 0: x_i is read per pair from xt (the loads of a wave are contiguous and
// stay in L1 / L2); wide d pays for it, the usual ranks do not take this path.
template <int DR>
__global__ __launch_bounds__(kTsneThreads) void k_tsne_force(const TsneForceArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double tsne_smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = A.n, d = A.d, stride = (DR > 0 ? DR : d) + kTsneTileHead;      // as tsne_force_lds() sizes it
    const TsneLanePoint pt = tsne_lane_point(n, lane);
    const int i = pt.i, ii = pt.ii;
    double xi[DR > 0 ? DR : 1];
    if (DR > 0) {
#pragma unroll
        for (int k = 0; k < DR; k++) xi[k] = k < d ? A.xt[(int64_t)k * n + ii] : 0.0;
    }
    const double *xti = A.xt + ii;
    const double bi = A.beta[ii], si = A.inv_s[ii], yi0 = A.y0[ii], yi1 = A.y1[ii];
    double a0 = 0.0, a1 = 0.0, r0 = 0.0, r1 = 0.0, z = 0.0, c1 = 0.0, c2 = 0.0, cp = 0.0;

    for (int j0 = 0; j0 < n; j0 += kTsneJTile) {
        __syncthreads();                                                       // the last tile has been read
        for (int idx = t; idx < kTsneJTile * stride; idx += kTsneThreads) {
            const int c = idx / kTsneJTile, jj = idx % kTsneJTile, j = j0 + jj;
            double v = 0.0;
            if (j < n) {
                if (c >= kTsneTileHead) v = c - kTsneTileHead < d ? A.xt[(int64_t)(c - kTsneTileHead) * n + j] : 0.0;
                else v = c == 0 ? A.y0[j] : (c == 1 ? A.y1[j] : (c == 2 ? A.beta[j] : A.inv_s[j]));
            }
            tsne_smem[jj * stride + c] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int q = 0; q < kTsneJTile / kTsneWaves; q++) {
            const int jj = wave * (kTsneJTile / kTsneWaves) + q, j = j0 + jj;
            if (j >= n) break;                                                 // (wave-uniform)
            const double *T = tsne_smem + jj * stride;
            double D = 0.0;
            if (DR > 0) {
#pragma unroll
                for (int k = 0; k < DR; k++) {                                   // k >= d: 0 - 0, and D + 0 is D
                    const double df = xi[k] - T[kTsneTileHead + k];
                    D += df * df;
                }
            } else {
                for (int k = 0; k < d; k++) {
                    const double df = xti[(int64_t)k * n] - T[kTsneTileHead + k];
                    D += df * df;
                }
            }
            if (pt.valid && j != i) {
                const double pij = exp(-bi * D) * si;
                const double pji = exp(-T[2] * D) * T[3];
                const double P = (pij + pji) * A.inv_2n;
                const double d0 = yi0 - T[0], d1 = yi1 - T[1];
                const double w = tsne_pair_w(d0, d1);
                const double pw = P * w, ww = w * w;
                a0 += pw * d0;
                a1 += pw * d1;
                r0 += ww * d0;
                r1 += ww * d1;
                z += w;
                if (A.cost && P > 0.0) {
                    c1 += P * log(P);
                    c2 += P * log(w);
                    cp += P;
                }
            }
        }
    }
    const double mine[kTsneForceSums] = {a0, a1, r0, r1, z, c1, c2, cp};
    tsne_merge_waves(mine, tsne_smem, A.sums, 0, n, pt, lane, wave);              // s_part [kTsneWaves][kTsneForceSums][64]
}

constexpr size_t kTsneForcePartBytes = (size_t)kTsneWaves * kTsneForceSums * kTsneWave * sizeof(double);
inline int tsne_force_width(int d) { return d <= 8 ? 8 : (d <= 16 ? 16 : (d <= 32 ? 32 : 0)); }     // DR of the launch
inline size_t tsne_force_lds(int d)
{
    const int DR = tsne_force_width(d);
    const size_t tile = (size_t)kTsneJTile * (size_t)((DR > 0 ? DR : d) + kTsneTileHead) * sizeof(double);
    return tile > kTsneForcePartBytes ? tile : kTsneForcePartBytes;
}

// ---- update ----------------------------------------------------------------------------------------------------------------
struct TsneUpdArgs {
    int32_t n;
    int32_t do_step, do_cost;
    double e, m, eta, min_gain;
    const double *sums;            // k_tsne_force's
    double *y0, *y1, *u0, *u1, *g0, *g1;
    double *cost_i;                // [n], written with do_cost
    double *cost_out;              // one double, written with do_cost
};

__device__ inline double tsne_block_sum(double v, double *s_red)
{
    v = tsne_wave_sum(v);
    __syncthreads();                                                           // s_red is free
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = s_red[0];
#pragma unroll
    for (int w = 1; w < kTsneUpdWaves; w++) s += s_red[w];
    return s;
}

__device__ inline int tsne_sign(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }

// One workgroup: thread t owns the points t, t + 1024, .. in every phase, so it reads back only what it wrote itself.
//   Z = sum_i z_i;  with do_cost: C_i = (sum P ln P - sum P ln w) + ln Z sum P and C = sum_i C_i, of the Y the sums were formed on;
//   with do_step: dY = e A - R / Z, the gains, uY = m uY - eta gains dY, Y += uY, then the column means are subtracted.
__global__ __launch_bounds__(kTsneUpdThreads) void k_tsne_update(const TsneUpdArgs A)
{
    __shared__ double s_red[kTsneUpdWaves];
    const int t = threadIdx.x, n = A.n;
    const double *S = A.sums;
    double zs = 0.0;
    for (int i = t; i < n; i += kTsneUpdThreads) zs += S[(int64_t)4 * n + i];
    const double Z = tsne_block_sum(zs, s_red);
    if (A.do_cost) {
        const double lnZ = log(Z);
        double cs = 0.0;
        for (int i = t; i < n; i += kTsneUpdThreads) {
            const double ci = (S[(int64_t)5 * n + i] - S[(int64_t)6 * n + i]) + lnZ * S[(int64_t)7 * n + i];
            A.cost_i[i] = ci;
            cs += ci;
        }
        const double C = tsne_block_sum(cs, s_red);
        if (t == 0) *A.cost_out = C;
    }
    if (!A.do_step) return;                                                    // (uniform)
    double m0 = 0.0, m1 = 0.0;
    for (int i = t; i < n; i += kTsneUpdThreads) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            double *y = c ? A.y1 : A.y0, *u = c ? A.u1 : A.u0, *g = c ? A.g1 : A.g0;
            const double dY = A.e * S[(int64_t)c * n + i] - S[(int64_t)(2 + c) * n + i] / Z;
            double gain = g[i];
            const double uy = u[i];
            gain = tsne_sign(dY) != tsne_sign(uy) ? gain + 0.2 : gain * 0.8;
            if (gain < A.min_gain) gain = A.min_gain;
            const double un = A.m * uy - A.eta * gain * dY;
            const double yn = y[i] + un;
            g[i] = gain;
            u[i] = un;
            y[i] = yn;
            if (c) m1 += yn; else m0 += yn;
        }
    }
    m0 = tsne_block_sum(m0, s_red) / (double)n;
    m1 = tsne_block_sum(m1, s_red) / (double)n;
    for (int i = t; i < n; i += kTsneUpdThreads) {
        A.y0[i] -= m0;
        A.y1[i] -= m1;
    }
}

}  // namespace vbnmf
