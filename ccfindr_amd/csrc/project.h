// project.h -- gfx950 kernel that places new cells on a fitted basis: ML-NMF with W held fixed (included once, by
// project.hip: its kernels are templates, but one unit launches them).
//
// Reference: the H half of nmf_updateR, R/factorize.R:8-15, iterated with w untouched, likelihood (:40-49) taken column by
// column, and factorize()'s stopping test (:208) applied to every cell on its own:
//   :8,:11  up_k = h_k * sum_i w_ik x_i / lambda_i  [+ gamma.a - 1],   lambda_i = sum_k w_ik h_k   (stored entries of the cell only)
//   :9,:12  dn_k = colSums(w)_k                     [+ gamma.a / gamma.b]
//   :14-15  h_k  = max(up_k / dn_k, eps)            (NaN stays NaN, as in R)
//   :40-49  lk   = sum_i x_i log lambda_i(h_new) - sum_k colSums(w)_k h_new,k + sum_{x>0}(-x log x + x)      (not divided by n m)
//   :208    stop when abs(lkold - lk) < Tol * abs(lkold)   (lkold = -Inf before the first step)
// With W fixed nothing couples two cells: no gene-side statistic, no partial rows, no all-reduce -- so no tiled layout.  A
// cell's working set is its stored entries and the W rows of the genes it expresses; one 256-thread workgroup takes a cell
// from the plain compressed columns to its stop inside one launch, and a persistent grid hands the cells out through a ticket
// counter (the cells' iteration counts differ widely).
//
// One pass over the cell's entries serves two iterations: lambda_i(h) gives step t's likelihood term x_i log lambda_i AND the
// quotient x_i / lambda_i that step t+1's update sums, so an iteration is one pass, two barriers and an R-wide update.
//
// Every pass reads the cell's entries and their W rows from global memory where they lie (the basis, n x R doubles, stays
// cache resident; a cell's own stretch of the entry stream is read by one workgroup only).  A form that staged the cell's
// rows (w_i. | x_i) in a 160 KB LDS image once and iterated out of LDS gave the same bits and was SLOWER at the C3 shape
// (profiles/project_times.txt; profiles/ubench/project_staged_form_experiment.patch), so it is not here.
//
// Order of every sum (it depends on the cell's entries and on r alone -- not on the grid, the workgroup or the other cells):
// SP = rank_shares(R) lanes share an entry, lane `sub` owning columns [sub RL, (sub + 1) RL), RL = R / SP; entry e of the
// cell goes to slot e mod kProjThreads / SP; a slot adds its entries in ascending order; slots are added by xor butterflies
// inside the wave (offsets SP, 2 SP, .. 32), the four waves in order 0..3.  No floating-point atomics.  Every loop is
// bounded by an entry count or by max_it: a NaN cannot hold one open.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"               // rank_shares
#include "special.h"              // dev_log

namespace vbnmf {

constexpr int kProjThreads = 256;
// entries of a cell the workgroup takes in one pass of its threads: columns longer than this go round again
constexpr int proj_pass_entries(int R) { return kProjThreads / rank_shares(R); }

struct ProjectArgs {
    const int64_t *colptr;     // [ncell + 1] pointers of the cells, as in the whole matrix
    int64_t base;              // ... whose entry `base` is the first one of row / val
    const int32_t *row;
    const double *val;
    const double *W;           // [n][R] (padding columns 0)
    const double *cw;          // [R] colSums(w) (padding 0)
    double *H;                 // [ncell][R] in: start (padding 0), out: result
    double *lk;                // [ncell]
    int32_t *it, *reason;      // [ncell]
    unsigned int *ticket;      // zero as the launch starts
    int64_t ncell;
    int32_t r, prior, max_it;
    double ga, gb, tol, eps;
};

template <int R>
__global__ __launch_bounds__(kProjThreads) void k_project(const ProjectArgs A)
{
    constexpr int SP = rank_shares(R), RL = R / SP, EPP = proj_pass_entries(R);
    __shared__ double s_h[R], s_cw[R], s_dn[R], s_red[4 * R], s_misc[8];
    __shared__ unsigned int s_ticket;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slot = t / SP, sub = t - slot * SP;
    const int r = A.r;
    const double inf = __builtin_huge_val();

    if (t < R) {
        const double c = A.cw[t];
        s_cw[t] = c;
        s_dn[t] = A.prior ? c + A.ga / A.gb : c;             // R/factorize.R:9,12
    }
    for (;;) {
        if (t == 0) s_ticket = atomicAdd(A.ticket, 1u);
        __syncthreads();
        const int64_t j = (int64_t)s_ticket;
        if (j >= A.ncell) break;                             // (block-uniform)
        const int64_t p0 = A.colptr[j] - A.base;
        const int len = (int)(A.colptr[j + 1] - A.colptr[j]);
        if (t < R) s_h[t] = A.H[(size_t)j * R + t];
        __syncthreads();

        double acc[RL], data, xl;
        // One pass over the cell with the h in s_h: acc = this slot's share of sum_i w_ik x_i / lambda_i, data = its share of
        // sum_i x_i log lambda_i, xl (first pass) = its share of sum(-x log x + x).
        auto pass = [&](bool first) {
#pragma unroll
            for (int c = 0; c < RL; c++) acc[c] = 0.0;
            data = 0.0; xl = 0.0;
            for (int e0 = 0; e0 < len; e0 += EPP) {          // (the trip count is the block's: the shuffles below see whole waves)
                const int e = e0 + slot;
                const bool live = e < len;
                double w[RL], x = 0.0, p = 0.0;
                if (live) {
                    const double *rowp = A.W + (size_t)A.row[p0 + e] * R + sub * RL;
                    x = A.val[p0 + e];
#pragma unroll
                    for (int c = 0; c < RL; c++) w[c] = rowp[c];
#pragma unroll
                    for (int c = 0; c < RL; c++) p += w[c] * s_h[sub * RL + c];
                }
#pragma unroll
                for (int off = 1; off < SP; off <<= 1) p += __shfl_xor(p, off);          // lambda_i: the same bits in the SP lanes
                if (live) {
                    const double q = x / p;
                    if (sub == 0) {
                        double lg = dev_log(p);
                        if (!(p > 0.0)) lg = p == 0.0 ? -inf : __builtin_nan("");        // log(0), log(negative or NaN)
                        if (p == inf) lg = inf;
                        data += x * lg;
                        if (first) xl += -x * dev_log(x) + x;
                    }
#pragma unroll
                    for (int c = 0; c < RL; c++) acc[c] += w[c] * q;
                }
            }
        };
        // the slots of a wave added by butterflies, one row of s_red and one slot of s_misc per wave; closed by a barrier
        auto publish = [&](bool first) {
#pragma unroll
            for (int c = 0; c < RL; c++) {
                double v = acc[c];
#pragma unroll
                for (int off = SP; off < 64; off <<= 1) v += __shfl_xor(v, off);
                if (lane < SP) s_red[wave * R + sub * RL + c] = v;
            }
#pragma unroll
            for (int off = SP; off < 64; off <<= 1) { data += __shfl_xor(data, off); xl += __shfl_xor(xl, off); }
            if (lane == 0) { s_misc[wave] = data; if (first) s_misc[4 + wave] = xl; }
            __syncthreads();
        };

        pass(true);
        publish(true);
        const double xlx = ((s_misc[4] + s_misc[5]) + s_misc[6]) + s_misc[7];
        double lkold = -inf, lk = 0.0;
        int it = 0, reason = 0;
        while (it < A.max_it) {
            it++;
            if (t < R) {
                double v = 0.0;
                if (t < r) {
                    const double s = ((s_red[t] + s_red[R + t]) + s_red[2 * R + t]) + s_red[3 * R + t];
                    double up = s_h[t] * s;                  // :8
                    if (A.prior) up = up + A.ga - 1.0;       // :11
                    v = up / s_dn[t];                        // :14
                    if (v < A.eps) v = A.eps;                // :15
                }
                s_h[t] = v;
            }
            __syncthreads();
            double cross = 0.0;
            for (int k = 0; k < r; k++) cross += s_cw[k] * s_h[k];
            pass(false);
            publish(false);
            const double dsum = ((s_misc[0] + s_misc[1]) + s_misc[2]) + s_misc[3];
            lk = (dsum - cross) + xlx;                       // :40-49 of this column
            if (lk != lk) reason = 3;
            else if (fabs(lkold - lk) < A.tol * fabs(lkold)) reason = 1;         // :208
            else { lkold = lk; if (it >= A.max_it) reason = 4; }
            if (reason) break;                               // (every thread holds the same lk)
        }
        if (t < R) A.H[(size_t)j * R + t] = s_h[t];
        if (t == 0) { A.lk[j] = lk; A.it[j] = it; A.reason[j] = reason; }
        __syncthreads();                                     // s_h and the ticket are free for the next cell
    }
}

}  // namespace vbnmf
