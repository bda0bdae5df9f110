// vbproject.h -- gfx950 kernel that places new cells on a VB fit's posterior basis: the H half of the VB-NMF update with
// q(W) held fixed (included once, by project.hip: k_vbp_control is no template, so a second unit would define it again).
//
// Reference: the H half of vbnmf_updateR, R/bayesian.R:71-95, iterated with lw, ew untouched, the evidence taken column by
// column (the cell's column of U1, :90-91, plus its column of U3, :94-95; U2 belongs to W), and vb_iterate's stopping test
// (:345-347) applied to every cell on its own:
//   :71      lambda_i = sum_k lw_ik lh_k                               (stored entries of the cell only)
//   :73      sh_k  = lh_k sum_i lw_ik x_i / lambda_i
//   :79      alh_k = ah + sh_k
//   :80      beh_k = 1 / (ah / bh + colSums(ew)_k)                     (the fitted ew: constant over cells and iterations)
//   :81,:103 eh_k  = alh_k beh_k ;  dh_k = alh_k beh_k^2
//   :84,:87  lh_k  = max(exp(psi(alh_k)) beh_k, fudge)                 (NaN stays NaN, as in R)
//   :90-91   - sum_k colSums(ew)_k eh_k - sum_i lgamma(x_i + 1)
//            - sum_i x_i [ (sum_k (lw log lw)_ik lh_k + sum_k lw_ik (lh log lh)_k) / lambda_i - log lambda_i ]     (at the NEW lh)
//   :94-95   + sum_k [ -(ah/bh) eh_k - lgamma(ah) + ah log(ah/bh) + alh_k (1 + log beh_k) + lgamma(alh_k) ]
//   :345-347 ev NaN: reason 3; after step it > 1, abs(1 - ev / lk0) < Tol: reason 1 (lk0 = 0 before the first step); max_it: 4.
// The reference's `lkh >= lk0` clause is left out on purpose: the evidence is not monotone under this update (DESIGN.md
// section 5g), and with the clause a cell's stop would hang on the sign of a rounding-level difference.  The n0 gate goes
// with the hyper-parameter updates, of which there are none here.
//
// The shape is k_project's (project.h): with q(W) fixed nothing couples two cells, so one 256-thread workgroup takes a cell
// from the plain compressed columns to its stop inside one launch, and a persistent grid hands the cells out through a
// ticket counter.  One pass over the cell's entries with the new lh serves two iterations: lambda_i(new) gives step t's
// evidence term AND the quotient x_i / lambda_i that step t + 1 sums.
//
// The table a cell gathers from holds, per gene, the row of lw and the row of lw log(lw) side by side ([n][2 R], padding
// columns 0; lw log lw is formed once per call on the host): an entry costs one gather of 2 R doubles and three R-wide dots,
// lw.lh, (lw log lw).lh and lw.(lh log lh) -- the last two added into one sum, term by term.  Per iteration thread k < r
// evaluates psi, lgamma (special.h, as the posterior update kernels) and exp for component k.
//
// Order of every sum: that of project.h (rank_shares lanes share an entry; entry e goes to slot e mod pass entries; a slot
// adds its entries in ascending order; slots by xor butterflies inside the wave; the four waves in order 0..3); the sums
// over k of the evidence are added by every thread alike, k ascending.  A cell's bits depend on its own entries and on r
// only.  No floating-point atomics.  Every loop is bounded by an entry count or by max_it.
#pragma once
#include "hyper.h"                // block_sum, dev_hyper_update_pair (the coupled form at the end of this file)
#include "project.h"
#include "special.h"

namespace vbnmf {

struct VbProjectArgs {
    const int64_t *colptr;     // [ncell + 1] pointers of the cells, as in the whole matrix
    int64_t base;              // ... whose entry `base` is the first one of row / val
    const int32_t *row;
    const double *val;
    const double *T;           // [n][2 R]: lw_i. | (lw log lw)_i.   (padding columns 0)
    const double *cew;         // [R] colSums(ew) (padding 0)
    double *LH;                // [ncell][R] in: start (padding 0), out: lh
    double *EH, *DH;           // [ncell][R] out
    double *ev;                // [ncell]
    int32_t *it, *reason;      // [ncell]
    unsigned int *ticket;      // zero as the launch starts
    int64_t ncell;
    int32_t r, max_it;
    double ah, bh, tol, fudge;
};

// ln(p) with R's edges: log(0) = -Inf, log(negative or NaN) = NaN, log(Inf) = Inf (dev_log itself covers finite p > 0)
__device__ __forceinline__ double vbp_log(double p)
{
    const double inf = __builtin_huge_val();
    double lg = dev_log(p);
    if (!(p > 0.0)) lg = p == 0.0 ? -inf : __builtin_nan("");
    if (p == inf) lg = inf;
    return lg;
}

// Waves per SIMD the kernel is compiled for: the second argument of HIP's __launch_bounds__ (NOT CUDA's blocks per
// multiprocessor).  A workgroup of kProjThreads = 256 is four waves, one per SIMD of a CU, so here -- and only while the
// workgroup stays that size -- two waves per SIMD means two workgroups per CU.
// A lane holds five vectors of RL = R / rank_shares(R) doubles (its share of lw_i., of the accumulators, of lh and of
// lh log lh, and the loads of lw log lw in flight), so from RL = 16 on the kernel takes more than 256 registers and only ONE
// workgroup fits a CU.  Capping it at 256 (two waves per SIMD) costs spills; measured at the C3 shape
// (profiles/vb_project_times.txt), that wins where RL is 16 to 24 (kernel time x 0.71 to 0.90 at ranks 16, 18, 20, 22, 40, 48,
// 80, 96; rank 24 alone, RL = 24 with one lane per entry, loses 2 %) and loses above (x 1.5 to 1.9 at RL = 32, where 184 to 243
// registers spill).  Below RL = 16 two workgroups fit as the kernel is.
constexpr int vbp_waves_per_simd(int R) { return R / rank_shares(R) >= 16 && R / rank_shares(R) <= 24 ? 2 : 1; }
static_assert(kProjThreads == 256, "vbp_waves_per_simd() was measured with four waves per workgroup");

template <int R>
__global__ __launch_bounds__(kProjThreads, vbp_waves_per_simd(R)) void k_vb_project(const VbProjectArgs A)
{
    constexpr int SP = rank_shares(R), RL = R / SP, EPP = proj_pass_entries(R);
    __shared__ double s_h[R], s_hl[R], s_cew[R], s_beh[R], s_lbeh[R], s_eh[R], s_dh[R], s_c[R], s_u[R], s_red[4 * R], s_misc[8];
    __shared__ unsigned int s_ticket;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slot = t / SP, sub = t - slot * SP;
    const int r = A.r;
    const double ab = A.ah / A.bh;
    double psi_a, lg_a;
    dev_psi_lgamma(A.ah, &psi_a, &lg_a);
    const double lga = -lg_a + A.ah * log(ab);               // :94  - lgamma(ah) + ah log(ah/bh)

    if (t < R) {
        const double c = A.cew[t];
        const double be = 1.0 / (ab + c);                    // :80
        s_cew[t] = c;
        s_beh[t] = be;
        s_lbeh[t] = log(be);
    }
    for (;;) {
        if (t == 0) s_ticket = atomicAdd(A.ticket, 1u);
        __syncthreads();
        const int64_t j = (int64_t)s_ticket;
        if (j >= A.ncell) break;                             // (block-uniform)
        const int64_t p0 = A.colptr[j] - A.base;
        const int len = (int)(A.colptr[j + 1] - A.colptr[j]);
        if (t < R) {
            const double h = A.LH[(size_t)j * R + t];
            s_h[t] = h;
            s_hl[t] = t < r ? h * vbp_log(h) : 0.0;
            s_eh[t] = 0.0; s_dh[t] = 0.0;
        }
        __syncthreads();

        double acc[RL], data, xl;
        // One pass over the cell with the lh in s_h: acc = this slot's share of sum_i lw_ik x_i / lambda_i, data = its share of
        // sum_i x_i [(..)/lambda_i - log lambda_i], xl (first pass) = its share of sum_i lgamma(x_i + 1).
        auto pass = [&](bool first) {
#pragma unroll
            for (int c = 0; c < RL; c++) acc[c] = 0.0;
            data = 0.0; xl = 0.0;
            for (int e0 = 0; e0 < len; e0 += EPP) {          // (the trip count is the block's: the shuffles below see whole waves)
                const int e = e0 + slot;
                const bool live = e < len;
                double w[RL], x = 0.0, p = 0.0, g = 0.0;
                if (live) {
                    const double *rowp = A.T + (size_t)A.row[p0 + e] * (2 * R) + sub * RL;
                    x = A.val[p0 + e];
#pragma unroll
                    for (int c = 0; c < RL; c++) w[c] = rowp[c];
#pragma unroll
                    for (int c = 0; c < RL; c++) p += w[c] * s_h[sub * RL + c];
#pragma unroll
                    for (int c = 0; c < RL; c++) g += rowp[R + c] * s_h[sub * RL + c] + w[c] * s_hl[sub * RL + c];
                }
#pragma unroll
                for (int off = 1; off < SP; off <<= 1) { p += __shfl_xor(p, off); g += __shfl_xor(g, off); }   // the same bits in the SP lanes
                if (live) {
                    const double q = x / p;
                    if (sub == 0) {
                        data += x * (g / p - vbp_log(p));
                        if (first) {
                            double ps, lg;
                            dev_psi_lgamma(x + 1.0, &ps, &lg);
                            xl += lg;
                        }
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
        const double lgx = ((s_misc[4] + s_misc[5]) + s_misc[6]) + s_misc[7];
        double lk0 = 0.0, ev = 0.0;
        int it = 0, reason = 0;
        while (it < A.max_it) {
            it++;
            if (t < R) {
                double lh = 0.0, hl = 0.0, eh = 0.0, dh = 0.0, cc = 0.0, u = 0.0;
                if (t < r) {
                    const double s = ((s_red[t] + s_red[R + t]) + s_red[2 * R + t]) + s_red[3 * R + t];
                    const double be = s_beh[t];
                    const double al = A.ah + s_h[t] * s;     // :73, :79
                    eh = al * be;                            // :81
                    dh = al * (be * be);                     // :103
                    double psi, lgam;
                    dev_psi_lgamma(al, &psi, &lgam);
                    if (!(al > 0.0)) { psi = __builtin_nan(""); lgam = __builtin_nan(""); }
                    lh = exp(psi) * be;                      // :84
                    if (lh < A.fudge) lh = A.fudge;          // :87
                    hl = lh * vbp_log(lh);
                    cc = s_cew[t] * eh;                      // the cell's column of ew %*% eh, :90
                    u = -ab * eh + lga + al * (1.0 + s_lbeh[t]) + lgam;      // :94-95
                }
                s_h[t] = lh; s_hl[t] = hl; s_eh[t] = eh; s_dh[t] = dh; s_c[t] = cc; s_u[t] = u;
            }
            __syncthreads();
            double cross = 0.0, u3 = 0.0;
            for (int k = 0; k < r; k++) { cross += s_c[k]; u3 += s_u[k]; }
            pass(false);
            publish(false);
            const double dsum = ((s_misc[0] + s_misc[1]) + s_misc[2]) + s_misc[3];
            ev = ((-cross - lgx) - dsum) + u3;               // :90-91 and :94-95 of this column
            if (ev != ev) reason = 3;                                            // :345
            else if (it > 1 && fabs(1.0 - ev / lk0) < A.tol) reason = 1;         // :346-347 without `lkh >= lk0`
            else { lk0 = ev; if (it >= A.max_it) reason = 4; }                   // :348
            if (reason) break;                               // (every thread holds the same ev)
        }
        if (t < R) {
            A.LH[(size_t)j * R + t] = s_h[t];
            A.EH[(size_t)j * R + t] = s_eh[t];
            A.DH[(size_t)j * R + t] = s_dh[t];
        }
        if (t == 0) { A.ev[j] = ev; A.it[j] = it; A.reason[j] = reason; }
        __syncthreads();                                     // the LDS rows and the ticket are free for the next cell
    }
}

// ---- the coupled form: the H half of vb_iterate with q(W) held, the hyper-parameters of H re-estimated on the cells of the
// call (R/bayesian.R:342-344, hyper_update :2-53 with hyper.update = (F, F, fa, fb)) and ONE stop for all cells.
//
// Once ah or bh moves with mean(eh) and mean(log lh) over all cells, every step of every cell waits for a sum over all of
// them, so "one launch takes a cell to its stop" no longer applies.  The loop is cut at that dependency into launches:
//   k_vbp_step<R>   one iteration of every cell under the (ah, bh) of the control block: the step of k_vb_project above,
//                   statement for statement and sum for sum, so with both flags off a cell's bits are that kernel's;
//   k_vbp_control   one workgroup: the totals over the cells in a fixed order, hyper_update (dev_hyper_update_pair, as
//                   the engine's device loop), the stopping rule in the reference's order (:342-348), a history row.
// A launch boundary is the only thing that orders a step and its reduction: no grid-wide barrier, no cooperative launch,
// no workgroup waits for another.  The host queues (step, control) pairs ahead and looks at the control block now and then;
// every kernel queued behind a raised `stop` returns at once without a write, so the state is that of the stopping step.
//
// What a cell carries between launches: lh, the sums S_k = sum_i lw_ik x_i / lambda_i its last pass left (the four waves'
// rows already added, in the order k_vb_project adds them) and sum_i lgamma(x_i + 1) of its first pass.  A step is then
// "update from S, one pass at the new lh": that pass yields this step's evidence term and the next step's S.  The launch
// that finds it = 0 in the control block makes the first pass, with the start lh, itself.
//
// Stop, after the hyper-update: 5 the hyper-parameter update failed to converge or took a non-finite step (ah, bh keep
// their values); 3 E is NaN; 1 it > 1, it > n0 and abs(1 - E / lk0) < tol; 4 max_it.  `lkh >= lk0` is left out as above.
struct VbpCtl {
    double hyper[4];               // (aw, bw: unused, 1), ah, bh -- the layout dev_hyper_update_pair works on
    double lk0, E, tol;
    double stats[2];               // mean(log lh), mean(eh) of the last step
    int32_t it, stop, reason;      // reason: 1 converged, 3 NaN evidence, 4 max_it, 5 hyper-parameter update failed
    int32_t max_it, n0, dn;
    int32_t flags[4];              // 0, 0, fa, fb
    unsigned int ticket;           // the step kernel's cell counter: zero at every launch of it (k_vbp_control zeroes it)
};

struct VbpStepArgs {
    const int64_t *colptr;         // as VbProjectArgs
    int64_t base;
    const int32_t *row;
    const double *val;
    const double *T;
    const double *cew;
    double *LH;                    // [ncell][R] in: the start / the last step's lh, out: lh
    double *EH, *DH;               // [ncell][R] out
    double *S;                     // [ncell][R] carried: sum_i lw_ik x_i / lambda_i at LH
    double *lgx;                   // [ncell] carried: sum_i lgamma(x_i + 1)
    double *ev, *seh, *sll;        // [ncell] out: ev_j, sum_k eh_kj, sum_k log lh_kj (k < r ascending)
    VbpCtl *ctl;
    int64_t ncell;
    int32_t r;
    double fudge;
};

template <int R>
__global__ __launch_bounds__(kProjThreads, vbp_waves_per_simd(R)) void k_vbp_step(const VbpStepArgs A)
{
    constexpr int SP = rank_shares(R), RL = R / SP, EPP = proj_pass_entries(R);
    __shared__ double s_h[R], s_hl[R], s_ll[R], s_cew[R], s_beh[R], s_lbeh[R], s_eh[R], s_dh[R], s_c[R], s_u[R], s_red[4 * R], s_misc[8];
    __shared__ unsigned int s_ticket;
    if (A.ctl->stop) return;                                 // (grid-uniform: written by the control launch before this one)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slot = t / SP, sub = t - slot * SP;
    const int r = A.r;
    const bool first = A.ctl->it == 0;                       // no step made yet: the cells hold their start and no sums
    const double ah = A.ctl->hyper[2], bh = A.ctl->hyper[3];
    const double ab = ah / bh;
    double psi_a, lg_a;
    dev_psi_lgamma(ah, &psi_a, &lg_a);
    const double lga = -lg_a + ah * log(ab);                 // :94  - lgamma(ah) + ah log(ah/bh)

    if (t < R) {
        const double c = A.cew[t];
        const double be = 1.0 / (ab + c);                    // :80
        s_cew[t] = c;
        s_beh[t] = be;
        s_lbeh[t] = log(be);
    }
    for (;;) {
        if (t == 0) s_ticket = atomicAdd(&A.ctl->ticket, 1u);
        __syncthreads();
        const int64_t j = (int64_t)s_ticket;
        if (j >= A.ncell) break;                             // (block-uniform)
        const int64_t p0 = A.colptr[j] - A.base;
        const int len = (int)(A.colptr[j + 1] - A.colptr[j]);
        if (t < R) {
            const double h = A.LH[(size_t)j * R + t];
            s_h[t] = h;
            s_hl[t] = first && t < r ? h * vbp_log(h) : 0.0;     // (read by the first pass only: the update below renews it)
        }
        __syncthreads();

        double acc[RL], data, xl;
        // k_vb_project's pass and publish: the same arithmetic in the same order.  Only the loads of an entry's row number and
        // count are issued one trip ahead: here a cell's entries come from memory at every step (no workgroup keeps a cell
        // between launches), and the gather of the next trip would otherwise wait for them.
        auto pass = [&](bool frst) {
#pragma unroll
            for (int c = 0; c < RL; c++) acc[c] = 0.0;
            data = 0.0; xl = 0.0;
            int rown = 0;
            double xn = 0.0;
            if (slot < len) { rown = A.row[p0 + slot]; xn = A.val[p0 + slot]; }
            for (int e0 = 0; e0 < len; e0 += EPP) {          // (the trip count is the block's: the shuffles below see whole waves)
                const int e = e0 + slot;
                const bool live = e < len;
                const int rowe = rown;
                double w[RL], x = xn, p = 0.0, g = 0.0;
                if (e + EPP < len) { rown = A.row[p0 + e + EPP]; xn = A.val[p0 + e + EPP]; }
                if (live) {
                    const double *rowp = A.T + (size_t)rowe * (2 * R) + sub * RL;
#pragma unroll
                    for (int c = 0; c < RL; c++) w[c] = rowp[c];
#pragma unroll
                    for (int c = 0; c < RL; c++) p += w[c] * s_h[sub * RL + c];
#pragma unroll
                    for (int c = 0; c < RL; c++) g += rowp[R + c] * s_h[sub * RL + c] + w[c] * s_hl[sub * RL + c];
                }
#pragma unroll
                for (int off = 1; off < SP; off <<= 1) { p += __shfl_xor(p, off); g += __shfl_xor(g, off); }   // the same bits in the SP lanes
                if (live) {
                    const double q = x / p;
                    if (sub == 0) {
                        data += x * (g / p - vbp_log(p));
                        if (frst) {
                            double ps, lg;
                            dev_psi_lgamma(x + 1.0, &ps, &lg);
                            xl += lg;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < RL; c++) acc[c] += w[c] * q;
                }
            }
        };
        auto publish = [&](bool frst) {
#pragma unroll
            for (int c = 0; c < RL; c++) {
                double v = acc[c];
#pragma unroll
                for (int off = SP; off < 64; off <<= 1) v += __shfl_xor(v, off);
                if (lane < SP) s_red[wave * R + sub * RL + c] = v;
            }
#pragma unroll
            for (int off = SP; off < 64; off <<= 1) { data += __shfl_xor(data, off); xl += __shfl_xor(xl, off); }
            if (lane == 0) { s_misc[wave] = data; if (frst) s_misc[4 + wave] = xl; }
            __syncthreads();
        };

        double lgx;
        if (first) {
            pass(true);
            publish(true);
            lgx = ((s_misc[4] + s_misc[5]) + s_misc[6]) + s_misc[7];
        } else {
            lgx = A.lgx[j];
        }
        if (t < R) {
            double lh = 0.0, hl = 0.0, ll = 0.0, eh = 0.0, dh = 0.0, cc = 0.0, u = 0.0;
            if (t < r) {
                const double s = first ? ((s_red[t] + s_red[R + t]) + s_red[2 * R + t]) + s_red[3 * R + t] : A.S[(size_t)j * R + t];
                const double be = s_beh[t];
                const double al = ah + s_h[t] * s;           // :73, :79
                eh = al * be;                                // :81
                dh = al * (be * be);                         // :103
                double psi, lgam;
                dev_psi_lgamma(al, &psi, &lgam);
                if (!(al > 0.0)) { psi = __builtin_nan(""); lgam = __builtin_nan(""); }
                lh = exp(psi) * be;                          // :84
                if (lh < A.fudge) lh = A.fudge;              // :87
                ll = vbp_log(lh);
                hl = lh * ll;
                cc = s_cew[t] * eh;                          // the cell's column of ew %*% eh, :90
                u = -ab * eh + lga + al * (1.0 + s_lbeh[t]) + lgam;      // :94-95
            }
            s_h[t] = lh; s_hl[t] = hl; s_ll[t] = ll; s_eh[t] = eh; s_dh[t] = dh; s_c[t] = cc; s_u[t] = u;
        }
        __syncthreads();
        double cross = 0.0, u3 = 0.0;
        for (int k = 0; k < r; k++) { cross += s_c[k]; u3 += s_u[k]; }
        pass(false);
        publish(false);
        const double dsum = ((s_misc[0] + s_misc[1]) + s_misc[2]) + s_misc[3];
        const double ev = ((-cross - lgx) - dsum) + u3;      // :90-91 and :94-95 of this column
        if (t < R) {
            A.LH[(size_t)j * R + t] = s_h[t];
            A.EH[(size_t)j * R + t] = s_eh[t];
            A.DH[(size_t)j * R + t] = s_dh[t];
            A.S[(size_t)j * R + t] = ((s_red[t] + s_red[R + t]) + s_red[2 * R + t]) + s_red[3 * R + t];
        }
        if (t == 0) {
            double seh = 0.0, sll = 0.0;                     // what hyper_update's means are made of (:9, :11)
            for (int k = 0; k < r; k++) { seh += s_eh[k]; sll += s_ll[k]; }
            A.ev[j] = ev; A.seh[j] = seh; A.sll[j] = sll;
            if (first) A.lgx[j] = lgx;
        }
        __syncthreads();                                     // the LDS rows and the ticket are free for the next cell
    }
}

// The control step behind every k_vbp_step: thread t adds cells t, t + 1024, .. in ascending order, then block_sum's fixed
// tree -- the totals depend on the number of cells only, not on the step kernel's grid.  Lanes 0 and 1 go on with
// hyper_update (the two lanes dev_hyper_update_pair wants; lane 0's side, aw, has its flag off) and lane 0 with the stop.
// history row it - 1 = [E, mean(log lh), mean(eh), ah, bh after the update], while it <= history_rows.
__global__ __launch_bounds__(1024) void k_vbp_control(const double *__restrict__ ev, const double *__restrict__ seh,
                                                      const double *__restrict__ sll, int64_t ncell, int r, VbpCtl *ctl,
                                                      double *__restrict__ history, int64_t history_rows)
{
    __shared__ double sm[1024];
    if (ctl->stop) return;
    double pe = 0.0, ph = 0.0, pl = 0.0;
    for (int64_t q = threadIdx.x; q < ncell; q += 1024) { pe += ev[q]; ph += seh[q]; pl += sll[q]; }
    const double E = block_sum(pe, sm);
    const double sh = block_sum(ph, sm);
    const double sl = block_sum(pl, sm);
    const int lane = threadIdx.x;
    if (lane > 1) return;
    const double cnt = (double)r * (double)ncell;
    double st[4] = {0.0, sl / cnt, 1.0, sh / cnt};           // mean log lw (unused), mean log lh, mean ew (unused), mean eh
    const int it = ctl->it + 1;
    int reason = 0;
    if (it > ctl->n0 && it % ctl->dn == 0) {                                         // :342
        if (dev_hyper_update_pair(ctl->flags, st, ctl->hyper, lane)) reason = 5;     // :343-344
    }
    if (lane != 0) return;
    if (!reason) {
        if (E != E) reason = 3;                                                      // :345
        else if (it > 1 && it > ctl->n0 && fabs(1.0 - E / ctl->lk0) < ctl->tol) reason = 1;   // :346-347 without `lkh >= lk0`
        else { ctl->lk0 = E; if (it >= ctl->max_it) reason = 4; }                    // :348
    }
    ctl->it = it; ctl->E = E; ctl->stats[0] = st[1]; ctl->stats[1] = st[3];
    ctl->ticket = 0u;
    if (history && it <= history_rows) {
        double *h = history + (size_t)(it - 1) * 5;
        h[0] = E; h[1] = st[1]; h[2] = st[3]; h[3] = ctl->hyper[2]; h[4] = ctl->hyper[3];
    }
    if (reason) { ctl->reason = reason; ctl->stop = 1; }
}

}  // namespace vbnmf
