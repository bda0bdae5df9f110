// mlnmf.h -- gfx950 kernels of the maximum-likelihood NMF step (included once, by mlnmf.hip).
//
// Reference: R/factorize.R:2-27 (nmf_updateR) and :40-49 (likelihood), behind factorize() (:140-320).
//   :8-15   h <- h .* (t(w) %*% (x / (w %*% h))) / colSums(w)   [+ Gamma prior: up + a - 1, down + a/b] ; clip at eps
//   :17-24  w <- w .* ((x / (w %*% h_new)) %*% t(h_new)) / rowSums(h_new)                               ; clip at eps
//   :40-49  lk = ( sum(x log(wh) - wh) + sum_{x>0}(-x log x + x) ) / n / m    on the NEW w, h
// The two updates are sequential (the W update sees the new h), so a step makes two single-side sweeps over
// X (k_sweep1 in kernels.h, same tiled layout and per-task partials as the VB sweep):
//   k_ml_update(H) -> k_sweep1(gene side: w, h_new) -> k_ml_update(W) -> k_sweep1(cell side: h_new, w_new) -> k_ml_final
// The cell-side sweep at the END of step t runs on (w_new, h_new): it yields the statistics the H update of
// step t+1 starts from AND sum x log(wh) of step t's likelihood; sum(wh) = sum_k colSum(w)_k rowSum(h)_k comes
// from the updates' block partials, and sum_{x>0}(-x log x + x) is a constant of X computed once at ingestion.
// Cells partitioned over several engines (W replicated, partition p holding its columns of h): the same kernels around two exchanges,
//   k_ml_update(H) -> k_sweep1(gene) -> k_pack_tail -> ALL-REDUCE [statistics n*R | rowSums(h_new)] -> k_ml_update(W, dense form)
//   -> k_sweep1(cell) -> k_tail_data -> ALL-REDUCE [sum x log(wh) | constant] -> k_ml_control / k_ml_final on the reduced values
// (criterion = 'connectivity': k_ml_tail_conn in k_tail_data's place, and the second all-reduce is [. | . | label table (r+1)^2])
// (mlnmf.hip: queue_ml_step; host-stepped: vbnmf_engine_ml_step_local / ml_step_finish).
#pragma once
#include "kernels.h"

namespace vbnmf {

// One factor's multiplicative update.  Thread (row_sub, k) walks its block's majors with a fixed k:
//   s    = sum of the major's task partials (fixed order)          = (t(w) %*% (x/wh))[k, major] or its W twin
//   up   = f * s [+ a - 1] ; down = colsum_other[k] [+ a/b] ; f <- max(up / down, eps)   (NaN stays NaN, as in R)
// other_bp[other_nb][R+2] are the OTHER factor's block partials of its column sums; this factor's go to bp.
// The control step of the device-driven ML loop (k_ml_control below) folded into the H update of the NEXT step, exactly as
// the VB loop folds its own into the gene-side update (kernels.h: ControlFold): every block forms it from the same
// inputs, block 0 writes it out, and what a block reads is never written in the same launch (the control block and the
// table of H-side block partials alternate between two buffers by step parity).
//
// criterion = 'connectivity' (R/factorize.R:198-208; MlConn, ids_out set): the H update of step t also forms the labels of
// its h_new -- which.max(h_new[, j]), k_argmax's rules, from the values its threads have just written -- and adds every
// cell to entry [label of step t-1][label of step t] of an (r+1) x (r+1) table (integer atomics: no order in the result).
// The control step of step t (in the NEXT launch of this kernel, or k_ml_control) reads the finished table:
//   nchange = pairs(rows) + pairs(cols) - 2 pairs(cells)   (k_label_pairs' arithmetic, below);  it == 1: m (m - 1) / 2
//   zstep   = nchange == 0 ? zstep + 1 : 0 ;  stop (reason 2) at zstep == ncnn_step, else (reason 4) at max_it
// Nothing is read and written in one launch: labels alternate between two arrays by step parity, tables rotate among four
// -- step t fills table t & 3, its control reads (t - 1) & 3, and it zeroes (t + 1) & 3 for the next step; a period of
// four (three would do for one engine) keeps the batch's pre-built argument blocks, which also alternate by parity, at four.
constexpr int kConnLdsTable = 33 * 33;     // counters of a block's own table in LDS: ranks up to 32
struct MlConn {
    int32_t *ids_out;                      // [nmaj] labels of this step's h_new, 1-based, 0 = all NaN (null: the rule is off)
    const int32_t *ids_prev;               // the previous step's (null at step 1: nothing to count against)
    unsigned long long *tab_add;           // the table this step fills (zero as the launch starts)
    unsigned long long *tab_zero;          // the table the next step fills
    const unsigned long long *tab_read;    // the table the previous step filled, for the control step
    int64_t *changes;                      // [max_it] nchange of every step, device-visible host memory (or null)
    int64_t npair;                         // m (m - 1) / 2
};

// pairs(rows) + pairs(cols) - 2 pairs(cells) of an (r+1) x (r+1) contingency table by the whole block, into *s_out (LDS),
// complete behind the closing barrier.  64-bit integers throughout; the threads' shares wrap, their total is the count.
// T = double: the table summed over the partitions of a cell-partitioned engine (k_ml_tail_conn below) -- every entry a cell
// count <= m_global < 2^53, so its double and the all-reduce's sum of such doubles are exact in any order, and the conversion
// back at the load gives every partition the integers of the whole matrix.
template <class T>
__device__ __forceinline__ void block_label_changes(const T *__restrict__ tab, int r, unsigned long long *s_out, int nthreads)
{
    const int t = threadIdx.x, q = r + 1;
    if (t == 0) *s_out = 0ull;
    __syncthreads();
    auto pairs = [](unsigned long long c) { return c * (c - (c > 0 ? 1ull : 0ull)) / 2ull; };
    auto at = [&](size_t i) { return (unsigned long long)tab[i]; };
    unsigned long long acc = 0ull;
    for (int i = t; i < q * q; i += nthreads) acc -= 2ull * pairs(at(i));
    for (int a = t; a < q; a += nthreads) {
        unsigned long long rs = 0ull, cs = 0ull;
        for (int b = 0; b < q; b++) { rs += at((size_t)a * q + b); cs += at((size_t)b * q + a); }
        acc += pairs(rs) + pairs(cs);
    }
    if (acc) atomicAdd(s_out, acc);
    __syncthreads();
}

// The rule itself, for the thread that writes the control block: -> reason (0: go on), zstep updated.
__device__ __forceinline__ int conn_decide(const MlConn &cn, int it, int max_it, int ncnn_step, unsigned long long counted, int &zstep,
                                           bool write)
{
    const int64_t nchange = it == 1 ? cn.npair : (int64_t)counted;         // :200
    zstep = nchange == 0 ? zstep + 1 : 0;                                  // :206-207
    if (write && cn.changes) cn.changes[it - 1] = nchange;
    if (zstep == ncnn_step) return 2;                                      // :208
    return it >= max_it ? 4 : 0;
}

// Likelihood (R/factorize.R:40-49) from colSums(w), rowSums(h) (sW, sH), data = sum x log(wh) and the constant xlx of X;
// cross = sum(wh).
__device__ __forceinline__ double ml_likelihood(const double *sW, const double *sH, double data, double xlx, int r, double n,
                                                double m, double &cross)
{
    cross = 0.0;
    for (int k = 0; k < r; k++) cross += sW[k] * sH[k];
    return ((data - cross) + xlx) / n / m;
}

// The control step of factorize()'s loop (R/factorize.R:194-213), by the thread that writes the control block, from the
// block as the previous step left it (read only): the likelihood, it <- it + 1, then under criterion = 'connectivity' the
// labels' rule (conn_decide; counted: the changed pairs, read only then; write: this thread records them) and under
// 'likelihood' `if (abs(lkold - lk0) < Tol * abs(lkold)) break ; lkold <- lk0` (:211-213; lkold starts at -Inf, so the
// first pass never breaks; a NaN likelihood never satisfies the test either).  Returns the reason (0: go on); lk, it,
// lk0 (lkold), zstep: the block's new values.
__device__ __forceinline__ int ml_control_step(const LoopCtl *pv, const double *sW, const double *sH, double data, double xlx, int r,
                                               double n, double m, const MlConn &cn, const unsigned long long *counted, bool write,
                                               double &lk, int &it, double &lk0, int &zstep)
{
    double cross;
    lk = ml_likelihood(sW, sH, data, xlx, r, n, m, cross);
    it = pv->it + 1;
    const double lkold = pv->lk0;
    lk0 = lkold; zstep = pv->zstep;
    if (cn.ids_out) { lk0 = lk; return conn_decide(cn, it, pv->max_it, pv->ncnn_step, *counted, zstep, write); }
    if (fabs(lkold - lk) < pv->tol * fabs(lkold)) return 2;               // converged (:211)
    lk0 = lk;
    return it >= pv->max_it ? 4 : 0;
}

struct MlFold {
    const LoopCtl *prev;           // null: no fold
    LoopCtl *next;
    const double *bpH_prev;        // [nb][R+2] block partials of the previous step's H update
    const double *epart;           // the previous cell-side sweep's sum x log(wh) partials
    int64_t nepart;
    double xlx, n, m;
    double *history, *out_host;
    int32_t do_control, control_only;
    MlConn cn;                     // criterion = 'connectivity' (also without a fold: prev null, cn.ids_out set)
};

template <int R>
__device__ __forceinline__ void ml_update_body(
    const double *__restrict__ part, const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_task,
    int64_t nmaj, int r, const double *__restrict__ other_bp, int other_nb, int prior, double ga, double gb, double eps,
    double *__restrict__ f, double *__restrict__ bp, const int32_t *__restrict__ stop, const MlFold &fold, int stage_ids)
{
    constexpr int RB = kUpdateThreads / R;       // majors per pass
    // Static LDS of every instantiation, the likelihood rule's and the W side's included: s_other, sH, s_e, the staged ids and
    // pointers, the connectivity rule's s_tab and s_nch, s_stop.  80 180 B at R = 128: 1 740 B short of the 80 KB up to which
    // two blocks share a CU's 160 KB -- a further buffer must fit into that, or alias one of these.
    static_assert(sizeof(double) * (2 * (R + 2) + kUpdateThreads) + sizeof(uint32_t) * (kStageIds + kStagePtr + kConnLdsTable) + 16
                      <= 80 * 1024, "k_ml_update: two blocks no longer fit a CU's LDS");
    __shared__ double s_other[R + 2];
    __shared__ double s_e[kUpdateThreads];
    __shared__ uint32_t s_ids[kStageIds];
    __shared__ int32_t s_ptr[kStagePtr];
    const int t = threadIdx.x;
    // Cell-partitioned engines, W side (the twin of k_update's dense form, kernels.h): `part` holds the statistics already summed
    // over a gene's tasks AND over the partitions -- the reduce buffer behind the all-reduce, [nmaj][R] -- and other_bp is ONE
    // row, its reduced tail rowSums(h_new) of all cells.  No inverse index: nothing to stage, no further LDS.
    const bool dense = row_ptr == nullptr;               // (uniform over the launch)
    // the block's stretch of the inverse index into LDS, first thing (kernels.h: stage_block_ids)
    const int64_t per0 = (nmaj + gridDim.x - 1) / gridDim.x;
    const int64_t bm0 = (int64_t)blockIdx.x * per0, bm1 = min(nmaj, bm0 + per0);
    int q_lo = 0;
    const bool staged = stage_ids && !dense && !fold.control_only && stage_block_ids(row_ptr, row_task, bm0, bm1, s_ids, s_ptr, q_lo);
    if (fold.prev) {
        // ---- the folded control step (ml_control_step, from prev to next) ----
        __shared__ double sH[R + 2];
        __shared__ int s_stop;
        const LoopCtl *pv = fold.prev;
        const int was_stopped = pv->stop;
        double pe = 0.0;
        if (fold.do_control) for (int64_t q = t; q < fold.nepart; q += kUpdateThreads) pe += fold.epart[q];
        bp_colsums2(other_bp, fold.bpH_prev, other_nb, R + 2, s_other, sH, kUpdateThreads);   // colSums(w) (this update's `down`), colSums(h)
        if (was_stopped) {                       // a step queued past the stop: everything travels on unchanged
            if (blockIdx.x == 0 && t == 0) *fold.next = *pv;
            if (!fold.control_only) carry_bp_row<R>(bp, fold.bpH_prev);
            return;
        }
        __shared__ unsigned long long s_nch;
        const bool conn = fold.cn.ids_out != nullptr;        // (uniform over the launch)
        if (conn && fold.do_control) block_label_changes(fold.cn.tab_read, r, &s_nch, kUpdateThreads);
        const double data = block_sum(pe, s_e);
        if (t == 0) {
            int reason = 0, it = pv->it, zstep = pv->zstep;
            double lk = pv->lkh, new_lk0 = pv->lk0;
            if (fold.do_control)
                reason = ml_control_step(pv, s_other, sH, data, fold.xlx, r, fold.n, fold.m, fold.cn, &s_nch, blockIdx.x == 0,
                                         lk, it, new_lk0, zstep);
            s_stop = reason != 0;
            if (blockIdx.x == 0) {
                LoopCtl nx = *pv;
                nx.it = it; nx.lkh = lk; nx.lk0 = new_lk0; nx.zstep = zstep;
                if (reason) { nx.reason = reason; nx.stop = 1; }
                *fold.next = nx;
                if (fold.do_control) {
                    if (fold.history) fold.history[it - 1] = lk;
                    publish_control_step(fold.out_host, lk, nullptr, nullptr, new_lk0, it, reason);
                }
            }
        }
        __syncthreads();
        if (fold.control_only) return;
        if (s_stop) {
            carry_bp_row<R>(bp, fold.bpH_prev);
            return;
        }
    } else {
    const int stopped = stop ? *stop : 0;        // device-driven loop: the run has ended, leave the factors as they are
    bp_colsums(other_bp, other_nb, R + 2, s_other, kUpdateThreads);       // (its loads travel with the flag's)
    if (stopped) return;
    __syncthreads();
    }

    const int row = t / R, k = t - row * R;
    const int64_t per = (nmaj + gridDim.x - 1) / gridDim.x;
    const int64_t m0 = (int64_t)blockIdx.x * per, m1 = min(nmaj, m0 + per);
    double down = s_other[k < R ? k : 0];
    if (prior) down = down + ga / gb;            // R/factorize.R:12,21
    double ve = 0.0;
    if (fold.cn.ids_out) {
        // criterion = 'connectivity': the same update, pass by pass for the whole block, so that the R threads of a major --
        // which straddle a wavefront boundary wherever R does not divide 64 -- can hand their new values over through LDS.
        // Up to rank 32 a block counts its cells in a table of its own in LDS and adds the entries it used to the global one at
        // the end (a block of a large matrix owns hundreds of cells, nearly all on the table's diagonal); the wider ranks'
        // tables go to the global one directly.
        __shared__ unsigned int s_tab[kConnLdsTable];
        const MlConn &cn = fold.cn;
        const int q = r + 1;
        const bool lds_tab = q * q <= kConnLdsTable;
        for (int64_t i = (int64_t)blockIdx.x * kUpdateThreads + t; i < (int64_t)q * q; i += (int64_t)gridDim.x * kUpdateThreads)
            cn.tab_zero[i] = 0ull;
        if (lds_tab) for (int i = t; i < q * q; i += kUpdateThreads) s_tab[i] = 0u;      // (a barrier follows before the first count)
        for (int64_t M0 = m0; M0 < m1; M0 += RB) {
            const int64_t M = M0 + row;
            const bool live = row < RB && M < m1;
            double v = 0.0;
            if (live) {
                const size_t o = (size_t)M * R + k;
                if (k < r) {
                    const double s = staged ? task_sum_lds(part, s_ids, s_ptr[M - bm0] - q_lo, s_ptr[M - bm0 + 1] - q_lo, R, k)
                                   : dense  ? part[o]
                                            : task_sum(part, row_task, row_ptr[M], row_ptr[M + 1], R, k);
                    double up = f[o] * s;
                    if (prior) up = up + ga - 1.0;
                    v = up / down;
                    if (v < eps) v = eps;
                    f[o] = v;
                    ve += v;
                } else {
                    f[o] = 0.0;
                }
            }
            s_e[t] = v;
            __syncthreads();
            if (live && k == 0) {                // which.max(h_new[, M]): first maximum, NaN never wins, 0 if all are NaN (k_argmax)
                int best = 0;
                double bv = 0.0;
                for (int j = 0; j < r; j++) {
                    const double u = s_e[t + j];
                    if (u == u && (best == 0 || u > bv)) { best = j + 1; bv = u; }
                }
                cn.ids_out[M] = best;
                if (cn.ids_prev) {
                    const int cell = cn.ids_prev[M] * q + best;
                    if (lds_tab) atomicAdd(&s_tab[cell], 1u);
                    else atomicAdd(&cn.tab_add[cell], 1ull);
                }
            }
            __syncthreads();
        }
        if (lds_tab && cn.ids_prev)
            for (int i = t; i < q * q; i += kUpdateThreads) {
                const unsigned int c = s_tab[i];
                if (c) atomicAdd(&cn.tab_add[i], (unsigned long long)c);
            }
    } else
    if (row < RB) {
        for (int64_t M = m0 + row; M < m1; M += RB) {
            const size_t o = (size_t)M * R + k;
            if (k < r) {
                const double s = staged ? task_sum_lds(part, s_ids, s_ptr[M - bm0] - q_lo, s_ptr[M - bm0 + 1] - q_lo, R, k)
                               : dense  ? part[o]
                                        : task_sum(part, row_task, row_ptr[M], row_ptr[M + 1], R, k);
                double up = f[o] * s;
                if (prior) up = up + ga - 1.0;   // :11,20
                double v = up / down;
                if (v < eps) v = eps;            // :15,24
                f[o] = v;
                ve += v;
            } else {
                f[o] = 0.0;
            }
        }
    }
    s_e[t] = ve;
    __syncthreads();
    double *const red[1] = {s_e};
    block_rows_sum<R, 1>(red);
    double *o = bp + (size_t)blockIdx.x * (R + 2);
    if (t < R) o[t] = s_e[t];
    if (t == 0) { o[R] = 0.0; o[R + 1] = 0.0; }
}

template <int R>
__global__ __launch_bounds__(kUpdateThreads) void k_ml_update(
    const double *__restrict__ part, const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_task,
    int64_t nmaj, int r, const double *__restrict__ other_bp, int other_nb, int prior, double ga, double gb, double eps,
    double *__restrict__ f, double *__restrict__ bp, const int32_t *__restrict__ stop, const MlFold fold, int stage_ids)
{
    ml_update_body<R>(part, row_ptr, row_task, nmaj, r, other_bp, other_nb, prior, ga, gb, eps, f, bp, stop, fold, stage_ids);
}

// A BATCH of engines stepped by one launch (kernels.h: k_update2_batch; here the restarts of factorize(), reference
// R/factorize.R:181: `for(irun in seq_len(nrun))`): blockIdx.y picks the engine's argument block, the body is the single engine's.
struct MlUpdJob {
    const double *part;
    const int32_t *row_ptr;
    const uint32_t *row_task;
    int64_t nmaj;
    const double *other_bp;
    double *f, *bp;
    const int32_t *stop;
    double ga, gb, eps;
    int32_t r, other_nb, prior, stage_ids;
    MlFold fold;
};

template <int R>
__global__ __launch_bounds__(kUpdateThreads) void k_ml_update_batch(const MlUpdJob *__restrict__ jobs)
{
    const MlUpdJob J = jobs[blockIdx.y];
    ml_update_body<R>(J.part, J.row_ptr, J.row_task, J.nmaj, J.r, J.other_bp, J.other_nb, J.prior, J.ga, J.gb, J.eps, J.f, J.bp, J.stop,
                      J.fold, J.stage_ids);
}

template <int R, bool WIDE, bool LOGTERM, int NT>
__global__ __launch_bounds__(NT) void k_sweep1_batch(const SweepSide *__restrict__ jobs)
{
    extern __shared__ double2 ldsG[];
    const SweepSide S = jobs[blockIdx.y];
    if (S.stop && *S.stop) return;
    sweep_side<R, WIDE, LOGTERM, NT, LOGTERM ? 2 : 0, 1>(S, ldsG);
}

// Likelihood (R/factorize.R:40-49).  One block.  out = [lk, sum x log(wh), sum(wh), 0, 0], out_host[kOutSeq] = seq.
// Cell-partitioned engines (tail != null): rowSums(h), the data term and the constant arrive summed over the partitions --
// tail = [rowSums(h)_k (R) | . | . | sum x log(wh) | sum_{x>0}(-x log x + x)], k_tail's shape behind the all-reduce -- and
// colSums(w) from bpW, which is replicated; m is then the GLOBAL cell count.
template <int R>
__global__ __launch_bounds__(1024) void k_ml_final(const double *__restrict__ bpW, const double *__restrict__ bpH, int nb,
                                                   const double *__restrict__ epart, int64_t nepart, double xlx, int r,
                                                   double n, double m, double seq, double *__restrict__ out,
                                                   double *__restrict__ out_host, const double *__restrict__ tail)
{
    __shared__ double sW[R + 2], sH[R + 2];
    __shared__ double sm[1024];
    double part = 0.0;                           // the three reductions' loads travel together
    if (tail) {
        bp_colsums(bpW, nb, R + 2, sW, 1024);
        if (threadIdx.x < R) sH[threadIdx.x] = tail[threadIdx.x];
        xlx = tail[R + 3];
    } else {
    for (int64_t q = threadIdx.x; q < nepart; q += 1024) part += epart[q];
    bp_colsums2(bpW, bpH, nb, R + 2, sW, sH, 1024);
    }
    double data = block_sum(part, sm);           // (its barriers also publish sW / sH)
    if (tail) data = tail[R + 2];
    if (threadIdx.x == 0) {
        double cross;
        const double lk = ml_likelihood(sW, sH, data, xlx, r, n, m, cross);
        const double st[4] = {data, cross, 0.0, 0.0};
        out[kOutLkh] = lk; out_host[kOutLkh] = lk;
        for (int q = 0; q < 4; q++) { out[kOutStats + q] = st[q]; out_host[kOutStats + q] = st[q]; }
        __threadfence_system();
        reinterpret_cast<volatile double *>(out_host)[kOutSeq] = seq;
    }
}

// Device-driven loop of factorize() (R/factorize.R:194-213): after each step ml_control_step on the control block in place.
// LoopCtl: lk0 holds lkold, lkh the last likelihood.  history[it-1] = lk.  The host's block: publish_control_step.
template <int R>
__global__ __launch_bounds__(1024) void k_ml_control(const double *__restrict__ bpW, const double *__restrict__ bpH, int nb,
                                                     const double *__restrict__ epart, int64_t nepart, double xlx, int r,
                                                     double n, double m, LoopCtl *ctl, double *__restrict__ history,
                                                     double *__restrict__ out_host, const MlConn cn,
                                                     const double *__restrict__ tail, const double *__restrict__ small)
{
    // Cell-partitioned engines (tail != null; as k_control, kernels.h): tail = rowSums(h_new) of ALL cells, the reduced tail of
    // the step's first all-reduce; small = [sum x log(wh) | sum_{x>0}(-x log x + x)] summed over the partitions by the second;
    // colSums(w_new) from bpW, replicated; m is the GLOBAL cell count.  Every partition forms the same decision from the same bits.
    // criterion = 'connectivity' there: the same exchange carries the partitions' label tables, small + 2 = their sum as
    // (r+1)^2 doubles (k_ml_tail_conn); a changed pair may straddle two partitions, so only the summed table counts them.
    __shared__ double sW[R + 2], sH[R + 2];
    __shared__ double sm[1024];
    __shared__ unsigned long long s_nch;
    const int stopped = ctl->stop;               // tested once the reductions' loads are in flight too
    double part = 0.0;
    if (tail) {
        bp_colsums(bpW, nb, R + 2, sW, 1024);
        if (threadIdx.x < R) sH[threadIdx.x] = tail[threadIdx.x];
    } else {
    for (int64_t q = threadIdx.x; q < nepart; q += 1024) part += epart[q];
    bp_colsums2(bpW, bpH, nb, R + 2, sW, sH, 1024);
    }
    if (stopped) return;
    if (cn.ids_out) {                            // criterion = 'connectivity': the table this step's H update filled
        if (tail) block_label_changes(small + 2, r, &s_nch, 1024);
        else block_label_changes(cn.tab_read, r, &s_nch, 1024);
    }
    double data = block_sum(part, sm);           // (its barriers also publish sW / sH)
    if (tail) { data = small[0]; xlx = small[1]; }
    if (threadIdx.x != 0) return;
    double lk, lk0;
    int it, zstep;
    const int reason = ml_control_step(ctl, sW, sH, data, xlx, r, n, m, cn, &s_nch, true, lk, it, lk0, zstep);
    ctl->lk0 = lk0; ctl->zstep = zstep; ctl->it = it; ctl->lkh = lk;      // the control block is updated in place
    if (history) history[it - 1] = lk;
    if (reason) { ctl->reason = reason; ctl->stop = 1; }
    publish_control_step(out_host, lk, nullptr, nullptr, lk0, it, reason);
}

// The second exchange of a cell-partitioned step under criterion = 'connectivity' (one block; k_tail_data's two doubles, kernels.h,
// and behind them the table this step's H update filled, as doubles): out = [sum x log(wh) | sum_{x>0}(-x log x + x) | (r+1)^2
// counts] of THIS partition.  Steps queued past the stop leave `out` as the stopping step wrote it.
__global__ __launch_bounds__(1024) void k_ml_tail_conn(const double *__restrict__ epart, int64_t nepart, double xlx,
                                                       const unsigned long long *__restrict__ tab, int q2,
                                                       double *__restrict__ out, const int32_t *__restrict__ stop)
{
    __shared__ double sm[1024];
    if (stop && *stop) return;
    for (int i = threadIdx.x; i < q2; i += 1024) out[2 + i] = (double)tab[i];
    const double data = block_vec_sum(epart, nepart, sm);
    if (threadIdx.x == 0) { out[0] = data; out[1] = xlx; }
}

// which.max(h[, j])[1] for every cell j (reference R/factorize.R:55-56, R/utils.R:906): 1-based index of the first
// maximum among the r components.  NaN entries never win (R's which.max skips them); a column of NaNs gives 0.
__global__ __launch_bounds__(256) void k_argmax(const double *__restrict__ h, int64_t m, int r, int R, int32_t *__restrict__ ids)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double *row = h + (size_t)j * R;
    int best = 0;
    double bv = 0.0;
    for (int k = 0; k < r; k++) {
        const double v = row[k];
        if (v == v && (best == 0 || v > bv)) { best = k + 1; bv = v; }
    }
    ids[j] = best;
}

// ---------------------------------------------------------------- connectivity change count
// table[old][new] += 1 per cell (integer atomics: order-independent).  ids are 1-based, 0 = no label (all-NaN column).
__global__ __launch_bounds__(256) void k_label_table(const int32_t *__restrict__ ids_old, const int32_t *__restrict__ ids_new,
                                                     int64_t m, int r, unsigned long long *__restrict__ table)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int a = ids_old[j], b = ids_new[j];
    atomicAdd(&table[(size_t)a * (r + 1) + b], 1ull);
}
// pairs together in exactly one of the two labelings = pairs(rows) + pairs(cols) - 2 pairs(cells of the table)
__global__ void k_label_pairs(const unsigned long long *__restrict__ table, int r, unsigned long long *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int q = r + 1;
    auto pairs = [](unsigned long long c) { return c * (c - (c > 0 ? 1ull : 0ull)) / 2ull; };
    unsigned long long both = 0, rows = 0, cols = 0;
    for (int a = 0; a < q; a++) {
        unsigned long long rs = 0;
        for (int b = 0; b < q; b++) { const unsigned long long c = table[(size_t)a * q + b]; rs += c; both += pairs(c); }
        rows += pairs(rs);
    }
    for (int b = 0; b < q; b++) {
        unsigned long long cs = 0;
        for (int a = 0; a < q; a++) cs += table[(size_t)a * q + b];
        cols += pairs(cs);
    }
    out[0] = rows + cols - 2ull * both;
}

}  // namespace vbnmf
