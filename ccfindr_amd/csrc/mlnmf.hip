// mlnmf.hip -- maximum-likelihood NMF on the engine (mlnmf.h; reference R/factorize.R:2-27 nmf_updateR, :40-49 likelihood): two
// single-side sweeps and two multiplicative updates per step, host-stepped, as the device-driven loop of one engine or of the
// partitions of a group under either stopping rule, and as a batch; the arg-max labels of the cells and the count of changed pairs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "comm.h"
#include "engine.h"
#include "loop.h"
#include "mlnmf.h"

using namespace vbnmf;

namespace {

// gene side: lanes own genes (F = w, G = h), statistics for the W update; cell side: F = h, G = w, statistics
// for the H update and sum x log(wh) in the cell half of epart.
int launch_sweep1(vbnmf_engine *e, bool gene_side)
{
    SweepSide a = sweep_side_args(e, gene_side);
    a.logterm = gene_side ? 0 : 1;
    hipEvent_t t0 = gene_side ? e->ev0 : e->ev2, t1 = gene_side ? e->ev1 : e->ev3;
    if (e->timing) { HIPCHECK(hipEventRecord(t0, e->stream)); }
    if (int rc = launch_side_sweep<false>(e, a, !gene_side)) return rc;
    if (e->timing) { HIPCHECK(hipEventRecord(t1, e->stream)); (gene_side ? e->ev_recorded : e->ev2_recorded) = true; }
    return VBNMF_OK;
}

// The W side of a partitioned engine is the dense form (mlnmf.h: ml_update_body): the statistics come summed over tasks and
// partitions from the reduce buffer, `down` = rowSums(h_new) of all cells from its reduced tail (one row of "block partials").
int launch_ml_update(vbnmf_engine *e, bool gene_side, int prior, double ga, double gb, double eps, const MlFold *foldp = nullptr)
{
    const SideView v = side_view(e, gene_side);
    const DeviceSide &S = v.S;
    const int32_t *stop = e->run_active ? (e->stop_ptr ? e->stop_ptr : &e->ctl->stop) : nullptr;
    MlFold fold{};
    if (foldp) fold = *foldp;
    const unsigned grid = fold.control_only ? 1 : (unsigned)e->ub;
    const bool dense = gene_side && e->partitioned;
    const double *redin = e->red_in ? e->red_in : e->red;
    const double *part = dense ? redin : S.part;
    const int32_t *row_ptr = dense ? nullptr : S.row_ptr;
    const uint32_t *row_task = dense ? nullptr : S.row_task;
    const double *other_bp = dense ? redin + (size_t)e->n * e->R : v.other_bp;
    const int other_nb = dense ? 1 : e->ub;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_ml_update<rt()>>(e, dim3(grid), kUpdateThreads, 0, part, row_ptr, row_task, v.nmaj, e->r,
                                                other_bp, other_nb, prior, ga, gb, eps, v.l, v.bp, stop, fold,
                                                stage_ids(S, grid, dense));
    });
}

// partitioned: rowSums(h), the data term and the constant come reduced from the tail of `red` (launch_ml_tail + the exchange)
int launch_ml_final(vbnmf_engine *e)
{
    e->seq += 1.0;
    const double *tail = e->partitioned ? e->red + (size_t)e->n * e->R : nullptr;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_ml_final<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->bpH, e->ub, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx,
                                               e->r, (double)e->n, (double)e->m_global, e->seq, e->d_out, e->h_out_dev, tail);
    });
}

// partitioned engines, host-stepped: the tail of `red` = [rowSums(h)_k of this partition (R) | 0 | 0 | sum x log(wh) | sum_{x>0}(-x log x + x)]
// (k_tail's shape with the ML constant in the last slot), what the exchange in front of ml_state_finish / ml_step_finish carries
// ... and the first exchange of a step is launch_pack_tail's: [gene-side statistics (n*R) | rowSums(h_new) (R) | 0 | 0]
int launch_ml_tail(vbnmf_engine *e)
{
    return launch_tail(e, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx);
}

// The fold of step t (1-based) of an unpartitioned engine's run, as vb_fold of the VB loop: the control step of the previous cell-side sweep, folded into step t's H update (mlnmf.h: MlFold);
// bpH_prev is the table of H-side partials the previous step wrote.
MlFold ml_fold(const vbnmf_engine *e, int t, bool hist, const double *bpH_prev)
{
    MlFold f{};
    f.prev = e->ctl2 + ((t - 1) & 1); f.next = e->ctl2 + (t & 1);
    f.bpH_prev = bpH_prev;
    f.epart = e->epart + e->n_wg; f.nepart = (int64_t)e->n_wg;
    f.xlx = e->xlx; f.n = (double)e->n; f.m = (double)e->m;
    f.history = hist ? e->h_hist_dev : nullptr; f.out_host = e->h_out_dev;
    f.do_control = t > 1 ? 1 : 0;
    return f;
}

// The control block of an ML loop
LoopCtl ml_ctl(double tol, int32_t max_it)
{
    LoopCtl c{};
    c.lk0 = -INFINITY;                                             // lkold <- -Inf (R/factorize.R:193)
    c.tol = tol; c.max_it = max_it;
    return c;
}

// counters of one (r+1) x (r+1) table of the connectivity rule (mlnmf.h: MlConn)
size_t conn_table_count(const vbnmf_engine *e) { return (size_t)(e->r + 1) * (e->r + 1); }

// ... under criterion = 'connectivity' (R/factorize.R:198-208): stop once the labels have stood still for ncnn_step steps
LoopCtl ml_conn_ctl(int32_t max_it, int32_t ncnn_step)
{
    LoopCtl c = ml_ctl(0.0, max_it);
    c.criterion = 1; c.zstep = 0; c.ncnn_step = ncnn_step;                // zstep <- 0 (:194)
    return c;
}

// What that rule needs on an engine beside the ML state: the two label arrays and the four tables ...
int conn_alloc(vbnmf_engine *e)
{
    for (int q = 0; q < 2; q++)
        if (!e->d_ids[q]) { if (int rc = dev_alloc(&e->d_ids[q], (size_t)e->m)) return rc; }
    if (!e->d_ctab) { if (int rc = dev_alloc(&e->d_ctab, 4 * conn_table_count(e))) return rc; }
    return VBNMF_OK;
}

// ... the tables zero as the run starts: queued on the stream the run's launches follow (call it inside the RunScope)
int conn_zero(vbnmf_engine *e)
{
    HIPCHECK(hipMemsetAsync(e->d_ctab, 0, 4 * conn_table_count(e) * sizeof(unsigned long long), e->stream));
    return VBNMF_OK;
}

// Step t's share of them (mlnmf.h: MlConn): labels by parity, tables by t & 3.  The control step of step t reads table t & 3:
// it sits in step t + 1's fold (tab_read), or takes conn_step(t + 1) as a kernel of its own.
MlConn conn_step(const vbnmf_engine *e, int t, bool changes)
{
    const size_t q2 = conn_table_count(e);
    MlConn c{};
    c.ids_out = e->d_ids[t & 1];
    c.ids_prev = t > 1 ? e->d_ids[(t - 1) & 1] : nullptr;
    c.tab_add = e->d_ctab + (size_t)(t & 3) * q2;
    c.tab_zero = e->d_ctab + (size_t)((t + 1) & 3) * q2;
    c.tab_read = e->d_ctab + (size_t)((t - 1) & 3) * q2;
    c.changes = changes ? reinterpret_cast<int64_t *>(e->h_hist_dev + e->chg_off) : nullptr;
    c.npair = e->m_global * (e->m_global - 1) / 2;                 // (pairs of ALL cells: a partition counts against the summed table)
    return c;
}

// After such a run the labels of the last step executed are the engine's "previous labels" (vbnmf_engine_cluster_changes);
// changes: the nchange of every step run, from the pinned block behind the history.
void conn_finish(vbnmf_engine *const *engs, int count, int64_t *changes, int64_t changes_rows)
{
    for (int b = 0; b < count; b++) {
        vbnmf_engine *e = engs[b];
        const int it = (int)e->h_out[kOutIt];
        e->ids_cur = it & 1;
        e->ids_valid = it >= 1;
        if (changes && it > 0) std::memcpy(changes + (size_t)b * changes_rows, e->h_hist + e->chg_off, (size_t)it * sizeof(int64_t));
    }
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- ML-NMF on the same engine
// (reference R/factorize.R:2-27 nmf_updateR, :40-49 likelihood; the factors live in the lw / lh arrays)
int vbnmf_engine_ml_set_state(vbnmf_engine *e, const double *w, const double *h)
{
    if (!e || !w || !h) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = use_device(e)) return rc;
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false; e->ml_ready = false; e->ids_valid = false;
    e->ml_prime_pending = false; e->ml_phase = 0;
    try {
        std::vector<double> tmp;
        to_index_major(w, e->n, e->r, e->R, false, tmp);
        HIPCHECK(hipMemcpyAsync(e->lw, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        to_index_major(h, e->m, e->r, e->R, true, tmp, &e->cell_perm);
        HIPCHECK(hipMemcpyAsync(e->lh, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the state");
    }
    // colSums(w) block partials, then the cell-side statistics the first H update starts from
    if (int rc = launch_prime(e, true, e->lw)) return rc;
    if (int rc = launch_prime(e, false, e->lh)) return rc;       // rowSums(h) block partials, for the likelihood of the loaded pair
    const bool timing = e->timing;
    e->timing = false;                               // the priming sweep is not a step
    int rc = launch_sweep1(e, false);
    e->timing = timing;
    if (rc) return rc;
    if (e->partitioned) {
        // the likelihood of the loaded pair needs rowSums(h), the data term and the constant of ALL cells: this partition's go
        // into the tail of the reduce buffer, the caller sums it over the partitions, vbnmf_engine_ml_state_finish follows
        if ((rc = launch_ml_tail(e))) return rc;
        e->ml_prime_pending = true;
        return VBNMF_OK;
    }
    if ((rc = launch_ml_final(e))) return rc;
    if ((rc = wait_result(e))) return rc;
    e->ml_ready = true;
    return VBNMF_OK;
}

// Partitioned engines: behind the exchange that follows ml_set_state (vbnmf_engine_allreduce, vbnmf_group_ml_state_finish or
// the caller's own sum of the reduce buffer) -- the likelihood of the loaded pair (R/factorize.R:40-49) from the reduced tail.
int vbnmf_engine_ml_state_finish(vbnmf_engine *e)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;
    if (!e->ml_prime_pending) return fail(VBNMF_ERR_STATE, "ml_state_finish without a pending ml_set_state on a partitioned engine");
    if (int rc = launch_ml_final(e)) return rc;
    if (int rc = wait_result(e)) return rc;          // (bounded: a state exchange whose peer never joined sits on this stream)
    e->ml_prime_pending = false;
    e->ml_ready = true;
    return VBNMF_OK;
}

int vbnmf_engine_ml_likelihood(vbnmf_engine *e, double *lk)
{
    if (!e || !lk) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (!e->ml_ready) return fail(VBNMF_ERR_STATE, "ml_likelihood before ml_set_state");
    *lk = e->h_out[kOutLkh];                               // left there by the last k_ml_final (set_state or step)
    return VBNMF_OK;
}

int vbnmf_engine_ml_step(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, double *lk)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (e->partitioned)
        return fail(VBNMF_ERR_STATE, "a partitioned engine needs ml_step_local / all-reduce / ml_step_local / all-reduce / ml_step_finish");
    if (!e->ml_ready) return fail(VBNMF_ERR_STATE, "ml_step before ml_set_state");
    if (e->ml_phase) return fail(VBNMF_ERR_STATE, "ml_step between ml_step_local and ml_step_finish");
    if (int rc = use_device(e)) return rc;
    const double eps = 2.220446049250313e-16;        // .Machine$double.eps (R/factorize.R:15,24)
    if (int rc = launch_ml_update(e, false, prior, gamma_a, gamma_b, eps)) return rc;   // H first (:8-15)
    if (int rc = launch_sweep1(e, true)) return rc;
    if (int rc = launch_ml_update(e, true, prior, gamma_a, gamma_b, eps)) return rc;    // then W on the new h (:17-24)
    if (int rc = launch_sweep1(e, false)) return rc;
    if (int rc = launch_ml_final(e)) return rc;
    if (int rc = wait_result(e)) return rc;
    if (int rc = harvest_timing(e)) return rc;
    if (lk) *lk = e->h_out[kOutLkh];
    return VBNMF_OK;
}

// The host-stepped step of a partitioned engine (reference R/factorize.R:2-27 on this partition's cells, :40-49): two local
// halves, each followed by one exchange of the reduce buffer, then the likelihood.
//   1st ml_step_local : k_ml_update(H) (:8-15)  k_sweep1(gene side: w, h_new)  pack -> red = [gene statistics n*R | rowSums(h_new) R | 0 0 | . .]
//   exchange          : sum over the partitions of red[0 : n*R + R + 2)
//   2nd ml_step_local : k_ml_update(W <- the reduced statistics) (:17-24)  k_sweep1(cell side: h_new, w_new)
//                       tail -> red[n*R ...) = [rowSums(h_new) R | 0 0 | sum x log(wh) | sum_{x>0}(-x log x + x)] of this partition
//   exchange          : sum over the partitions of the tail red[n*R : n*R + R + 4)
//   ml_step_finish    : lk (:40-49) from the reduced tail and the replicated colSums(w_new)
// An unpartitioned engine takes the same calls (nothing is packed and there is nothing to exchange).
int vbnmf_engine_ml_step_local(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;
    if (!e->ml_ready) return fail(VBNMF_ERR_STATE, "ml_step_local before ml_set_state (or before ml_state_finish on a partitioned engine)");
    if (e->ml_phase >= 2) return fail(VBNMF_ERR_STATE, "ml_step_local called a third time without ml_step_finish");
    const double eps = 2.220446049250313e-16;        // .Machine$double.eps (R/factorize.R:15,24)
    if (e->ml_phase == 0) {
        if (int rc = launch_ml_update(e, false, prior, gamma_a, gamma_b, eps)) return rc;   // H first (:8-15)
        if (int rc = launch_sweep1(e, true)) return rc;
        if (e->partitioned) { if (int rc = launch_pack_tail(e, nullptr)) return rc; }
    } else {
        if (int rc = launch_ml_update(e, true, prior, gamma_a, gamma_b, eps)) return rc;    // then W on the new h (:17-24)
        if (int rc = launch_sweep1(e, false)) return rc;
        if (e->partitioned) { if (int rc = launch_ml_tail(e)) return rc; }
    }
    e->ml_phase++;
    return VBNMF_OK;
}

int vbnmf_engine_ml_step_finish(vbnmf_engine *e, double *lk)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;
    if (e->ml_phase != 2) return fail(VBNMF_ERR_STATE, "ml_step_finish without ml_step_local (a step has two, each followed by an exchange)");
    if (int rc = launch_ml_final(e)) return rc;
    if (int rc = wait_result(e)) return rc;
    e->ml_phase = 0;
    if (int rc = harvest_timing(e)) return rc;
    if (lk) *lk = e->h_out[kOutLkh];
    return VBNMF_OK;
}

}  // extern "C"

namespace {

// What a step of the device-driven ML loop is run with (the arguments of vbnmf_engine_ml_run* that do not change over the run).
struct MlStepArgs {
    int32_t prior;
    double ga, gb;
    bool hist, chg, conn;
    int max_it;
};

// k_ml_control as a kernel of its own behind the step (no fold; partitioned engines).  reduced: the inputs come summed over the
// partitions from red_g -- rowSums(h_new) in the tail of the first exchange, [data term | constant] from the second.
int launch_ml_control(vbnmf_engine *e, bool hist, const MlConn &cn, bool reduced)
{
    const size_t nR = (size_t)e->n * e->R;
    const double *tail = reduced ? e->red_g + nR : nullptr;
    const double *small = reduced ? e->red_g + nR + e->R + 2 : nullptr;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_ml_control<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->bpH, e->ub, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx,
                                                 e->r, (double)e->n, (double)e->m_global, e->ctl, hist ? e->h_hist_dev : nullptr,
                                                 e->h_out_dev, cn, tail, small);
    });
}

// One step of the device-driven ML loop (reference R/factorize.R:194-213 around nmf_updateR, :2-27), queued on every engine of the group.
//   unpartitioned : k_ml_update(H, + the control step of the previous cell-side sweep)  k_sweep1(gene)  k_ml_update(W)  k_sweep1(cell)
//   partitioned   : k_ml_update(H)  k_sweep1(gene side: w, h_new)  k_pack_tail | event
//                   -> comm stream: all-reduce [gene statistics n*R | rowSums(h_new) R | 2]        (RCCL, or k_group_sum)
//                   -> main stream: k_ml_update(W <- the reduced statistics)  k_sweep1(cell side: h_new, w_new)  k_tail_data
//                   -> main stream: all-reduce [sum x log(wh) | sum_{x>0}(-x log x + x)]           (two doubles)
//                   -> k_ml_control on the reduced inputs: the same decision on every partition
//   ... under criterion = 'connectivity' (a.conn): each H update also forms its cells' labels and adds them to its engine's own
//                   table t & 3 (MlFold without a fold, as the unfolded unpartitioned path below); k_ml_tail_conn in
//                   k_tail_data's place appends that table as doubles, the second all-reduce is [. | . | table (r+1)^2]
//                   -- a length fixed by the call's arguments, never by device state -- and k_ml_control counts the changed
//                   pairs on the SUM: pairs straddle partitions.  No third collective.
// The W update needs the first exchange, so unlike the VB step nothing runs beside it; it still goes on the comm stream, as
// queue_vb_step's, so that both loops order their collectives the same way.  The all-reduces are out of place (red -> red_g):
// behind the stop every kernel returns at once, `red` keeps what the stopping step packed, and the exchanges queued past the
// stop deliver the same sums again.
int queue_ml_step(const LoopGroup &G, const MlStepArgs &a)
{
    const double eps = 2.220446049250313e-16;        // .Machine$double.eps (R/factorize.R:15,24)
    if (!G.comm) {
        vbnmf_engine *e = G.e[0];
        if (e->fold) {
            // k_ml_update(H, with the control step of the PREVIOUS cell-side sweep folded in)  sweep  k_ml_update(W)  sweep ;
            // behind the last step of the run the control step alone (mlnmf.h: MlFold)
            const int t = ++e->fold_step;
            MlFold f = ml_fold(e, t, a.hist, e->bpH);
            if (a.conn) f.cn = conn_step(e, t, a.chg);
            std::swap(e->bpH, e->bpH_alt);                          // this step's H-side partials go to the other table
            int q = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps, &f);
            e->stop_ptr = &f.next->stop;
            if (!q) q = launch_sweep1(e, true);
            if (!q) q = launch_ml_update(e, true, a.prior, a.ga, a.gb, eps);
            if (!q) q = launch_sweep1(e, false);
            if (!q && t == a.max_it) {
                MlFold g = ml_fold(e, t + 1, a.hist, e->bpH);
                if (a.conn) g.cn = conn_step(e, t + 1, a.chg);
                g.control_only = 1;
                q = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps, &g);
            }
            return q;
        }
        int q;
        MlConn cn{};                                                // (what k_ml_control reads: the table this step fills)
        if (a.conn) {
            const int t = ++e->fold_step;                           // (no fold: only the rule's step counter here)
            MlFold f{};
            f.cn = conn_step(e, t, a.chg);
            cn = conn_step(e, t + 1, a.chg);
            q = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps, &f);
        } else {
            q = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps);
        }
        if (!q) q = launch_sweep1(e, true);
        if (!q) q = launch_ml_update(e, true, a.prior, a.ga, a.gb, eps);
        if (!q) q = launch_sweep1(e, false);
        if (!q) q = launch_ml_control(e, a.hist, cn, false);
        return q;
    }
    vbnmf_comm *c = G.comm;
    const int P = G.count;
    vbnmf_engine *L = G.e[0];                                  // leader: owner of the comm stream used by a local group
    const int64_t nconn = a.conn ? (int64_t)conn_table_count(L) : 0;
    const int64_t nbig = L->n * L->R + L->R + 2, nsmall = 2 + nconn;
    hipEvent_t evA[64], evB[64];
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        int rc;                                                                 // H: this partition's cells, colSums(w) replicated
        if (a.conn) {
            MlFold f{};
            f.cn = conn_step(e, ++e->fold_step, a.chg);                         // (no fold: only the rule's step counter here)
            rc = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps, &f);
        } else {
            rc = launch_ml_update(e, false, a.prior, a.ga, a.gb, eps);
        }
        if (!rc) rc = launch_sweep1(e, true);
        if (!rc) rc = launch_pack_tail(e, &e->ctl->stop);
        if (rc) return rc;
        evA[p] = next_event(e);
        HIPCHECK(hipEventRecord(evA[p], e->stream));
    }
    if (c->kind == 0) {
        HIPCHECK(hipStreamWaitEvent(L->cstream, evA[0], 0));
        if (int rc = rccl_check(rccl_api().AllReduce(L->red, L->red_g, (size_t)nbig, ncclDouble, ncclSum, c->nc, L->cstream), "ncclAllReduce")) return rc;
    } else {
        for (int p = 0; p < P; p++) HIPCHECK(hipStreamWaitEvent(L->cstream, evA[p], 0));
        if (int rc = launch_group_sum(L->cstream, c->d_send_big, c->d_recv_big, P, nbig)) return rc;
    }
    hipEvent_t evBig = next_event(L);
    HIPCHECK(hipEventRecord(evBig, L->cstream));
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        HIPCHECK(hipStreamWaitEvent(e->stream, evBig, 0));
        int rc = launch_ml_update(e, true, a.prior, a.ga, a.gb, eps);           // W <- red_g (e->red_in), on every partition the same bits
        if (!rc) rc = launch_sweep1(e, false);
        if (rc) return rc;
        if (a.conn) {
            hipLaunchKernelGGL(k_ml_tail_conn, dim3(1), dim3(1024), 0, e->stream, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx,
                               conn_step(e, e->fold_step, false).tab_add, (int)nconn, e->red + nbig, &e->ctl->stop);
            HIPCHECK(hipGetLastError());
        } else if ((rc = launch_tail_data(e, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx, e->red + nbig))) return rc;
        if (p > 0) {                                           // (only where another stream waits on it)
            evB[p] = next_event(e);
            HIPCHECK(hipEventRecord(evB[p], e->stream));
        }
    }
    // the second exchange on the leader's main stream, behind the first (queue_vb_step: same order of collectives on every rank)
    hipEvent_t evD = P > 1 ? next_event(L) : nullptr;
    if (c->kind == 0) {
        if (int rc = rccl_check(rccl_api().AllReduce(L->red + nbig, L->red_g + nbig, (size_t)nsmall, ncclDouble, ncclSum, c->nc, L->stream), "ncclAllReduce")) return rc;
    } else {
        for (int p = 1; p < P; p++) HIPCHECK(hipStreamWaitEvent(L->stream, evB[p], 0));
        if (int rc = launch_group_sum_at(L->stream, c->d_send_big, c->d_recv_big, P, nbig, nsmall)) return rc;
    }
    if (evD) HIPCHECK(hipEventRecord(evD, L->stream));
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        if (evD && e->stream != L->stream) HIPCHECK(hipStreamWaitEvent(e->stream, evD, 0));
        // (the rule's control step reads the summed table behind the exchange's two doubles, not cn.tab_read)
        if (int rc = launch_ml_control(e, a.hist && p == 0, a.conn ? conn_step(e, e->fold_step + 1, a.chg) : MlConn{}, true)) return rc;
    }
    return VBNMF_OK;
}

// The device-driven ML loop under either stopping rule (ncnn_step 0: the likelihood's, with tol) of one unpartitioned engine, or
// of the partitions of one factorisation: a local group, or this process's engine with its RCCL communicator.  Under the
// connectivity rule every partition keeps labels and tables of its own cells and writes the per-step counts -- the same on
// all of them -- to its own history block; the caller's come from partition 0.
int ml_run_group(const LoopGroup &G, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol, int32_t ncnn_step,
                 int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows, int64_t *changes)
{
    vbnmf_engine *e = G.e[0];
    const bool conn = ncnn_step > 0;
    for (int p = 0; p < G.count; p++) {
        if (int rc = use_device(G.e[p])) return rc;
        if (!G.e[p]->ml_ready) return fail(VBNMF_ERR_STATE, "ml_run before ml_set_state (or before the state exchange of a partitioned engine)");
        if (G.e[p]->ml_phase) return fail(VBNMF_ERR_STATE, "ml_run between ml_step_local and ml_step_finish");
    }
    if (int rc = use_device(e)) return rc;
    if (history || changes) { if (int rc = ensure_history(e, (size_t)max_it * (changes ? 2 : 1))) return rc; }
    for (int p = 0; p < G.count; p++) {
        vbnmf_engine *x = G.e[p];
        if (changes && p > 0) { if (int rc = ensure_history(x, (size_t)max_it * 2)) return rc; }
        x->chg_off = (size_t)max_it;
        if (conn) { if (int rc = conn_alloc(x)) return rc; }
    }

    const MlStepArgs a{prior, gamma_a, gamma_b, history != nullptr, changes != nullptr, conn, max_it};
    RunScope S{G.e, G.count};
    S.plain_ctl = G.comm != nullptr;                               // partitioned: the control step is a kernel of its own, on e->ctl
    int rc = S.begin([&](int) { return conn ? ml_conn_ctl(max_it, ncnn_step) : ml_ctl(tol, max_it); });
    for (int p = 0; p < G.count && conn && !rc; p++) rc = conn_zero(G.e[p]);
    if (G.comm) for (int p = 0; p < G.count; p++) G.e[p]->red_in = G.e[p]->red_g;      // what the W updates read: the receive side
    if (!rc) rc = drive_loop(G.e, 1, true, max_it, !G.comm && e->fold, [&](int) { return queue_ml_step(G, a); });
    rc = S.end(rc);
    if (G.comm) for (int p = 0; p < G.count; p++) G.e[p]->red_in = nullptr;
    if (rc) return rc;
    for (int p = 1; p < G.count; p++)                              // (replicated decisions: anything else is a broken exchange)
        if (G.e[p]->h_out[kOutIt] != e->h_out[kOutIt] || G.e[p]->h_out[kOutReason] != e->h_out[kOutReason])
            return fail(VBNMF_ERR_STATE, "partition %d ended the loop at step %d (reason %d), partition 0 at step %d (reason %d)", p,
                        (int)G.e[p]->h_out[kOutIt], (int)G.e[p]->h_out[kOutReason], (int)e->h_out[kOutIt], (int)e->h_out[kOutReason]);
    read_out(G.e, 1, it_out, nullptr, lk_out, reason_out, nullptr, history, history_rows, 1);
    if (conn) {
        conn_finish(G.e, 1, changes, max_it);
        conn_finish(G.e + 1, G.count - 1, nullptr, 0);             // (the other partitions: their labels of the last step)
    }
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// Device-driven form of factorize()'s inner loop under criterion = 'likelihood' (reference R/factorize.R:194-213).
int vbnmf_engine_ml_run(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol,
                        int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (max_it < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles");
    LoopGroup G{&e, 1, nullptr};
    if (e->partitioned) {
        if (!e->comm || e->comm->kind != 0)
            return fail(VBNMF_ERR_STATE, "the device-driven ML loop of a partitioned engine needs an RCCL communicator (vbnmf_engine_attach_comm), or vbnmf_group_ml_run for a local group");
        if (int rc = use_device(e)) return rc;
        if (int rc = ensure_comm_resources(e)) return rc;
        G.comm = e->comm;
    }
    return ml_run_group(G, prior, gamma_a, gamma_b, max_it, tol, 0, it_out, lk_out, reason_out, history, history_rows, nullptr);
}

// Local group: the exchange behind ml_set_state on every member (the reduce buffers summed in place, partition order), then
// vbnmf_engine_ml_state_finish on each (the likelihood of the loaded pair, R/factorize.R:40-49).
int vbnmf_group_ml_state_finish(vbnmf_comm *c)
{
    LoopGroup G{};
    if (int rc = group_members(c, G)) return rc;
    if (int rc = use_device(G.e[0])) return rc;
    if (int rc = group_tables(c)) return rc;
    for (int p = 0; p < G.count; p++)
        if (!G.e[p]->ml_prime_pending) return fail(VBNMF_ERR_STATE, "group_ml_state_finish: partition %d has no pending ml_set_state", p);
    if (int rc = group_sum_in_place(G)) return rc;
    for (int p = 0; p < G.count; p++)
        if (int rc = vbnmf_engine_ml_state_finish(G.e[p])) return rc;
    return VBNMF_OK;
}

// Local group: vbnmf_engine_ml_run (R/factorize.R:194-213, criterion = 'likelihood') for the partitions of one factorisation.
int vbnmf_group_ml_run(vbnmf_comm *c, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol,
                       int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows)
{
    if (max_it < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles");
    LoopGroup G{};
    if (int rc = group_members(c, G)) return rc;
    if (int rc = use_device(G.e[0])) return rc;
    if (int rc = group_tables(c)) return rc;
    return ml_run_group(G, prior, gamma_a, gamma_b, max_it, tol, 0, it_out, lk_out, reason_out, history, history_rows, nullptr);
}

// ... under criterion = 'connectivity' (reference R/factorize.R:198-208): the labels which.max(h[, j]) of every step are formed
// by the step's own H update, the count of changed pairs by the control step; stop (reason 2) once it has been 0 for ncnn_step
// steps in a row, else (reason 4) at max_it.  The likelihood is computed and reported as in vbnmf_engine_ml_run and stops nothing.
int vbnmf_engine_ml_run_connectivity(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, int32_t ncnn_step,
                                     int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows,
                                     int64_t *changes, int64_t changes_rows)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (max_it < 1 || ncnn_step < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it and ncnn_step must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles");
    if (changes && changes_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "changes needs max_it counts");
    LoopGroup G{&e, 1, nullptr};
    if (e->partitioned) {                                          // (as vbnmf_engine_ml_run)
        if (!e->comm || e->comm->kind != 0)
            return fail(VBNMF_ERR_STATE, "criterion = 'connectivity' on a partitioned engine needs an RCCL communicator (vbnmf_engine_attach_comm), "
                                         "or vbnmf_group_ml_run_connectivity for a local group");
        if (int rc = use_device(e)) return rc;
        if (int rc = ensure_comm_resources(e)) return rc;
        G.comm = e->comm;
    }
    return ml_run_group(G, prior, gamma_a, gamma_b, max_it, 0.0, ncnn_step, it_out, lk_out, reason_out, history, history_rows, changes);
}

// Local group: the same rule (R/factorize.R:198-208) for the partitions of one factorisation.  A changed pair of cells may lie
// in two partitions, so the partitions' (r+1) x (r+1) label tables are summed -- inside the step's second exchange -- before
// nchange is formed; every partition then takes the same decision.  changes: from partition 0; changes[0] = the pairs of ALL cells.
int vbnmf_group_ml_run_connectivity(vbnmf_comm *c, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, int32_t ncnn_step,
                                    int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows,
                                    int64_t *changes, int64_t changes_rows)
{
    if (max_it < 1 || ncnn_step < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it and ncnn_step must be >= 1");      // (before the handle is read)
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles");
    if (changes && changes_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "changes needs max_it counts");
    LoopGroup G{};
    if (int rc = group_members(c, G)) return rc;
    if (int rc = use_device(G.e[0])) return rc;
    if (int rc = group_tables(c)) return rc;
    return ml_run_group(G, prior, gamma_a, gamma_b, max_it, 0.0, ncnn_step, it_out, lk_out, reason_out, history, history_rows, changes);
}

int vbnmf_engine_ml_get_state(vbnmf_engine *e, double *w, double *h)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!e->ml_ready) return fail(VBNMF_ERR_STATE, "ml_get_state before ml_set_state");
    if (int rc = use_device(e)) return rc;
    HIPCHECK(hipStreamSynchronize(e->stream));
    try {
        std::vector<double> tmp;
        if (w) {
            tmp.resize((size_t)e->n * e->R);
            HIPCHECK(hipMemcpy(tmp.data(), e->lw, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            from_index_major(tmp, e->n, e->r, e->R, false, w);
        }
        if (h) {
            tmp.resize((size_t)e->m * e->R);
            HIPCHECK(hipMemcpy(tmp.data(), e->lh, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            from_index_major(tmp, e->m, e->r, e->R, true, h, &e->cell_perm);
        }
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the state");
    }
    return VBNMF_OK;
}

int vbnmf_engine_cluster_ids(vbnmf_engine *e, int32_t *ids)
{
    if (!e || !ids) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (!e->ml_ready && !e->has_state) return fail(VBNMF_ERR_STATE, "cluster_ids before a state was loaded");
    if (int rc = use_device(e)) return rc;
    const double *h = e->ml_ready ? e->lh : e->eh;   // ML: the coefficient matrix itself; VB: its posterior mean E[H]
    int32_t *d_ids = nullptr;
    if (int rc = dev_alloc(&d_ids, (size_t)e->m)) return rc;
    hipLaunchKernelGGL(k_argmax, dim3((unsigned)((e->m + 255) / 256)), dim3(256), 0, e->stream, h, e->m, e->r, e->R, d_ids);
    hipError_t he = hipGetLastError();
    std::vector<int32_t> stage;
    int32_t *host = ids;
    if (!e->cell_perm.empty()) { stage.resize((size_t)e->m); host = stage.data(); }      // labels arrive in the layout's cell order
    if (he == hipSuccess) he = hipMemcpyAsync(host, d_ids, (size_t)e->m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    dev_free(d_ids);
    if (he != hipSuccess) return fail(VBNMF_ERR_HIP, "cluster_ids failed: %s", hipGetErrorString(he));
    if (!e->cell_perm.empty()) for (int64_t p = 0; p < e->m; p++) ids[e->cell_perm[p]] = stage[p];
    return VBNMF_OK;
}

// The connectivity stopping count of factorize() (reference R/factorize.R:198-208) on the device: the labels of the
// state held now against the labels of the previous call, as sum(cnn != cnn0) over all pairs of cells -- from the
// contingency table of the two labelings, never from the O(m^2) vectors.  changed = -1 on the first call after a
// state was loaded (the reference starts from nchange = npair, :200).  ids (optional): the new labels, m_local int32.
int vbnmf_engine_cluster_changes(vbnmf_engine *e, int64_t *changed, int32_t *ids)
{
    if (!e || !changed) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (!e->ml_ready && !e->has_state) return fail(VBNMF_ERR_STATE, "cluster_changes before a state was loaded");
    if (int rc = use_device(e)) return rc;
    for (int q = 0; q < 2; q++)
        if (!e->d_ids[q]) { if (int rc = dev_alloc(&e->d_ids[q], (size_t)e->m)) return rc; }
    const size_t tcount = (size_t)(e->r + 1) * (e->r + 1) + 1;
    if (!e->d_table) { if (int rc = dev_alloc(&e->d_table, tcount)) return rc; }
    const double *h = e->ml_ready ? e->lh : e->eh;
    const int cur = e->ids_cur ^ 1;
    hipLaunchKernelGGL(k_argmax, dim3((unsigned)((e->m + 255) / 256)), dim3(256), 0, e->stream, h, e->m, e->r, e->R, e->d_ids[cur]);
    HIPCHECK(hipGetLastError());
    unsigned long long n = 0;
    if (e->ids_valid) {
        HIPCHECK(hipMemsetAsync(e->d_table, 0, tcount * sizeof(unsigned long long), e->stream));
        hipLaunchKernelGGL(k_label_table, dim3((unsigned)((e->m + 255) / 256)), dim3(256), 0, e->stream, e->d_ids[cur ^ 1], e->d_ids[cur], e->m, e->r, e->d_table);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(k_label_pairs, dim3(1), dim3(1), 0, e->stream, e->d_table, e->r, e->d_table + (tcount - 1));
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(&n, e->d_table + (tcount - 1), sizeof n, hipMemcpyDeviceToHost, e->stream));
    }
    std::vector<int32_t> stage;
    int32_t *host = ids;
    if (ids && !e->cell_perm.empty()) { stage.resize((size_t)e->m); host = stage.data(); }
    if (ids) HIPCHECK(hipMemcpyAsync(host, e->d_ids[cur], (size_t)e->m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (ids && !e->cell_perm.empty()) for (int64_t p = 0; p < e->m; p++) ids[e->cell_perm[p]] = stage[p];
    *changed = e->ids_valid ? (int64_t)n : -1;
    e->ids_cur = cur;
    e->ids_valid = true;
    return VBNMF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- a batch of engines stepped by one launch (mlnmf.h: k_ml_update_batch)
namespace {

int launch_sweep1_batch(vbnmf_engine *e, const SweepSide *jobs, int B, bool logterm)
{
    return with_batch_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return with_flag(logterm, [&](auto lt) {
                return launch_lds_kernel<k_sweep1_batch<s.R, s.WIDE, lt(), s.NT>>(e, dim3((unsigned)e->n_wg, (unsigned)B), s.NT, jobs);
            });
        });
    });
}

int launch_ml_update_batch(vbnmf_engine *e, const MlUpdJob *jobs, int B)
{
    return with_batch_rank(e->R, [&](auto rt) {
        return launch_kernel<k_ml_update_batch<rt()>>(e, dim3((unsigned)e->ub, (unsigned)B), kUpdateThreads, 0, jobs);
    });
}

// The batch's ML loops under either stopping rule (ncnn_step 0: the likelihood's, with tol); arguments checked by the entries.
int batch_ml_run(vbnmf_engine **engs, int32_t count, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol,
                 int32_t ncnn_step, int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows,
                 int64_t *changes, int64_t changes_rows)
{
    const int B = count;
    const bool conn = ncnn_step > 0, chg = changes != nullptr;
    if (int rc = batch_admit(engs, B, false, (history || chg) ? (size_t)max_it * (chg ? 2 : 1) : 0)) return rc;
    vbnmf_engine *e0 = engs[0];
    const double eps = 2.220446049250313e-16;

    const bool hist = history != nullptr;
    // jobs: the H update's of step 1, of the odd and of the even steps (criterion = 'connectivity': of step 1 and of the steps
    // t & 3 = 0..3, the period of its tables); the W update's and the two sweeps' by parity
    const int NV = conn ? 5 : 3;
    auto variant = [&](int t) { return t == 1 ? 0 : conn ? 1 + (t & 3) : ((t & 1) ? 1 : 2); };
    std::vector<MlUpdJob> jh((size_t)NV * B), jw((size_t)2 * B);
    std::vector<SweepSide> jg((size_t)2 * B), jc((size_t)2 * B);
    for (int b = 0; b < B; b++) {
        vbnmf_engine *e = engs[b];
        double *Ht[2] = {e->bpH, e->bpH_alt};                                    // [0]: the latest table as the run starts
        e->chg_off = (size_t)max_it;
        if (conn) { if (int rc = conn_alloc(e)) return rc; }                     // (the tables are zeroed inside the run's scope)
        for (int v = 0; v < NV; v++) {
            const int t = v == 0 ? 1 : conn ? 4 + (v - 1) : (v == 1 ? 3 : 2);          // a step of that variant
            MlUpdJob &J = jh[(size_t)v * B + b];
            J.part = e->B.part; J.row_ptr = e->B.row_ptr; J.row_task = e->B.row_task; J.nmaj = e->m;
            J.other_bp = e->bpW; J.f = e->lh; J.bp = Ht[t & 1]; J.stop = nullptr;
            J.ga = gamma_a; J.gb = gamma_b; J.eps = eps;
            J.r = e->r; J.other_nb = e->ub; J.prior = prior;
            J.stage_ids = stage_ids(e->B, e->ub);
            J.fold = ml_fold(e, t, hist, Ht[(t - 1) & 1]);
            if (conn) J.fold.cn = conn_step(e, t, chg);
        }
        for (int par = 0; par < 2; par++) {                                      // step t of parity par = t & 1
            const int32_t *stop = &(e->ctl2 + par)->stop;                        // what that step's H update left
            MlUpdJob &J = jw[(size_t)par * B + b];
            J.part = e->A.part; J.row_ptr = e->A.row_ptr; J.row_task = e->A.row_task; J.nmaj = e->n;
            J.other_bp = Ht[par]; J.f = e->lw; J.bp = e->bpW; J.stop = stop;
            J.ga = gamma_a; J.gb = gamma_b; J.eps = eps;
            J.r = e->r; J.other_nb = e->ub; J.prior = prior;
            J.stage_ids = stage_ids(e->A, e->ub);
            J.fold = MlFold{};
            SweepSide g = sweep_side_args(e, true);
            g.logterm = 0;
            SweepSide c = sweep_side_args(e, false);
            c.logterm = 1;
            g.stop = c.stop = stop;
            jg[(size_t)par * B + b] = g; jc[(size_t)par * B + b] = c;
        }
    }
    MlUpdJob *d_jh = nullptr, *d_jw = nullptr;
    SweepSide *d_jg = nullptr, *d_jc = nullptr;
    auto free_jobs = [&] { dev_free(d_jh); dev_free(d_jw); dev_free(d_jg); dev_free(d_jc); };
    int rc = dev_upload(&d_jh, jh);
    if (!rc) rc = dev_upload(&d_jw, jw);
    if (!rc) rc = dev_upload(&d_jg, jg);
    if (!rc) rc = dev_upload(&d_jc, jc);
    if (rc) { free_jobs(); return rc; }

    RunScope S{engs, B, e0->stream};
    rc = S.begin([&](int) { return conn ? ml_conn_ctl(max_it, ncnn_step) : ml_ctl(tol, max_it); });
    for (int b = 0; b < B && conn && !rc; b++) rc = conn_zero(engs[b]);
    if (!rc) rc = drive_loop(engs, B, false, max_it, true, [&](int t) -> int {
        const int v = variant(t), par = t & 1;
        if (int q = launch_ml_update_batch(e0, d_jh + (size_t)v * B, B)) return q;           // H <- , the previous step's control folded in
        for (int b = 0; b < B; b++) { vbnmf_engine *e = engs[b]; std::swap(e->bpH, e->bpH_alt); e->fold_step = t; }
        if (int q = launch_sweep1_batch(e0, d_jg + (size_t)par * B, B, false)) return q;     // gene side on (w, h_new)
        if (int q = launch_ml_update_batch(e0, d_jw + (size_t)par * B, B)) return q;         // W <-
        if (int q = launch_sweep1_batch(e0, d_jc + (size_t)par * B, B, true)) return q;      // cell side on (h_new, w_new): next step's statistics + sum x log(wh)
        if (t == max_it) {
            for (int b = 0; b < B; b++) {
                vbnmf_engine *e = engs[b];
                MlFold g = ml_fold(e, t + 1, hist, e->bpH);
                if (conn) g.cn = conn_step(e, t + 1, chg);
                g.control_only = 1;
                if (int q = launch_ml_update(e, false, prior, gamma_a, gamma_b, eps, &g)) return q;
            }
        }
        return VBNMF_OK;
    });
    rc = S.end(rc);
    if (e0->poisoned) return rc;                                   // (the jobs may still be read)
    free_jobs();
    if (rc) return rc;
    read_out(engs, B, it_out, nullptr, lk_out, reason_out, nullptr, history, history_rows, 1);
    if (conn) conn_finish(engs, B, changes, changes_rows);
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// The device-driven ML-NMF loops (vbnmf_engine_ml_run; factorize() under criterion = 'likelihood', reference
// R/factorize.R:194-213) of `count` engines of ONE rank on ONE matrix -- the `nrun` restarts factorize() makes of every rank
// (R/factorize.R:181; its default is nrun = 20) -- stepped together: four launches per step for the whole batch.  Per engine
// the results are those of vbnmf_engine_ml_run on it alone, bit for bit.  it_out, lk_out, reason_out: [count]; history (or
// NULL): [count][history_rows], history_rows >= max_it.  Engines as for vbnmf_batch_run, their states set by ml_set_state.
int vbnmf_batch_ml_run(vbnmf_engine **engs, int32_t count, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol,
                       int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows)
{
    if (!engs) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (count < 1 || count > kBatchMax) return fail(VBNMF_ERR_BAD_ARG, "a batch holds 1 to %d engines", kBatchMax);
    if (max_it < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles per engine");
    return batch_ml_run(engs, count, prior, gamma_a, gamma_b, max_it, tol, 0, it_out, lk_out, reason_out, history, history_rows, nullptr, 0);
}

// The same batch under criterion = 'connectivity' (vbnmf_engine_ml_run_connectivity: R/factorize.R:198-208): still four launches
// per step, every engine's H update forming its own labels and table, its own control block counting and deciding.  Per engine
// the results are those of vbnmf_engine_ml_run_connectivity on it alone, bit for bit.  changes (or NULL): [count][changes_rows].
int vbnmf_batch_ml_run_connectivity(vbnmf_engine **engs, int32_t count, int32_t prior, double gamma_a, double gamma_b, int32_t max_it,
                                    int32_t ncnn_step, int32_t *it_out, double *lk_out, int32_t *reason_out, double *history,
                                    int64_t history_rows, int64_t *changes, int64_t changes_rows)
{
    if (!engs) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (count < 1 || count > kBatchMax) return fail(VBNMF_ERR_BAD_ARG, "a batch holds 1 to %d engines", kBatchMax);
    if (max_it < 1 || ncnn_step < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it and ncnn_step must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it doubles per engine");
    if (changes && changes_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "changes needs max_it counts per engine");
    return batch_ml_run(engs, count, prior, gamma_a, gamma_b, max_it, 0.0, ncnn_step, it_out, lk_out, reason_out, history, history_rows,
                        changes, changes_rows);
}

}  // extern "C"
