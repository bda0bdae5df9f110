// batch.hip -- a batch of engines stepped by one launch (kernels.h: k_update2_batch, k_sweep_batch): the device-driven VB
// loops of the restarts of one rank on one matrix, two launches per step for all of them (vbnmf_batch_run), and the admission
// check both batch forms share (the ML batch is in mlnmf.hip).
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "engine.h"
#include "loop.h"

using namespace vbnmf;

namespace {

int launch_sweep_batch(vbnmf_engine *e, const SweepSide *jobs, int B)
{
    return with_batch_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return launch_lds_kernel<k_sweep_batch<s.R, s.WIDE, s.NT, 1>>(e, dim3((unsigned)e->n_wg, (unsigned)B), s.NT, jobs);
        });
    });
}

int launch_update2_batch(vbnmf_engine *e, const Upd2Job *jobs, int B)
{
    return with_batch_rank(e->R, [&](auto rt) {
        return launch_kernel<k_update2_batch<rt()>>(e, dim3((unsigned)e->ub, (unsigned)B), kUpdateThreads, 0, jobs);
    });
}

}  // namespace

namespace vbnmf {

// The engines a batch run takes (vb: vbnmf_batch_run, else vbnmf_batch_ml_run): no null or repeated handle; unpartitioned, the
// control step folded in (VB: the one-launch update form; ML: both tables of H-side partials), padded rank <= 16; one row width
// on one matrix; a state set.  Their history buffers are made to hold `hist_doubles` (0: no history), the streams of all but
// the first are idle on return.
int batch_admit(vbnmf_engine **engs, int B, bool vb, size_t hist_doubles)
{
    vbnmf_engine *e0 = engs[0];
    if (!e0) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    for (int b = 0; b < B; b++) {
        vbnmf_engine *e = engs[b];
        if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
        for (int q = 0; q < b; q++) if (engs[q] == e) return fail(VBNMF_ERR_BAD_ARG, "the same engine twice in a batch");
        if (int rc = use_device(e)) return rc;
        if (e->partitioned || e->comm || !e->fold || !(vb ? e->pair : e->bpH_alt != nullptr) || e->R > kBatchMaxPaddedRank)
            return fail(VBNMF_ERR_STATE, "a batch takes unpartitioned engines %s and padded rank <= %d",
                        vb ? "of the one-launch update form" : "with the control step folded in", kBatchMaxPaddedRank);
        if (e->device != e0->device || e->n != e0->n || e->m != e0->m || e->R != e0->R || e->n_wg != e0->n_wg || e->ub != e0->ub ||
            e->NT != e0->NT || e->wide != e0->wide || e->lds_bytes != e0->lds_bytes || e->A.n_slices != e0->A.n_slices ||
            e->B.n_slices != e0->B.n_slices ||
            (vb && (e->upd_stride4 != e0->upd_stride4 || e->upd_V != e0->upd_V || e->upd_ids_off != e0->upd_ids_off)))
            return fail(VBNMF_ERR_STATE, "the engines of a batch must be of one row width on one matrix (same padded rank, layouts%s)",
                        vb ? ", grids and update table" : " and grids");
        if (vb && (!e->has_state || !e->stats_ready)) return fail(VBNMF_ERR_STATE, "batch run before set_state");
        if (vb && e->step_pending) return fail(VBNMF_ERR_STATE, "batch run between step_local and step_finish");
        if (!vb && !e->ml_ready) return fail(VBNMF_ERR_STATE, "batch ML run before ml_set_state");
        if (hist_doubles) { if (int rc = ensure_history(e, hist_doubles)) return rc; }
    }
    for (int b = 1; b < B; b++) HIPCHECK(hipStreamSynchronize(engs[b]->stream));      // (idle already: set_state ends with a synchronise)
    return VBNMF_OK;
}

}  // namespace vbnmf

extern "C" {

// The device-driven loops of `count` engines of ONE rank on ONE matrix (the restarts of a rank: same layouts, grids and update
// table; each engine its own state), stepped TOGETHER: two launches per step for the whole batch, every engine's blocks
// following its own control block (its own hyper-parameters, evidence, stop).  Results per engine are those of
// vbnmf_engine_run on it alone, bit for bit.  hyper: [count][4] in / out; it / lk0 / lkh / reason: [count]; history (or
// null): [count][history_rows][9].  Engines must be unpartitioned, of the one-launch update form, of padded rank <= 16.
int vbnmf_batch_run(vbnmf_engine **engs, int32_t count, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0,
                    int32_t dn, const int32_t *flags, int32_t *it_out, double *lk0_out, double *lkh_out, int32_t *reason_out,
                    double *history, int64_t history_rows)
{
    if (!engs || !hyper || !flags) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (count < 1 || count > kBatchMax) return fail(VBNMF_ERR_BAD_ARG, "a batch holds 1 to %d engines", kBatchMax);
    if (max_it < 1 || dn < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it and dn must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it rows of 9 doubles per engine");
    const int B = count;
    for (int b = 0; b < B; b++) { if (int rc = check_hyper(hyper + (size_t)b * 4)) return rc; }
    if (int rc = batch_admit(engs, B, true, history ? (size_t)max_it * 9 : 0)) return rc;
    vbnmf_engine *e0 = engs[0];

    // ---- the jobs: the update's of step 1 (nothing to evaluate yet), of the odd and of the even steps; the sweep's by parity
    const bool hist = history != nullptr;
    std::vector<Upd2Job> ju((size_t)3 * B);
    std::vector<SweepSide> js((size_t)2 * 2 * B);
    for (int b = 0; b < B; b++) {
        vbnmf_engine *e = engs[b];
        double *Wt[2] = {e->bpW, e->bpW_alt}, *Ht[2] = {e->bpH, e->bpH_alt};          // [0]: the latest tables as the run starts
        for (int v = 0; v < 3; v++) {
            const int t = v == 0 ? 1 : (v == 1 ? 3 : 2);
            Upd2Job &J = ju[(size_t)v * B + b];
            J.W = upd_side(e, true, Wt[(t - 1) & 1], Wt[t & 1]);
            J.H = upd_side(e, false, Ht[(t - 1) & 1], Ht[t & 1]);
            J.T = UpdTable{e->upd_tab, e->upd_stride4, e->upd_V, e->upd_ids_off};
            J.r = e->r; J.nb = e->ub; J.ncs = e->n_wg; J.csum = e->csum; J.fudge = fudge;
            J.fold = vb_fold(e, t, hist);
        }
        for (int par = 0; par < 2; par++) {                       // the sweep of step t reads the stop flag that step's update left
            SweepSide *s = &js[((size_t)par * B + b) * 2];
            s[0] = sweep_side_args(e, true);
            s[1] = sweep_side_args(e, false);
            s[0].stop = s[1].stop = &(e->ctl2 + par)->stop;
        }
    }
    Upd2Job *d_ju = nullptr;
    SweepSide *d_js = nullptr;
    int rc = dev_upload(&d_ju, ju);
    if (!rc) rc = dev_upload(&d_js, js);
    if (rc) { dev_free(d_ju); dev_free(d_js); return rc; }

    RunScope S{engs, B, e0->stream};                              // every launch of the run goes on the first engine's stream
    rc = S.begin([&](int b) { return vb_ctl(hyper + (size_t)b * 4, flags, tol, max_it, n0, dn); });
    if (!rc) rc = drive_loop(engs, B, false, max_it, true, [&](int t) -> int {
        const int v = t == 1 ? 0 : ((t & 1) ? 1 : 2);
        if (int q = launch_update2_batch(e0, d_ju + (size_t)v * B, B)) return q;
        if (int q = launch_sweep_batch(e0, d_js + (size_t)(t & 1) * B * 2, B)) return q;
        for (int b = 0; b < B; b++) {
            vbnmf_engine *e = engs[b];
            std::swap(e->bpW, e->bpW_alt); std::swap(e->bpH, e->bpH_alt);      // (e->bpW / e->bpH name the latest tables, as launch_update2 keeps them)
            e->fold_step = t;
        }
        if (t == max_it) {                                       // behind the last step: every engine's control step alone
            for (int b = 0; b < B; b++) {
                vbnmf_engine *e = engs[b];
                ControlFold g = vb_fold(e, t + 1, hist);
                g.bpW_prev = e->bpW; g.control_only = 1;
                if (int q = launch_update(e, true, 0, 0, fudge, nullptr, &g)) return q;
            }
        }
        return VBNMF_OK;
    });
    rc = S.end(rc);
    if (e0->poisoned) return rc;                                   // (the jobs may still be read)
    dev_free(d_ju); dev_free(d_js);
    if (rc) return rc;
    read_out(engs, B, it_out, lk0_out, lkh_out, reason_out, hyper, history, history_rows, 9);
    return VBNMF_OK;
}

}  // extern "C"
