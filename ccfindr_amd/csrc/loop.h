// loop.h -- the host side of every device-driven loop (VB single and group: engine.hip; VB batch: batch.hip; ML single, group
// and batch: mlnmf.hip): the group of engines a loop advances, the driver that queues its steps ahead of the device, and the
// scope that saves and restores what a run changes on its engines.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "engine.h"

namespace vbnmf {

// The engines one device-driven loop advances together: a single engine, or the partition engines of a local group.
struct LoopGroup {
    vbnmf_engine **e;
    int count;
    vbnmf_comm *comm;      // null: one unpartitioned engine
};

constexpr int kBatchMax = 64;        // engines of one batch run

// ---- defined in engine.hip ----
void launch_ctl_init(hipStream_t stream, LoopCtl *ctl, const LoopCtl &v);      // k_ctl_init: the launch error is left for the caller
int group_tables(vbnmf_comm *c);
int group_members(vbnmf_comm *c, LoopGroup &G);
int group_sum_in_place(const LoopGroup &G);
ControlFold vb_fold(const vbnmf_engine *e, int t, bool hist);
LoopCtl vb_ctl(const double *hyper, const int32_t *flags, double tol, int32_t max_it, int32_t n0, int32_t dn);
int check_hyper(const double *hyper);
void read_out(vbnmf_engine *const *engs, int count, int32_t *it_out, double *lk0_out, double *lk_out, int32_t *reason_out,
              double *hyper, double *history, int64_t rows, int width);
// ---- defined in batch.hip ----
int batch_admit(vbnmf_engine **engs, int B, bool vb, size_t hist_doubles);

// Host side of every device-driven loop: a single engine, a local group, a batch.  Steps are queued in batches of eight, two
// batches ahead of the device, by queue_step(t) (t: the 1-based step); the host polls the pinned result blocks of `polled`
// engines (engine 0 for a single engine or a group, every engine for a batch): [5] = steps done, [6] = reason (raised after
// [5]), [7] = steps done (raised last).  Batch b + 2 is queued
//   replicated  (single engine, group): unless the loop stopped at or before the last step of batch b -- a function of the
//               device's (replicated) decisions alone, never of when this host happened to look, so every process of a
//               partitioned run queues the same number of steps, i.e. the same sequence of collectives;
//   !replicated (batch): unless every engine has stopped.
// `fold`: the control step is folded into the NEXT step's update (ControlFold / MlFold).  A timed-out wait sets poisoned on
// engine 0 (RunScope::end passes it on to the run's other engines).
template <class QueueStep>
int drive_loop(vbnmf_engine *const *engs, int polled, bool replicated, int max_it, bool fold, QueueStep &&queue_step)
{
    vbnmf_engine *e0 = engs[0];
    const int B = 8;
    int queued = 0;
    auto queue_batch = [&]() -> int {
        for (int q = 0; q < B && queued < max_it; q++, queued++)
            if (int rc = queue_step(queued + 1)) return rc;
        return VBNMF_OK;
    };
    // every polled engine has stopped or reported `target` steps; all_stopped: every one has stopped
    auto reached = [&](int target, bool &all_stopped) {
        bool ok = true;
        all_stopped = true;
        for (int p = 0; p < polled; p++) {
            volatile double *ho = engs[p]->h_out;
            const bool stopped = ho[kOutReason] != 0.0;
            all_stopped = all_stopped && stopped;
            ok = ok && (stopped || (int)ho[kOutSeq] >= target);
        }
        return ok;
    };
    // "The stream is idle and an engine that raised no stop reports fewer steps than a drained stream must show": something
    // was lost on the device.  With the fold, step t is only reported by step t + 1's launch, so a fully drained, healthy
    // stream shows queued - 1 until the closing control-only launch behind step max_it has been queued.
    auto idle_check = [&](int target) -> int {
        hipError_t q = hipStreamQuery(e0->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return fail(VBNMF_ERR_HIP, "the device-driven loop failed on the device: %s", hipGetErrorString(q));
        const int expect = queued - ((fold && queued < max_it) ? 1 : 0);
        bool all_stopped;
        if (q == hipSuccess && !reached(std::min(target, expect), all_stopped))
            return fail(VBNMF_ERR_HIP, "the device went idle before the queued steps of the device-driven loop finished");
        return VBNMF_OK;
    };
    // test hook (tests/test_gpu_control_fold.py): drain the stream before every look, i.e. the host thread stalled between
    // queueing and polling -- the case the idle check must not mistake for a lost step
    const char *drain_env = getenv("VBNMF_TEST_DRAIN_BEFORE_POLL");
    const bool drain_first = drain_env && drain_env[0] == '1';
    if (int rc = queue_batch()) return rc;
    if (int rc = queue_batch()) return rc;
    const double limit = wait_timeout_s();
    for (int b = 0;; b++) {
        const int target = (int)std::min<int64_t>((int64_t)(b + 1) * B, max_it);
        const auto t0 = std::chrono::steady_clock::now();          // the bound is per batch of B steps
        if (drain_first) {
            (void)hipStreamSynchronize(e0->stream);
            if (int rc = idle_check(target)) return rc;
        }
        bool all_stopped = false;
        for (long spins = 1; !reached(target, all_stopped); spins++) {
            if ((spins & 0xFFFF) == 0) {
                const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (waited > limit) {
                    e0->poisoned = true;
                    return fail(VBNMF_ERR_HIP, "timed out after %.1f s (VBNMF_WAIT_TIMEOUT_S) waiting for step %d of the device-driven loop; "
                                "the last completed step is %d (%d queued)", waited, target, (int)e0->h_out[kOutSeq], queued);
                }
                if (int rc = idle_check(target)) return rc;
            }
        }
        volatile double *ho = e0->h_out;
        if (replicated ? ho[kOutReason] != 0.0 && (int)ho[kOutIt] <= target : all_stopped) break;
        if (target >= max_it) break;
        if (int rc = queue_batch()) return rc;
    }
    return VBNMF_OK;
}

// What a device-driven run changes on its engines: begin() saves it and loads every engine's control block, end() waits for
// the streams and puts it back.  shared: the stream every launch of a batch goes on (null: each engine its own).
struct RunScope {
    vbnmf_engine *const *e;
    int count;
    hipStream_t shared = nullptr;
    bool plain_ctl = false;            // the loop keeps its control block in e->ctl whatever e->fold says (partitioned ML loop)
    std::vector<hipStream_t> own;
    std::vector<char> timing;

    // ctl(p): the control block engine p's loop starts from
    template <class CtlOf>
    int begin(CtlOf &&ctl)
    {
        own.resize(count); timing.resize(count);
        for (int p = 0; p < count; p++) {
            vbnmf_engine *x = e[p];
            own[p] = x->stream; timing[p] = x->timing;
            x->timing = false;                                     // event pairs cannot follow launches queued ahead
            x->ev_recorded = false; x->ev2_recorded = false;
            if (shared) x->stream = shared;
            launch_ctl_init(x->stream, x->fold && !plain_ctl ? x->ctl2 : x->ctl, ctl(p));
            x->fold_step = 0;
            volatile double *ho = x->h_out;
            ho[kOutIt] = 0.0; ho[kOutReason] = 0.0; ho[kOutSeq] = 0.0;
            x->run_active = true;
        }
        hipError_t he = hipGetLastError();
        if (he != hipSuccess) return end(fail(VBNMF_ERR_HIP, "loading the loop control block failed: %s", hipGetErrorString(he)));
        return VBNMF_OK;
    }

    // After a timeout (engine 0 poisoned) the streams may never drain: every engine is poisoned and gets its own stream back,
    // nothing is waited for.  Otherwise a failed synchronise becomes the result of a run that had succeeded.
    int end(int rc)
    {
        if (e[0]->poisoned) {
            for (int p = 0; p < count; p++) { e[p]->poisoned = true; e[p]->stream = own[p]; }
            return rc;
        }
        for (int p = 0; p < (shared ? 1 : count); p++) {
            vbnmf_engine *x = e[p];
            hipError_t he = hipStreamSynchronize(x->stream);
            if (he == hipSuccess && x->cstream) he = hipStreamSynchronize(x->cstream);
            if (he != hipSuccess && !rc) rc = fail(VBNMF_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(he));
        }
        for (int p = 0; p < count; p++) {
            vbnmf_engine *x = e[p];
            x->stream = own[p];
            x->run_active = false; x->timing = timing[p];
            x->stop_ptr = nullptr;
            x->seq = 0.0; x->h_out[kOutSeq] = 0.0;                       // the step path's sequence flag restarts
        }
        return rc;
    }
};

}  // namespace vbnmf
