// engine.h -- the engine as its units see it (engine.hip, batch.hip, mlnmf.hip, svd.hip, labels.hip, hooks.hip): the state
// behind a vbnmf_engine handle, the launch templates, and the helpers of engine.hip that the other units call.  Every helper
// is defined once, in engine.hip; a kernel is launched by the unit that owns it and by no other (a template launched
// through launch_kernel / launch_lds_kernel is emitted where that call is instantiated).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <vector>

#include "common.h"
#include "device.h"
#include "kernels.h"
#include "rank.h"

struct vbnmf_comm;

namespace vbnmf {

// The layout's arrays on the device.  Engines made from a cached layout (same matrix, same geometry, same device)
// share one of these; the per-engine part is DeviceSide::part.
struct DeviceArrays {
    int device = 0;
    uint32_t *packed = nullptr, *widx = nullptr, *task_major = nullptr, *row_task = nullptr;
    double *wval = nullptr;
    int32_t *slice_width = nullptr, *seg_block = nullptr, *seg_ptr = nullptr, *wg_seg0 = nullptr, *row_ptr = nullptr;
    int32_t *slice_fast = nullptr, *block_start = nullptr;
    int64_t *slice_off = nullptr;
    ~DeviceArrays()
    {
        int cur = -1;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        dev_free(packed); dev_free(widx); dev_free(wval); dev_free(task_major); dev_free(row_task);
        dev_free(slice_width); dev_free(seg_block); dev_free(seg_ptr); dev_free(wg_seg0); dev_free(row_ptr);
        dev_free(slice_off); dev_free(slice_fast); dev_free(block_start);
        if (cur >= 0) (void)hipSetDevice(cur);
    }
};

struct DeviceSide {
    std::shared_ptr<DeviceArrays> arrays;      // owner of the pointers below (possibly shared with other engines)
    uint32_t *packed = nullptr, *widx = nullptr, *task_major = nullptr, *row_task = nullptr;
    double *wval = nullptr;
    int32_t *slice_width = nullptr, *seg_block = nullptr, *seg_ptr = nullptr, *wg_seg0 = nullptr, *row_ptr = nullptr;
    int32_t *slice_fast = nullptr, *block_start = nullptr;
    int64_t *slice_off = nullptr;
    double *part = nullptr;                    // this engine's per-task partial statistics
    int64_t n_major = 0, n_minor = 0, n_tasks = 0, n_rows = 0, n_slices = 0, n_slots = 0;
    int32_t block_width = 0, n_blocks = 0, n_wg = 0, row_slots = 0;
    bool wide = false;
    bool merge = false;                        // the sweep adds the runs of a slice in the wave: one partial row per run (Layout::merge)
};

}  // namespace vbnmf

struct vbnmf_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0, m = 0, m_global = 0, nnz = 0;
    int64_t col_begin = 0;            // first cell of this partition (0 for an unpartitioned engine)
    // The layout's internal renumbering of this engine's cells (csrc/order.cpp): the cell-indexed arrays (lh, llh, eh, dh,
    // the labels) hold position p = original local column cell_perm[p]; empty = as stored.  Every boundary that takes or
    // returns cell-indexed data translates through it; d_perm is its device copy (random_state's per-element counters).
    std::vector<int32_t> cell_perm;
    int32_t *d_perm = nullptr;
    int32_t *d_ids[2] = {nullptr, nullptr};   // arg-max labels of the cells: current / previous (cluster_changes)
    int ids_cur = 0;
    bool ids_valid = false;
    unsigned long long *d_table = nullptr;    // [(r+1)^2 + 1] contingency table of two labelings, then the pair count
    unsigned long long *d_ctab = nullptr;     // [4][(r+1)^2] the tables of the device-driven connectivity rule (mlnmf.h: MlConn)
    size_t chg_off = 0;                       // ... and where its per-step counts start in h_hist (behind the run's history rows)
    double *svd_ws = nullptr;         // truncated SVD work space: Gram block partials, two k x k matrices, values
    int32_t *svd_status = nullptr;
    int r = 0, R = 0, NT = 0, n_wg = 0;
    bool wide = false, partitioned = false;
    double lgx = 0.0;
    double xlx = 0.0;                 // sum over stored entries of -x log x + x (ML-NMF likelihood constant)
    vbnmf::DeviceSide A, B;           // A: lanes own genes ; B: lanes own cells
    double *lw = nullptr, *llw = nullptr, *ew = nullptr, *dw = nullptr;
    double *lh = nullptr, *llh = nullptr, *eh = nullptr, *dh = nullptr;
    double *epart = nullptr;          // [2 * n_wg] evidence partials: gene side, then cell side
    double *bpW = nullptr, *bpH = nullptr;   // [ub][R+2] block partials of the two updates (allocated for kUpdateBlocks rows)
    // Both posterior updates in one launch (kernels.h: k_update2; unpartitioned engines): the gene side of the sweep leaves
    // per-slice column sums of sw (csl) and their per-workgroup sums (csum); both tables of block partials alternate.
    double *csl = nullptr, *csum = nullptr;  // [A.n_slices][R], [n_wg][R]
    bool pair = false;
    bool stream_nt = false;                  // the sweeps read the entry stream non-temporally (kernels.h: ld_stream)
    uint4 *upd_tab = nullptr;                // k_update2's work table, one row per block (build_update_table)
    int32_t upd_stride4 = 0, upd_V = 0, upd_ids_off = 0;
    int ub = vbnmf::kUpdateBlocks;    // blocks of the update kernels (one per CU; VBNMF_UPDATE_BLOCKS for experiments)
    double *red = nullptr;            // [n*R | R+4]  (partitioned engines only use the first part)
    int64_t red_count = 0;
    bool epart_in_red = false;        // partitioned engines: the evidence partials live at red[red_ev_off) (kEvSlots + 1 doubles:
                                      // the second all-reduce of a device-driven step sends them as they are)
    double *red_g = nullptr;          // same shape: receive side of the all-reduce in a device-driven partitioned loop
    const double *red_in = nullptr;   // what the W update and the control kernel read: red (reduced in place by the
                                      // caller) or red_g (out of place, so that steps queued past the stop stay no-ops)
    vbnmf_comm *comm = nullptr;       // attached communicator (not owned)
    int comm_rank = 0;
    hipStream_t cstream = nullptr;    // the all-reduces of a partitioned loop are enqueued here, beside the cell-side sweep
    std::vector<hipEvent_t> ev_ring;  // events ordering the two streams, cycled (a step uses 3)
    size_t ev_next = 0;
    double *d_out = nullptr;          // [8]
    double *h_out = nullptr;          // pinned, device-visible [kHostOut]: the slots are HostOutSlot's (kernels.h)
    double *h_out_dev = nullptr;      // device address of h_out
    double *h_stage = nullptr;        // pinned staging of set_state / get_state (index-major copies of the state arrays)
    size_t h_stage_count = 0;
    double *h_hist = nullptr;         // pinned, device-visible per-step history of the device-driven loops (grown on demand)
    double *h_hist_dev = nullptr;
    size_t h_hist_count = 0;
    double seq = 0.0;
    vbnmf::LogTabEntry *logtab = nullptr;   // [128] ln table of the sweep
    vbnmf::LoopCtl *ctl = nullptr;    // control block of the device-driven loop
    // Unpartitioned VB loop with the control step folded into the gene-side update (kernels.h: ControlFold): two control
    // blocks and a second table of gene-side block partials, alternating by step; bpW always names the table the latest
    // queued gene-side update writes (the one every later kernel reads), bpW_alt the other.
    vbnmf::LoopCtl *ctl2 = nullptr;
    double *bpW_alt = nullptr;
    double *bpH_alt = nullptr;           // the ML loop folds its control step into the H update: the same alternation for bpH
    const int32_t *stop_ptr = nullptr;   // the stop flag the kernels of the step being queued read (null: ctl->stop)
    int fold_step = 0;
    bool fold = false;
    bool run_active = false;
    unsigned long long *dbg = nullptr;   // diagnostic timestamps of the sweep (VBNMF_DEBUG_TIMES=1)
    size_t dbg_count = 0;
    size_t lds_bytes = 0;
    bool has_state = false, stats_ready = false, step_pending = false, prime_pending = false;
    bool poisoned = false;            // a wait on the device timed out: work may still be queued, nothing is waited for or freed
    bool ml_ready = false;            // lw / lh hold an ML-NMF state (w, h) and the cell-side statistics are current
    bool ml_prime_pending = false;    // partitioned engine: ml_set_state left its partials in `red`, ml_state_finish has not run
    int ml_phase = 0;                 // host-stepped ML step: 0 idle, 1 / 2 behind the first / second ml_step_local
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    bool ev_recorded = false, ev2_recorded = false;
    double sweep_ms = 0.0;
    int64_t sweep_launches = 0;
};

namespace vbnmf {

// doubles behind `red` / `red_g`: the reduce buffer proper (red_count, what the host-stepped exchange carries), then
//   [red_count, red_ev_off)  the (r+1) x (r+1) label table of the connectivity rule as doubles (mlnmf.h: MlConn): directly behind
//                            the two doubles of the group ML step's second all-reduce, which carries it under that rule (on every
//                            engine: a group of ONE partition that covers all cells is an unpartitioned engine, and takes that step)
//   [red_ev_off, ...)        partitioned engines: the evidence slots of the device-driven VB loop's second all-reduce (kEvSlots
//                            partials + sum lgamma(x+1))
inline int64_t red_ev_off(const vbnmf_engine *e)
{
    return e->red_count + (int64_t)(e->r + 1) * (e->r + 1);
}
inline int64_t red_alloc_count(const vbnmf_engine *e)
{
    return red_ev_off(e) + ((e->partitioned && 2 * (int64_t)e->n_wg <= kEvSlots) ? kEvSlots + 1 : 0);
}

// One side of the factorisation as the launch functions see it: the gene side (W; lanes own genes) or the cell side (H).
struct SideView {
    const DeviceSide &S;
    int64_t nmaj;                     // the side's majors: genes / this engine's cells
    double *l, *ll, *e, *d;           // its state arrays
    double *other_l;                  // the other side's factor (what its sweep gathers)
    double *bp, *other_bp;            // block partials of its update and of the other side's
    double *epart;                    // its half of the evidence partials
    int idx;                          // 0: gene side, 1: cell side
};

inline SideView side_view(const vbnmf_engine *e, bool gene_side)
{
    if (gene_side) return {e->A, e->n, e->lw, e->llw, e->ew, e->dw, e->lh, e->bpW, e->bpH, e->epart, 0};
    return {e->B, e->m, e->lh, e->llh, e->eh, e->dh, e->lw, e->bpH, e->bpW, e->epart + e->n_wg, 1};
}

// ---- defined in engine.hip ----
SweepSide sweep_side_args(const vbnmf_engine *e, bool gene_side);
int prepare_sweep_kernel(const void *fn);
int use_device(const vbnmf_engine *e);
double wait_timeout_s();
int wait_result(vbnmf_engine *e);
int harvest_timing(vbnmf_engine *e);
int ensure_history(vbnmf_engine *e, size_t doubles);
int ensure_comm_resources(vbnmf_engine *e);
hipEvent_t next_event(vbnmf_engine *e);
int stage_ids(const DeviceSide &S, unsigned grid, bool dense = false);
void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, double *dst,
                    const std::vector<int32_t> *perm = nullptr);
void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, std::vector<double> &dst,
                    const std::vector<int32_t> *perm = nullptr);
void from_index_major(const double *src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                      const std::vector<int32_t> *perm = nullptr);
void from_index_major(const std::vector<double> &src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                      const std::vector<int32_t> *perm = nullptr);
// the launchers of engine.hip's kernels
int launch_update(vbnmf_engine *e, bool gene_side, double a, double b, double fudge, const LoopCtl *ctl = nullptr,
                  const ControlFold *foldp = nullptr);
UpdSide upd_side(const vbnmf_engine *e, bool gene_side, const double *bp_prev, double *bp);
int launch_prime(vbnmf_engine *e, bool gene_side, const double *ev);
int launch_side_pack(vbnmf_engine *e, bool gene_side, double *target);
int launch_tail(vbnmf_engine *e, const double *epart, int64_t nepart, double constant);
int launch_pack_tail(vbnmf_engine *e, const int32_t *stop);
int launch_tail_data(vbnmf_engine *e, const double *epart, int64_t nepart, double constant, double *out2);
int launch_group_sum(hipStream_t stream, const double *const *send, double *const *recv, int parts, int64_t count);
int launch_group_sum_at(hipStream_t stream, const double *const *send, double *const *recv, int parts, int64_t off, int64_t count);

// Launch of kernel K on the engine's stream, with the launch error turned into a status.
template <auto K, class... Args>
int launch_kernel(vbnmf_engine *e, dim3 grid, int threads, size_t lds, const Args &...args)
{
    hipLaunchKernelGGL(K, grid, dim3(threads), lds, e->stream, args...);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

// The kernels that stage the 160 KB LDS image (k_sweep, k_sweep1, k_spmm and the two batch sweeps): prepared once per
// kernel instantiation and device (the flags live with the instantiation of this template; devices from 16 on prepare on
// every launch).
template <auto K, class... Args>
int launch_lds_kernel(vbnmf_engine *e, dim3 grid, int threads, const Args &...args)
{
    static std::atomic<bool> attr_set[16];
    if (e->device >= 16 || !attr_set[e->device].load(std::memory_order_acquire)) {
        if (int rc = prepare_sweep_kernel((const void *)K)) return rc;
        if (e->device < 16) attr_set[e->device].store(true, std::memory_order_release);
    }
    return launch_kernel<K>(e, grid, threads, e->lds_bytes, args...);
}

// The template arguments the sweep family shares, for the padded rank RT and the engine's entry format: above 32 the
// sweep's lanes share the rank (SP lanes of R = RT / SP columns each, kernels.h).  f(shape) reads them as shape.R, shape.WIDE,
// shape.NT and shape.SP.
template <int R_, bool WIDE_, int NT_, int SP_>
struct SweepShape { static constexpr int R = R_, NT = NT_, SP = SP_; static constexpr bool WIDE = WIDE_; };

template <int RT, class F>
int with_sweep_shape(const vbnmf_engine *e, F &&f)
{
    constexpr int SP = rank_shares(RT), R = RT / SP, NT = sweep_threads(RT);
    return e->wide ? f(SweepShape<R, true, NT, SP>{}) : f(SweepShape<R, false, NT, SP>{});
}

// One side's sweep alone (k_sweep1: mlnmf.hip launches the VB = false forms, engine.hip the VB = true ones).  VB = false: the ML step's, whose cell side carries the log term (sum x log(wh));
// VB = true: one side of the VB sweep (cell-partitioned device loop), gene side with the log term, cell side without.
template <bool VB>
int launch_side_sweep(vbnmf_engine *e, const SweepSide &a, bool logterm)
{
    return with_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return with_flag(logterm, [&](auto lt) {
                return launch_lds_kernel<k_sweep1<s.R, s.WIDE, lt(), s.NT, VB, s.SP>>(e, dim3((unsigned)e->n_wg), s.NT, a);
            });
        });
    });
}

}  // namespace vbnmf
