// engine.hip -- the device-resident VB-NMF engine behind the C ABI of include/vbnmf.h.
//
// One step (reference src/vbnmf_update.cpp:33-90) is four launches on one HIP stream:
//   k_update(W)  k_update(H)  k_sweep(both sides)  k_final
// The sweep at the end of step t produces the sufficient statistics that step t+1 starts
// from AND the data term of step t's evidence (see kernels.h), so X is streamed once per
// step and side.  k_final leaves lkh and the hyper statistics in pinned host memory and
// raises a sequence flag the host polls (no memcpy, no stream synchronise on the hot path).
// A cell-partitioned engine adds k_pack + k_tail, which fill the reduce buffer
// [swsum | rowSum(eh) | scalars] that the caller all-reduces between step_local and step_finish.
// vbnmf_engine_run drives the whole loop of vb_iterate from the device (hyper_update, stopping rule, per-step history;
// steps queued ahead of the GPU): the control step is folded into the next step's gene-side update (kernels.h:
// ControlFold; three launches per step), partitioned engines run it as the one-block kernel k_control behind each sweep.
// The same engine also runs the maximum-likelihood NMF step of factorize() (mlnmf.h: two single-side sweeps
// per step) and the sparse products of the svd2 initialiser's truncated SVD (k_spmm).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <queue>
#include <string>
#include <system_error>
#include <thread>
#include <utility>

#include "common.h"
#include "comm.h"
#include "device.h"
#include "kernels.h"
#include "mlnmf.h"
#include "rank.h"
#include "init.h"
#include "consensus.h"

using namespace vbnmf;

namespace {

constexpr int kHostOut = 16;        // doubles in the pinned result block of an engine

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

}  // namespace

namespace vbnmf {
// vbnmf_set_engine_grid: the grids of the engines THIS host thread creates next (0: the defaults)
static thread_local int tl_grid_nwg = 0, tl_grid_ub = 0;
// vbnmf_set_engine_padding: the padded rank (row width) of the engines THIS host thread creates next (0: the rank's own)
static thread_local int tl_pad_R = 0;

int sweep_workgroups(int device, bool partitioned, int &n_wg)
{
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    n_wg = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;      // one persistent workgroup per CU
    const char *forced = getenv("VBNMF_NWG");
    if (forced) { int v = atoi(forced); if (v > 0) n_wg = v; }
    if (partitioned && !forced) {
        // A partition's sweep leaves CUs free: its workgroups own all 160 KB of a CU's LDS, so the all-reduce kernels that
        // should run BESIDE the cell-side sweep could not start on a chip filled by it.  How many: ONE PER SHADER ENGINE
        // (8 XCDs x 4 engines = 32).  Measured in round 5 with the collective carried by kernels of RCCL's launch shape
        // (tests/fake_rccl, FAKE_RCCL_KERNEL=1: 24 or 64 blocks x 512 threads, 4 KB of LDS; profiles/r05_c5_overlap.txt, one C5
        // partition): with 8 or 16 CUs free the collective's first kernel still ENDS WITH the sweep (155-166 us instead of
        // 25 alone) -- a queue's workgroups are dealt to the shader engines in turn, and the first one dealt to an engine
        // whose CUs are all full stalls the whole queue behind it -- with 32 free it runs inside the sweep (37 + 40 us,
        // done 170 us before the sweep ends).  Price: the two sweeps on 224 instead of 248 workgroups, +21 us per step
        // (0.427 against 0.411 ms with no reserve and this one-rank collective trailing the sweep): the reserve pays as soon
        // as the real all-reduce over xGMI takes more than ~25 us alone (4.8 MB: >= 55 us by SURVEY.md section 5's ring estimate).
        // VBNMF_COMM_CUS overrides (0: no reserve).
        int spare = 32;
        if (const char *sv = getenv("VBNMF_COMM_CUS")) spare = atoi(sv);
        if (spare >= 0 && n_wg - spare >= 8) n_wg -= spare;
    }
    return VBNMF_OK;
}
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
    DeviceSide A, B;                  // A: lanes own genes ; B: lanes own cells
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
    int ub = kUpdateBlocks;           // blocks of the update kernels (one per CU; VBNMF_UPDATE_BLOCKS for experiments)
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
    double *h_out = nullptr;          // pinned, device-visible [kHostOut]; [7] = sequence flag; [8..12] = hyper, lk0 of a device-driven loop
    double *h_out_dev = nullptr;      // device address of h_out
    double *h_stage = nullptr;        // pinned staging of set_state / get_state (index-major copies of the state arrays)
    size_t h_stage_count = 0;
    double *h_hist = nullptr;         // pinned, device-visible per-step history of the device-driven loops (grown on demand)
    double *h_hist_dev = nullptr;
    size_t h_hist_count = 0;
    double seq = 0.0;
    LogTabEntry *logtab = nullptr;    // [128] ln table of the sweep
    LoopCtl *ctl = nullptr;           // control block of the device-driven loop
    // Unpartitioned VB loop with the control step folded into the gene-side update (kernels.h: ControlFold): two control
    // blocks and a second table of gene-side block partials, alternating by step; bpW always names the table the latest
    // queued gene-side update writes (the one every later kernel reads), bpW_alt the other.
    LoopCtl *ctl2 = nullptr;
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

namespace {

// Pinned staging buffer of an engine's state transfers (true asynchronous DMA instead of the runtime's bounce through its
// own staging for pageable memory).  Engines hand theirs on through a small per-process list when they are destroyed.
struct StagePool { std::mutex mu; std::vector<std::pair<double *, size_t>> free_list; };
StagePool &stage_pool() { static StagePool *P = new StagePool(); return *P; }

int ensure_stage(vbnmf_engine *e, size_t count)
{
    if (count <= e->h_stage_count) return VBNMF_OK;
    StagePool &P = stage_pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        if (e->h_stage) { P.free_list.emplace_back(e->h_stage, e->h_stage_count); e->h_stage = nullptr; e->h_stage_count = 0; }
        int best = -1;
        for (int q = 0; q < (int)P.free_list.size(); q++)
            if (P.free_list[q].second >= count && (best < 0 || P.free_list[q].second < P.free_list[best].second)) best = q;
        if (best >= 0) {
            e->h_stage = P.free_list[best].first; e->h_stage_count = P.free_list[best].second;
            P.free_list.erase(P.free_list.begin() + best);
            return VBNMF_OK;
        }
    }
    double *p = nullptr;
    hipError_t he = hipHostMalloc((void **)&p, count * sizeof(double), hipHostMallocDefault);
    if (he != hipSuccess) { (void)hipGetLastError(); return fail(VBNMF_ERR_OOM, "pinned staging buffer (%zu bytes): %s", count * sizeof(double), hipGetErrorString(he)); }
    e->h_stage = p; e->h_stage_count = count;
    return VBNMF_OK;
}

void release_stage(vbnmf_engine *e)
{
    if (!e->h_stage) return;
    StagePool &P = stage_pool();
    std::vector<std::pair<double *, size_t>> drop;
    {
        std::lock_guard<std::mutex> g(P.mu);
        P.free_list.emplace_back(e->h_stage, e->h_stage_count);
        size_t held = 0;
        for (auto &b : P.free_list) held += b.second * sizeof(double);
        while (P.free_list.size() > 8 || held > ((size_t)1 << 30)) {           // at most 8 buffers / 1 GiB kept
            held -= P.free_list.front().second * sizeof(double);
            drop.push_back(P.free_list.front());
            P.free_list.erase(P.free_list.begin());
        }
    }
    for (auto &b : drop) (void)hipHostFree(b.first);
    e->h_stage = nullptr; e->h_stage_count = 0;
}

void free_side(DeviceSide &S)
{
    dev_free(S.part);
    S = DeviceSide();                          // drops this engine's reference to the (shared) layout arrays
}

// Device copy of a layout's arrays; `X` != null: the layout is (possibly) cached on the matrix and so is its copy.
int upload_side(const Layout &L, int R, int device, const vbnmf_matrix *X, DeviceSide &S, bool with_part = true)
{
    S.n_major = L.n_major; S.n_minor = L.n_minor; S.n_tasks = L.n_tasks; S.n_slices = L.n_slices;
    S.n_slots = L.n_slots; S.block_width = L.block_width; S.n_blocks = L.n_blocks; S.n_wg = L.n_wg; S.wide = L.wide;
    S.row_slots = L.row_slots;
    S.n_rows = L.n_rows; S.merge = L.merge;
    if (L.merge && rank_shares(R) != 1)
        return fail(VBNMF_ERR_BAD_ARG, "a layout with merged pieces serves ranks up to 32 only (padded rank %d)", R);
    if (S.row_slots < R / 2 / rank_shares(R) * rank_shares(R) || !(S.row_slots & 1))
        return fail(VBNMF_ERR_BAD_ARG, "layout row stride of %d slots cannot hold rows of padded rank %d", S.row_slots, R);
    std::shared_ptr<DeviceArrays> A;
    if (X) A = std::static_pointer_cast<DeviceArrays>(cached_device_copy(X, &L, device));
    if (!A) {
        A = std::make_shared<DeviceArrays>();
        A->device = device;
        if (L.wide) {
            if (int rc = dev_upload(&A->widx, L.wide_idx)) return rc;
            if (int rc = dev_upload(&A->wval, L.wide_val)) return rc;
        } else {
            if (int rc = dev_upload(&A->packed, L.packed)) return rc;
        }
        if (int rc = dev_upload(&A->task_major, L.task_major)) return rc;
        if (int rc = dev_upload(&A->slice_width, L.slice_width)) return rc;
        if (int rc = dev_upload(&A->slice_off, L.slice_off)) return rc;
        if (int rc = dev_upload(&A->slice_fast, L.slice_fast)) return rc;
        {
            std::vector<int32_t> bs(L.block_start.begin(), L.block_start.end());      // minors are < 2^31
            if (int rc = dev_upload(&A->block_start, bs)) return rc;
        }
        if (int rc = dev_upload(&A->seg_block, L.seg_block)) return rc;
        if (int rc = dev_upload(&A->seg_ptr, L.seg_ptr)) return rc;
        if (int rc = dev_upload(&A->wg_seg0, L.wg_seg0)) return rc;
        if (int rc = dev_upload(&A->row_ptr, L.row_ptr)) return rc;
        if (int rc = dev_upload(&A->row_task, L.row_task)) return rc;
        if (X) store_device_copy(X, &L, device, A);
    }
    S.arrays = A;
    S.packed = A->packed; S.widx = A->widx; S.wval = A->wval; S.task_major = A->task_major; S.row_task = A->row_task;
    S.slice_width = A->slice_width; S.seg_block = A->seg_block; S.seg_ptr = A->seg_ptr; S.wg_seg0 = A->wg_seg0;
    S.row_ptr = A->row_ptr; S.slice_off = A->slice_off; S.slice_fast = A->slice_fast; S.block_start = A->block_start;
    if (with_part) { if (int rc = dev_alloc(&S.part, (size_t)L.n_slices * kLanes * R)) return rc; }
    return VBNMF_OK;
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

SideView side_view(const vbnmf_engine *e, bool gene_side)
{
    if (gene_side) return {e->A, e->n, e->lw, e->llw, e->ew, e->dw, e->lh, e->bpW, e->bpH, e->epart, 0};
    return {e->B, e->m, e->lh, e->llh, e->eh, e->dh, e->lw, e->bpH, e->bpW, e->epart + e->n_wg, 1};
}

SweepSide sweep_side_args(const vbnmf_engine *e, bool gene_side)
{
    const SideView v = side_view(e, gene_side);
    const DeviceSide &S = v.S;
    SweepSide P;
    P.packed = S.packed; P.widx = S.widx; P.wval = S.wval;
    P.task_major = S.task_major; P.slice_width = S.slice_width; P.slice_off = S.slice_off; P.slice_fast = S.slice_fast;
    P.seg_block = S.seg_block; P.wg_seg0 = S.wg_seg0; P.seg_ptr = S.seg_ptr;
    P.F = v.l;
    P.llF = v.ll;
    P.G = v.other_l;
    P.part = S.part; P.epart = v.epart;
    P.csl = gene_side ? e->csl : nullptr; P.csum = gene_side ? e->csum : nullptr;      // (the pair form's column sums: gene side only)
    P.n_minor = (int32_t)S.n_minor; P.block_start = S.block_start;
    P.row_slots = S.row_slots;
    P.merge = S.merge ? 1 : 0;
    {
        // The youngest third of the workgroup's waves pull slices from the SHORT end of a segment's list (kernels.h:
        // take_ticket_ends).  Measured per side, interleaved, on two boxes (k_sweep us, rank 10, 768 threads: neither side /
        // gene side only / cell side only / both): 171.5 / 170.0 / 175.5 / 172.5 and 168.7 / 166.7 / 171.9 / 169.9 -- the gene
        // side gains, the cell side (no logarithm, shorter slices) loses at this geometry; at the 512-thread ranks both
        // sides gain (neither / gene / both: rank 16 294.1 / 285.7 / 284.8, rank 20 378.9 / 369.0 / 365.3, rank 32 859 / 845 /
        // 838); below padded rank 8 it loses on both (rank 5: 121.1 / 127.3 / 129.3).  So: the gene side from padded rank
        // 8, the cell side from 16.  VBNMF_PULL_ENDS=k overrides the count on both sides, VBNMF_PULL_ENDS_A / _B per side.
        static const int pe = [] { const char *v = getenv("VBNMF_PULL_ENDS"); return v ? atoi(v) : -1; }();
        static const int pes[2] = {[] { const char *v = getenv("VBNMF_PULL_ENDS_A"); return v ? atoi(v) : -1; }(),
                                   [] { const char *v = getenv("VBNMF_PULL_ENDS_B"); return v ? atoi(v) : -1; }()};
        const int third = (e->NT / 64) / 3;
        int k = gene_side ? (e->R >= 8 ? third : 0) : (e->R >= 16 ? third : 0);
        if (pe >= 0) k = pe;
        if (pes[v.idx] >= 0) k = pes[v.idx];
        P.pull_ends = std::min(k, e->NT / 64);
    }
    P.logterm = gene_side ? 1 : 0;
    P.stream_nt = e->stream_nt ? 1 : 0;
    P.n_wg = S.n_wg;
    P.logtab = e->logtab;
    P.stop = e->run_active ? (e->stop_ptr ? e->stop_ptr : &e->ctl->stop) : nullptr;
    P.dbg = e->dbg ? e->dbg + v.idx * (e->dbg_count / 2) : nullptr;
    return P;
}

// First use of a sweep kernel on a device: allow the 160 KB dynamic LDS image, and make sure the kernel has no
// static LDS in front of it -- lds_row() (kernels.h) addresses the staged block from LDS address 0.
int prepare_sweep_kernel(const void *fn)
{
    HIPCHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipFuncAttributes fa;
    HIPCHECK(hipFuncGetAttributes(&fa, fn));
    if (fa.sharedSizeBytes != 0)
        return fail(VBNMF_ERR_HIP, "sweep kernel carries %zu bytes of static LDS; its dynamic LDS would not start at 0", (size_t)fa.sharedSizeBytes);
    return VBNMF_OK;
}

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

int launch_sweep(vbnmf_engine *e)
{
    SweepSide a = sweep_side_args(e, true);
    SweepSide b = sweep_side_args(e, false);
    if (e->timing) { HIPCHECK(hipEventRecord(e->ev0, e->stream)); }
    int rc = with_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return launch_lds_kernel<k_sweep<s.R, s.WIDE, s.NT, s.SP>>(e, dim3((unsigned)e->n_wg), s.NT, a, b);
        });
    });
    if (rc) return rc;
    if (e->timing) { HIPCHECK(hipEventRecord(e->ev1, e->stream)); e->ev_recorded = true; }
    return VBNMF_OK;
}

// Whether an update of `grid` blocks stages the inverse index of side S in LDS: it pays from a few hundred task ids per block
// on (on tiny matrices its two leading round trips are all there is to the kernel -- 200 x 500 at rank 3: 30.7 -> 31.3 us per
// step with it).  `dense`: the partitioned gene side, whose statistics are already summed into `red` -- no index to stage.
int stage_ids(const DeviceSide &S, unsigned grid, bool dense = false)
{
    return !dense && S.n_rows >= (int64_t)256 * grid ? 1 : 0;
}

// ctl != nullptr: device-driven loop, the hyper-parameters are read from the control block on the device
int launch_update(vbnmf_engine *e, bool gene_side, double a, double b, double fudge, const LoopCtl *ctl = nullptr,
                  const ControlFold *foldp = nullptr)
{
    ControlFold fold{};
    if (foldp) fold = *foldp;
    const unsigned grid = fold.control_only ? 1 : e->ub;
    const double lga = (ctl || foldp) ? 0.0 : -std::lgamma(a) + a * std::log(a / b);     // reference :82 / :87
    const SideView v = side_view(e, gene_side);
    const DeviceSide &S = v.S;
    const bool dense = gene_side && e->partitioned;               // statistics already summed into `red`
    const double *redin = e->red_in ? e->red_in : e->red;
    const double *acc = dense ? redin : S.part;
    const int32_t *row_ptr = dense ? nullptr : S.row_ptr;
    const uint32_t *row_task = dense ? nullptr : S.row_task;
    const double *other = dense ? redin + (size_t)e->n * e->R : nullptr;
    const double *other_bp = dense ? nullptr : v.other_bp;
    const int other_nb = dense ? 0 : e->ub;
    const int stage = stage_ids(S, grid, dense);
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_update<rt()>>(e, dim3(grid), kUpdateThreads, 0, acc, row_ptr, row_task, v.nmaj, e->r, other, other_bp,
                                             other_nb, a, b, lga, fudge, v.l, v.ll, v.e, v.d, v.bp, ctl, v.idx, fold, stage);
    });
}

// The work table of k_update2 (kernels.h): per block of the update, the visits of every thread row -- the block's genes
// and cells dealt to the rows longest-processing-time first -- and the task ids of those majors.  The gather is bound by the
// task rows it moves (a round of 16 scattered loads takes about as long as the whole posterior arithmetic behind it,
// in-kernel stamps), so a major costs its task count plus a few loads' worth of fixed work.  Every block's row has the same
// shape (stride, visits per thread row, offset of the ids), so the kernel loads it without knowing anything first.
// Returns false when a block's row does not fit the kernel's LDS copy: the engine then keeps the two-launch form.
bool build_update_table(const Layout &LA, const Layout &LB, int ub, int R, std::vector<uint32_t> &tab, int32_t &stride4, int32_t &V,
                        int32_t &ids_off)
{
    const int RB = kUpdateThreads / R;
    const int64_t nm[2] = {LA.n_major, LB.n_major};
    const Layout *Ls[2] = {&LA, &LB};
    const int64_t per[2] = {(nm[0] + ub - 1) / ub, (nm[1] + ub - 1) / ub};
    struct Item { int32_t cost; uint32_t code; int32_t cnt; };
    struct Plan { std::vector<std::vector<Item>> rows; int64_t ids = 0; int vmax = 0; };
    std::vector<Plan> plans(ub);
    // (a thread per 16 K majors: on a small matrix starting threads costs more than the table -- 1 ms of a 1.7 ms engine creation)
    const int table_threads = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (nm[0] + nm[1]) >> 14));
    // The plan over an index of the layouts: the row index (what the kernel walks), or the inverse index (every task).
    auto plan_over = [&](bool by_rows, int64_t &stride_out, int64_t &vis_words_out) {
    for (Plan &P : plans) P = Plan();
    parallel_for(ub, [&](int64_t b0, int64_t b1, int) {
        std::vector<Item> items;
        for (int64_t b = b0; b < b1; b++) {
            Plan &P = plans[b];
            items.clear();
            for (int sd = 0; sd < 2; sd++) {
                const int64_t m0 = std::min(nm[sd], b * per[sd]), m1 = std::min(nm[sd], m0 + per[sd]);
                for (int64_t M = m0; M < m1; M++) {
                    const std::vector<int32_t> &ptr = by_rows ? Ls[sd]->row_ptr : Ls[sd]->inv_ptr;
                    const int32_t cnt = ptr[M + 1] - ptr[M];
                    items.push_back({cnt + 4, ((uint32_t)sd << 31) | (uint32_t)(M - m0), cnt});
                    P.ids += cnt;
                }
            }
            std::sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.cost != y.cost ? x.cost > y.cost : x.code < y.code; });
            P.rows.assign(RB, {});
            // (load, row): the least loaded row takes the next item; ties go to the lowest row -- the plan is a function of the layouts alone
            std::priority_queue<std::pair<int64_t, int>, std::vector<std::pair<int64_t, int>>, std::greater<std::pair<int64_t, int>>> pq;
            for (int q = 0; q < RB; q++) pq.push({0, q});
            for (const Item &it : items) {
                auto top = pq.top(); pq.pop();
                P.rows[top.second].push_back(it);
                pq.push({top.first + it.cost, top.second});
            }
            for (int q = 0; q < RB; q++) {                  // a row visits its genes first, then its cells (k_update2's two loops)
                std::stable_sort(P.rows[q].begin(), P.rows[q].end(), [](const Item &x, const Item &y) { return (x.code >> 31) < (y.code >> 31); });
                P.vmax = std::max(P.vmax, (int)P.rows[q].size());
            }
        }
    }, table_threads);
    int64_t max_ids = 0;
    V = 1;
    for (const Plan &P : plans) { max_ids = std::max(max_ids, P.ids); V = std::max(V, (int32_t)P.vmax); }
    vis_words_out = ((int64_t)RB * V * 3 + 3) & ~(int64_t)3;
    stride_out = (vis_words_out + max_ids + 3) & ~(int64_t)3;
    };
    // Which form an engine takes stays a function of its TASKS, as before the pieces were merged (a table of rows is never
    // longer than the table of tasks): the table is sized over the inverse index first, then cut over the row index.
    int64_t stride = 0, vis_words = 0;
    if (LA.merge || LB.merge) {
        plan_over(false, stride, vis_words);
        if (stride > kUpdTabWords) return false;
    }
    plan_over(true, stride, vis_words);
    if (stride > kUpdTabWords) return false;
    ids_off = (int32_t)vis_words;
    stride4 = (int32_t)(stride / 4);
    tab.assign((size_t)ub * stride, 0u);
    parallel_for(ub, [&](int64_t b0, int64_t b1, int) {
        std::vector<int32_t> first[2];                      // first id slot of each of the block's majors, by side
        for (int64_t b = b0; b < b1; b++) {
            uint32_t *row = tab.data() + (size_t)b * stride;
            int32_t q = 0;
            for (int sd = 0; sd < 2; sd++) {
                const int64_t m0 = std::min(nm[sd], b * per[sd]), m1 = std::min(nm[sd], m0 + per[sd]);
                first[sd].assign((size_t)(m1 - m0) + 1, 0);
                for (int64_t M = m0; M < m1; M++) {
                    first[sd][M - m0] = q;
                    for (int32_t u = Ls[sd]->row_ptr[M]; u < Ls[sd]->row_ptr[M + 1]; u++) row[ids_off + q++] = Ls[sd]->row_task[u];
                }
                first[sd][m1 - m0] = q;
            }
            const Plan &P = plans[b];
            for (int rr = 0; rr < RB; rr++) {
                uint32_t *vis = row + (size_t)rr * V * 3;
                int v = 0;
                for (const Item &it : P.rows[rr]) {
                    const int sd = (int)(it.code >> 31);
                    const uint32_t loc = it.code & 0x7FFFFFFFu;
                    vis[3 * v] = it.code; vis[3 * v + 1] = (uint32_t)first[sd][loc]; vis[3 * v + 2] = (uint32_t)(first[sd][loc] + it.cnt);
                    v++;
                }
                for (; v < V; v++) { vis[3 * v] = 0xFFFFFFFFu; vis[3 * v + 1] = 0; vis[3 * v + 2] = 0; }
            }
        }
    }, table_threads);
    return true;
}

// A side as k_update2 takes it; bp_prev / bp: the tables of block partials the launch reads and writes.
UpdSide upd_side(const vbnmf_engine *e, bool gene_side, const double *bp_prev, double *bp)
{
    const SideView v = side_view(e, gene_side);
    return UpdSide{v.S.part, v.nmaj, v.l, v.ll, v.e, v.d, bp, bp_prev};
}

// Both posterior updates in one launch (kernels.h: k_update2).  Both tables of block partials alternate: the launch reads
// the previous ones and writes the others; e->bpW / e->bpH always name the latest.
int launch_update2(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge, const LoopCtl *ctl = nullptr,
                   const ControlFold *foldp = nullptr)
{
    ControlFold fold{};
    if (foldp) fold = *foldp;
    const unsigned grid = (unsigned)e->ub;
    const UpdSide W = upd_side(e, true, e->bpW, e->bpW_alt), H = upd_side(e, false, e->bpH, e->bpH_alt);
    std::swap(e->bpW, e->bpW_alt); std::swap(e->bpH, e->bpH_alt);
    UpdTable T{e->upd_tab, e->upd_stride4, e->upd_V, e->upd_ids_off};
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_update2<rt()>>(e, dim3(grid), kUpdateThreads, 0, W, H, T, e->r, e->ub, (const double *)e->csum, e->n_wg,
                                              aw, bw, ah, bh, fudge, ctl, fold);
    });
}

// ev: the array whose column sums go to the side's block partials (null: none)
int launch_prime(vbnmf_engine *e, bool gene_side, const double *ev)
{
    const SideView v = side_view(e, gene_side);
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_prime<rt()>>(e, dim3(e->ub), kUpdateThreads, 0, v.nmaj, e->r, (const double *)v.l, v.ll, ev, v.bp);
    });
}

int launch_final(vbnmf_engine *e)
{
    const double *tail = e->partitioned ? e->red + (size_t)e->n * e->R : nullptr;
    const int64_t nep = 2 * (int64_t)e->n_wg;
    e->seq += 1.0;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_final<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->ub, tail, e->bpH, e->ub, e->epart, nep, e->lgx, e->r,
                                            (double)e->n, (double)e->m_global, e->seq, e->d_out, e->h_out_dev);
    });
}

// partitioned engines: sweep output -> reduce buffer = [swsum | rowSum(eh) | sum H-terms | sum log lh | data term | lgx]
int launch_pack(vbnmf_engine *e)
{
    const int64_t cnt = e->n * e->R;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, e->stream, e->A.part, e->A.row_ptr, e->A.row_task, e->n, e->R, e->red);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(1024), 0, e->stream, e->bpH, e->ub, e->R, e->epart,
                       2 * (int64_t)e->n_wg, e->lgx, e->red + cnt);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

// ---- ML-NMF (mlnmf.h): single-side sweeps and the multiplicative updates ----
// One side's sweep alone (k_sweep1).  VB = false: the ML step's, whose cell side carries the log term (sum x log(wh));
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

int launch_vb_side(vbnmf_engine *e, bool gene_side)
{
    return launch_side_sweep<true>(e, sweep_side_args(e, gene_side), gene_side);
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
int launch_ml_tail(vbnmf_engine *e)
{
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(1024), 0, e->stream, e->bpH, e->ub, e->R, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx,
                       e->red + (size_t)e->n * e->R);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

// ... and the first exchange of a step: [sum over a gene's tasks of the gene-side partial rows (n*R) | rowSums(h_new) (R) | 0 | 0]
int launch_ml_pack(vbnmf_engine *e, const int32_t *stop)
{
    const int64_t cnt = e->n * e->R;
    hipLaunchKernelGGL(k_pack_tail, dim3((unsigned)((cnt + 255) / 256) + 1), dim3(256), 0, e->stream, e->A.part, e->A.row_ptr, e->A.row_task, e->n, e->R, e->red,
                       e->bpH, e->ub, stop);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

// ---- sparse products on the tiled layout (k_spmm) ----
int launch_spmm(vbnmf_engine *e, const SweepSide &a)
{
    return with_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return launch_lds_kernel<k_spmm<s.R, s.WIDE, s.NT, s.SP>>(e, dim3((unsigned)e->n_wg), s.NT, a);
        });
    });
}

// Wall-clock bound of the host's waits on the device (seconds): VBNMF_WAIT_TIMEOUT_S, default 300.  A wait that
// exceeds it returns VBNMF_ERR_HIP instead of spinning for ever -- e.g. a cell-partitioned run whose peer died or never
// enqueued its collective leaves this process's stream on hipErrorNotReady for good (failure modes).
double wait_timeout_s()
{
    if (const char *s = getenv("VBNMF_WAIT_TIMEOUT_S")) {
        const double v = atof(s);
        if (v > 0.0) return v;
    }
    return 300.0;
}

// Wait for k_final's sequence flag in pinned memory; falls back to the stream if it takes long.
int wait_result(vbnmf_engine *e)
{
    volatile double *flag = e->h_out + 7;
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = wait_timeout_s();
    for (long spins = 0; *flag != e->seq; spins++) {
        if (spins > 0 && (spins & 0xFFFF) == 0) {
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (waited > limit) {
                e->poisoned = true;
                return fail(VBNMF_ERR_HIP, "timed out after %.1f s (VBNMF_WAIT_TIMEOUT_S) waiting for step %.0f; the last completed step is %.0f",
                            waited, e->seq, (double)*flag);
            }
            hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) {
                if (*flag == e->seq) break;
                HIPCHECK(hipStreamSynchronize(e->stream));
                if (*flag != e->seq) return fail(VBNMF_ERR_HIP, "the step finished but its result flag was never raised");
                break;
            }
            if (q != hipErrorNotReady) return fail(VBNMF_ERR_HIP, "the step failed on the device: %s", hipGetErrorString(q));
        }
    }
    return VBNMF_OK;
}

// hipStreamSynchronize with the bound of wait_timeout_s(): for streams that may sit behind a collective whose peer is
// gone (partitioned engines).  On a timeout the engine is poisoned like the bounded waits of the step paths.
int bounded_stream_sync(vbnmf_engine *e, hipStream_t stream, const char *what)
{
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = wait_timeout_s();
    for (long spins = 0;; spins++) {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) return VBNMF_OK;
        if (q != hipErrorNotReady) return fail(VBNMF_ERR_HIP, "%s failed on the device: %s", what, hipGetErrorString(q));
        if ((spins & 0xFF) == 0xFF) {
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (waited > limit) {
                e->poisoned = true;
                return fail(VBNMF_ERR_HIP, "timed out after %.1f s (VBNMF_WAIT_TIMEOUT_S) waiting for %s", waited, what);
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
}

int harvest_timing(vbnmf_engine *e)
{
    if (e->timing && e->ev_recorded) {
        float ms = 0.f;
        HIPCHECK(hipEventSynchronize(e->ev1));
        HIPCHECK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        e->sweep_ms += ms;
        e->sweep_launches++;
        e->ev_recorded = false;
    }
    if (e->timing && e->ev2_recorded) {
        float ms = 0.f;
        HIPCHECK(hipEventSynchronize(e->ev3));
        HIPCHECK(hipEventElapsedTime(&ms, e->ev2, e->ev3));
        e->sweep_ms += ms;
        e->sweep_launches++;
        e->ev2_recorded = false;
    }
    return VBNMF_OK;
}

int use_device(const vbnmf_engine *e)
{
    // A bounded wait gave up earlier: work may still sit on the engine's streams behind a collective whose peer is gone,
    // so any call that synchronises (get_state's memcpy, set_state, another run) would block without bound -- the very
    // hang the timeout exists to prevent.  Every entry point passes through here: fail fast, only destroy is left.
    if (e->poisoned)
        return fail(VBNMF_ERR_STATE, "the engine timed out earlier (VBNMF_WAIT_TIMEOUT_S) and may still have work queued; destroy it");
    HIPCHECK(hipSetDevice(e->device));
    return VBNMF_OK;
}

// Statistics of a freshly loaded state (lw, lh, eh on the device): rowSum(eh), then the sweep (its evidence partials
// are not used); a partitioned engine leaves them in the reduce buffer for the exchange (state_finish follows).
int prime_state(vbnmf_engine *e)
{
    e->has_state = true;
    e->ids_valid = false;
    if (int rc = launch_prime(e, true, nullptr)) return rc;
    if (int rc = launch_prime(e, false, e->eh)) return rc;
    if (int rc = launch_sweep(e)) return rc;
    if (e->partitioned) { if (int rc = launch_pack(e)) return rc; }
    e->prime_pending = true;
    if (!e->partitioned) return vbnmf_engine_state_finish(e);
    return VBNMF_OK;
}

// ---------------------------------------------------------------- engine creation (vbnmf_engine_create_geom), one step per function
struct CreateArgs {
    const vbnmf_matrix *X;
    int64_t cb, ce, m_global;
    int32_t r, geometry_rank, device;
    bool whole_matrix() const { return cb == 0 && ce == X->M.m; }
};

// VBNMF_BUILD_TIMES=1: where the seconds of this creation go (offsets from here; the layouts' own phases come from layout.cpp)
struct BuildClock {
    const bool on = getenv("VBNMF_BUILD_TIMES") != nullptr;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char *what) const
    {
        if (on) fprintf(stderr, "  engine create +%.3f s  %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), what);
    }
};

// Owner of the engine under construction: destroyed on every exit of create_engine but the release into *out.
struct EngineDestroy { void operator()(vbnmf_engine *e) const { vbnmf_engine_destroy(e); } };
using EngineGuard = std::unique_ptr<vbnmf_engine, EngineDestroy>;

// A helper thread of engine creation, joined on every exit of its scope.  start() answers false when the process cannot
// have another thread (std::system_error: a thread or process limit, which parallel_for in host.cpp survives the same
// way): the caller then does the work itself.  join() may be called from several threads.
class HelperThread {
    std::thread t;
    std::mutex mu;
public:
    template <class F>
    bool start(F &&f)
    {
        try { t = std::thread(std::forward<F>(f)); } catch (const std::system_error &) { return false; }
        return true;
    }
    void join() { std::lock_guard<std::mutex> g(mu); if (t.joinable()) t.join(); }
    ~HelperThread() { join(); }
};

// The two sides' layouts while the engine is made: the matrix's cached ones (shared) or this partition's own.
struct SideLayouts {
    std::shared_ptr<const Layout> shared[2];
    Layout own[2];
    const Layout *L[2] = {nullptr, nullptr};
};

int check_create_args(const CreateArgs &a)
{
    const vbnmf_matrix *X = a.X;
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (a.r < 1 || a.r > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", a.r, VBNMF_MAX_RANK);
    if (a.geometry_rank != 0 && (a.geometry_rank < a.r || a.geometry_rank > VBNMF_MAX_RANK))
        return fail(VBNMF_ERR_BAD_ARG, "geometry rank %d cannot serve rank %d (it must lie in [rank, %d])", a.geometry_rank, a.r, VBNMF_MAX_RANK);
    if (a.cb < 0 || a.ce > X->M.m || a.cb >= a.ce)
        return fail(VBNMF_ERR_BAD_ARG, "column range [%lld, %lld) is outside the matrix", (long long)a.cb, (long long)a.ce);
    if (a.m_global < a.ce - a.cb) return fail(VBNMF_ERR_BAD_ARG, "m_global is smaller than the partition");
    if (X->M.shell && !a.whole_matrix())
        return fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries to cut a partition's layout from");
    return check_device(a.device);
}

// Dimensions, padded rank and the grids of the sweep and of the updates.
int choose_grid(vbnmf_engine *e, const CreateArgs &a)
{
    e->device = a.device;
    e->n = a.X->M.n; e->m = a.ce - a.cb; e->m_global = a.m_global; e->col_begin = a.cb;
    e->r = a.r; e->R = padded_rank(a.r);
    if (tl_pad_R > e->R) e->R = tl_pad_R;                    // (engines of several ranks meant for ONE batch: vbnmf_set_engine_padding)
    e->NT = sweep_threads(e->R);
    {
        // Blocks of the update kernels.  Fewer than one per CU on small matrices (one pass of the longer factor per block)
        // was measured and is SLOWER: 200 x 500 at rank 3 36.1 against 30.9 us per step with 2 blocks, 2 000 x 10 000 at
        // rank 5 82.7 against 79.2 with 59 -- the gather of the task partials is address work (64 scattered 8-byte loads
        // per wave instruction) that 256 CUs' texture units share and 2 do not.  VBNMF_UPDATE_BLOCKS overrides (experiments).
        int ub = kUpdateBlocks;
        if (const char *sv = getenv("VBNMF_UPDATE_BLOCKS")) { int v = atoi(sv); if (v >= 1 && v <= kUpdateBlocks) ub = v; }
        if (tl_grid_ub > 0) ub = std::min(ub, tl_grid_ub);          // (engines meant for a batch: vbnmf_set_engine_grid)
        e->ub = ub;
    }
    e->wide = !a.X->M.counts_int;
    e->partitioned = (a.ce - a.cb) != a.m_global;
    if (int rc = sweep_workgroups(a.device, e->partitioned, e->n_wg)) return rc;
    if (!e->partitioned && tl_grid_nwg > 0) e->n_wg = std::min(e->n_wg, tl_grid_nwg);
    return VBNMF_OK;
}

// The two sides' layouts, cut or taken from the matrix's cache, and their device copies.
int build_sides(vbnmf_engine *e, const CreateArgs &a, const BuildClock &clock, SideLayouts &lay)
{
    const vbnmf_matrix *X = a.X;
    const int device = a.device;
    // This process's FIRST use of the device (HIP context, first allocation, code object: 0.1-0.15 s, once) runs on a helper
    // thread beside the host's cut of the layouts and is waited for where the first upload needs it (a failure there
    // resurfaces at that upload).  Later engines find the device warm and start no thread.
    // (Where no thread can be started the warm-up runs here instead, so the flag stays set on either path.)
    static std::atomic<bool> warm_started[16];
    HelperThread warm;
    if (device < 16 && !warm_started[device].exchange(true)) {
        auto warm_up = [device] { try { (void)vbnmf_device_warmup(device); } catch (...) {} };
        if (!warm.start(warm_up)) warm_up();
    }

    std::vector<int32_t> part_order;                         // a partition orders its own cells (both sides alike)
    if (!a.whole_matrix()) part_order = compute_cell_order(X->M, a.cb, a.ce);
    // The two sides are cut (or taken from the matrix's cache) and uploaded SIDE BY SIDE: the cell side on a second host
    // thread, the gene side here.  Each cut is memory-bound well before it uses all host threads, and a side's upload
    // (200 MB of pageable memory at the headline size) runs beside the other side's cut.  Engine creation at the headline
    // size: 0.41 -> 0.3 s on the GPU box (profiles/r05_setup_times.txt).  VBNMF_SERIAL_SIDES=1: one after the other.
    clock.mark("start");
    if (a.whole_matrix() && !X->M.shell) (void)X->M.cell_order();          // (both sides start from it: formed once, here)
    clock.mark("cell order");
    auto do_side = [&](int side) -> int {
        int src = VBNMF_OK;
        const int64_t nmaj = side == 0 ? e->n : e->m, nmin = side == 0 ? e->m : e->n;
        // The geometry is that of the matrix's rank CLASS (vbnmf_matrix_plan_ranks; without a plan the class is this
        // rank's own): the ranks of a sweep share one pair of layouts, cut for the widest rows among them.
        const int Rc = std::max(e->R, a.geometry_rank ? padded_rank(a.geometry_rank) : plan_class(X, e->R));
        const int64_t nnz_part = a.whole_matrix() ? X->M.nnz : X->M.colptr[a.ce] - X->M.colptr[a.cb];
        LayoutParams lp = default_layout_params(nmaj, nmin, Rc, e->n_wg, nnz_part);
        std::shared_ptr<const Layout> &shared = lay.shared[side];
        const Layout *L = &lay.own[side];
        if (a.whole_matrix()) {                          // whole matrix: the layout may already exist (another rank, a restart)
            shared = shared_layout(X, side, lp, src);
            L = shared.get();
        } else {
            src = build_layout(X->M, a.cb, a.ce, side, lp, &part_order, lay.own[side]);
        }
        clock.mark(side == 0 ? "gene side cut" : "cell side cut");
        warm.join();
        if (!src) src = upload_side(*L, e->R, device, shared ? X : nullptr, side == 0 ? e->A : e->B);
        clock.mark(side == 0 ? "gene side uploaded" : "cell side uploaded");
        lay.L[side] = L;
        return src;
    };
    static const bool serial_sides = [] { const char *v = getenv("VBNMF_SERIAL_SIDES"); return v && v[0] == '1'; }();
    static const int side_share = [] { const char *v = getenv("VBNMF_SIDE_THREAD_SHARE"); return v ? std::max(1, atoi(v)) : 1; }();
    int rc = VBNMF_OK, rc1 = VBNMF_OK;
    std::string msg1;
    std::exception_ptr thrown1;                              // what the cell side's thread threw: rethrown on this one
    HelperThread cell_side;                                  // (declared after everything its thread touches: joined first)
    const bool side_by_side = !serial_sides && cell_side.start([&] {
        try {
            if (hipSetDevice(device) != hipSuccess) { rc1 = VBNMF_ERR_HIP; msg1 = "hipSetDevice failed on the layout thread"; return; }
            set_thread_share(side_share);
            rc1 = do_side(1);
            if (rc1) msg1 = last_error_cstr();               // (error messages are per host thread)
        } catch (...) { thrown1 = std::current_exception(); }
    });
    if (side_by_side) {
        set_thread_share(side_share);
        try { rc = do_side(0); } catch (...) { set_thread_share(1); throw; }
        set_thread_share(1);
        cell_side.join();
        if (thrown1) std::rethrow_exception(thrown1);
        if (!rc && rc1) rc = fail(rc1, "%s", msg1.c_str());
    } else {
        rc = do_side(0);
        if (!rc) rc = do_side(1);
    }
    if (rc) return rc;
    e->nnz = lay.L[0]->nnz; e->cell_perm = lay.L[0]->cell_perm;
    if (lay.L[1]->cell_perm != e->cell_perm) return fail(VBNMF_ERR_STATE, "the two sides' layouts disagree on the order of the cells");
    return VBNMF_OK;
}

int build_pair_table(vbnmf_engine *e, const SideLayouts &lay)
{
    // One launch for both posterior updates (k_update2): unpartitioned engines whose blocks' work fits the kernel's
    // table; VBNMF_NO_UPDATE_PAIR=1 keeps the two launches (A/B switch, and the form the pair is held to in
    // tests/test_gpu_update_pair.py).
    // Where it pays (round 5, same-box A/Bs in profiles/r05_pair_ab*.txt, r05_small_pair_ab.txt): the launch it saves is
    // worth ~3 us of a step whatever the size, the column sums it needs cost the gene side of the sweep ~60 + 4 R
    // instructions per SLICE.  5 000 x 20 000 at rank 8: 64.0 -> 60.1 us per step (+6 %); C2 (2 000 x 10 000 dense,
    // rank 5) +1.9 %; C1 and the PBMC-sized sample +-0; the headline (4.9e7 entries, rank 10) -0.3 %, rank 20 -1.2 %.
    // So: on up to 2.5e8 entries x padded rank, off beyond.  VBNMF_UPDATE_PAIR=1 / VBNMF_NO_UPDATE_PAIR=1 force it.
    const char *np = getenv("VBNMF_NO_UPDATE_PAIR"), *fp = getenv("VBNMF_UPDATE_PAIR");
    const bool forced = fp && fp[0] == '1';
    const bool pays = (double)lay.L[0]->nnz * (double)e->R <= 2.5e8;
    e->pair = !e->partitioned && !(np && np[0] == '1') && (forced || pays) && lay.L[0]->n_wg == lay.L[1]->n_wg;
    if (!e->pair) return VBNMF_OK;
    std::vector<uint32_t> tab;
    e->pair = build_update_table(*lay.L[0], *lay.L[1], e->ub, e->R, tab, e->upd_stride4, e->upd_V, e->upd_ids_off);
    if (!e->pair) return VBNMF_OK;
    uint32_t *d = nullptr;
    const int rc = dev_upload(&d, tab);
    e->upd_tab = reinterpret_cast<uint4 *>(d);
    return rc;
}

int create_stream_and_events(vbnmf_engine *e)
{
    // The engine's stream, before the first fill: everything that initialises the engine's own buffers below is queued ON it
    // (hipMemsetAsync), so it is ordered with the engine's kernels.  A plain hipMemset goes to the device's null stream,
    // which this non-blocking stream does not wait for, and may return before the fill has run: with several host threads
    // creating engines side by side (vb_factorize(concurrent=K)) a fill queued behind the other threads' null-stream work
    // could land AFTER the engine's first kernels had written the buffer -- zeroed block partials, a different trajectory
    // (seen once in round 5, tests/test_gpu_end_to_end.py::test_concurrent_units_give_the_same_result).
    // (Created HERE and not at the top: this process's first use of the device -- 0.1 s of HIP start-up -- then happens on the
    // cell side's thread, at its upload, beside the gene side's cut, instead of in front of both.)
    hipError_t hs;
    if ((hs = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess ||
        (hs = hipEventCreate(&e->ev0)) != hipSuccess || (hs = hipEventCreate(&e->ev1)) != hipSuccess ||
        (hs = hipEventCreate(&e->ev2)) != hipSuccess || (hs = hipEventCreate(&e->ev3)) != hipSuccess)
        return fail(VBNMF_ERR_HIP, "engine setup failed: %s", hipGetErrorString(hs));
    e->own_stream = true;
    return VBNMF_OK;
}

// The cells' order on the device, the constants of the two likelihoods, the cache policy and the sweep's LDS size.
int scalar_terms(vbnmf_engine *e, const CreateArgs &a, const BuildClock &clock)
{
    const vbnmf_matrix *X = a.X;
    if (!e->cell_perm.empty()) { if (int rc = dev_upload(&e->d_perm, e->cell_perm)) return rc; }
    e->lgx = a.whole_matrix() ? X->lgx : sum_lgamma_x1(X->M, a.cb, a.ce);
    if (a.whole_matrix()) {                           // whole matrix: formed once per matrix, not per engine (a pass over X)
        std::call_once(X->xlx_once, [&] { X->xlx = sum_xlogx(X->M, 0, X->M.m); });      // (a shell carries the value already)
        e->xlx = X->xlx;
    } else {
        e->xlx = sum_xlogx(X->M, a.cb, a.ce);
    }
    {
        // Cache policy of the entry stream (kernels.h: ld_stream).  What a step moves between two uses of a line: both sides' entry
        // streams and the per-task partial rows, written and read back.  Beyond the Infinity Cache (256 MB: the headline moves
        // 410 + 2 x 75 MB) the stream is read non-temporally so that the partial rows and the state stay on the die; inside it
        // (C2: 130 MB; 5 000 x 20 000: 61 MB) the stream itself stays resident from step to step and the default policy is the
        // faster one (profiles/r05_nt_ab.txt, r05_small_nt_ab.txt).  VBNMF_STREAM_NT=0 / 1 forces it.
        const double entry_b = e->wide ? 12.0 : 4.0;
        const double moved = entry_b * ((double)e->A.n_slots + (double)e->B.n_slots) +
                             2.0 * 8.0 * e->R * 64.0 * ((double)e->A.n_slices + (double)e->B.n_slices);
        e->stream_nt = moved > 200e6;
        if (const char *v = getenv("VBNMF_STREAM_NT")) e->stream_nt = v[0] == '1';
    }
    clock.mark("sum x log x");
    static_assert(kLdsRowBase == kLdsReserveBytes, "host and device disagree on the sweep's LDS reserve");
    e->lds_bytes = kLdsRowBase + std::max((size_t)e->A.block_width * e->A.row_slots, (size_t)e->B.block_width * e->B.row_slots) * 16;
    if (e->lds_bytes > 160 * 1024) return fail(VBNMF_ERR_BAD_ARG, "the layout's blocks need %zu bytes of LDS", e->lds_bytes);
    return VBNMF_OK;
}

// The ln table, the control blocks of the device-driven loops and the alternate tables of the folded and the pair form.
int control_blocks(vbnmf_engine *e)
{
    std::vector<LogTabEntry> tab(kLogTabSize);
    fill_log_table(tab.data());
    if (int rc = dev_upload(&e->logtab, tab)) return rc;
    if (int rc = dev_alloc(&e->ctl, 1)) return rc;
    const char *nf = getenv("VBNMF_NO_CONTROL_FOLD");
    // (partitioned engines: the evidence partials of the two sweeps must fit the fixed slots of the second all-reduce)
    e->fold = !(nf && nf[0] == '1') && (!e->partitioned || 2 * (int64_t)e->n_wg <= kEvSlots);
    if (e->fold) { if (int rc = dev_alloc(&e->ctl2, 2)) return rc; }
    if (e->fold || e->pair) {
        const size_t bpn = (size_t)kUpdateBlocks * (e->R + 2);
        if (int rc = dev_alloc(&e->bpW_alt, bpn)) return rc;
        if (int rc = dev_alloc(&e->bpH_alt, bpn)) return rc;
        if (hipMemsetAsync(e->bpW_alt, 0, bpn * sizeof(double), e->stream) != hipSuccess ||
            hipMemsetAsync(e->bpH_alt, 0, bpn * sizeof(double), e->stream) != hipSuccess) return fail(VBNMF_ERR_HIP, "hipMemsetAsync failed");
    }
    if (e->pair) {
        if (int rc = dev_alloc(&e->csl, (size_t)std::max<int64_t>(e->A.n_slices, 1) * e->R)) return rc;
        if (int rc = dev_alloc(&e->csum, (size_t)e->n_wg * e->R)) return rc;
        if (hipMemsetAsync(e->csum, 0, (size_t)e->n_wg * e->R * sizeof(double), e->stream) != hipSuccess) return fail(VBNMF_ERR_HIP, "hipMemsetAsync failed");
    }
    return VBNMF_OK;
}

// The state arrays, the reduce buffer and the result blocks, and their initial fills on the engine's stream.
int state_arrays(vbnmf_engine *e)
{
    int rc = VBNMF_OK;
    const size_t nR = (size_t)e->n * e->R, mR = (size_t)e->m * e->R;
    const size_t bpn = (size_t)kUpdateBlocks * (e->R + 2);
    e->red_count = (int64_t)nR + e->R + 4;
    if ((rc = dev_alloc(&e->lw, nR)) || (rc = dev_alloc(&e->llw, nR)) || (rc = dev_alloc(&e->ew, nR)) || (rc = dev_alloc(&e->dw, nR)) ||
        (rc = dev_alloc(&e->lh, mR)) || (rc = dev_alloc(&e->llh, mR)) || (rc = dev_alloc(&e->eh, mR)) || (rc = dev_alloc(&e->dh, mR)) ||
        (rc = dev_alloc(&e->bpW, bpn)) || (rc = dev_alloc(&e->bpH, bpn)) ||
        (rc = dev_alloc(&e->red, (size_t)red_alloc_count(e))) || (rc = dev_alloc(&e->d_out, 8)))
        return rc;
    if (e->partitioned && 2 * (int64_t)e->n_wg <= kEvSlots) { e->epart = e->red + red_ev_off(e); e->epart_in_red = true; }
    else if ((rc = dev_alloc(&e->epart, 2 * (size_t)e->n_wg))) return rc;
    hipError_t he;
    if ((he = hipHostMalloc((void **)&e->h_out, kHostOut * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (he = hipHostGetDevicePointer((void **)&e->h_out_dev, e->h_out, 0)) != hipSuccess)
        return fail(VBNMF_ERR_HIP, "engine setup failed: %s", hipGetErrorString(he));
    std::memset(e->h_out, 0, kHostOut * sizeof(double));
    if (getenv("VBNMF_DEBUG_TIMES")) {
        e->dbg_count = 2 * (size_t)e->n_wg * (2 + 2 * (e->NT / 64));
        if ((rc = dev_alloc(&e->dbg, e->dbg_count))) return rc;
    }
    if ((he = hipMemsetAsync(e->ew, 0, nR * sizeof(double), e->stream)) != hipSuccess || (he = hipMemsetAsync(e->dw, 0, nR * sizeof(double), e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(e->dh, 0, mR * sizeof(double), e->stream)) != hipSuccess || (he = hipMemsetAsync(e->bpW, 0, bpn * sizeof(double), e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(e->bpH, 0, bpn * sizeof(double), e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(e->red, 0, (size_t)red_alloc_count(e) * sizeof(double), e->stream)) != hipSuccess)
        return fail(VBNMF_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(he));
    // (sum lgamma(x + 1) into its slot of the reduce buffer: BEHIND the fill above, on the same stream; e->lgx lives as long as the engine)
    if (e->epart_in_red && (he = hipMemcpyAsync(e->red + red_ev_off(e) + kEvSlots, &e->lgx, sizeof(double), hipMemcpyHostToDevice, e->stream)) != hipSuccess)
        return fail(VBNMF_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(he));
    // creation ends with the engine's buffers in their initial state whatever else the device is doing
    if ((he = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(VBNMF_ERR_HIP, "engine setup failed: %s", hipGetErrorString(he));
    return VBNMF_OK;
}

// The steps in order.  Every exit, a return or an exception, frees the engine through `e` and joins the helper threads
// through the guards inside build_sides; only the last line hands the engine on.
int create_engine(const CreateArgs &a, vbnmf_engine **out)
{
    if (int rc = check_create_args(a)) return rc;
    HIPCHECK(hipSetDevice(a.device));
    EngineGuard e(new (std::nothrow) vbnmf_engine());
    if (!e) return fail(VBNMF_ERR_OOM, "out of host memory");
    const BuildClock clock;
    if (int rc = choose_grid(e.get(), a)) return rc;
    {
        SideLayouts lay;
        if (int rc = build_sides(e.get(), a, clock, lay)) return rc;
        if (int rc = build_pair_table(e.get(), lay)) return rc;
    }
    clock.mark("both sides, update table");
    if (int rc = create_stream_and_events(e.get())) return rc;
    if (int rc = scalar_terms(e.get(), a, clock)) return rc;
    if (int rc = control_blocks(e.get())) return rc;
    if (int rc = state_arrays(e.get())) return rc;
    clock.mark("state arrays, initial fills, done");
    *out = e.release();
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int32_t vbnmf_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return cnt;
}

void vbnmf_engine_destroy(vbnmf_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->poisoned) {
        // A wait timed out earlier.  If the streams have drained since, destroy as usual; if work is still queued (a
        // collective whose peer is gone), waiting would hang and freeing would pull memory from under queued kernels:
        // the handle is abandoned -- the process is expected to end with the error it was given.
        const bool busy = (e->stream && hipStreamQuery(e->stream) == hipErrorNotReady) ||
                          (e->cstream && hipStreamQuery(e->cstream) == hipErrorNotReady);
        (void)hipGetLastError();
        if (busy) {
            if (e->comm) for (vbnmf_engine *&q : e->comm->members) if (q == e) q = nullptr;
            return;
        }
    }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->cstream) (void)hipStreamSynchronize(e->cstream);
    if (e->comm) {
        for (vbnmf_engine *&q : e->comm->members) if (q == e) q = nullptr;
        e->comm->tables_ready = false;
    }
    free_side(e->A); free_side(e->B);
    dev_free(e->lw); dev_free(e->llw); dev_free(e->ew); dev_free(e->dw);
    dev_free(e->lh); dev_free(e->llh); dev_free(e->eh); dev_free(e->dh);
    if (!e->epart_in_red) dev_free(e->epart);
    dev_free(e->bpW); dev_free(e->bpH); dev_free(e->csl); dev_free(e->csum); dev_free(e->upd_tab);
    dev_free(e->d_perm); dev_free(e->d_ids[0]); dev_free(e->d_ids[1]); dev_free(e->d_table); dev_free(e->d_ctab); dev_free(e->svd_ws); dev_free(e->svd_status);
    dev_free(e->red); dev_free(e->red_g); dev_free(e->d_out);
    for (hipEvent_t ev : e->ev_ring) (void)hipEventDestroy(ev);
    if (e->cstream) (void)hipStreamDestroy(e->cstream); dev_free(e->dbg); dev_free(e->logtab); dev_free(e->ctl);
    dev_free(e->ctl2); dev_free(e->bpW_alt); dev_free(e->bpH_alt);
    release_stage(e);
    if (e->h_out) (void)hipHostFree(e->h_out);
    if (e->h_hist) (void)hipHostFree(e->h_hist);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev2) (void)hipEventDestroy(e->ev2);
    if (e->ev3) (void)hipEventDestroy(e->ev3);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// geometry_rank: the rank whose LDS row size the tiled layouts are cut for (>= r: several ranks of a sweep share one pair
// of layouts); 0: this rank's class in the matrix's plan (vbnmf_matrix_plan_ranks), its own geometry without one.
int vbnmf_engine_create_geom(const vbnmf_matrix *X, int64_t cb, int64_t ce, int64_t m_global, int32_t r, int32_t geometry_rank,
                             int32_t device, vbnmf_engine **out)
{
    if (!out) return fail(VBNMF_ERR_BAD_ARG, "out pointer is NULL");
    *out = nullptr;
    // nothing thrown crosses the C ABI: the guards of create_engine have joined its threads and freed the engine by here
    try {
        return create_engine(CreateArgs{X, cb, ce, m_global, r, geometry_rank, device}, out);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory building the tiled layout");
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_STATE, "engine creation failed: %s", ex.what());
    } catch (...) {
        return fail(VBNMF_ERR_STATE, "engine creation failed: unknown exception");
    }
}

int vbnmf_engine_create_part(const vbnmf_matrix *X, int64_t cb, int64_t ce, int64_t m_global, int32_t r,
                             int32_t device, vbnmf_engine **out)
{
    return vbnmf_engine_create_geom(X, cb, ce, m_global, r, 0, device, out);
}

int vbnmf_matrix_preload_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg, int32_t device)
{
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (side != 0 && side != 1) return fail(VBNMF_ERR_BAD_ARG, "side must be 0 or 1");
    if (geometry_rank < 1 || geometry_rank > VBNMF_MAX_RANK || n_wg < 1) return fail(VBNMF_ERR_BAD_ARG, "bad geometry");
    if (int rc = use_device(device)) return rc;
    const int R = padded_rank(geometry_rank);
    const int64_t nmaj = side == 0 ? X->M.n : X->M.m, nmin = side == 0 ? X->M.m : X->M.n;
    int rc = VBNMF_OK;
    try {
        const LayoutParams lp = default_layout_params(nmaj, nmin, R, n_wg, X->M.nnz);
        std::shared_ptr<const Layout> L = shared_layout(X, side, lp, rc);
        if (rc) return rc;
        DeviceSide S;                                // the shared arrays stay in the matrix's cache; the per-engine part goes
        rc = upload_side(*L, R, device, X, S, false);
        free_side(S);
    } catch (const std::bad_alloc &) {
        rc = fail(VBNMF_ERR_OOM, "out of host memory building the tiled layout");
    }
    return rc;
}

// First use of a device by this process, ahead of need: the HIP context, the first allocation and the load of the
// library's code object cost ~0.15 s the first time and nothing afterwards.  A process that has to wait for something else
// first (a sharded sweep's peers waiting for the layouts) spends that wait here.
int vbnmf_device_warmup(int32_t device)
{
    if (int rc = use_device(device)) return rc;
    double *p = nullptr;
    if (int rc = dev_alloc(&p, 1024)) return rc;
    double host[8] = {0};
    hipError_t he = hipMemcpy(p, host, sizeof host, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_test_special, dim3(1), dim3(64), 0, nullptr, 3, (int64_t)0, (const double *)p, p, (const LogTabEntry *)nullptr);   // n = 0: loads the module, touches nothing
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipDeviceSynchronize();
    dev_free(p);
    if (he != hipSuccess) return fail(VBNMF_ERR_HIP, "device warm-up failed: %s", hipGetErrorString(he));
    return VBNMF_OK;
}

int vbnmf_device_sweep_workgroups(int32_t device, int32_t *n_wg)
{
    if (!n_wg) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_device(device)) return rc;
    int v = 0;
    if (int rc = sweep_workgroups(device, false, v)) return rc;
    *n_wg = v;
    return VBNMF_OK;
}

int vbnmf_engine_create(const vbnmf_matrix *X, int32_t r, int32_t device, vbnmf_engine **out)
{
    if (!X) { if (out) *out = nullptr; return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL"); }
    return vbnmf_engine_create_part(X, 0, X->M.m, X->M.m, r, device, out);
}

int vbnmf_engine_dims(const vbnmf_engine *e, int64_t *n, int64_t *m_local, int32_t *r)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (n) *n = e->n;
    if (m_local) *m_local = e->m;
    if (r) *r = e->r;
    return VBNMF_OK;
}

int vbnmf_engine_get_stream(vbnmf_engine *e, void **stream)
{
    if (!e || !stream) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *stream = (void *)e->stream;
    return VBNMF_OK;
}

int vbnmf_engine_set_stream(vbnmf_engine *e, void *stream)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (e->own_stream) { (void)hipStreamDestroy(e->stream); e->own_stream = false; }
    e->stream = (hipStream_t)stream;
    return VBNMF_OK;
}

// column-major n x r (R matrix) -> device [n][R]; or r x m column-major (already index-major) -> [m][R].
// perm (cell-indexed arrays only): device row p holds the caller's major perm[p] (the layout's order of the cells).
// host threads for a conversion of a factor's arrays: one per 32 K elements (a 200 x 3 factor is not worth waking anyone for)
static int state_threads(int64_t nmaj, int R)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (nmaj * (int64_t)R) >> 15));
}

static void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, double *dst,
                           const std::vector<int32_t> *perm = nullptr)
{
    const int32_t *pm = (perm && !perm->empty()) ? perm->data() : nullptr;
    parallel_for(nmaj, [&](int64_t b, int64_t e, int) {
        for (int64_t M = b; M < e; M++) {
            const int64_t S = pm ? pm[M] : M;
            double *d = dst + (size_t)M * R;
            for (int k = 0; k < r; k++) d[k] = src_is_major_contiguous ? src[(size_t)S * r + k] : src[S + (size_t)k * nmaj];
            for (int k = r; k < R; k++) d[k] = 0.0;
        }
    }, state_threads(nmaj, R));
}

static void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, std::vector<double> &dst,
                           const std::vector<int32_t> *perm = nullptr)
{
    dst.resize((size_t)nmaj * R);
    to_index_major(src, nmaj, r, R, src_is_major_contiguous, dst.data(), perm);
}

static void from_index_major(const double *src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                             const std::vector<int32_t> *perm = nullptr)
{
    const int32_t *pm = (perm && !perm->empty()) ? perm->data() : nullptr;
    parallel_for(nmaj, [&](int64_t b, int64_t e, int) {
        for (int64_t M = b; M < e; M++) {
            const int64_t D = pm ? pm[M] : M;
            for (int k = 0; k < r; k++) {
                double v = src[(size_t)M * R + k];
                if (dst_is_major_contiguous) dst[(size_t)D * r + k] = v; else dst[D + (size_t)k * nmaj] = v;
            }
        }
    }, state_threads(nmaj, R));
}

static void from_index_major(const std::vector<double> &src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                             const std::vector<int32_t> *perm = nullptr)
{
    from_index_major(src.data(), nmaj, r, R, dst_is_major_contiguous, dst, perm);
}

int vbnmf_engine_set_state(vbnmf_engine *e, const double *lw, const double *lh, const double *eh)
{
    if (!e || !lw || !lh || !eh) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = use_device(e)) return rc;
    if (e->prime_pending) {
        // A partitioned engine's previous set_state returned with its copies out of the pinned staging buffer still queued
        // (state_finish waits for them): rewriting that buffer -- or handing it to the pool when it grows -- under in-flight
        // DMA would load a corrupted state without any error.  Wait for the stream first (bounded: a state exchange whose peer
        // never joined sits on it).
        if (int rc = bounded_stream_sync(e, e->stream, "the previous set_state of this engine")) return rc;
    }
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false;
    e->ml_ready = false; e->ml_prime_pending = false; e->ml_phase = 0;
    {
        // the three arrays in index-major form in ONE pinned staging buffer, three asynchronous copies, one wait
        const size_t nR = (size_t)e->n * e->R, mR = (size_t)e->m * e->R;
        if (int rc = ensure_stage(e, nR + 2 * mR)) return rc;
        double *s_lw = e->h_stage, *s_lh = s_lw + nR, *s_eh = s_lh + mR;
        to_index_major(lw, e->n, e->r, e->R, false, s_lw);
        HIPCHECK(hipMemcpyAsync(e->lw, s_lw, nR * sizeof(double), hipMemcpyHostToDevice, e->stream));
        to_index_major(lh, e->m, e->r, e->R, true, s_lh, &e->cell_perm);
        HIPCHECK(hipMemcpyAsync(e->lh, s_lh, mR * sizeof(double), hipMemcpyHostToDevice, e->stream));
        to_index_major(eh, e->m, e->r, e->R, true, s_eh, &e->cell_perm);
        HIPCHECK(hipMemcpyAsync(e->eh, s_eh, mR * sizeof(double), hipMemcpyHostToDevice, e->stream));
        // (prime_state's kernels follow on the same stream; its closing synchronise also covers the staging buffer)
    }
    return prime_state(e);
}

// The 'random' initialiser of vb_init (reference R/bayesian.R:111-115, 162-170) drawn on the device (init.h):
// lw = ew ~ Gamma(shape aw, scale bw / aw), lh = eh ~ Gamma(ah, bh / ah), dw = dh = 0, then the statistics of that state.
int vbnmf_engine_random_state(vbnmf_engine *e, double aw, double bw, double ah, double bh, uint64_t seed)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!(aw > 0.0) || !(bw > 0.0) || !(ah > 0.0) || !(bh > 0.0)) return fail(VBNMF_ERR_BAD_ARG, "Gamma shapes and means must be positive");
    if (int rc = use_device(e)) return rc;
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false;
    e->ml_ready = false; e->ids_valid = false; e->ml_prime_pending = false; e->ml_phase = 0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t nw = e->n * e->R, nh = e->m * e->R;
    hipLaunchKernelGGL(k_gamma_init, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, e->stream, e->lw, e->ew, e->dw, e->n, (int64_t)0, e->r, e->R, aw, bw, 0u, k0, k1, (const int32_t *)nullptr);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_gamma_init, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, e->stream, e->lh, e->eh, e->dh, e->m, e->col_begin, e->r, e->R, ah, bh, 1u, k0, k1, (const int32_t *)e->d_perm);
    HIPCHECK(hipGetLastError());
    return prime_state(e);
}

int vbnmf_engine_state_finish(vbnmf_engine *e)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!e->prime_pending) return fail(VBNMF_ERR_STATE, "state_finish without a pending set_state");
    if (int rc = use_device(e)) return rc;
    if (e->partitioned) {                            // the state exchange sits on this stream: a peer that never joins it must not hang us
        if (int rc = bounded_stream_sync(e, e->stream, "the state exchange of a partitioned engine")) return rc;
    } else {
        HIPCHECK(hipStreamSynchronize(e->stream));
    }
    if (int rc = harvest_timing(e)) return rc;
    e->sweep_ms = 0.0; e->sweep_launches = 0;        // the priming sweep is not a step
    e->prime_pending = false;
    e->stats_ready = true;
    return VBNMF_OK;
}

int vbnmf_engine_step_local(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;                                   // (first: an engine that timed out says so, whatever its state)
    if (!e->has_state || !e->stats_ready) return fail(VBNMF_ERR_STATE, "step before set_state (or before state_finish on a partitioned engine)");
    if (e->step_pending) return fail(VBNMF_ERR_STATE, "step_local called twice without step_finish");
    if (e->pair) {
        if (int rc = launch_update2(e, aw, bw, ah, bh, fudge)) return rc;
    } else {
        if (int rc = launch_update(e, true, aw, bw, fudge)) return rc;
        if (int rc = launch_update(e, false, ah, bh, fudge)) return rc;
    }
    if (int rc = launch_sweep(e)) return rc;
    if (e->partitioned) { if (int rc = launch_pack(e)) return rc; }
    e->step_pending = true;
    return VBNMF_OK;
}

int vbnmf_engine_reduce_buffer(vbnmf_engine *e, void **device_ptr, int64_t *count)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (device_ptr) *device_ptr = e->red;
    if (count) *count = e->red_count;
    return VBNMF_OK;
}

int vbnmf_engine_reduce_tail(const vbnmf_engine *e, int64_t *offset, int64_t *count)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (offset) *offset = e->n * e->R;
    if (count) *count = e->red_count - e->n * e->R;
    return VBNMF_OK;
}

int vbnmf_engine_step_finish(vbnmf_engine *e, double *lkh, double *stats)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = use_device(e)) return rc;
    if (!e->step_pending) return fail(VBNMF_ERR_STATE, "step_finish without step_local");
    if (int rc = launch_final(e)) return rc;
    if (int rc = wait_result(e)) return rc;
    e->step_pending = false;
    if (int rc = harvest_timing(e)) return rc;
    if (lkh) *lkh = e->h_out[0];
    if (stats) for (int q = 0; q < 4; q++) stats[q] = e->h_out[1 + q];
    return VBNMF_OK;
}

int vbnmf_engine_step(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge, double *lkh, double *stats)
{
    if (e && e->partitioned) return fail(VBNMF_ERR_STATE, "a partitioned engine needs step_local / all-reduce / step_finish");
    if (int rc = vbnmf_engine_step_local(e, aw, bw, ah, bh, fudge)) return rc;
    return vbnmf_engine_step_finish(e, lkh, stats);
}

// ---------------------------------------------------------------- device-driven loops
}  // extern "C"

namespace {

// Pinned, device-visible history of a device-driven loop (k_control / k_ml_control write one row per step straight
// into host memory); kept by the engine and grown on demand, so a run allocates nothing.
int ensure_history(vbnmf_engine *e, size_t doubles)
{
    if (doubles <= e->h_hist_count) return VBNMF_OK;
    if (e->h_hist) {
        HIPCHECK(hipStreamSynchronize(e->stream));
        (void)hipHostFree(e->h_hist);
        e->h_hist = nullptr; e->h_hist_dev = nullptr; e->h_hist_count = 0;
    }
    const size_t want = std::max<size_t>(doubles, 9 * 1024);
    hipError_t he = hipHostMalloc((void **)&e->h_hist, want * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
    if (he == hipSuccess) he = hipHostGetDevicePointer((void **)&e->h_hist_dev, e->h_hist, 0);
    if (he != hipSuccess) {
        (void)hipGetLastError();
        if (e->h_hist) { (void)hipHostFree(e->h_hist); e->h_hist = nullptr; }
        return fail(VBNMF_ERR_OOM, "pinned history buffer (%zu bytes): %s", want * sizeof(double), hipGetErrorString(he));
    }
    e->h_hist_count = want;
    return VBNMF_OK;
}

// What a partitioned engine needs beside its own stream: the stream the all-reduces go on, the receive buffer, and
// a ring of events (five per step, steps queued at most three batches of eight ahead: 160 never wraps onto a pending one).
int ensure_comm_resources(vbnmf_engine *e)
{
    if (!e->cstream) HIPCHECK(hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking));
    if (!e->red_g) {
        if (int rc = dev_alloc(&e->red_g, (size_t)red_alloc_count(e))) return rc;
        HIPCHECK(hipMemsetAsync(e->red_g, 0, (size_t)red_alloc_count(e) * sizeof(double), e->stream));      // (ordered with the engine's kernels; see engine creation)
        HIPCHECK(hipStreamSynchronize(e->stream));
    }
    while (e->ev_ring.size() < 160) {
        hipEvent_t ev;
        HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->ev_ring.push_back(ev);
    }
    return VBNMF_OK;
}

hipEvent_t next_event(vbnmf_engine *e)
{
    hipEvent_t ev = e->ev_ring[e->ev_next];
    e->ev_next = (e->ev_next + 1) % e->ev_ring.size();
    return ev;
}

int rccl_check(ncclResult_t r, const char *what)
{
    if (r == ncclSuccess) return VBNMF_OK;
    RcclApi &api = rccl_api();
    return fail(VBNMF_ERR_HIP, "%s failed: %s", what, api.GetErrorString ? api.GetErrorString(r) : "RCCL error");
}

int launch_control(vbnmf_engine *e, double *hist_dev, bool reduced)
{
    const int64_t nep = 2 * (int64_t)e->n_wg;
    const double *tail = reduced ? e->red_g + (size_t)e->n * e->R : nullptr;
    const double *small = reduced ? e->red_g + (size_t)e->n * e->R + e->R + 2 : nullptr;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_control<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->bpH, e->ub, e->epart, nep, e->lgx, e->r, (double)e->n,
                                              (double)e->m_global, e->ctl, hist_dev, e->h_out_dev, tail, small);
    });
}

// The engines one device-driven loop advances together: a single engine, or the partition engines of a local group.
struct LoopGroup {
    vbnmf_engine **e;
    int count;
    vbnmf_comm *comm;      // null: one unpartitioned engine
};

// Device pointer tables of a local group's send / receive buffers (built once all members are attached).
int group_tables(vbnmf_comm *c)
{
    if (c->tables_ready) return VBNMF_OK;
    const int P = (int)c->members.size();
    std::vector<const double *> sb(P), ss(P);
    std::vector<double *> rb(P), rs(P);
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = c->members[p];
        if (int rc = ensure_comm_resources(e)) return rc;
        // second exchange of a device-driven step: the evidence slots behind the reduce buffer (control step folded into
        // the next update), or the two doubles k_tail_data forms (VBNMF_NO_CONTROL_FOLD=1)
        const size_t off = e->fold ? (size_t)red_ev_off(e) : (size_t)e->n * e->R + e->R + 2;
        sb[p] = e->red; rb[p] = e->red_g; ss[p] = e->red + off; rs[p] = e->red_g + off;
    }
    dev_free(c->d_send_big); dev_free(c->d_send_small); dev_free(c->d_recv_big); dev_free(c->d_recv_small);
    c->d_send_big = c->d_send_small = nullptr; c->d_recv_big = c->d_recv_small = nullptr;      // (tables of an earlier membership)
    if (int rc = dev_alloc(&c->d_send_big, (size_t)P)) return rc;
    if (int rc = dev_alloc(&c->d_send_small, (size_t)P)) return rc;
    if (int rc = dev_alloc(&c->d_recv_big, (size_t)P)) return rc;
    if (int rc = dev_alloc(&c->d_recv_small, (size_t)P)) return rc;
    HIPCHECK(hipMemcpy(c->d_send_big, sb.data(), P * sizeof(void *), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(c->d_send_small, ss.data(), P * sizeof(void *), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(c->d_recv_big, rb.data(), P * sizeof(void *), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(c->d_recv_small, rs.data(), P * sizeof(void *), hipMemcpyHostToDevice));
    c->tables_ready = true;
    return VBNMF_OK;
}

// The fold of step t (1-based) of an unpartitioned engine's run: the control step of the previous sweep, folded into this
// step's gene-side update (kernels.h: ControlFold).  Step t + 1's fold, with bpW_prev and control_only set, is the control
// step alone behind the last step.
ControlFold vb_fold(const vbnmf_engine *e, int t, bool hist)
{
    ControlFold f{};
    f.prev = e->ctl2 + ((t - 1) & 1); f.next = e->ctl2 + (t & 1);
    f.epart = e->epart; f.nepart = 2 * (int64_t)e->n_wg;
    f.lgx = e->lgx; f.n = (double)e->n; f.m_global = (double)e->m_global;
    f.history = hist ? e->h_hist_dev : nullptr; f.out_host = e->h_out_dev;
    f.do_control = t > 1 ? 1 : 0;
    return f;
}

// The same for the ML loop: the control step of the previous cell-side sweep, folded into step t's H update (mlnmf.h: MlFold);
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

// One step of the device-driven VB loop, queued on every engine of the group.
//   unpartitioned : k_update(W, + the control step of the previous sweep) k_update(H) k_sweep(both sides)
//   partitioned   : k_update(W <- reduced statistics, + the control step of the previous sweeps) k_update(H) | gene-side sweep
//                   | k_pack_tail | event
//                   -> comm stream: all-reduce [swsum | rowSum(eh) | 2 scalars]     (RCCL, or k_group_sum)
//                   || main stream: cell-side sweep
//                   -> main stream: all-reduce [evidence slots | sum lgamma(x+1)]   (behind an event after the first one)
// so the n*R-double exchange travels while the cell-side sweep runs and only the small one sits
// between the sweep and the next update.  (VBNMF_NO_CONTROL_FOLD=1: k_tail_data, a two-double exchange and k_control
// close the step instead.)  The all-reduces are out of place (red -> red_g): steps queued past the stop leave `red`
// untouched, so repeating them reproduces the same sums.
int queue_vb_step(const LoopGroup &G, double fudge, bool hist, int max_it)
{
    if (!G.comm && G.e[0]->fold) {
        // k_update(W, with the control step of the PREVIOUS sweep folded in)  k_update(H)  k_sweep ; behind the last step of
        // the run, the control step alone (kernels.h: ControlFold)
        vbnmf_engine *e = G.e[0];
        const int t = ++e->fold_step;                               // 1-based step of this run
        ControlFold f = vb_fold(e, t, hist);
        int rc;
        if (e->pair) {
            // k_update2(W and H, with the control step of the previous sweep folded in)  k_sweep : two launches per step
            rc = launch_update2(e, 0, 0, 0, 0, fudge, nullptr, &f);
            e->stop_ptr = &f.next->stop;
        } else {
            f.bpW_prev = e->bpW;
            std::swap(e->bpW, e->bpW_alt);                          // this step's gene-side partials go to the other table
            rc = launch_update(e, true, 0, 0, fudge, nullptr, &f);
            e->stop_ptr = &f.next->stop;
            if (!rc) rc = launch_update(e, false, 0, 0, fudge, f.next);
        }
        if (!rc) rc = launch_sweep(e);
        if (!rc && t == max_it) {
            ControlFold g = vb_fold(e, t + 1, hist);
            g.bpW_prev = e->bpW; g.control_only = 1;
            rc = launch_update(e, true, 0, 0, fudge, nullptr, &g);
        }
        return rc;
    }
    if (!G.comm) {
        vbnmf_engine *e = G.e[0];
        int rc;
        if (e->pair) rc = launch_update2(e, 0, 0, 0, 0, fudge, e->ctl);
        else {
            rc = launch_update(e, true, 0, 0, fudge, e->ctl);
            if (!rc) rc = launch_update(e, false, 0, 0, fudge, e->ctl);
        }
        if (!rc) rc = launch_sweep(e);
        if (!rc) rc = launch_control(e, hist ? e->h_hist_dev : nullptr, false);
        return rc;
    }
    vbnmf_comm *c = G.comm;
    const int P = G.count;
    vbnmf_engine *L = G.e[0];                                  // leader: owner of the comm stream used by a local group
    const int64_t nbig = L->n * L->R + L->R + 2;
    const bool fold = L->fold;
    hipEvent_t evA[64], evB[64];
    ControlFold last{};                                        // (fold) the control-only launch behind step max_it
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        int rc;
        if (fold) {
            // k_update(W <- reduced statistics, with the control step of the PREVIOUS sweeps folded in: no k_control launch
            // and no k_tail_data between the second all-reduce and the next update -- that exchange carries the evidence
            // partials of the two sweeps as they are, element-wise, and the fold adds them up)
            const int t = ++e->fold_step;
            ControlFold f{};
            f.prev = e->ctl2 + ((t - 1) & 1); f.next = e->ctl2 + (t & 1);
            f.bpW_prev = e->bpW; f.nbW = e->ub;
            std::swap(e->bpW, e->bpW_alt);
            f.tail_in = e->red_g + (size_t)e->n * e->R;
            f.epart = e->red_g + red_ev_off(e); f.nepart = kEvSlots;
            f.lgx_in = e->red_g + red_ev_off(e) + kEvSlots;
            f.lgx = 0.0; f.n = (double)e->n; f.m_global = (double)e->m_global;
            f.history = hist && p == 0 ? e->h_hist_dev : nullptr; f.out_host = e->h_out_dev;
            f.do_control = t > 1 ? 1 : 0;
            rc = launch_update(e, true, 0, 0, fudge, nullptr, &f);
            e->stop_ptr = &f.next->stop;
            if (!rc) rc = launch_update(e, false, 0, 0, fudge, f.next);
            if (t == max_it) {
                last = f;
                last.prev = f.next; last.next = e->ctl2 + ((t + 1) & 1);
                last.do_control = 1; last.control_only = 1;
            }
        } else {
            rc = launch_update(e, true, 0, 0, fudge, e->ctl);
            if (!rc) rc = launch_update(e, false, 0, 0, fudge, e->ctl);
        }
        if (!rc) rc = launch_vb_side(e, true);
        if (rc) return rc;
        const int32_t *stop = e->stop_ptr ? e->stop_ptr : &e->ctl->stop;
        // The gene-side partials are packed into the send buffer (k_pack_tail: a gather of 100 MB of task rows at C5, 26 us
        // with the chip to itself, + the cell side's column sums) on the MAIN stream, between the two sweeps: the all-reduce
        // of n * R doubles must travel WHILE the cell-side sweep runs, and a pack queued beside that sweep on the comm
        // stream is starved by its persistent workgroups (profiles/r04_c5_step_timeline.txt: 168 us, ending after the
        // sweep -- the collective would start when the sweep is over).  Round 4's first half ran it on the comm stream; on
        // the final build that is slower for a local group of eight as well, 0.373-0.376 against 0.370-0.371 ms per
        // partition step on the same box.
        const int64_t cnt = e->n * e->R;
        hipLaunchKernelGGL(k_pack_tail, dim3((unsigned)((cnt + 255) / 256) + 1), dim3(256), 0, e->stream, e->A.part, e->A.row_ptr, e->A.row_task, e->n, e->R, e->red,
                           e->bpH, e->ub, stop);
        HIPCHECK(hipGetLastError());
        evA[p] = next_event(e);
        HIPCHECK(hipEventRecord(evA[p], e->stream));
    }
    if (c->kind == 0) {
        HIPCHECK(hipStreamWaitEvent(L->cstream, evA[0], 0));
        if (int rc = rccl_check(rccl_api().AllReduce(L->red, L->red_g, (size_t)nbig, ncclDouble, ncclSum, c->nc, L->cstream), "ncclAllReduce")) return rc;
    } else {
        for (int p = 0; p < P; p++) HIPCHECK(hipStreamWaitEvent(L->cstream, evA[p], 0));
        hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((nbig + 255) / 256)), dim3(256), 0, L->cstream, c->d_send_big, c->d_recv_big, P, nbig);
        HIPCHECK(hipGetLastError());
    }
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        if (int rc = launch_vb_side(e, false)) return rc;
        if (!fold) {
            hipLaunchKernelGGL(k_tail_data, dim3(1), dim3(1024), 0, e->stream, e->epart, 2 * (int64_t)e->n_wg, e->lgx, e->red + nbig, &e->ctl->stop);
            HIPCHECK(hipGetLastError());
        }
        if (p > 0) {                                           // (an event costs the stream a barrier packet: only where another stream waits on it)
            evB[p] = next_event(e);
            HIPCHECK(hipEventRecord(evB[p], e->stream));
        }
    }
    // The second exchange sits between the cell-side sweep and the next update on every rank's critical path, so it is
    // issued on the leader's MAIN stream: no hand-over to the comm stream and back (two cross-queue waits, microseconds
    // each, for a collective of a few KB).  It follows the first exchange through an event recorded behind it on the comm
    // stream -- long satisfied by then -- so the two collectives of a step never overlap and every rank issues them in the
    // same order.
    hipEvent_t evBig = next_event(L);
    HIPCHECK(hipEventRecord(evBig, L->cstream));
    HIPCHECK(hipStreamWaitEvent(L->stream, evBig, 0));
    hipEvent_t evD = P > 1 ? next_event(L) : nullptr;
    const int64_t nsmall = fold ? kEvSlots + 1 : 2;
    if (c->kind == 0) {
        const int64_t off = fold ? red_ev_off(L) : nbig;
        if (int rc = rccl_check(rccl_api().AllReduce(L->red + off, L->red_g + off, (size_t)nsmall, ncclDouble, ncclSum, c->nc, L->stream), "ncclAllReduce")) return rc;
    } else {
        for (int p = 1; p < P; p++) HIPCHECK(hipStreamWaitEvent(L->stream, evB[p], 0));
        hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((nsmall + 255) / 256)), dim3(256), 0, L->stream, c->d_send_small, c->d_recv_small, P, nsmall);
        HIPCHECK(hipGetLastError());
    }
    if (evD) HIPCHECK(hipEventRecord(evD, L->stream));
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        if (evD && e->stream != L->stream) HIPCHECK(hipStreamWaitEvent(e->stream, evD, 0));
        if (!fold) { if (int rc = launch_control(e, hist && p == 0 ? e->h_hist_dev : nullptr, true)) return rc; }
        else if (last.control_only) {                           // behind the last step of the run: the control step alone
            ControlFold g = last;
            g.prev = e->ctl2 + (e->fold_step & 1); g.next = e->ctl2 + ((e->fold_step + 1) & 1);
            g.bpW_prev = e->bpW; g.nbW = e->ub;
            g.tail_in = e->red_g + (size_t)e->n * e->R;
            g.epart = e->red_g + red_ev_off(e); g.lgx_in = e->red_g + red_ev_off(e) + kEvSlots;
            g.history = hist && p == 0 ? e->h_hist_dev : nullptr; g.out_host = e->h_out_dev;
            if (int rc = launch_update(e, true, 0, 0, fudge, nullptr, &g)) return rc;
        }
    }
    return VBNMF_OK;
}

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
            const bool stopped = ho[6] != 0.0;
            all_stopped = all_stopped && stopped;
            ok = ok && (stopped || (int)ho[7] >= target);
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
                                "the last completed step is %d (%d queued)", waited, target, (int)e0->h_out[7], queued);
                }
                if (int rc = idle_check(target)) return rc;
            }
        }
        volatile double *ho = e0->h_out;
        if (replicated ? ho[6] != 0.0 && (int)ho[5] <= target : all_stopped) break;
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
            hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(1), 0, x->stream, x->fold && !plain_ctl ? x->ctl2 : x->ctl, ctl(p));
            x->fold_step = 0;
            volatile double *ho = x->h_out;
            ho[5] = 0.0; ho[6] = 0.0; ho[7] = 0.0;
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
            x->seq = 0.0; x->h_out[7] = 0.0;                       // the step path's sequence flag restarts
        }
        return rc;
    }
};

// The results the last live control step of each of `count` engines left in its h_out: [5] steps, [6] reason, [0] the last
// likelihood (lk: lkh of the VB loop, lk of the ML loop -- [0] itself stays, ml_likelihood() keeps answering for the pair
// held now), [12] lk0 and [8..11] the hyper-parameters (VB); history: `rows` rows of `width` doubles per engine.
void read_out(vbnmf_engine *const *engs, int count, int32_t *it_out, double *lk0_out, double *lk_out, int32_t *reason_out,
              double *hyper, double *history, int64_t rows, int width)
{
    for (int b = 0; b < count; b++) {
        const double *ho = engs[b]->h_out;
        const int it = (int)ho[5];
        if (hyper) for (int q = 0; q < 4; q++) hyper[(size_t)b * 4 + q] = ho[8 + q];
        if (it_out) it_out[b] = it;
        if (lk0_out) lk0_out[b] = ho[12];
        if (lk_out) lk_out[b] = ho[0];
        if (reason_out) reason_out[b] = (int)ho[6];
        if (history && it > 0) std::memcpy(history + (size_t)b * rows * width, engs[b]->h_hist, (size_t)it * width * sizeof(double));
    }
}

// The control block of a VB loop: hyper[0..3] and flags[0..3] as hyper.update
LoopCtl vb_ctl(const double *hyper, const int32_t *flags, double tol, int32_t max_it, int32_t n0, int32_t dn)
{
    LoopCtl c{};
    for (int q = 0; q < 4; q++) { c.hyper[q] = hyper[q]; c.flags[q] = flags[q] ? 1 : 0; }
    c.lk0 = 0.0;                                                   // :336
    c.tol = tol; c.max_it = max_it; c.n0 = n0; c.dn = dn;
    return c;
}

// ... of an ML loop
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
        const int it = (int)e->h_out[5];
        e->ids_cur = it & 1;
        e->ids_valid = it >= 1;
        if (changes && it > 0) std::memcpy(changes + (size_t)b * changes_rows, e->h_hist + e->chg_off, (size_t)it * sizeof(int64_t));
    }
}

// The four hyper-parameters a device-driven loop starts from: finite and > 0, or the Newton iteration of hyper_update
// (dev_hyper_update_pair) would be handed a shape its special functions are not written for.  Checked before any launch.
int check_hyper(const double *hyper)
{
    for (int q = 0; q < 4; q++)
        if (!(hyper[q] > 0.0) || !std::isfinite(hyper[q]))
            return fail(VBNMF_ERR_BAD_ARG, "aw, bw, ah and bh must be finite and > 0 (got %g, %g, %g, %g)", hyper[0], hyper[1], hyper[2], hyper[3]);
    return VBNMF_OK;
}

int run_group(const LoopGroup &G, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0, int32_t dn,
              const int32_t *flags, int32_t *it_out, double *lk0_out, double *lkh_out, int32_t *reason_out,
              double *history, int64_t history_rows)
{
    if (!hyper || !flags) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_hyper(hyper)) return rc;
    if (max_it < 1 || dn < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it and dn must be >= 1");
    if (history && history_rows < max_it) return fail(VBNMF_ERR_BAD_ARG, "history needs max_it rows of 9 doubles");
    for (int p = 0; p < G.count; p++) {
        vbnmf_engine *e = G.e[p];
        if (int rc = use_device(e)) return rc;
        if (!e->has_state || !e->stats_ready) return fail(VBNMF_ERR_STATE, "run before set_state (or before the state exchange of a partitioned engine)");
        if (e->step_pending) return fail(VBNMF_ERR_STATE, "run between step_local and step_finish");
    }
    vbnmf_engine *e0 = G.e[0];
    if (int rc = use_device(e0)) return rc;
    if (history) { if (int rc = ensure_history(e0, (size_t)max_it * 9)) return rc; }

    const LoopCtl c = vb_ctl(hyper, flags, tol, max_it, n0, dn);
    RunScope S{G.e, G.count};
    if (int rc = S.begin([&](int) { return c; })) return rc;
    if (G.comm)                                                    // the reduced statistics of the loaded state
        for (int p = 0; p < G.count; p++) {
            vbnmf_engine *e = G.e[p];
            e->red_in = e->red_g;
            (void)hipMemcpyAsync(e->red_g, e->red, (size_t)e->red_count * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
        }
    int rc = drive_loop(G.e, 1, true, max_it, e0->fold, [&](int) { return queue_vb_step(G, fudge, history != nullptr, max_it); });
    rc = S.end(rc);
    if (G.comm && !e0->poisoned)                                   // host-stepped calls read the reduced statistics from `red`
        for (int p = 0; p < G.count; p++) {
            vbnmf_engine *e = G.e[p];
            (void)hipMemcpy(e->red, e->red_g, (size_t)e->red_count * sizeof(double), hipMemcpyDeviceToDevice);
            e->red_in = nullptr;
        }
    if (rc) return rc;
    read_out(G.e, 1, it_out, lk0_out, lkh_out, reason_out, hyper, history, history_rows, 9);
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// Device-driven form of the per-rank loop of vb_iterate (reference R/bayesian.R:336-352).
int vbnmf_engine_run(vbnmf_engine *e, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0, int32_t dn,
                     const int32_t *flags, int32_t *it_out, double *lk0_out, double *lkh_out, int32_t *reason_out,
                     double *history, int64_t history_rows)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    LoopGroup G{&e, 1, nullptr};
    if (e->partitioned) {
        if (!e->comm || e->comm->kind != 0)
            return fail(VBNMF_ERR_STATE, "the device-driven loop of a partitioned engine needs an RCCL communicator (vbnmf_engine_attach_comm), or vbnmf_group_run for a local group");
        if (int rc = use_device(e)) return rc;
        if (int rc = ensure_comm_resources(e)) return rc;
        G.comm = e->comm;
    }
    return run_group(G, hyper, fudge, max_it, tol, n0, dn, flags, it_out, lk0_out, lkh_out, reason_out, history, history_rows);
}

}  // extern "C"

// ---------------------------------------------------------------- a batch of engines stepped by one launch (kernels.h: k_update2_batch)
namespace {

constexpr int kBatchMax = 64;

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

}  // namespace

extern "C" {

// Grids of the engines the CALLING host thread creates from now on: `n_wg` persistent workgroups of the sweep (the layouts
// are cut for that many) and `update_blocks` blocks of the update; 0 = the default (one per CU).  For the engines of a batch:
// B engines step in one launch of B x grid workgroups, so a batch of 8 wants grids of 32 -- a single small engine is
// faster on 256 (every block's share of a 15 us kernel is its prologue), eight of them are not (eight such blocks per CU).
// The grid fixes the order of the block-wise sums: engines of different grids agree to rounding, not bit for bit.
int vbnmf_set_engine_grid(int32_t n_wg, int32_t update_blocks)
{
    if (n_wg < 0 || update_blocks < 0 || update_blocks > kUpdateBlocks) return fail(VBNMF_ERR_BAD_ARG, "grid sizes must lie in [0, %d]", kUpdateBlocks);
    tl_grid_nwg = n_wg; tl_grid_ub = update_blocks;
    return VBNMF_OK;
}

// Row width of the engines the CALLING host thread creates from now on: their factors are stored `padded_rank` columns wide
// (a padded rank the kernels are built for, >= the engine's own; 0: back to the rank's own width), the columns beyond the rank
// held at zero as the padding always is.  Engines of DIFFERENT ranks made this way share kernels, layouts and update table, i.e.
// a batch: a whole rank sweep of a small matrix steps in one launch.  The width fixes the update's thread mapping, hence the
// order of its block-wise sums: a padded engine agrees with the unpadded one to rounding, not bit for bit.
int vbnmf_set_engine_padding(int32_t padded)
{
    if (padded != 0 && (padded < 2 || padded > VBNMF_MAX_RANK || padded_rank(padded) != padded))
        return fail(VBNMF_ERR_BAD_ARG, "%d is not a padded rank (even up to 32, a multiple of 8 up to 64, of 16 up to %d)", padded, VBNMF_MAX_RANK);
    tl_pad_R = padded;
    return VBNMF_OK;
}

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

}  // namespace

extern "C" {

}  // extern "C"

namespace {

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

// ---------------------------------------------------------------- communicators (comm.h)
int vbnmf_comm_unique_id(void *id, int64_t bytes)
{
    if (!id || bytes < (int64_t)sizeof(ncclUniqueId)) return fail(VBNMF_ERR_BAD_ARG, "the id buffer needs %d bytes", (int)sizeof(ncclUniqueId));
    RcclApi &api = rccl_api();
    if (!api.error.empty()) return fail(VBNMF_ERR_NO_DEVICE, "%s", api.error.c_str());
    ncclUniqueId u;
    if (int rc = rccl_check(api.GetUniqueId(&u), "ncclGetUniqueId")) return rc;
    std::memcpy(id, &u, sizeof u);
    return VBNMF_OK;
}

int vbnmf_comm_create(const void *id, int64_t bytes, int32_t nranks, int32_t rank, int32_t device, vbnmf_comm **out)
{
    if (!out) return fail(VBNMF_ERR_BAD_ARG, "out pointer is NULL");
    *out = nullptr;
    if (!id || bytes < (int64_t)sizeof(ncclUniqueId)) return fail(VBNMF_ERR_BAD_ARG, "the id buffer needs %d bytes", (int)sizeof(ncclUniqueId));
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [0, %d)", rank, nranks);
    if (int rc = check_device(device)) return rc;
    RcclApi &api = rccl_api();
    if (!api.error.empty()) return fail(VBNMF_ERR_NO_DEVICE, "%s", api.error.c_str());
    HIPCHECK(hipSetDevice(device));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    vbnmf_comm *c = new (std::nothrow) vbnmf_comm();
    if (!c) return fail(VBNMF_ERR_OOM, "out of host memory");
    c->kind = 0; c->nranks = nranks; c->rank = rank; c->device = device;
    if (int rc = rccl_check(api.CommInitRank(&c->nc, nranks, u, rank), "ncclCommInitRank")) { delete c; return rc; }
    *out = c;
    return VBNMF_OK;
}

int vbnmf_comm_create_local(int32_t nranks, int32_t device, vbnmf_comm **out)
{
    if (!out) return fail(VBNMF_ERR_BAD_ARG, "out pointer is NULL");
    *out = nullptr;
    if (nranks < 1 || nranks > 64) return fail(VBNMF_ERR_BAD_ARG, "a local group holds 1..64 partitions");
    if (int rc = check_device(device)) return rc;
    vbnmf_comm *c = new (std::nothrow) vbnmf_comm();
    if (!c) return fail(VBNMF_ERR_OOM, "out of host memory");
    c->kind = 1; c->nranks = nranks; c->rank = 0; c->device = device;
    *out = c;
    return VBNMF_OK;
}

void vbnmf_comm_destroy(vbnmf_comm *c)
{
    if (!c) return;
    for (vbnmf_engine *e : c->members) if (e && e->comm == c) e->comm = nullptr;
    if (c->kind == 0 && c->nc) (void)rccl_api().CommDestroy(c->nc);
    dev_free(c->d_send_big); dev_free(c->d_send_small); dev_free(c->d_recv_big); dev_free(c->d_recv_small);
    delete c;
}

int vbnmf_comm_info(const vbnmf_comm *c, int32_t *nranks, int32_t *rank, int32_t *kind)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "communicator handle is NULL");
    if (nranks) *nranks = c->nranks;
    if (rank) *rank = c->rank;
    if (kind) *kind = c->kind;
    return VBNMF_OK;
}

int vbnmf_engine_attach_comm(vbnmf_engine *e, vbnmf_comm *c)
{
    if (!e || !c) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (e->comm) return fail(VBNMF_ERR_STATE, "the engine already has a communicator");
    {   // engines that were destroyed while attached leave empty seats: a communicator none of whose engines is alive starts over
        bool any = false;
        for (vbnmf_engine *q : c->members) any |= q != nullptr;
        if (!any) c->members.clear();
    }
    if (e->device != c->device) return fail(VBNMF_ERR_BAD_ARG, "engine on device %d, communicator on device %d", e->device, c->device);
    if (c->kind == 0 && !c->members.empty()) return fail(VBNMF_ERR_STATE, "an RCCL communicator serves one engine per process");
    if (c->kind == 1 && (int)c->members.size() >= c->nranks) return fail(VBNMF_ERR_STATE, "the local group is full");
    if (c->kind == 1 && !c->members.empty() && (c->members[0]->n != e->n || c->members[0]->R != e->R || c->members[0]->m_global != e->m_global))
        return fail(VBNMF_ERR_BAD_ARG, "partition engines of one group must share genes, rank and the global cell count");
    if (int rc = use_device(e)) return rc;
    if (int rc = ensure_comm_resources(e)) return rc;
    e->comm = c;
    e->comm_rank = c->kind == 0 ? c->rank : (int)c->members.size();
    c->members.push_back(e);
    c->tables_ready = false;
    return VBNMF_OK;
}

// In-place all-reduce of the reduce buffer on the engine's stream: the exchange between step_local and step_finish
// (and between set_state and state_finish) of a host-stepped partitioned run, from C (RCCL communicators).
int vbnmf_engine_allreduce(vbnmf_engine *e)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!e->comm || e->comm->kind != 0) return fail(VBNMF_ERR_STATE, "allreduce needs an RCCL communicator attached to the engine");
    if (int rc = use_device(e)) return rc;
    // Behind ml_set_state and the second ml_step_local only the tail [rowSums(h) | 0 0 | data term | constant] is read afterwards.
    // Sending the tail alone there is an OPTIMISATION, not part of the protocol (it spares a second n*R all-reduce per step): a
    // caller that sums the whole buffer at every exchange gets the same results.
    const size_t off = (e->ml_prime_pending || e->ml_phase == 2) ? (size_t)e->n * e->R : 0;
    return rccl_check(rccl_api().AllReduce(e->red + off, e->red + off, (size_t)e->red_count - off, ncclDouble, ncclSum, e->comm->nc, e->stream), "ncclAllReduce");
}

static int group_members(vbnmf_comm *c, LoopGroup &G)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "communicator handle is NULL");
    if (c->kind != 1) return fail(VBNMF_ERR_STATE, "not a local group (an RCCL communicator is driven through its engine)");
    if ((int)c->members.size() != c->nranks) return fail(VBNMF_ERR_STATE, "the local group has %d of its %d partitions attached", (int)c->members.size(), c->nranks);
    for (vbnmf_engine *q : c->members) if (!q) return fail(VBNMF_ERR_STATE, "a partition engine of the group has been destroyed");
    G.e = c->members.data(); G.count = c->nranks; G.comm = c;
    return VBNMF_OK;
}

// The reduce buffers of a local group summed in place, partition order, behind everything queued on the members' streams.
static int group_sum_in_place(const LoopGroup &G)
{
    for (int p = 0; p < G.count; p++) HIPCHECK(hipStreamSynchronize(G.e[p]->stream));
    vbnmf_engine *L = G.e[0];
    // in place: every element is read from all partitions before it is written to any
    std::vector<double *> ptr(G.count);
    for (int p = 0; p < G.count; p++) ptr[p] = G.e[p]->red;
    double **d_ptr = nullptr;
    if (int rc = dev_alloc(&d_ptr, (size_t)G.count)) return rc;
    hipError_t he = hipMemcpy(d_ptr, ptr.data(), G.count * sizeof(void *), hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((L->red_count + 255) / 256)), dim3(256), 0, L->stream, (const double *const *)d_ptr, d_ptr, G.count, L->red_count);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipStreamSynchronize(L->stream);
    dev_free(d_ptr);
    if (he != hipSuccess) return fail(VBNMF_ERR_HIP, "group state exchange failed: %s", hipGetErrorString(he));
    return VBNMF_OK;
}

// Local group: the state exchange after set_state on every member (sums the reduce buffers in place, partition
// order), then state_finish on each.
int vbnmf_group_state_finish(vbnmf_comm *c)
{
    LoopGroup G{};
    if (int rc = group_members(c, G)) return rc;
    if (int rc = use_device(G.e[0])) return rc;
    if (int rc = group_tables(c)) return rc;
    for (int p = 0; p < G.count; p++)
        if (!G.e[p]->prime_pending) return fail(VBNMF_ERR_STATE, "group_state_finish: partition %d has no pending set_state", p);
    if (int rc = group_sum_in_place(G)) return rc;
    for (int p = 0; p < G.count; p++)
        if (int rc = vbnmf_engine_state_finish(G.e[p])) return rc;
    return VBNMF_OK;
}

int vbnmf_group_run(vbnmf_comm *c, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0, int32_t dn,
                    const int32_t *flags, int32_t *it_out, double *lk0_out, double *lkh_out, int32_t *reason_out,
                    double *history, int64_t history_rows)
{
    LoopGroup G{};
    if (int rc = group_members(c, G)) return rc;
    if (int rc = use_device(G.e[0])) return rc;
    if (int rc = group_tables(c)) return rc;
    return run_group(G, hyper, fudge, max_it, tol, n0, dn, flags, it_out, lk0_out, lkh_out, reason_out, history, history_rows);
}

int vbnmf_engine_get_state(vbnmf_engine *e, double *lw, double *lh, double *ew, double *eh, double *dw, double *dh)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!e->has_state) return fail(VBNMF_ERR_STATE, "get_state before set_state");
    if (int rc = use_device(e)) return rc;
    {
        struct Item { double *dst; const double *src; bool gene; };
        const Item items[6] = {{lw, e->lw, true}, {ew, e->ew, true}, {dw, e->dw, true},
                               {lh, e->lh, false}, {eh, e->eh, false}, {dh, e->dh, false}};
        size_t need = 0;
        for (const Item &it : items) if (it.dst) need += (size_t)(it.gene ? e->n : e->m) * e->R;
        if (int rc = ensure_stage(e, need)) return rc;
        size_t off = 0;
        for (const Item &it : items) {                   // every requested array into the pinned staging buffer, asynchronously ...
            if (!it.dst) continue;
            const size_t cnt = (size_t)(it.gene ? e->n : e->m) * e->R;
            HIPCHECK(hipMemcpyAsync(e->h_stage + off, it.src, cnt * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            off += cnt;
        }
        HIPCHECK(hipStreamSynchronize(e->stream));        // ... one wait (it also covers whatever was queued before) ...
        off = 0;
        for (const Item &it : items) {                   // ... then into the caller's column-major arrays
            if (!it.dst) continue;
            const int64_t nmaj = it.gene ? e->n : e->m;
            from_index_major(e->h_stage + off, nmaj, e->r, e->R, !it.gene, it.dst, it.gene ? nullptr : &e->cell_perm);
            off += (size_t)nmaj * e->R;
        }
    }
    return VBNMF_OK;
}

int vbnmf_engine_timing_enable(vbnmf_engine *e, int32_t on)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    e->timing = on != 0;
    e->sweep_ms = 0.0; e->sweep_launches = 0; e->ev_recorded = false; e->ev2_recorded = false;
    return VBNMF_OK;
}

int vbnmf_engine_timing_get(vbnmf_engine *e, double *sweep_ms, int64_t *sweep_launches)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (sweep_ms) *sweep_ms = e->sweep_ms;
    if (sweep_launches) *sweep_launches = e->sweep_launches;
    e->sweep_ms = 0.0; e->sweep_launches = 0;
    return VBNMF_OK;
}

int vbnmf_engine_layout_info(const vbnmf_engine *e, int64_t *nnz, int64_t *slots_gene, int64_t *slots_cell,
                             int64_t *stream_bytes, int64_t *tiles_gene, int64_t *tiles_cell)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (nnz) *nnz = e->nnz;
    if (slots_gene) *slots_gene = e->A.n_slots;
    if (slots_cell) *slots_cell = e->B.n_slots;
    if (stream_bytes) *stream_bytes = (e->A.n_slots + e->B.n_slots) * (int64_t)(e->wide ? 12 : 4);
    if (tiles_gene) *tiles_gene = e->A.n_tasks;
    if (tiles_cell) *tiles_cell = e->B.n_tasks;
    return VBNMF_OK;
}

// Diagnostic: per-workgroup / per-wave 100 MHz timestamps of the last sweep (engine created with
// VBNMF_DEBUG_TIMES=1): out[side][wg][2 + 2*waves] = {wg start, wg end, (wave start, wave end)...}.
int vbnmf_engine_debug_times(vbnmf_engine *e, unsigned long long *out, int64_t capacity, int32_t *n_wg, int32_t *waves)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (!e->dbg) return fail(VBNMF_ERR_STATE, "engine was not created with VBNMF_DEBUG_TIMES=1");
    if (n_wg) *n_wg = e->n_wg;
    if (waves) *waves = e->NT / 64;
    if (out) {
        if ((size_t)capacity < e->dbg_count) return fail(VBNMF_ERR_BAD_ARG, "buffer too small");
        if (int rc = use_device(e)) return rc;
        HIPCHECK(hipStreamSynchronize(e->stream));
        HIPCHECK(hipMemcpy(out, e->dbg, e->dbg_count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return VBNMF_OK;
}

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
    *lk = e->h_out[0];                               // left there by the last k_ml_final (set_state or step)
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
    if (lk) *lk = e->h_out[0];
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
        if (e->partitioned) { if (int rc = launch_ml_pack(e, nullptr)) return rc; }
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
    if (lk) *lk = e->h_out[0];
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
        if (!rc) rc = launch_ml_pack(e, &e->ctl->stop);
        if (rc) return rc;
        evA[p] = next_event(e);
        HIPCHECK(hipEventRecord(evA[p], e->stream));
    }
    if (c->kind == 0) {
        HIPCHECK(hipStreamWaitEvent(L->cstream, evA[0], 0));
        if (int rc = rccl_check(rccl_api().AllReduce(L->red, L->red_g, (size_t)nbig, ncclDouble, ncclSum, c->nc, L->cstream), "ncclAllReduce")) return rc;
    } else {
        for (int p = 0; p < P; p++) HIPCHECK(hipStreamWaitEvent(L->cstream, evA[p], 0));
        hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((nbig + 255) / 256)), dim3(256), 0, L->cstream, c->d_send_big, c->d_recv_big, P, nbig);
        HIPCHECK(hipGetLastError());
    }
    hipEvent_t evBig = next_event(L);
    HIPCHECK(hipEventRecord(evBig, L->cstream));
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        HIPCHECK(hipStreamWaitEvent(e->stream, evBig, 0));
        int rc = launch_ml_update(e, true, a.prior, a.ga, a.gb, eps);           // W <- red_g (e->red_in), on every partition the same bits
        if (!rc) rc = launch_sweep1(e, false);
        if (rc) return rc;
        if (a.conn)
            hipLaunchKernelGGL(k_ml_tail_conn, dim3(1), dim3(1024), 0, e->stream, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx,
                               conn_step(e, e->fold_step, false).tab_add, (int)nconn, e->red + nbig, &e->ctl->stop);
        else
            hipLaunchKernelGGL(k_tail_data, dim3(1), dim3(1024), 0, e->stream, e->epart + e->n_wg, (int64_t)e->n_wg, e->xlx, e->red + nbig, &e->ctl->stop);
        HIPCHECK(hipGetLastError());
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
        hipLaunchKernelGGL(k_group_sum_at, dim3((unsigned)((nsmall + 255) / 256)), dim3(256), 0, L->stream, c->d_send_big, c->d_recv_big, P, nbig, nsmall);
        HIPCHECK(hipGetLastError());
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
        if (G.e[p]->h_out[5] != e->h_out[5] || G.e[p]->h_out[6] != e->h_out[6])
            return fail(VBNMF_ERR_STATE, "partition %d ended the loop at step %d (reason %d), partition 0 at step %d (reason %d)", p,
                        (int)G.e[p]->h_out[5], (int)G.e[p]->h_out[6], (int)e->h_out[5], (int)e->h_out[6]);
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

// ---- consensus accumulator (include/vbnmf.h; kernels: consensus.h) ----
struct vbnmf_consensus {
    int device = 0;
    int64_t m = 0;
    int r = 0, max_runs = 0, runs = 0;
    hipStream_t stream = nullptr;             // add_labels, reset, downloads; add_engine works on the engine's stream
    uint8_t *labels = nullptr;                // [max_runs][m]
    unsigned long long *tables = nullptr;     // [max_runs][(r+1)^2] contingency tables of the run being added
    unsigned long long *sums = nullptr;       // [2] S1, S2, then (as int32) the "saw label 0" flag in the third word
    unsigned long long h_sums[3] = {0, 0, 0}; // host copy, refreshed by every add
    bool broken = false;                      // an add failed half way: the device sums may miss terms
};

namespace {

int consensus_use(vbnmf_consensus *c)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "consensus handle is NULL");
    if (c->broken) return fail(VBNMF_ERR_STATE, "an earlier add to this accumulator failed; reset it");
    HIPCHECK(hipSetDevice(c->device));
    return VBNMF_OK;
}

// Row c->runs of the label matrix has just been written on `stream`: its tables against every stored row and itself, the
// sums, the host copy of the sums; returns with the stream idle, so the next add may come from another stream.
int consensus_count_row(vbnmf_consensus *c, hipStream_t stream)
{
    const int t = c->runs;
    const size_t bins = (size_t)(c->r + 1) * (c->r + 1);
    HIPCHECK(hipMemsetAsync(c->tables, 0, (size_t)(t + 1) * bins * sizeof(unsigned long long), stream));
    const unsigned chunks = (unsigned)((c->m + kCoinChunk - 1) / kCoinChunk);
    hipLaunchKernelGGL(k_label_coincidence, dim3(chunks, (unsigned)(t + 1)), dim3(kCoinThreads), bins * sizeof(uint32_t), stream,
                       (const uint8_t *)c->labels, c->m, c->r, t, c->tables);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_coincidence_pairs, dim3((unsigned)(t + 1)), dim3(kCoinThreads), 0, stream,
                       (const unsigned long long *)c->tables, c->r, t, c->sums);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(c->h_sums, c->sums, sizeof c->h_sums, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    c->runs = t + 1;
    return VBNMF_OK;
}

}  // namespace

namespace vbnmf {
int consensus_download(vbnmf_consensus *c, std::vector<uint8_t> &labels, int64_t &m, int32_t &runs, int32_t &unlabelled, int32_t *device)
{
    if (int rc = consensus_use(c)) return rc;
    if (device) *device = c->device;
    m = c->m; runs = c->runs; unlabelled = (int32_t)(c->h_sums[2] != 0);
    try { labels.resize((size_t)c->runs * c->m); } catch (const std::bad_alloc &) { return fail(VBNMF_ERR_OOM, "out of host memory for the label matrix"); }
    if (!labels.empty()) HIPCHECK(hipMemcpy(labels.data(), c->labels, labels.size(), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}
}  // namespace vbnmf

extern "C" {

void vbnmf_consensus_destroy(vbnmf_consensus *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    dev_free(c->labels); dev_free(c->tables); dev_free(c->sums);
    delete c;
}

int vbnmf_consensus_create(int64_t m, int32_t rank, int32_t max_runs, int32_t device, vbnmf_consensus **out)
{
    if (!out) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    if (m < 1 || rank < 1 || rank > VBNMF_MAX_RANK || max_runs < 1)
        return fail(VBNMF_ERR_BAD_ARG, "consensus accumulator needs m >= 1, 1 <= rank <= %d, max_runs >= 1", VBNMF_MAX_RANK);
    if (int rc = use_device(device)) return rc;
    std::unique_ptr<vbnmf_consensus, void (*)(vbnmf_consensus *)> c(new (std::nothrow) vbnmf_consensus(), vbnmf_consensus_destroy);
    if (!c) return fail(VBNMF_ERR_OOM, "out of host memory");
    c->device = device; c->m = m; c->r = rank; c->max_runs = max_runs;
    const size_t bins = (size_t)(rank + 1) * (rank + 1);
    // the coincidence kernel's LDS table passes 64 KB at rank 128 (129^2 uint32 = 66.6 KB)
    HIPCHECK(hipFuncSetAttribute((const void *)k_label_coincidence, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (int rc = dev_alloc(&c->labels, (size_t)max_runs * (size_t)m)) return rc;
    if (int rc = dev_alloc(&c->tables, (size_t)max_runs * bins)) return rc;
    if (int rc = dev_alloc(&c->sums, 3)) return rc;
    if (int rc = vbnmf_consensus_reset(c.get())) return rc;
    *out = c.release();
    return VBNMF_OK;
}

int vbnmf_consensus_reset(vbnmf_consensus *c)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "consensus handle is NULL");
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemsetAsync(c->sums, 0, 3 * sizeof(unsigned long long), c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    c->runs = 0;
    c->h_sums[0] = c->h_sums[1] = c->h_sums[2] = 0;
    c->broken = false;
    return VBNMF_OK;
}

int vbnmf_consensus_add_engine(vbnmf_consensus *c, vbnmf_engine *e)
{
    if (!e) return fail(VBNMF_ERR_BAD_ARG, "engine handle is NULL");
    if (int rc = consensus_use(c)) return rc;
    if (e->partitioned)
        return fail(VBNMF_ERR_STATE, "a partitioned engine holds a part of the cells (the label tables are not all-reduced); "
                                     "add the gathered labels with vbnmf_consensus_add_labels");
    if (!e->ml_ready && !e->has_state) return fail(VBNMF_ERR_STATE, "consensus add before a state was loaded");
    if (e->m != c->m || e->r != c->r || e->device != c->device)
        return fail(VBNMF_ERR_BAD_ARG, "the engine (m %lld, rank %d, device %d) does not match the accumulator (m %lld, rank %d, device %d)",
                    (long long)e->m, e->r, e->device, (long long)c->m, c->r, c->device);
    if (c->runs >= c->max_runs) return fail(VBNMF_ERR_BAD_ARG, "the accumulator already holds its max_runs = %d runs", c->max_runs);
    if (int rc = use_device(e)) return rc;
    const double *h = e->ml_ready ? e->lh : e->eh;
    c->broken = true;
    hipLaunchKernelGGL(k_argmax_row, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, e->stream, h, e->m, e->r, e->R,
                       (const int32_t *)e->d_perm, c->labels + (size_t)c->runs * c->m, reinterpret_cast<int32_t *>(c->sums + 2));
    HIPCHECK(hipGetLastError());
    if (int rc = consensus_count_row(c, e->stream)) return rc;
    c->broken = false;
    return VBNMF_OK;
}

int vbnmf_consensus_add_labels(vbnmf_consensus *c, const int32_t *ids)
{
    if (!ids) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = consensus_use(c)) return rc;
    if (c->runs >= c->max_runs) return fail(VBNMF_ERR_BAD_ARG, "the accumulator already holds its max_runs = %d runs", c->max_runs);
    std::vector<uint8_t> row;
    try { row.resize((size_t)c->m); } catch (const std::bad_alloc &) { return fail(VBNMF_ERR_OOM, "out of host memory for a label row"); }
    unsigned long long zero = 0;
    for (int64_t j = 0; j < c->m; j++) {
        if (ids[j] < 0 || ids[j] > c->r) return fail(VBNMF_ERR_BAD_ARG, "label %d of cell %lld is outside 0..%d", ids[j], (long long)j, c->r);
        row[(size_t)j] = (uint8_t)ids[j];
        zero |= (ids[j] == 0);
    }
    c->broken = true;
    HIPCHECK(hipMemcpyAsync(c->labels + (size_t)c->runs * c->m, row.data(), row.size(), hipMemcpyHostToDevice, c->stream));
    if (zero) { const unsigned long long one = 1; HIPCHECK(hipMemcpyAsync(c->sums + 2, &one, sizeof one, hipMemcpyHostToDevice, c->stream)); }
    if (int rc = consensus_count_row(c, c->stream)) return rc;      // (synchronises: `row` and `one` outlive their copies)
    c->broken = false;
    return VBNMF_OK;
}

int vbnmf_consensus_sums(vbnmf_consensus *c, int32_t *runs, uint64_t *s1, uint64_t *s2, int32_t *unlabelled)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "consensus handle is NULL");
    if (c->broken) return fail(VBNMF_ERR_STATE, "an earlier add to this accumulator failed; reset it");
    if (runs) *runs = c->runs;
    if (s1) *s1 = c->h_sums[0];
    if (s2) *s2 = c->h_sums[1];
    if (unlabelled) *unlabelled = (int32_t)(c->h_sums[2] != 0);
    return VBNMF_OK;
}

int vbnmf_consensus_dispersion(vbnmf_consensus *c, double *disp)
{
    if (!c || !disp) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (c->broken) return fail(VBNMF_ERR_STATE, "an earlier add to this accumulator failed; reset it");
    if (c->runs < 1) return fail(VBNMF_ERR_STATE, "dispersion before the first run was added");
    if (c->h_sums[2] != 0) { *disp = std::nan(""); return VBNMF_OK; }
    // con = S2/R^2 - S1/R + npair/4 = (4 S2 - 4 R S1 + R^2 npair) / (4 R^2): the numerator exactly, then one division
    const unsigned __int128 R = (unsigned __int128)c->runs, m = (unsigned __int128)c->m;
    const unsigned __int128 npair = m * (m - 1) / 2;
    const unsigned __int128 num = 4 * (unsigned __int128)c->h_sums[1] + R * R * npair - 4 * R * (unsigned __int128)c->h_sums[0];
    const double con = (double)num / (4.0 * (double)c->runs * (double)c->runs);
    const double md = (double)c->m;
    *disp = 1.0 / md + 8.0 * con / (md * md);
    return VBNMF_OK;
}

int vbnmf_consensus_labels(vbnmf_consensus *c, int32_t run, int32_t *ids)
{
    if (!ids) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = consensus_use(c)) return rc;
    if (run < 0 || run >= c->runs) return fail(VBNMF_ERR_BAD_ARG, "run %d is outside [0, %d)", run, c->runs);
    std::vector<uint8_t> row;
    try { row.resize((size_t)c->m); } catch (const std::bad_alloc &) { return fail(VBNMF_ERR_OOM, "out of host memory for a label row"); }
    HIPCHECK(hipMemcpy(row.data(), c->labels + (size_t)run * c->m, row.size(), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < c->m; j++) ids[j] = row[(size_t)j];
    return VBNMF_OK;
}

}  // extern "C"

namespace {

// Sparse product with the resident X on operands that are ALREADY on the device: gene side C[n][R] = X B (B = the lh
// array, one row per cell), cell side C[m][R] = t(X) W (W = the lw array); the per-task partials are summed per
// major straight into `target`.
int spmm_device(vbnmf_engine *e, bool gene_side, double *target)
{
    SweepSide a = sweep_side_args(e, gene_side);
    a.logterm = 0;
    a.stop = nullptr;
    if (int rc = launch_spmm(e, a)) return rc;
    const SideView v = side_view(e, gene_side);
    const int64_t cnt = v.nmaj * e->R;
    return launch_kernel<k_pack>(e, dim3((unsigned)((cnt + 255) / 256)), 256, 0, v.S.part, v.S.row_ptr, v.S.row_task, v.nmaj, e->R, target);
}

// work space of the truncated SVD: [gram partials kGramBlocks * R*R | S (R*R) | S2 (R*R) | vals (R)]
struct SvdWs { double *gp, *S, *S2, *vals; };
SvdWs svd_ws(vbnmf_engine *e)
{
    const size_t RR = (size_t)e->R * e->R;
    SvdWs w;
    w.gp = e->svd_ws; w.S = w.gp + (size_t)kGramBlocks * RR; w.S2 = w.S + RR; w.vals = w.S2 + RR;
    return w;
}

int launch_gram(vbnmf_engine *e, const double *A, int64_t N)
{
    SvdWs w = svd_ws(e);
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_gram<rt()>>(e, dim3(kGramBlocks), 1024, 0, A, N, w.gp);
    });
}

int launch_small(vbnmf_engine *e, int mode, bool want_s2, double *vals_host, double seq)
{
    SvdWs w = svd_ws(e);
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_small<rt()>>(e, dim3(1), 1024, 0, w.gp, kGramBlocks, e->r, mode, w.S, want_s2 ? w.S2 : nullptr, w.vals,
                                            vals_host, seq, e->svd_status);
    });
}

int launch_apply(vbnmf_engine *e, const double *A, const double *S, int64_t N, double *B)
{
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_apply<rt()>>(e, dim3((unsigned)((N + 255) / 256)), 256, 0, A, S, N, B);
    });
}

// A <- orthonormal basis of range(A), A tall [N][R]: CholeskyQR twice (Gram matrix, its Cholesky factor's inverse,
// A times that) -- the second pass repairs the orthogonality the first loses to the condition number.  When `gram_ready`
// the block partials of t(A) A are already in the work space.
int orthonormalise(vbnmf_engine *e, double *A, int64_t N, bool gram_ready)
{
    SvdWs w = svd_ws(e);
    for (int pass = 0; pass < 2; pass++) {
        if (!(pass == 0 && gram_ready)) { if (int rc = launch_gram(e, A, N)) return rc; }
        if (int rc = launch_small(e, 0, false, nullptr, 0.0)) return rc;
        if (int rc = launch_apply(e, A, w.S, N, A)) return rc;
    }
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// Truncated SVD of the resident X by block subspace iteration, ENTIRELY on the device (the
// irlba::irlba(mat, rank) of the svd2 initialiser, reference R/bayesian.R:150-159): the subspace has k = the engine's
// rank columns (rank_out of them are returned); per iteration two sparse products (k_spmm), two CholeskyQR2
// orthonormalisations (k_gram / k_small / k_apply) and the k x k eigen-problem that yields the current singular values
// (k_small, Jacobi) -- the host only reads those k values from pinned memory for the stopping rule
// max |s - s_old| <= tol * s[0] over the leading rank_out.  No host <-> device copy inside the iteration.
// Outputs: u (n x rank_out, column-major), d (rank_out), vt (rank_out x m, column-major), iterations done.
int vbnmf_engine_svd(vbnmf_engine *e, int32_t rank_out, double tol, int32_t maxit, uint64_t seed, double *u, double *d,
                     double *vt, int32_t *iterations)
{
    if (!e || !u || !d || !vt) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (e->partitioned) return fail(VBNMF_ERR_STATE, "the truncated SVD needs an unpartitioned engine");
    if (rank_out < 1 || rank_out > e->r) return fail(VBNMF_ERR_BAD_ARG, "rank_out must be in [1, engine rank]");
    if (e->R > VBNMF_MAX_SVD_COLUMNS)
        return fail(VBNMF_ERR_BAD_ARG, "the device-resident SVD holds at most %d subspace columns (engine rank %d); use the sparse products (vbnmf_engine_spmm) with a host QR", VBNMF_MAX_SVD_COLUMNS, e->r);
    if (maxit < 1) return fail(VBNMF_ERR_BAD_ARG, "maxit must be >= 1");
    if (int rc = use_device(e)) return rc;
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false; e->ml_ready = false;
    const size_t RR = (size_t)e->R * e->R;
    if (!e->svd_ws) { if (int rc = dev_alloc(&e->svd_ws, (size_t)kGramBlocks * RR + 2 * RR + e->R)) return rc; }
    if (!e->svd_status) { if (int rc = dev_alloc(&e->svd_status, 1)) return rc; }
    HIPCHECK(hipMemsetAsync(e->svd_status, 0, sizeof(int32_t), e->stream));
    if (int rc = ensure_history(e, (size_t)e->R + 2)) return rc;             // pinned [R values | sequence number]
    SvdWs w = svd_ws(e);
    volatile double *hv = e->h_hist;
    hv[e->R] = 0.0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t nh = e->m * e->R;
    double *Q = e->lw, *Z = e->lh;                                           // n x k and m x k, index-major
    // range finder: Q = orth(X G), G standard normal m x k
    hipLaunchKernelGGL(k_normal_init, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, e->stream, Z, e->m, e->r, e->R, k0, k1);
    HIPCHECK(hipGetLastError());
    if (int rc = spmm_device(e, true, Q)) return rc;
    if (int rc = orthonormalise(e, Q, e->n, false)) return rc;
    std::vector<double> s_old;
    int it = 0;
    for (it = 1; it <= maxit; it++) {
        if (int rc = spmm_device(e, false, Z)) return rc;                    // Z = t(X) Q
        if (int rc = orthonormalise(e, Z, e->m, false)) return rc;
        if (int rc = spmm_device(e, true, Q)) return rc;                     // Y = X Z = Q Rm
        if (int rc = launch_gram(e, Q, e->n)) return rc;                     // t(Y) Y = t(Rm) Rm: eigenvalues = sigma^2
        if (int rc = launch_small(e, 1, false, e->h_hist_dev, (double)it)) return rc;
        if (int rc = orthonormalise(e, Q, e->n, true)) return rc;            // (the Gram partials are still in place)
        HIPCHECK(hipStreamSynchronize(e->stream));
        if (hv[e->R] != (double)it) return fail(VBNMF_ERR_HIP, "the singular values of iteration %d never arrived", it);
        std::vector<double> sv(rank_out);
        for (int q = 0; q < rank_out; q++) sv[q] = std::sqrt(std::max(0.0, (double)hv[q]));
        bool done = false;
        if (!s_old.empty()) {
            double dmax = 0.0;
            for (int q = 0; q < rank_out; q++) dmax = std::max(dmax, std::fabs(sv[q] - s_old[q]));
            done = dmax <= tol * sv[0];
        }
        s_old.swap(sv);
        if (done) break;
    }
    if (it > maxit) it = maxit;
    // B = t(Q) X = t(P), P = t(X) Q (m x k): B t(B) = t(P) P = Ub D^2 t(Ub); u = Q Ub, rows of vt = P Ub / D
    if (int rc = spmm_device(e, false, Z)) return rc;
    if (int rc = launch_gram(e, Z, e->m)) return rc;
    if (int rc = launch_small(e, 1, true, e->h_hist_dev, (double)(maxit + 1))) return rc;
    if (int rc = launch_apply(e, Q, w.S, e->n, e->ew)) return rc;
    if (int rc = launch_apply(e, Z, w.S2, e->m, e->eh)) return rc;
    HIPCHECK(hipStreamSynchronize(e->stream));
    int32_t status = 0;
    HIPCHECK(hipMemcpy(&status, e->svd_status, sizeof status, hipMemcpyDeviceToHost));
    if (status) return fail(VBNMF_ERR_STATE, "the subspace lost rank (a Gram matrix was not positive definite): fewer independent directions than the engine's rank");
    for (int q = 0; q < rank_out; q++) d[q] = std::sqrt(std::max(0.0, (double)hv[q]));
    try {
        std::vector<double> tmp((size_t)std::max(e->n, e->m) * e->R);
        HIPCHECK(hipMemcpy(tmp.data(), e->ew, (size_t)e->n * e->R * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < e->n; i++) for (int q = 0; q < rank_out; q++) u[i + (size_t)q * e->n] = tmp[(size_t)i * e->R + q];
        HIPCHECK(hipMemcpy(tmp.data(), e->eh, (size_t)e->m * e->R * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < e->m; j++) {
            const int64_t col = e->cell_perm.empty() ? j : e->cell_perm[j];
            for (int q = 0; q < rank_out; q++) vt[q + (size_t)col * rank_out] = tmp[(size_t)j * e->R + q];
        }
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the singular vectors");
    }
    if (iterations) *iterations = it;
    return VBNMF_OK;
}

// ---------------------------------------------------------------- sparse products (truncated SVD of the svd2 initialiser)
int vbnmf_engine_spmm(vbnmf_engine *e, int32_t transpose, const double *B, double *C)
{
    if (!e || !B || !C) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (e->partitioned) return fail(VBNMF_ERR_STATE, "spmm needs an unpartitioned engine");
    if (int rc = use_device(e)) return rc;
    // the factor arrays serve as operand storage: whatever state the engine held is gone
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false; e->ml_ready = false;
    const bool gene_side = transpose == 0;             // C = X t(B): lanes own genes and gather rows of B (one per cell)
    const SideView out = side_view(e, gene_side), in = side_view(e, !gene_side);
    const int64_t n_in = in.nmaj, n_out = out.nmaj;
    double *operand = in.l;                            // gathered through LDS
    double *dense = out.e;                             // [n_out][R] result before the download
    try {
        std::vector<double> tmp;
        to_index_major(B, n_in, e->r, e->R, gene_side, tmp, gene_side ? &e->cell_perm : nullptr);     // B: one row per cell on the gene side
        HIPCHECK(hipMemcpyAsync(operand, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        if (int rc = spmm_device(e, gene_side, dense)) return rc;
        const int64_t cnt = n_out * e->R;
        tmp.resize((size_t)cnt);
        HIPCHECK(hipMemcpyAsync(tmp.data(), dense, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        from_index_major(tmp, n_out, e->r, e->R, !gene_side, C, gene_side ? nullptr : &e->cell_perm);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the operands");
    }
    return VBNMF_OK;
}

// ---------------------------------------------------------------- test hooks
int vbnmf_test_special_host(int32_t kind, int64_t n, const double *x, double *y)
{
    if (!x || !y || n < 0) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    for (int64_t i = 0; i < n; i++) {
        double psi, lg;
        switch (kind) {
            case 0: y[i] = dev_log(x[i]); break;
            case 1: dev_psi_lgamma(x[i], &psi, &lg); y[i] = psi; break;
            case 2: dev_psi_lgamma(x[i], &psi, &lg); y[i] = lg; break;
            case 6: { static LogTabEntry tab[kLogTabSize]; static bool init = false; if (!init) { fill_log_table(tab); init = true; } y[i] = dev_log_tab(x[i], tab); break; }
            case 7: y[i] = dev_trigamma(x[i]); break;
            case 8:                                          // the pair form: quads wa, wb, xa, xb in; qa, qb, r, 0 out
                if (i % 4 == 0 && i + 3 < n) { y[i + 2] = dev_div_pair(x[i + 2], x[i], x[i + 3], x[i + 1], &y[i], &y[i + 1]); y[i + 3] = 0.0; }
                break;
            default: y[i] = dev_div(1.0, x[i]); break;
        }
    }
    return VBNMF_OK;
}

int vbnmf_test_special_device(int32_t kind, int64_t n, const double *x, double *y)
{
    if (!x || !y || n < 0) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = use_device(0)) return rc;
    double *dx = nullptr, *dy = nullptr;
    LogTabEntry *dt = nullptr;
    std::vector<LogTabEntry> tab(kLogTabSize);
    fill_log_table(tab.data());
    if (int rc = dev_alloc(&dx, (size_t)n)) return rc;
    if (int rc = dev_alloc(&dy, (size_t)n)) { dev_free(dx); return rc; }
    if (int rc = dev_upload(&dt, tab)) { dev_free(dx); dev_free(dy); return rc; }
    int rc = VBNMF_OK;
    hipError_t he = hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (he == hipSuccess && n > 0) {
        hipLaunchKernelGGL(k_test_special, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, n, dx, dy, dt);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpy(y, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (he != hipSuccess) rc = fail(VBNMF_ERR_HIP, "special-function test kernel failed: %s", hipGetErrorString(he));
    dev_free(dx); dev_free(dy); dev_free(dt);
    return rc;
}

}  // extern "C"

namespace {

// What a dense-SVD test hook holds on the device (DeviceCall's alloc / upload; never entered: use_device(0) chose the device)
// and pinned: released on every return path.
struct HookBuffers : DeviceCall {
    void *pinned = nullptr;
    ~HookBuffers() { if (pinned) (void)hipHostFree(pinned); }
};

int download(double *dst, const double *src, size_t count)
{
    HIPCHECK(hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

// R must be a width the dense kernels are instantiated for
int hook_width(int32_t R)
{
    return with_rank_up_to_64(R, [](auto) { return (int)VBNMF_OK; });
}

constexpr int64_t kHookMaxRows = (int64_t)1 << 24;           // 8 GB of doubles at R = 64: a test has no use for more

}  // namespace

extern "C" {

// ---- test hooks into hyper_update (reference R/bayesian.R:2-53) as the device-driven loops run it: `count` independent
// cases, each with its flags[4], stats[4] = (mean log lw, mean log lh, mean ew, mean eh) and hyper_in[4] = (aw, bw, ah, bh).
// Out per case: hyper_out[4], failed, iters (Newton iterations run) and trace[2][100]: side s's a1 of iteration k at
// [100 s + k] (s = 0: aw, 1: ah), NaN where nothing was stored.
// The host form runs the two sides one after the other through hyper_newton_side (special.h), the arithmetic the device's
// lanes run; it takes any double (a shape that is not a positive number comes back failed).
int vbnmf_test_hyper_update_host(int64_t count, const int32_t *flags, const double *stats, const double *hyper_in, double *hyper_out,
                                 int32_t *failed, int32_t *iters, double *trace)
{
    if (!flags || !stats || !hyper_in || !hyper_out || !failed || !iters || !trace || count < 0) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    for (int64_t c = 0; c < count; c++) {
        const int32_t *fl = flags + 4 * c;
        const double *st = stats + 4 * c, *hi = hyper_in + 4 * c;
        double *ho = hyper_out + 4 * c, *tr = trace + 200 * c;
        for (int q = 0; q < 4; q++) ho[q] = hi[q];
        for (int q = 0; q < 200; q++) tr[q] = __builtin_nan("");
        failed[c] = 0; iters[c] = 0;
        if (fl[0] + fl[1] + fl[2] + fl[3] == 0) continue;                                  // :4
        double a0[2] = {hi[0], hi[2]}, a1[2] = {hi[0], hi[2]};
        int f = 0, done = 0;
        if (fl[0] + fl[2] > 0) {                                                           // :15
            int i = 1;
            while (i < 100) {
                double u[2];
                int bad = 0;
                for (int s = 0; s < 2; s++) {
                    int hv, b;
                    a1[s] = hyper_newton_side(a0[s], hi[2 * s + 1], st[s], st[2 + s], fl[2 * s], &hv, &b);
                    tr[100 * s + done] = a1[s];
                    u[s] = b ? 0.0 : 1.0 - a1[s] / a0[s];
                    bad |= b;
                }
                done++;
                if (bad) { f = 1; break; }
                if (u[0] * u[0] + u[1] * u[1] < 1e-3) break;                               // :37-38
                a0[0] = a1[0]; a0[1] = a1[1]; i++;
            }
            if (i == 100) f = 1;                                                           // :43
        }
        iters[c] = done; failed[c] = f;
        if (!f) { ho[0] = a1[0]; ho[1] = fl[1] ? st[2] : hi[1]; ho[2] = a1[1]; ho[3] = st[3]; }   // :48-51
    }
    return VBNMF_OK;
}

// The device form: one launch of k_test_hyper_update on device 0, one wave per case, lanes 0 and 1 in dev_hyper_update_pair.
// A shape or scale that is not a positive finite number is VBNMF_ERR_BAD_ARG before any launch.
int vbnmf_test_hyper_update_device(int64_t count, const int32_t *flags, const double *stats, const double *hyper_in, double *hyper_out,
                                   int32_t *failed, int32_t *iters, double *trace)
{
    if (!flags || !stats || !hyper_in || !hyper_out || !failed || !iters || !trace) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (count < 1 || count > (1 << 20)) return fail(VBNMF_ERR_BAD_ARG, "count must be in [1, 2^20]");
    for (int64_t q = 0; q < 4 * count; q++)
        if (!(hyper_in[q] > 0.0) || !std::isfinite(hyper_in[q])) return fail(VBNMF_ERR_BAD_ARG, "hyper-parameters must be finite and > 0");
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    const size_t n = (size_t)count;
    double *dfl = nullptr, *dst = nullptr, *dhy = nullptr, *dfa = nullptr, *dit = nullptr, *dtr = nullptr;   // (the int32 arrays in double-sized buffers)
    if (int rc = hb.alloc(&dfl, 2 * n)) return rc;
    HIPCHECK(hipMemcpy(dfl, flags, 4 * n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (int rc = hb.upload(&dst, stats, 4 * n)) return rc;
    if (int rc = hb.upload(&dhy, hyper_in, 4 * n)) return rc;
    if (int rc = hb.alloc(&dfa, (n + 1) / 2)) return rc;
    if (int rc = hb.alloc(&dit, (n + 1) / 2)) return rc;
    if (int rc = hb.alloc(&dtr, 200 * n)) return rc;
    HIPCHECK(hipMemset(dfa, 0, (n + 1) / 2 * sizeof(double)));
    HIPCHECK(hipMemset(dit, 0, (n + 1) / 2 * sizeof(double)));
    HIPCHECK(hipMemset(dtr, 0xFF, 200 * n * sizeof(double)));                              // NaN
    hipLaunchKernelGGL(k_test_hyper_update, dim3((unsigned)n), dim3(64), 0, nullptr, (int)count, (const int32_t *)dfl, (const double *)dst,
                       dhy, (int32_t *)dfa, (int32_t *)dit, dtr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(failed, dfa, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(iters, dit, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (int rc = download(hyper_out, dhy, 4 * n)) return rc;
    return download(trace, dtr, 200 * n);
}

// ---- test hooks into the dense kernels of the truncated SVD (init.h), each with the launch geometry of
// vbnmf_engine_svd: upload, one launch of the product's kernel on the null stream, download
int vbnmf_test_svd_gram(int32_t R, int64_t N, const double *A, double *gp)
{
    if (!A || !gp || N < 1 || N > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or N outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dA = nullptr, *dgp = nullptr;
    const size_t RR = (size_t)R * R;
    if (int rc = hb.upload(&dA, A, (size_t)N * R)) return rc;
    if (int rc = hb.alloc(&dgp, (size_t)kGramBlocks * RR)) return rc;
    HIPCHECK(hipMemset(dgp, 0xFF, (size_t)kGramBlocks * RR * sizeof(double)));       // NaN: the kernel writes every partial
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_gram<rt()>, dim3(kGramBlocks), dim3(1024), 0, nullptr, (const double *)dA, N, dgp);
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    return download(gp, dgp, (size_t)kGramBlocks * RR);
}

int vbnmf_test_svd_small(int32_t R, int32_t k, int32_t mode, int32_t nb, const double *gp, double seq, double *S, double *S2,
                         double *vals, double *vals_host, int32_t *status)
{
    if (!gp || !S || !vals || !status) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (mode != 0 && mode != 1) return fail(VBNMF_ERR_BAD_ARG, "mode must be 0 (Cholesky) or 1 (Jacobi)");
    if (nb < 1 || nb > 65536) return fail(VBNMF_ERR_BAD_ARG, "nb must be in [1, 65536]");
    if (int rc = hook_width(R)) return rc;
    if (k < 1 || k > R) return fail(VBNMF_ERR_BAD_ARG, "k must be in [1, R]");
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    const size_t RR = (size_t)R * R;
    double *dgp = nullptr, *dS = nullptr, *dS2 = nullptr, *dvals = nullptr, *dstat = nullptr, *hv = nullptr, *hv_dev = nullptr;
    if (int rc = hb.upload(&dgp, gp, (size_t)nb * RR)) return rc;
    if (int rc = hb.alloc(&dS, RR)) return rc;
    if (S2) { if (int rc = hb.alloc(&dS2, RR)) return rc; }
    if (int rc = hb.alloc(&dvals, (size_t)R)) return rc;
    if (int rc = hb.alloc(&dstat, 1)) return rc;                               // (8 bytes: the status is its first 4)
    HIPCHECK(hipMemset(dS, 0xFF, RR * sizeof(double)));
    if (dS2) HIPCHECK(hipMemset(dS2, 0xFF, RR * sizeof(double)));
    HIPCHECK(hipMemset(dvals, 0, (size_t)R * sizeof(double)));
    HIPCHECK(hipMemset(dstat, 0, sizeof(double)));
    if (vals_host) {                                                           // pinned and device-visible, as the engine's history block
        hipError_t he = hipHostMalloc(&hb.pinned, ((size_t)R + 2) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
        if (he != hipSuccess) { (void)hipGetLastError(); hb.pinned = nullptr; return fail(VBNMF_ERR_OOM, "pinned values block: %s", hipGetErrorString(he)); }
        hv = static_cast<double *>(hb.pinned);
        for (int q = 0; q <= R; q++) hv[q] = 0.0;
        HIPCHECK(hipHostGetDevicePointer((void **)&hv_dev, hv, 0));
    }
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_small<rt()>, dim3(1), dim3(1024), 0, nullptr, (const double *)dgp, (int)nb, (int)k, (int)mode, dS, dS2, dvals,
                               hv_dev, seq, reinterpret_cast<int32_t *>(dstat));
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    HIPCHECK(hipDeviceSynchronize());
    if (int rc = download(S, dS, RR)) return rc;
    if (S2) { if (int rc = download(S2, dS2, RR)) return rc; }
    if (int rc = download(vals, dvals, (size_t)R)) return rc;
    HIPCHECK(hipMemcpy(status, dstat, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vals_host) { const volatile double *v = hv; for (int q = 0; q <= R; q++) vals_host[q] = v[q]; }
    return VBNMF_OK;
}

int vbnmf_test_svd_apply(int32_t R, int64_t N, const double *A, const double *S, int32_t in_place, double *B)
{
    if (!A || !S || !B || N < 1 || N > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or N outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dA = nullptr, *dS = nullptr, *dB = nullptr;
    if (int rc = hb.upload(&dA, A, (size_t)N * R)) return rc;
    if (int rc = hb.upload(&dS, S, (size_t)R * R)) return rc;
    if (in_place) dB = dA;
    else {
        if (int rc = hb.alloc(&dB, (size_t)N * R)) return rc;
        HIPCHECK(hipMemset(dB, 0xFF, (size_t)N * R * sizeof(double)));
    }
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_apply<rt()>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, (const double *)dA, (const double *)dS, N, dB);
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    return download(B, dB, (size_t)N * R);
}

int vbnmf_test_svd_normal(int64_t nmaj, int32_t r, int32_t R, uint64_t seed, double *g)
{
    if (!g || nmaj < 1 || nmaj > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or nmaj outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (r < 1 || r > R) return fail(VBNMF_ERR_BAD_ARG, "r must be in [1, R]");
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dg = nullptr;
    const int64_t cnt = nmaj * R;
    if (int rc = hb.alloc(&dg, (size_t)cnt)) return rc;
    HIPCHECK(hipMemset(dg, 0xFF, (size_t)cnt * sizeof(double)));
    hipLaunchKernelGGL(k_normal_init, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, nullptr, dg, nmaj, (int)r, (int)R, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
    HIPCHECK(hipGetLastError());
    return download(g, dg, (size_t)cnt);
}

// Test hook: a host function that sleeps `seconds` is enqueued on the engine's stream, so everything queued behind it
// waits that long without the GPU being busy or hung (tests/test_gpu_timeouts.py: the bounded waits).
static void sleep_host_fn(void *arg)
{
    const double s = *static_cast<double *>(arg);
    std::this_thread::sleep_for(std::chrono::duration<double>(s));
    delete static_cast<double *>(arg);
}

int vbnmf_test_stream_sleep(vbnmf_engine *e, double seconds)
{
    if (!e || !(seconds >= 0.0) || seconds > 60.0) return fail(VBNMF_ERR_BAD_ARG, "engine is NULL or seconds outside [0, 60]");
    if (int rc = use_device(e)) return rc;
    double *arg = new (std::nothrow) double(seconds);
    if (!arg) return fail(VBNMF_ERR_OOM, "out of host memory");
    hipError_t he = hipLaunchHostFunc(e->stream, sleep_host_fn, arg);
    if (he != hipSuccess) { delete arg; return fail(VBNMF_ERR_HIP, "hipLaunchHostFunc failed: %s", hipGetErrorString(he)); }
    return VBNMF_OK;
}

// ---------------------------------------------------------------- stateless forms
}  // extern "C"

namespace { uint64_t hash_bytes(const void *data, size_t bytes, uint64_t seed); }
extern "C" {
// Test hook (no device needed): the content hash of the stateless cache, for tests/test_cabi_symbols.py.
#ifdef VBNMF_ABL_STAMPS                                       /* instrumented builds only (profiles/ubench/r04/update_stamps.sh) */
int vbnmf_test_update_stamps(unsigned long long *out)
{
    if (hipDeviceSynchronize() != hipSuccess) return VBNMF_ERR_HIP;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_upd_stamps), sizeof(unsigned long long) * 2 * kUpdateBlocks * 12) == hipSuccess ? VBNMF_OK : VBNMF_ERR_HIP;
}
#endif
uint64_t vbnmf_test_hash_bytes(const void *data, int64_t bytes, uint64_t seed) { return (data && bytes >= 0) ? hash_bytes(data, (size_t)bytes, seed) : 0; }
}

namespace {

// The reference's caller hands the SAME X to every one of its thousands of calls (R/bayesian.R:339).  The stateless
// entries therefore keep the last ingested matrix and its engine alive, keyed by the CONTENT of X (dimensions + a
// 64-bit hash of every byte of the arrays handed in, formed by all host threads): a call with an X seen before costs
// the hash, the state upload, one step and the state download instead of ingestion + two layouts + an engine.
// VBNMF_STATELESS_CACHE=0 turns it off; vbnmf_stateless_cache_clear() releases what is held.
struct StatelessCache {
    std::mutex mu;                    // held for the whole call: stateless calls are serialised
    bool valid = false;
    int kind = 0;                     // 0 dense, 1 csc
    int64_t n = 0, m = 0, nnz = 0;
    uint64_t hash = 0, hash2 = 0;     // two independently seeded 64-bit hashes of the content: a 128-bit key
    std::vector<int32_t> colptr;      // csc: a copy of the pointer array, compared on a hit (not only hashed)
    std::vector<double> sample;       // dense: a strided sample of X (<= 4096 values), compared on a hit as well
    vbnmf_matrix *X = nullptr;
    vbnmf_engine *e = nullptr;
    int r = 0;
    void drop()
    {
        vbnmf_engine_destroy(e); e = nullptr;
        vbnmf_matrix_destroy(X); X = nullptr;
        valid = false;
        colptr.clear();
        sample.clear();
    }
};
StatelessCache &stateless_cache() { static StatelessCache c; return c; }

// Two independently seeded hashes of the same bytes in ONE pass over them (the stateless cache's 128-bit key).  Per 4 MB chunk
// FOUR multiply-xorshift chains per seed, fed the chunk's 8-byte words in turn (word q goes to chain q mod 4), so eight independent
// chains are in flight and a thread hashes at memory speed instead of at one multiply latency per word (a 3.7 MB dense matrix
// -- the reference's shipped data set -- used to take 0.7 ms of every literal drop-in call); chains and chunks are combined in
// order: the value does not depend on the thread count.  The seed starts EVERY chain of every chunk (not only the final combine),
// so two seeds give two INDEPENDENT 64-bit hashes: contents that collide in a chain under one seed do not under the other
// (tests/test_node_shared_cpu.py).  Small inputs are hashed by few threads (a thread is worth starting for a chunk or more).
void hash_bytes2(const void *data, size_t bytes, uint64_t seed_a, uint64_t seed_b, uint64_t &out_a, uint64_t &out_b)
{
    const size_t chunk = (size_t)1 << 22;
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    std::vector<uint64_t> part_a(nchunks ? nchunks : 1, 0), part_b(nchunks ? nchunks : 1, 0);
    const unsigned char *p = static_cast<const unsigned char *>(data);
    constexpr uint64_t K = 0xFF51AFD7ED558CCDull, KL = 0xA24BAED4963EE407ull, KC = 0xC4CEB9FE1A85EC53ull;
    parallel_for((int64_t)nchunks, [&](int64_t b, int64_t e, int) {
        for (int64_t c = b; c < e; c++) {
            const size_t o = (size_t)c * chunk, len = std::min(chunk, bytes - o);
            const uint64_t salt = 0x9E3779B97F4A7C15ull ^ ((uint64_t)c * 0xD6E8FEB86659FD93ull);
            uint64_t ha[4], hb[4];
            for (int j = 0; j < 4; j++) { ha[j] = seed_a ^ salt ^ ((uint64_t)j * KL); hb[j] = seed_b ^ salt ^ ((uint64_t)j * KL); }
            size_t q = 0;
            for (; q + 32 <= len; q += 32) {
                uint64_t w[4];
                std::memcpy(w, p + o + q, 32);
                for (int j = 0; j < 4; j++) {
                    ha[j] = (ha[j] ^ w[j]) * K; hb[j] = (hb[j] ^ w[j]) * K;
                    ha[j] ^= ha[j] >> 32; hb[j] ^= hb[j] >> 32;
                }
            }
            for (int j = 0; q + 8 <= len; q += 8, j++) {
                uint64_t w;
                std::memcpy(&w, p + o + q, 8);
                ha[j] = (ha[j] ^ w) * K; hb[j] = (hb[j] ^ w) * K;
                ha[j] ^= ha[j] >> 32; hb[j] ^= hb[j] >> 32;
            }
            for (; q < len; q++) { ha[0] = (ha[0] ^ p[o + q]) * 0x100000001B3ull; hb[0] = (hb[0] ^ p[o + q]) * 0x100000001B3ull; }
            uint64_t da = ha[0], db = hb[0];
            for (int j = 1; j < 4; j++) { da = (da ^ ha[j]) * KC; da ^= da >> 29; db = (db ^ hb[j]) * KC; db ^= db >> 29; }
            part_a[c] = da; part_b[c] = db;
        }
    });
    uint64_t ha = seed_a, hb = seed_b;
    for (uint64_t v : part_a) { ha = (ha ^ v) * KC; ha ^= ha >> 29; }
    for (uint64_t v : part_b) { hb = (hb ^ v) * KC; hb ^= hb >> 29; }
    out_a = ha; out_b = hb;
}
uint64_t hash_bytes(const void *data, size_t bytes, uint64_t seed)
{
    uint64_t a, b;
    hash_bytes2(data, bytes, seed, ~seed, a, b);
    return a;
}

bool stateless_cache_enabled()
{
    const char *sv = getenv("VBNMF_STATELESS_CACHE");
    return !(sv && sv[0] == '0');
}

// The engine of rank r on the matrix with this key: from the cache, or ingested now through `ingest`.
int stateless_engine(int kind, int64_t n, int64_t m, int64_t nnz, uint64_t hash, uint64_t hash2, const int32_t *colptr, const double *dense, int32_t r,
                     const std::function<int(vbnmf_matrix **)> &ingest, vbnmf_engine **out)
{
    StatelessCache &C = stateless_cache();
    bool hit = C.valid && C.kind == kind && C.n == n && C.m == m && C.nnz == nnz && C.hash == hash && C.hash2 == hash2;
    if (hit && colptr) hit = C.colptr.size() == (size_t)m + 1 && std::memcmp(C.colptr.data(), colptr, ((size_t)m + 1) * sizeof(int32_t)) == 0;
    // dense: every 1/4096-th value (an odd stride, so the sample walks through all rows) beside the two hashes
    const size_t total = dense ? (size_t)n * (size_t)m : 0, stride = std::max<size_t>(1, total / 4096) | 1;
    if (hit && dense) {
        size_t q = 0;
        for (size_t o = 0; o < total && hit; o += stride, q++) hit = q < C.sample.size() && std::memcmp(&C.sample[q], dense + o, sizeof(double)) == 0;
        hit = hit && q == C.sample.size();
    }
    if (!hit) {
        C.drop();
        if (int rc = ingest(&C.X)) { C.X = nullptr; return rc; }
        C.kind = kind; C.n = n; C.m = m; C.nnz = nnz; C.hash = hash; C.hash2 = hash2; C.valid = true;
        if (colptr) C.colptr.assign(colptr, colptr + m + 1);
        if (dense) for (size_t o = 0; o < total; o += stride) C.sample.push_back(dense[o]);
    }
    // The stateless entries take no device argument (the reference's signature has none): VBNMF_DEVICE names it, read at
    // every call, so the slaves of Rmpi::mpi.applyLB (reference R/bayesian.R:262-263) that call the plain shim can each be
    // given their own GPU; default device 0.
    int device = 0;
    if (const char *dv = getenv("VBNMF_DEVICE")) device = atoi(dv);
    if (!C.e || C.r != r || C.e->device != device) {
        vbnmf_engine_destroy(C.e); C.e = nullptr;
        if (int rc = vbnmf_engine_create(C.X, r, device, &C.e)) { C.e = nullptr; return rc; }
        C.r = r;
    }
    *out = C.e;
    return VBNMF_OK;
}

int update_once(vbnmf_engine *e, const double *lw_in, const double *lh_in, const double *eh_in,
                double aw, double bw, double ah, double bh, double fudge,
                double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    int rc = vbnmf_engine_set_state(e, lw_in, lh_in, eh_in);
    if (!rc) rc = vbnmf_engine_step(e, aw, bw, ah, bh, fudge, lkh, nullptr);
    if (!rc) rc = vbnmf_engine_get_state(e, lw, lh, ew, eh, dw, dh);
    return rc;
}

int ml_update_once(vbnmf_engine *e, const double *w_in, const double *h_in, int32_t prior, double gamma_a, double gamma_b,
                   double *w, double *h, double *lk)
{
    int rc = vbnmf_engine_ml_set_state(e, w_in, h_in);
    if (!rc) rc = vbnmf_engine_ml_step(e, prior, gamma_a, gamma_b, lk);
    if (!rc) rc = vbnmf_engine_ml_get_state(e, w, h);
    return rc;
}

// dense / CSC front ends shared by the VB and ML stateless calls: `use(engine)` runs under the cache's lock
int with_dense(int64_t n, int64_t m, int32_t r, const double *X, const std::function<int(vbnmf_engine *)> &use)
{
    if (n <= 0 || m <= 0 || !X) return fail(VBNMF_ERR_BAD_ARG, "X is NULL or has a non-positive dimension");
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    const bool cache = stateless_cache_enabled();
    uint64_t h = 0, h2 = 0;
    if (cache) hash_bytes2(X, (size_t)n * (size_t)m * sizeof(double), 0x64656E7365ull, 0x3243F6A8885A308Dull, h, h2);
    if (!cache) C.drop();
    vbnmf_engine *e = nullptr;
    int rc = stateless_engine(0, n, m, 0, h, h2, nullptr, X, r, [&](vbnmf_matrix **M) { return vbnmf_matrix_from_dense(n, m, X, M); }, &e);
    if (!rc) rc = use(e);
    if (!cache || rc) C.drop();
    return rc;
}

int with_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
             const std::function<int(vbnmf_engine *)> &use)
{
    if (n <= 0 || m <= 0 || !p) return fail(VBNMF_ERR_BAD_ARG, "a CSC slot pointer is NULL or a dimension is non-positive");
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    const bool cache = stateless_cache_enabled();
    // the pointer array is checked BEFORE anything is read through it (the hash below walks nnz elements of i and x)
    if (p[0] != 0) return fail(VBNMF_ERR_BAD_ARG, "pointer array must start at 0");
    for (int64_t j = 0; j < m; j++)
        if (p[j + 1] < p[j]) return fail(VBNMF_ERR_BAD_ARG, "pointer array is not non-decreasing at %lld", (long long)j);
    const int64_t nnz = p[m];
    if (nnz > 0 && (!i || !x)) return fail(VBNMF_ERR_BAD_ARG, "a CSC slot pointer is NULL");
    uint64_t h = 0, h2 = 0;
    if (cache) {
        hash_bytes2(i, (size_t)nnz * sizeof(int32_t), 0x637363ull, 0x3243F6A8885A308Dull, h, h2);
        hash_bytes2(x, (size_t)nnz * sizeof(double), h, h2, h, h2);
    }
    if (!cache) C.drop();
    vbnmf_engine *e = nullptr;
    int rc = stateless_engine(1, n, m, nnz, h, h2, p, nullptr, r, [&](vbnmf_matrix **M) { return vbnmf_matrix_from_csc(n, m, p, i, x, M); }, &e);
    if (!rc) rc = use(e);
    if (!cache || rc) C.drop();
    return rc;
}

}  // namespace

extern "C" {

void vbnmf_stateless_cache_clear(void)
{
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    C.drop();
}

int vbnmf_update_dense(int64_t n, int64_t m, int32_t r, const double *X, const double *lw_in, const double *lh_in,
                       const double *eh_in, double aw, double bw, double ah, double bh, double fudge,
                       double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    if (!lw_in || !lh_in || !eh_in) return fail(VBNMF_ERR_BAD_ARG, "a wh member is NULL");
    return with_dense(n, m, r, X, [&](vbnmf_engine *e) {
        return update_once(e, lw_in, lh_in, eh_in, aw, bw, ah, bh, fudge, lw, lh, ew, eh, dw, dh, lkh); });
}

int vbnmf_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
                     const double *lw_in, const double *lh_in, const double *eh_in,
                     double aw, double bw, double ah, double bh, double fudge,
                     double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    if (!lw_in || !lh_in || !eh_in) return fail(VBNMF_ERR_BAD_ARG, "a wh member is NULL");
    return with_csc(n, m, r, p, i, x, [&](vbnmf_engine *e) {
        return update_once(e, lw_in, lh_in, eh_in, aw, bw, ah, bh, fudge, lw, lh, ew, eh, dw, dh, lkh); });
}

int vbnmf_ml_update_dense(int64_t n, int64_t m, int32_t r, const double *X, const double *w_in, const double *h_in,
                          int32_t prior, double gamma_a, double gamma_b, double *w, double *h, double *lk)
{
    if (!w_in || !h_in) return fail(VBNMF_ERR_BAD_ARG, "w or h is NULL");
    return with_dense(n, m, r, X, [&](vbnmf_engine *e) { return ml_update_once(e, w_in, h_in, prior, gamma_a, gamma_b, w, h, lk); });
}

int vbnmf_ml_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
                        const double *w_in, const double *h_in, int32_t prior, double gamma_a, double gamma_b,
                        double *w, double *h, double *lk)
{
    if (!w_in || !h_in) return fail(VBNMF_ERR_BAD_ARG, "w or h is NULL");
    return with_csc(n, m, r, p, i, x, [&](vbnmf_engine *e) { return ml_update_once(e, w_in, h_in, prior, gamma_a, gamma_b, w, h, lk); });
}

}  // extern "C"
