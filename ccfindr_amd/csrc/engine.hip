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
// Here: creation and destroy, state in and out, the host-stepped step, the VB loops of one engine and of a group, the
// communicators -- and the helpers of engine.h that the units on the same engine call (batch.hip, mlnmf.hip, svd.hip,
// labels.hip, hooks.hip).
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
#include "engine.h"
#include "loop.h"
#include "step.h"

using namespace vbnmf;

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

}  // namespace

namespace vbnmf {

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

static int launch_sweep(vbnmf_engine *e)
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
int stage_ids(const DeviceSide &S, unsigned grid, bool dense)
{
    return !dense && S.n_rows >= (int64_t)256 * grid ? 1 : 0;
}

// ctl != nullptr: device-driven loop, the hyper-parameters are read from the control block on the device
int launch_update(vbnmf_engine *e, bool gene_side, double a, double b, double fudge, const LoopCtl *ctl, const ControlFold *foldp)
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
static bool build_update_table(const Layout &LA, const Layout &LB, int ub, int R, std::vector<uint32_t> &tab, int32_t &stride4, int32_t &V,
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
static int launch_update2(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge, const LoopCtl *ctl = nullptr,
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

static int launch_final(vbnmf_engine *e)
{
    const double *tail = e->partitioned ? e->red + (size_t)e->n * e->R : nullptr;
    const int64_t nep = 2 * (int64_t)e->n_wg;
    e->seq += 1.0;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_final<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->ub, tail, e->bpH, e->ub, e->epart, nep, e->lgx, e->r,
                                            (double)e->n, (double)e->m_global, e->seq, e->d_out, e->h_out_dev);
    });
}

// out[major][k] of one side = the sum of the major's task partials (k_pack)
int launch_side_pack(vbnmf_engine *e, bool gene_side, double *target)
{
    const SideView v = side_view(e, gene_side);
    const int64_t cnt = v.nmaj * e->R;
    return launch_kernel<k_pack>(e, dim3((unsigned)((cnt + 255) / 256)), 256, 0, v.S.part, v.S.row_ptr, v.S.row_task, v.nmaj, e->R, target);
}

// the tail of `red` = [column sums of bpH (R + 2) | sum of the evidence partials | constant] of this partition (k_tail)
int launch_tail(vbnmf_engine *e, const double *epart, int64_t nepart, double constant)
{
    return launch_kernel<k_tail>(e, dim3(1), 1024, 0, e->bpH, e->ub, e->R, epart, nepart, constant, e->red + (size_t)e->n * e->R);
}

// partitioned engines: sweep output -> reduce buffer = [swsum | rowSum(eh) | sum H-terms | sum log lh | data term | lgx]
static int launch_pack(vbnmf_engine *e)
{
    if (int rc = launch_side_pack(e, true, e->red)) return rc;
    return launch_tail(e, e->epart, 2 * (int64_t)e->n_wg, e->lgx);
}

// the first exchange of a device-driven partitioned step, VB or ML (k_pack_tail): [sum over a gene's tasks of the gene-side
// partial rows (n*R) | column sums of bpH (R + 2)]
int launch_pack_tail(vbnmf_engine *e, const int32_t *stop)
{
    const int64_t cnt = e->n * e->R;
    return launch_kernel<k_pack_tail>(e, dim3((unsigned)((cnt + 255) / 256) + 1), 256, 0, e->A.part, e->A.row_ptr, e->A.row_task, e->n, e->R, e->red,
                                      e->bpH, e->ub, stop);
}

// ... and what its second exchange sends where no control step is folded in (k_tail_data): [sum of the evidence partials | constant]
int launch_tail_data(vbnmf_engine *e, const double *epart, int64_t nepart, double constant, double *out2)
{
    return launch_kernel<k_tail_data>(e, dim3(1), 1024, 0, epart, nepart, constant, out2, (const int32_t *)&e->ctl->stop);
}

// the local group's all-reduce (k_group_sum; k_group_sum_at: `count` doubles from offset `off` of the buffers)
int launch_group_sum(hipStream_t stream, const double *const *send, double *const *recv, int parts, int64_t count)
{
    hipLaunchKernelGGL(k_group_sum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, send, recv, parts, count);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int launch_group_sum_at(hipStream_t stream, const double *const *send, double *const *recv, int parts, int64_t off, int64_t count)
{
    hipLaunchKernelGGL(k_group_sum_at, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, send, recv, parts, off, count);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

static int launch_vb_side(vbnmf_engine *e, bool gene_side)
{
    return launch_side_sweep<true>(e, sweep_side_args(e, gene_side), gene_side);
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
    volatile double *flag = e->h_out + kOutSeq;
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
static int bounded_stream_sync(vbnmf_engine *e, hipStream_t stream, const char *what)
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

}  // namespace vbnmf

namespace {

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
        hipLaunchKernelGGL(k_pack, dim3(1), dim3(256), 0, nullptr, (const double *)p, (const int32_t *)nullptr, (const uint32_t *)nullptr, (int64_t)0, 2, p);   // no majors: loads the module, touches nothing
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

}  // extern "C"

namespace vbnmf {

// column-major n x r (R matrix) -> device [n][R]; or r x m column-major (already index-major) -> [m][R].
// perm (cell-indexed arrays only): device row p holds the caller's major perm[p] (the layout's order of the cells).
// host threads for a conversion of a factor's arrays: one per 32 K elements (a 200 x 3 factor is not worth waking anyone for)
static int state_threads(int64_t nmaj, int R)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (nmaj * (int64_t)R) >> 15));
}

void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, double *dst,
                    const std::vector<int32_t> *perm)
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

void to_index_major(const double *src, int64_t nmaj, int r, int R, bool src_is_major_contiguous, std::vector<double> &dst,
                    const std::vector<int32_t> *perm)
{
    dst.resize((size_t)nmaj * R);
    to_index_major(src, nmaj, r, R, src_is_major_contiguous, dst.data(), perm);
}

void from_index_major(const double *src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                      const std::vector<int32_t> *perm)
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

void from_index_major(const std::vector<double> &src, int64_t nmaj, int r, int R, bool dst_is_major_contiguous, double *dst,
                      const std::vector<int32_t> *perm)
{
    from_index_major(src.data(), nmaj, r, R, dst_is_major_contiguous, dst, perm);
}

}  // namespace vbnmf

extern "C" {

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
    if (lkh) *lkh = e->h_out[kOutLkh];
    if (stats) for (int q = 0; q < 4; q++) stats[q] = e->h_out[kOutStats + q];
    return VBNMF_OK;
}

int vbnmf_engine_step(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge, double *lkh, double *stats)
{
    if (e && e->partitioned) return fail(VBNMF_ERR_STATE, "a partitioned engine needs step_local / all-reduce / step_finish");
    if (int rc = vbnmf_engine_step_local(e, aw, bw, ah, bh, fudge)) return rc;
    return vbnmf_engine_step_finish(e, lkh, stats);
}

}  // extern "C"

// ---------------------------------------------------------------- device-driven loops (their host driver: loop.h)
namespace vbnmf {

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

static int launch_control(vbnmf_engine *e, double *hist_dev, bool reduced)
{
    const int64_t nep = 2 * (int64_t)e->n_wg;
    const double *tail = reduced ? e->red_g + (size_t)e->n * e->R : nullptr;
    const double *small = reduced ? e->red_g + (size_t)e->n * e->R + e->R + 2 : nullptr;
    return with_rank(e->R, [&](auto rt) {
        return launch_kernel<k_control<rt()>>(e, dim3(1), 1024, 0, e->bpW, e->bpH, e->ub, e->epart, nep, e->lgx, e->r, (double)e->n,
                                              (double)e->m_global, e->ctl, hist_dev, e->h_out_dev, tail, small);
    });
}

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
static int queue_vb_step(const LoopGroup &G, double fudge, bool hist, int max_it)
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
        if (int q = launch_pack_tail(e, stop)) return q;
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
    for (int p = 0; p < P; p++) {
        vbnmf_engine *e = G.e[p];
        if (int rc = launch_vb_side(e, false)) return rc;
        if (!fold) { if (int rc = launch_tail_data(e, e->epart, 2 * (int64_t)e->n_wg, e->lgx, e->red + nbig)) return rc; }
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
        if (int rc = launch_group_sum(L->stream, c->d_send_small, c->d_recv_small, P, nsmall)) return rc;
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

// k_ctl_init for RunScope::begin (loop.h), which checks the launches of all its engines at once
void launch_ctl_init(hipStream_t stream, LoopCtl *ctl, const LoopCtl &v)
{
    hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(1), 0, stream, ctl, v);
}

// The results the last live control step of each of `count` engines left in its h_out (HostOutSlot, kernels.h): kOutIt steps,
// kOutReason, kOutLkh the last likelihood (lk: lkh of the VB loop, lk of the ML loop -- the slot itself stays, ml_likelihood()
// keeps answering for the pair held now), kOutLk0 and kOutHyper, the hyper-parameters (VB); history: `rows` rows of `width`
// doubles per engine.
void read_out(vbnmf_engine *const *engs, int count, int32_t *it_out, double *lk0_out, double *lk_out, int32_t *reason_out,
              double *hyper, double *history, int64_t rows, int width)
{
    for (int b = 0; b < count; b++) {
        const double *ho = engs[b]->h_out;
        const int it = (int)ho[kOutIt];
        if (hyper) for (int q = 0; q < 4; q++) hyper[(size_t)b * 4 + q] = ho[kOutHyper + q];
        if (it_out) it_out[b] = it;
        if (lk0_out) lk0_out[b] = ho[kOutLk0];
        if (lk_out) lk_out[b] = ho[kOutLkh];
        if (reason_out) reason_out[b] = (int)ho[kOutReason];
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

// The four hyper-parameters a device-driven loop starts from: finite and > 0, or the Newton iteration of hyper_update
// (dev_hyper_update_pair) would be handed a shape its special functions are not written for.  Checked before any launch.
int check_hyper(const double *hyper)
{
    for (int q = 0; q < 4; q++)
        if (!(hyper[q] > 0.0) || !std::isfinite(hyper[q]))
            return fail(VBNMF_ERR_BAD_ARG, "aw, bw, ah and bh must be finite and > 0 (got %g, %g, %g, %g)", hyper[0], hyper[1], hyper[2], hyper[3]);
    return VBNMF_OK;
}

static int run_group(const LoopGroup &G, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0, int32_t dn,
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

}  // namespace vbnmf

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

}  // extern "C"

namespace vbnmf {

int group_members(vbnmf_comm *c, LoopGroup &G)
{
    if (!c) return fail(VBNMF_ERR_BAD_ARG, "communicator handle is NULL");
    if (c->kind != 1) return fail(VBNMF_ERR_STATE, "not a local group (an RCCL communicator is driven through its engine)");
    if ((int)c->members.size() != c->nranks) return fail(VBNMF_ERR_STATE, "the local group has %d of its %d partitions attached", (int)c->members.size(), c->nranks);
    for (vbnmf_engine *q : c->members) if (!q) return fail(VBNMF_ERR_STATE, "a partition engine of the group has been destroyed");
    G.e = c->members.data(); G.count = c->nranks; G.comm = c;
    return VBNMF_OK;
}

// The reduce buffers of a local group summed in place, partition order, behind everything queued on the members' streams.
int group_sum_in_place(const LoopGroup &G)
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

}  // namespace vbnmf

extern "C" {

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

#ifdef VBNMF_ABL_STAMPS                                       /* instrumented builds only (profiles/ubench/r04/update_stamps.sh) */
int vbnmf_test_update_stamps(unsigned long long *out)
{
    if (hipDeviceSynchronize() != hipSuccess) return VBNMF_ERR_HIP;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_upd_stamps), sizeof(unsigned long long) * 2 * kUpdateBlocks * 12) == hipSuccess ? VBNMF_OK : VBNMF_ERR_HIP;
}
#endif

}  // extern "C"
