// step.h -- the kernels of the engine that are no templates (included once, by engine.hip: a second unit would emit them
// again): the 'random' initial state of vb_init (reference R/bayesian.R:111-115: w ~ Gamma(shape aw, scale bw/aw),
// h ~ Gamma(ah, bh/ah); philox.h), the reduce buffer of cell-partitioned runs, the local group's sum, the control block's load.
#pragma once
#include "kernels.h"
#include "philox.h"

namespace vbnmf {

// f[major][k] = e[major][k] = Gamma(shape a, scale b / a) for k < r (pad columns 0); factor 0 = W, 1 = H.  The element
// index is the GLOBAL (major, k) position (major0 = first cell of a partition), so a partitioned run draws the same H.
__global__ __launch_bounds__(256) void k_gamma_init(double *__restrict__ f, double *__restrict__ e, double *__restrict__ dvar,
                                                    int64_t nmaj, int64_t major0, int r, int R, double a, double b,
                                                    uint32_t factor, uint32_t k0, uint32_t k1, const int32_t *__restrict__ perm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nmaj * R) return;
    const int64_t M = i / R;
    const int k = (int)(i - M * R);
    double v = 0.0;
    // (perm: the layout's order of the cells -- row M of the array is the caller's major perm[M]; the draw is keyed by the
    // CALLER's global element index, so it does not depend on the order, the launch geometry or the partitioning)
    if (k < r) v = gamma_draw(a, b / a, (uint64_t)(major0 + (perm ? (int64_t)perm[M] : M)) * (uint64_t)r + (uint64_t)k, factor, k0, k1);
    f[i] = v;
    if (e) e[i] = v;
    if (dvar) dvar[i] = 0.0;
}

// ------------------------------------------------------------------------------------
// Cell-partitioned runs: the gene-side statistics and the cell-side scalars go into the
// reduce buffer [swsum n*R | tail R+4] that the caller all-reduces.
// ------------------------------------------------------------------------------------
// out[major][k] = sum of the major's task partials, fixed order.
__global__ __launch_bounds__(256) void k_pack(const double *__restrict__ part, const int32_t *__restrict__ row_ptr,
                                              const uint32_t *__restrict__ row_task, int64_t nmaj, int R,
                                              double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nmaj * R) return;
    const int64_t M = e / R;
    const int k = (int)(e - M * R);
    out[e] = task_sum(part, row_task, row_ptr[M], row_ptr[M + 1], R, k);
}

// k_pack and k_tail_h in one launch (the device-driven partitioned loop): one extra block forms the cell side's column sums.
__global__ __launch_bounds__(256) void k_pack_tail(const double *__restrict__ part, const int32_t *__restrict__ row_ptr,
                                                   const uint32_t *__restrict__ row_task, int64_t nmaj, int R,
                                                   double *__restrict__ out, const double *__restrict__ bpH, int nbH,
                                                   const int32_t *__restrict__ stop)
{
    if (blockIdx.x == gridDim.x - 1) {
        if (stop && *stop) return;                         // (as k_tail_h: steps queued past the stop leave the tail as it is)
        bp_colsums(bpH, nbH, R + 2, out + nmaj * R, 256);
        return;
    }
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nmaj * R) return;
    const int64_t M = e / R;
    const int k = (int)(e - M * R);
    out[e] = task_sum(part, row_task, row_ptr[M], row_ptr[M + 1], R, k);
}

// Device-driven loop of a cell-partitioned engine: the reduce buffer is sent in two pieces.  The first,
// [swsum n*R | rowSum(eh)_k (R) | sum H-terms | sum log lh], is complete once the gene-side sweep and the H update are
// done (k_pack + k_tail_h) and travels while the cell-side sweep runs; the second, [data term | sum lgamma(x+1)], needs
// both sweeps (k_tail_data) and is two doubles.
__global__ __launch_bounds__(1024) void k_tail_h(const double *__restrict__ bpH, int nbH, int R, double *__restrict__ tail,
                                                 const int32_t *__restrict__ stop)
{
    if (stop && *stop) return;
    bp_colsums(bpH, nbH, R + 2, tail, 1024);
}

// In-process stand-in for the all-reduce between partition engines that share one device (tests, single-GPU
// rehearsals of a partitioned run): recv[p][i] = send[0][i] + send[1][i] + ... in partition order, for every p.
__global__ __launch_bounds__(256) void k_group_sum(const double *const *__restrict__ send, double *const *__restrict__ recv,
                                                   int parts, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double s = send[0][i];
    for (int p = 1; p < parts; p++) s += send[p][i];
    for (int p = 0; p < parts; p++) recv[p][i] = s;
}

// The same on `count` doubles from offset `off` of every partition's buffer (the two-double exchange of the partitioned ML loop,
// mlnmf.h, whose offset does not depend on the VB loop's fold as the send / receive tables of its own small exchange do).
__global__ __launch_bounds__(256) void k_group_sum_at(const double *const *__restrict__ send, double *const *__restrict__ recv,
                                                      int parts, int64_t off, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double s = send[0][off + i];
    for (int p = 1; p < parts; p++) s += send[p][off + i];
    for (int p = 0; p < parts; p++) recv[p][off + i] = s;
}

// tail = [rowSum(eh)_k (R) | sum H-terms | sum log lh | data term | sum lgamma(x+1)] of THIS partition.
__global__ __launch_bounds__(1024) void k_tail(const double *__restrict__ bpH, int nbH, int R,
                                               const double *__restrict__ epart, int64_t nepart, double lgx,
                                               double *__restrict__ tail)
{
    __shared__ double sm[1024];
    bp_colsums(bpH, nbH, R + 2, tail, 1024);
    const double data = block_vec_sum(epart, nepart, sm);
    if (threadIdx.x == 0) { tail[R + 2] = data; tail[R + 3] = lgx; }
}

__global__ __launch_bounds__(1024) void k_tail_data(const double *__restrict__ epart, int64_t nepart, double lgx,
                                                    double *__restrict__ out2, const int32_t *__restrict__ stop)
{
    __shared__ double sm[1024];
    if (stop && *stop) return;
    const double data = block_vec_sum(epart, nepart, sm);
    if (threadIdx.x == 0) { out2[0] = data; out2[1] = lgx; }
}

// Loads the control block of a device-driven loop (stream-ordered, no host copy to wait for).
__global__ void k_ctl_init(LoopCtl *ctl, const LoopCtl v) { *ctl = v; }

}  // namespace vbnmf
