// hyper.h -- device code shared by the step kernels (kernels.h) and the coupled VB projection (vbproject.h): the wave and
// block sums and hyper_update.  Inline and template device functions only -- no kernel is defined here, so any number of
// translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "special.h"

namespace vbnmf {

// the value of lane ^ MASK by DPP (the levels of the sweep's lane tree, kernels.h)
template <int MASK, bool XOR4 = false>
__device__ __forceinline__ double lane_pair_value(double v)
{
    static_assert(MASK == 8 || MASK == 4 || MASK == 2 || MASK == 1, "DPP levels");
    if constexpr (MASK == 4 && XOR4) return __shfl_xor(v, 4, 64);
    constexpr int ctrl = MASK == 8 ? 0x128 : MASK == 4 ? 0x141 : MASK == 2 ? 0x4E : 0xB1;
    return __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xF, 0xF, false),
                            __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xF, 0xF, false));
}
// wave sum without LDS round trips: DPP inside the rows of 16 lanes (quads, half rows, rows), then gfx950's permlane swaps
// across the rows.  Valid in every lane; a fixed tree.
__device__ __forceinline__ double wave_sum_dpp(double v)
{
    v += lane_pair_value<1>(v);
    v += lane_pair_value<2>(v);
    v += lane_pair_value<4>(v);
    v += lane_pair_value<8>(v);
    {   // rows 0+1, 2+3: v_permlane16_swap of the value with a copy of itself leaves (own row, partner row) in the two registers
        const int lo = __double2loint(v), hi = __double2hiint(v);
        const auto r0 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), r1 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
    }
    {   // the two halves of the wave
        const int lo = __double2loint(v), hi = __double2hiint(v);
        const auto r0 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), r1 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
    }
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_dpp(v); }     // (valid in every lane; no LDS round trips)

// Sum of v[0..count) by one 1024-thread block, fixed order: thread t adds t, t+1024, ...; a shuffle tree per wave; the
// 16 wave sums through LDS and one more shuffle tree.  Two barriers (the ten-round LDS tree it replaces cost k_control
// and k_final about a microsecond each).
__device__ __forceinline__ double block_sum(double s, double *sm);
__device__ __forceinline__ double block_vec_sum(const double *__restrict__ v, int64_t count, double *sm)
{
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < count; q += 1024) s += v[q];
    return block_sum(s, sm);
}
// the block's total of one value per thread (1024 threads), same order as above
__device__ __forceinline__ double block_sum(double s, double *sm)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    s = wave_sum(s);
    if (lane == 0) sm[wave] = s;
    __syncthreads();
    double r = lane < 16 ? sm[lane] : 0.0;
    r = wave_sum(r);                                  // every wave forms the same total in its lane 0 ...
    r = __shfl(r, 0, 64);                             // ... and hands it to all its lanes
    __syncthreads();                                  // sm may be reused by the caller
    return r;
}

// (digamma, trigamma and one side's share of a Newton iteration: special.h, dev_digamma1 / dev_trigamma / hyper_newton_side.)
// hyper_update (R/bayesian.R:2-53) by lanes 0 and 1 of a wave side by side: lane 0 iterates aw, lane 1 ah -- the two
// Newton recurrences (:19-27) only meet in the convergence test (:37), which the lanes form by exchanging their
// terms, so both run the same number of iterations as the sequential form and reach the same values.  A dependent fp64
// chain (log, digamma, trigamma) costs microseconds on one lane; this halves it.
// Returns 0, or 1 when the Newton iteration does not converge ("Hyper-parameter update failed to converge", :43);
// lane 0 stores the four new hyper-parameters.
// TRACE (the test hook k_test_hyper_update only; the loops instantiate TRACE = false, which compiles the stores away):
// each lane stores its a1 of iteration k (0-based) to trace[100 * lane + k], lane 0 the number of iterations to *iters.
template <bool TRACE = false>
__device__ inline int dev_hyper_update_pair(const int32_t *flags, const double *stats, double *hyper, int lane,
                                            double *trace = nullptr, int32_t *iters = nullptr)
{
    if (flags[0] + flags[1] + flags[2] + flags[3] == 0) return 0;                          // :4
    double a0 = hyper[2 * lane];                           // aw (lane 0) or ah (lane 1)
    const double b0 = hyper[2 * lane + 1];                 // bw or bh
    const double lm = lane ? stats[1] : stats[0], em = lane ? stats[3] : stats[2];   // mean log l, mean e of this side (:8-11)
    const int fa = flags[2 * lane];
    double a1 = a0;
    int failed = 0;
    [[maybe_unused]] int done = 0;                         // iterations run (TRACE)
    if (flags[0] + flags[2] > 0) {                                                         // :15
        int i = 1;
        while (i < 100) {                                                                  // Niter = 100 (:343)
            // A non-finite step is reported as a failed hyper-parameter update (reason 3): see hyper_newton_side.
            int hv, bad;
            a1 = hyper_newton_side(a0, b0, lm, em, fa, &hv, &bad);                         // :18-35
            if constexpr (TRACE) trace[100 * lane + done++] = a1;
            const double u = bad ? 0.0 : 1.0 - a1 / a0;
            const double uw = __shfl(u, 0, 64), uh = __shfl(u, 1, 64);
            bad = __shfl(bad, 0, 64) | __shfl(bad, 1, 64);
            if (bad) { failed = 1; break; }
            if (uw * uw + uh * uh < 1e-3) break;                                           // Tol = 1e-3 (:344)
            a0 = a1; i++;
        }
        if (i == 100) failed = 1;
    }
    if constexpr (TRACE) { if (lane == 0) *iters = done; }
    const double aw1 = __shfl(a1, 0, 64), ah1 = __shfl(a1, 1, 64);
    if (lane == 0 && !failed) {
        hyper[0] = aw1; hyper[1] = flags[1] ? stats[2] : hyper[1];                         // :48-49
        hyper[2] = ah1; hyper[3] = stats[3];                                               // :50-51 (both branches assign ehm)
    }
    return failed;
}

}  // namespace vbnmf
