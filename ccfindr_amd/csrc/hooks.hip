// hooks.hip -- test hooks: the special functions and hyper_update as the device evaluates them, each beside its host form, and
// a host function that holds an engine's stream for a while.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <new>
#include <thread>
#include <vector>

#include "engine.h"

namespace vbnmf {

// Device-side evaluation of the special functions, for tests (tests/test_gpu_special.py).
__global__ void k_test_special(int kind, int64_t n, const double *__restrict__ x, double *__restrict__ y,
                               const LogTabEntry *__restrict__ tab)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double psi, lg;
    switch (kind) {
        case 0: y[i] = dev_log(x[i]); break;
        case 1: dev_psi_lgamma(x[i], &psi, &lg); y[i] = psi; break;
        case 2: dev_psi_lgamma(x[i], &psi, &lg); y[i] = lg; break;
        case 3: y[i] = dev_div(1.0, x[i]); break;
        case 4: y[i] = sp_rcp_seed(x[i]); break;             // raw v_rcp_f64
        case 5: y[i] = (double)__builtin_amdgcn_rcpf((float)x[i]); break;   // raw v_rcp_f32
        case 7: y[i] = dev_trigamma(x[i]); break;
        case 8:                                              // the pair form: quads wa, wb, xa, xb in; qa, qb, r, 0 out
            if (i % 4 == 0 && i + 3 < n) { y[i + 2] = dev_div_pair(x[i + 2], x[i], x[i + 3], x[i + 1], &y[i], &y[i + 1]); y[i + 3] = 0.0; }
            break;
        default: y[i] = dev_log_tab(x[i], tab); break;
    }
}

// Device-side evaluation of hyper_update, for tests (tests/test_gpu_hyper_update.py): one wave per case, lanes 0 and 1 in
// the loops' own dev_hyper_update_pair, traced.  hyper: [count][4] in / out; trace: [count][2][100]; iters, failed: [count].
__global__ __launch_bounds__(64) void k_test_hyper_update(int count, const int32_t *__restrict__ flags, const double *__restrict__ stats,
                                                          double *hyper, int32_t *__restrict__ failed, int32_t *__restrict__ iters,
                                                          double *trace)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= count || lane > 1) return;
    const int f = dev_hyper_update_pair<true>(flags + 4 * (size_t)c, stats + 4 * (size_t)c, hyper + 4 * (size_t)c, lane,
                                              trace + 200 * (size_t)c, iters + c);
    if (lane == 0) failed[c] = f;
}

}  // namespace vbnmf

using namespace vbnmf;

extern "C" {

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
    DeviceCall hb;                                       // (never entered: use_device(0) chose the device)
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
    HIPCHECK(hipMemcpy(hyper_out, dhy, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(trace, dtr, 200 * n * sizeof(double), hipMemcpyDeviceToHost));
    return VBNMF_OK;
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

}  // extern "C"
