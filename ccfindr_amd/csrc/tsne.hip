// tsne.hip -- the t-SNE map behind visualize_clusters (tsne.h): arguments are checked and x is normalised on the host, the
// affinities are one launch at creation, an iteration of the descent is a force launch and an update launch on the handle's
// stream.  The handle lives across calls and regrows one of its buffers (tsne_costs_reserve), so it frees what it owns in
// vbnmf_tsne_destroy and not through a DeviceCall.
#include <algorithm>
#include <cmath>
#include <new>

#include "device.h"
#include "tsne.h"

using namespace vbnmf;

struct vbnmf_tsne {
    int device = 0;
    int32_t n = 0, d = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    double *xt = nullptr, *beta = nullptr, *sum_p = nullptr, *inv_s = nullptr;
    int32_t *trips = nullptr;
    double *state = nullptr;       // [6][n]: y0 y1 u0 u1 g0 g1
    double *sums = nullptr;        // [kTsneForceSums][n]
    double *cost_i = nullptr;      // [n]
    double *costs = nullptr;       // [costs_cap] the run's cost values
    int64_t costs_cap = 0;
    int aff_grid = 0, force_grid = 0;
    bool has_state = false;
    double times_ms[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};

namespace {

thread_local double tl_tsne_create_ms[3] = {0.0, 0.0, 0.0};

int tsne_use(vbnmf_tsne *t)
{
    if (!t) return fail(VBNMF_ERR_BAD_ARG, "NULL t-SNE handle");
    HIPCHECK(hipSetDevice(t->device));
    return VBNMF_OK;
}

int tsne_launch_force(vbnmf_tsne *t, int cost)
{
    const int64_t n = t->n;
    TsneForceArgs a;
    a.n = t->n; a.d = t->d; a.cost = cost; a.xt = t->xt; a.beta = t->beta; a.inv_s = t->inv_s;
    a.y0 = t->state; a.y1 = t->state + n; a.inv_2n = 1.0 / (2.0 * (double)n); a.sums = t->sums;
    const dim3 grid((unsigned)t->force_grid), block(kTsneThreads);
    const size_t lds = tsne_force_lds(t->d);
    const int DR = tsne_force_width(t->d);
    if (DR == 8) hipLaunchKernelGGL(k_tsne_force<8>, grid, block, lds, t->stream, a);
    else if (DR == 16) hipLaunchKernelGGL(k_tsne_force<16>, grid, block, lds, t->stream, a);
    else if (DR == 32) hipLaunchKernelGGL(k_tsne_force<32>, grid, block, lds, t->stream, a);
    else hipLaunchKernelGGL(k_tsne_force<0>, grid, block, lds, t->stream, a);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int tsne_launch_update(vbnmf_tsne *t, int do_step, int do_cost, double e, double m, double eta, double min_gain, double *cost_out)
{
    const int64_t n = t->n;
    TsneUpdArgs a;
    a.n = t->n; a.do_step = do_step; a.do_cost = do_cost; a.e = e; a.m = m; a.eta = eta; a.min_gain = min_gain; a.sums = t->sums;
    a.y0 = t->state; a.y1 = t->state + n; a.u0 = t->state + 2 * n; a.u1 = t->state + 3 * n; a.g0 = t->state + 4 * n; a.g1 = t->state + 5 * n;
    a.cost_i = t->cost_i; a.cost_out = cost_out;
    hipLaunchKernelGGL(k_tsne_update, dim3(1), dim3(kTsneUpdThreads), 0, t->stream, a);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int tsne_costs_reserve(vbnmf_tsne *t, int64_t count)
{
    if (count <= t->costs_cap) return VBNMF_OK;
    HIPCHECK(hipStreamSynchronize(t->stream));
    dev_free(t->costs);
    t->costs = nullptr; t->costs_cap = 0;
    if (int rc = dev_alloc(&t->costs, (size_t)count)) return rc;
    t->costs_cap = count;
    return VBNMF_OK;
}

// n x 2 row-major <-> two columns
void tsne_split(const double *a, int64_t n, double *c0, double *c1)
{
    for (int64_t i = 0; i < n; i++) { c0[i] = a[2 * i]; c1[i] = a[2 * i + 1]; }
}
void tsne_join(const double *c0, const double *c1, int64_t n, double *a)
{
    for (int64_t i = 0; i < n; i++) { a[2 * i] = c0[i]; a[2 * i + 1] = c1[i]; }
}

int tsne_create(vbnmf_tsne *t, int32_t device, const std::vector<double> &xt, double perplexity)
{
    const int64_t n = t->n;
    const int d = t->d;
    t->device = device;
    HIPCHECK(hipSetDevice(device));
    int cus = 0;
    if (int rc = device_cus(device, cus)) return rc;
    const auto t0 = host_clock::now();
    HIPCHECK(hipStreamCreate(&t->stream));
    HIPCHECK(hipEventCreate(&t->ev0));
    HIPCHECK(hipEventCreate(&t->ev1));
    HIPCHECK(hipEventCreate(&t->ev2));
    HIPCHECK(hipEventCreate(&t->ev3));
    int rc;
    if ((rc = dev_alloc(&t->xt, (size_t)n * d)) || (rc = dev_alloc(&t->beta, (size_t)n)) || (rc = dev_alloc(&t->sum_p, (size_t)n)) ||
        (rc = dev_alloc(&t->inv_s, (size_t)n)) || (rc = dev_alloc(&t->trips, (size_t)n)) || (rc = dev_alloc(&t->state, 6 * (size_t)n)) ||
        (rc = dev_alloc(&t->sums, (size_t)kTsneForceSums * n)) || (rc = dev_alloc(&t->cost_i, (size_t)n)))
        return rc;
    t->aff_grid = (int)std::min<int64_t>(n, (int64_t)cus * 4);
    t->force_grid = (int)((n + kTsneIBlock - 1) / kTsneIBlock);
    double *scratch = nullptr;
    if (n > kTsneLdsRow) { if ((rc = dev_alloc(&scratch, (size_t)t->aff_grid * (size_t)n))) return rc; }
    hipError_t err = hipMemcpy(t->xt, xt.data(), (size_t)n * d * sizeof(double), hipMemcpyHostToDevice);
    tl_tsne_create_ms[1] = ms_since(t0);
    if (err == hipSuccess) {
        TsneAffArgs a;
        a.n = t->n; a.d = d; a.xt = t->xt; a.scratch = scratch; a.log_u = std::log(perplexity);
        a.beta = t->beta; a.sum_p = t->sum_p; a.inv_s = t->inv_s; a.trips = t->trips;
        err = hipEventRecord(t->ev0, t->stream);
        hipLaunchKernelGGL(k_tsne_affinity, dim3((unsigned)t->aff_grid), dim3(kTsneThreads), 0, t->stream, a);
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipEventRecord(t->ev1, t->stream);
    }
    const hipError_t serr = hipStreamSynchronize(t->stream);                  // scratch is free after this whatever happened
    dev_free(scratch);
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) return fail(VBNMF_ERR_HIP, "vbnmf_tsne_create: %s", hipGetErrorString(err));
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, t->ev0, t->ev1));
    tl_tsne_create_ms[2] = ms;
    for (int k = 0; k < 3; k++) t->times_ms[k] = tl_tsne_create_ms[k];
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int vbnmf_tsne_create(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, vbnmf_tsne **handle)
{
    for (double &v : tl_tsne_create_ms) v = 0.0;
    if (!handle) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *handle = nullptr;
    if (!x) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (n < 1 || n > 2147481600ll) return fail(VBNMF_ERR_BAD_ARG, "n = %lld points is outside [1, 2^31 - 2048]", (long long)n);   // (int loop counters step by <= 1024)
    if (d < 1 || d > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "d = %d is outside [1, %d]", d, VBNMF_MAX_RANK);
    if (!std::isfinite(perplexity) || perplexity < 1.0) return fail(VBNMF_ERR_BAD_ARG, "the perplexity must be finite and >= 1");
    if (!(3.0 * perplexity < (double)(n - 1)))
        return fail(VBNMF_ERR_BAD_ARG, "the perplexity %g is too large for %lld points: 3 perplexity < n - 1 is required", perplexity, (long long)n);
    try {
        const auto t0 = host_clock::now();
        for (int64_t q = 0; q < n * d; q++)
            if (!std::isfinite(x[q])) return fail(VBNMF_ERR_BAD_ARG, "x[%lld, %lld] is not finite", (long long)(q / d), (long long)(q % d));
        // the device's copy is xt[d][n]; the normalisation runs on it in a fixed order: column means, then the largest |value|
        std::vector<double> xt((size_t)n * d);
        for (int64_t i = 0; i < n; i++)
            for (int k = 0; k < d; k++) xt[(size_t)k * n + i] = x[i * d + k];
        if (normalize) {
            double mx = 0.0;
            for (int k = 0; k < d; k++) {
                double *c = xt.data() + (size_t)k * n;
                double s = 0.0;
                for (int64_t i = 0; i < n; i++) s += c[i];
                const double mean = s / (double)n;
                for (int64_t i = 0; i < n; i++) { c[i] -= mean; mx = std::max(mx, std::fabs(c[i])); }
            }
            if (mx > 0.0)
                for (double &v : xt) v /= mx;
        }
        tl_tsne_create_ms[0] = ms_since(t0);
        if (int rc = check_device(device)) return rc;
        std::unique_ptr<vbnmf_tsne, void (*)(vbnmf_tsne *)> t(new vbnmf_tsne(), vbnmf_tsne_destroy);
        t->n = (int32_t)n; t->d = d;
        if (int rc = tsne_create(t.get(), device, xt, perplexity)) return rc;
        *handle = t.release();
        return VBNMF_OK;
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for %lld x %d points", (long long)n, d);
    }
}

void vbnmf_tsne_destroy(vbnmf_tsne *t)
{
    if (!t) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    dev_free(t->xt); dev_free(t->beta); dev_free(t->sum_p); dev_free(t->inv_s); dev_free(t->trips); dev_free(t->state);
    dev_free(t->sums); dev_free(t->cost_i); dev_free(t->costs);
    if (t->ev0) (void)hipEventDestroy(t->ev0);
    if (t->ev1) (void)hipEventDestroy(t->ev1);
    if (t->ev2) (void)hipEventDestroy(t->ev2);
    if (t->ev3) (void)hipEventDestroy(t->ev3);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    if (cur >= 0) (void)hipSetDevice(cur);
    delete t;
}

int vbnmf_tsne_affinity(vbnmf_tsne *t, double *beta, double *sum_p, int32_t *trips)
{
    if (int rc = tsne_use(t)) return rc;
    const size_t n = (size_t)t->n;
    if (beta) HIPCHECK(hipMemcpy(beta, t->beta, n * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_p) HIPCHECK(hipMemcpy(sum_p, t->sum_p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (trips) HIPCHECK(hipMemcpy(trips, t->trips, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

int vbnmf_tsne_set_state(vbnmf_tsne *t, const double *Y, const double *uY, const double *gains)
{
    if (!t || !Y) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    const int64_t n = t->n;
    for (int64_t q = 0; q < 2 * n; q++)
        if (!std::isfinite(Y[q]) || (uY && !std::isfinite(uY[q])) || (gains && !std::isfinite(gains[q])))
            return fail(VBNMF_ERR_BAD_ARG, "the state is not finite at point %lld", (long long)(q / 2));
    try {
        std::vector<double> s(6 * (size_t)n, 0.0);
        tsne_split(Y, n, s.data(), s.data() + n);
        if (uY) tsne_split(uY, n, s.data() + 2 * n, s.data() + 3 * n);
        if (gains) tsne_split(gains, n, s.data() + 4 * n, s.data() + 5 * n);
        else std::fill(s.begin() + 4 * n, s.end(), 1.0);
        if (int rc = tsne_use(t)) return rc;
        HIPCHECK(hipStreamSynchronize(t->stream));
        HIPCHECK(hipMemcpy(t->state, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory");
    }
    t->has_state = true;
    return VBNMF_OK;
}

int vbnmf_tsne_get_state(vbnmf_tsne *t, double *Y, double *uY, double *gains)
{
    if (int rc = tsne_use(t)) return rc;
    if (!t->has_state) return fail(VBNMF_ERR_STATE, "the handle has no state yet: call vbnmf_tsne_set_state");
    const int64_t n = t->n;
    try {
        std::vector<double> s(6 * (size_t)n);
        HIPCHECK(hipStreamSynchronize(t->stream));
        HIPCHECK(hipMemcpy(s.data(), t->state, s.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (Y) tsne_join(s.data(), s.data() + n, n, Y);
        if (uY) tsne_join(s.data() + 2 * n, s.data() + 3 * n, n, uY);
        if (gains) tsne_join(s.data() + 4 * n, s.data() + 5 * n, n, gains);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory");
    }
    return VBNMF_OK;
}

int vbnmf_tsne_forces(vbnmf_tsne *t, double exaggeration, double *A, double *R, double *z, double *cost_i)
{
    if (!t) return fail(VBNMF_ERR_BAD_ARG, "NULL t-SNE handle");
    if (!std::isfinite(exaggeration)) return fail(VBNMF_ERR_BAD_ARG, "the exaggeration is not finite");
    if (int rc = tsne_use(t)) return rc;
    if (!t->has_state) return fail(VBNMF_ERR_STATE, "the handle has no state yet: call vbnmf_tsne_set_state");
    const int64_t n = t->n;
    if (int rc = tsne_costs_reserve(t, 1)) return rc;
    if (int rc = tsne_launch_force(t, 1)) return rc;
    if (int rc = tsne_launch_update(t, 0, 1, 1.0, 0.0, 0.0, 0.0, t->costs)) return rc;
    HIPCHECK(hipStreamSynchronize(t->stream));
    try {
        std::vector<double> s(5 * (size_t)n);
        HIPCHECK(hipMemcpy(s.data(), t->sums, s.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (A) {
            tsne_join(s.data(), s.data() + n, n, A);
            for (int64_t q = 0; q < 2 * n; q++) A[q] = exaggeration * A[q];
        }
        if (R) tsne_join(s.data() + 2 * n, s.data() + 3 * n, n, R);
        if (z) std::copy(s.begin() + 4 * n, s.end(), z);
        if (cost_i) HIPCHECK(hipMemcpy(cost_i, t->cost_i, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory");
    }
    return VBNMF_OK;
}

int vbnmf_tsne_run(vbnmf_tsne *t, int32_t first_iter, int32_t n_iter, double exaggeration, int32_t stop_lying_iter,
                   int32_t mom_switch_iter, double momentum, double final_momentum, double eta, double min_gain, int32_t cost_every,
                   double *itercosts, int32_t *cost_iters, int32_t *n_costs)
{
    if (!t || !itercosts || !cost_iters || !n_costs) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *n_costs = 0;
    if (first_iter < 1 || n_iter < 0 || (int64_t)first_iter + n_iter > 2147483647ll)
        return fail(VBNMF_ERR_BAD_ARG, "iterations %d .. %d + %d are outside [1, 2^31)", first_iter, first_iter, n_iter);
    if (!std::isfinite(exaggeration) || !std::isfinite(momentum) || !std::isfinite(final_momentum) || !std::isfinite(eta) || !std::isfinite(min_gain))
        return fail(VBNMF_ERR_BAD_ARG, "a schedule value is not finite");
    if (int rc = tsne_use(t)) return rc;
    if (!t->has_state) return fail(VBNMF_ERR_STATE, "the handle has no state yet: call vbnmf_tsne_set_state");
    if (n_iter == 0) return VBNMF_OK;
    const int32_t last = first_iter + n_iter - 1;
    auto due = [&](int32_t it) { return it == last || (cost_every > 0 && it % cost_every == 0); };
    int32_t count = 0;
    for (int32_t it = first_iter; it <= last; it++) count += due(it) ? 1 : 0;
    if (int rc = tsne_costs_reserve(t, count)) return rc;
    HIPCHECK(hipEventRecord(t->ev0, t->stream));
    int32_t slot = 0;
    for (int32_t it = first_iter; it <= last; it++) {
        // the cost of the Y that iteration it - 1 left is formed by this iteration's force launch
        const int cost = it > first_iter && due(it - 1) ? 1 : 0;
        const double e = it <= stop_lying_iter ? exaggeration : 1.0, m = it <= mom_switch_iter ? momentum : final_momentum;
        if (it == last) HIPCHECK(hipEventRecord(t->ev2, t->stream));            // the last iteration's two launches, each by itself
        if (int rc = tsne_launch_force(t, cost)) return rc;
        if (it == last) HIPCHECK(hipEventRecord(t->ev3, t->stream));
        if (int rc = tsne_launch_update(t, 1, cost, e, m, eta, min_gain, t->costs + slot)) return rc;
        if (it == last) HIPCHECK(hipEventRecord(t->ev1, t->stream));
        if (cost) cost_iters[slot++] = it - 1;
    }
    if (int rc = tsne_launch_force(t, 1)) return rc;
    if (int rc = tsne_launch_update(t, 0, 1, 1.0, 0.0, 0.0, 0.0, t->costs + slot)) return rc;
    cost_iters[slot++] = last;
    HIPCHECK(hipStreamSynchronize(t->stream));
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, t->ev0, t->ev1));                         // the iterations, without the closing cost evaluation
    t->times_ms[3] = ms;
    HIPCHECK(hipEventElapsedTime(&ms, t->ev2, t->ev3));
    t->times_ms[5] = ms;
    HIPCHECK(hipEventElapsedTime(&ms, t->ev3, t->ev1));
    t->times_ms[6] = ms;
    const auto t0 = host_clock::now();
    HIPCHECK(hipMemcpy(itercosts, t->costs, (size_t)slot * sizeof(double), hipMemcpyDeviceToHost));
    t->times_ms[4] = ms_since(t0);
    *n_costs = slot;
    return VBNMF_OK;
}

int vbnmf_tsne_info(vbnmf_tsne *t, int32_t *ints, double *times_ms)
{
    if (ints) {
        const int32_t v[8] = {kTsneWave, kTsneThreads, kTsneIBlock, kTsneJTile, kTsneLdsRow, t ? t->aff_grid : 0, t ? t->force_grid : 0, kTsneUpdThreads};
        for (int k = 0; k < 8; k++) ints[k] = v[k];
    }
    if (times_ms)
        for (int k = 0; k < 7; k++) times_ms[k] = t ? t->times_ms[k] : (k < 3 ? tl_tsne_create_ms[k] : 0.0);
    return VBNMF_OK;
}

}  // extern "C"
