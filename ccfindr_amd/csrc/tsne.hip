// tsne.hip -- the t-SNE map behind visualize_clusters (tsne.h): arguments are checked and x is normalised on the host, the
// affinities are one launch at creation, an iteration of the descent is a force launch and an update launch on the handle's
// stream.  The handle lives across calls and regrows one of its buffers (tsne_costs_reserve), so it frees what it owns in
// vbnmf_tsne_destroy and not through a DeviceCall.
// A neighbour handle (vbnmf_tsne_create_knn, tsne_knn.h) is the same handle: its creation is the search with the
// bisection in one launch and the sparse P's pattern built here on the host; its force stage is two launches.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "device.h"
#include "tsne.h"
#include "tsne_knn.h"

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
    // a neighbour handle's (K > 0)
    int32_t K = 0;
    hipEvent_t ev4 = nullptr;
    int32_t *nb_idx = nullptr;     // [n][K]
    double *nb_dist = nullptr;     // [n][K]
    double *pcond = nullptr;       // [n][K] p_{j|i}
    int64_t *indptr = nullptr;     // [n + 1]
    int32_t *indices = nullptr;    // [nnz]
    double *values = nullptr;      // [nnz]
    std::vector<int64_t> h_indptr;
    int64_t nnz = 0, max_row = 0;
    int att_grid = 0;
    double knn_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // search, pattern, last attract, last repulse, last update
};

namespace {

thread_local double tl_tsne_create_ms[3] = {0.0, 0.0, 0.0};

int tsne_use(vbnmf_tsne *t)
{
    if (!t) return fail(VBNMF_ERR_BAD_ARG, "NULL t-SNE handle");
    HIPCHECK(hipSetDevice(t->device));
    return VBNMF_OK;
}

// the force stage of a neighbour handle: the sparse rows, then all pairs of Y; `mid` (if given) is recorded between the two
int tsne_launch_force_knn(vbnmf_tsne *t, int cost, hipEvent_t mid)
{
    const int64_t n = t->n;
    TsneAttArgs a;
    a.n = t->n; a.cost = cost; a.indptr = t->indptr; a.indices = t->indices; a.values = t->values;
    a.y0 = t->state; a.y1 = t->state + n; a.sums = t->sums;
    hipLaunchKernelGGL(k_tsne_attract, dim3((unsigned)t->att_grid), dim3(kTsneThreads), 0, t->stream, a);
    HIPCHECK(hipGetLastError());
    if (mid) HIPCHECK(hipEventRecord(mid, t->stream));
    TsneRepArgs r;
    r.n = t->n; r.y0 = t->state; r.y1 = t->state + n; r.sums = t->sums;
    hipLaunchKernelGGL(k_tsne_repulse, dim3((unsigned)t->force_grid), dim3(kTsneThreads), 0, t->stream, r);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int tsne_launch_force(vbnmf_tsne *t, int cost, hipEvent_t mid = nullptr)
{
    if (t->K > 0) return tsne_launch_force_knn(t, cost, mid);
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

thread_local double tl_knn_search_ms = 0.0;

// k_tsne_knn over the handle's xt into nb_idx, nb_dist (and, with `affinity`, beta, sum_p, inv_s, trips, pcond); waits for it
int tsne_knn_search(vbnmf_tsne *t, int cus, int affinity, double log_u)
{
    const int64_t n = t->n;
    t->aff_grid = (int)std::min<int64_t>(n, (int64_t)cus * 4);
    double *scratch = nullptr;
    if (n > kTsneLdsRow) { if (int rc = dev_alloc(&scratch, (size_t)t->aff_grid * (size_t)n)) return rc; }
    TsneKnnArgs a;
    a.n = t->n; a.d = t->d; a.K = t->K; a.affinity = affinity; a.xt = t->xt; a.scratch = scratch; a.log_u = log_u;
    a.idx = t->nb_idx; a.dist = t->nb_dist; a.beta = t->beta; a.sum_p = t->sum_p; a.inv_s = t->inv_s; a.trips = t->trips; a.pcond = t->pcond;
    hipError_t err = hipEventRecord(t->ev0, t->stream);
    hipLaunchKernelGGL(k_tsne_knn, dim3((unsigned)t->aff_grid), dim3(kTsneThreads), 0, t->stream, a);
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipEventRecord(t->ev1, t->stream);
    const hipError_t serr = hipStreamSynchronize(t->stream);                  // scratch is free after this whatever happened
    dev_free(scratch);
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) return fail(VBNMF_ERR_HIP, "the neighbour search: %s", hipGetErrorString(err));
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, t->ev0, t->ev1));
    t->knn_ms[0] = tl_knn_search_ms = ms;
    return VBNMF_OK;
}

// The sparse P from the lists and their p_{j|i}: the pattern {(i, j): j in N_i or i in N_j}, rows with ascending j, the value
// (p_{j|i} + p_{i|j}) * 1/(2n) as k_tsne_force forms it (an absent half is 0; the sum commutes, so P_ij and P_ji have the same
// bits).  Index arithmetic only, sequential: the reverse lists by a counting sort over ascending i, each forward list sorted
// by j, the two merged.  The result is a function of the lists alone.
int tsne_knn_pattern(vbnmf_tsne *t)
{
    const int64_t n = t->n;
    const int K = t->K;
    const auto t0 = host_clock::now();
    try {
        const size_t nk = (size_t)n * (size_t)K;
        std::vector<int32_t> idx(nk);
        std::vector<double> pc(nk);
        HIPCHECK(hipMemcpy(idx.data(), t->nb_idx, nk * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(pc.data(), t->pcond, nk * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<int64_t> rptr((size_t)n + 1, 0);
        for (size_t q = 0; q < nk; q++) {
            if (idx[q] < 0 || idx[q] >= n) return fail(VBNMF_ERR_HIP, "the neighbour search left the index %d at point %lld", idx[q], (long long)(q / K));
            rptr[(size_t)idx[q] + 1]++;                                          // (the attraction kernel gathers y by these)
        }
        for (int64_t j = 0; j < n; j++) rptr[j + 1] += rptr[j];
        std::vector<int32_t> rsrc(nk);
        std::vector<double> rval(nk);
        {
            std::vector<int64_t> fill(rptr.begin(), rptr.end() - 1);
            for (int64_t i = 0; i < n; i++)
                for (int q = 0; q < K; q++) {
                    const int64_t pos = fill[idx[i * K + q]]++;
                    rsrc[pos] = (int32_t)i;
                    rval[pos] = pc[i * K + q];
                }
        }
        std::vector<int64_t> indptr((size_t)n + 1, 0);
        std::vector<int32_t> indices;
        std::vector<double> values;
        indices.reserve(2 * nk);
        values.reserve(2 * nk);
        std::vector<std::pair<int32_t, double>> fwd((size_t)K);
        const double inv_2n = 1.0 / (2.0 * (double)n);
        int64_t longest = 0;
        for (int64_t i = 0; i < n; i++) {
            for (int q = 0; q < K; q++) fwd[q] = {idx[i * K + q], pc[i * K + q]};
            std::sort(fwd.begin(), fwd.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) { return a.first < b.first; });
            int a = 0;
            int64_t b = rptr[i];
            const int64_t be = rptr[i + 1];
            while (a < K || b < be) {
                const int32_t ja = a < K ? fwd[a].first : INT32_MAX, jb = b < be ? rsrc[b] : INT32_MAX;
                const int32_t j = std::min(ja, jb);
                const double pij = ja == j ? fwd[a++].second : 0.0;
                const double pji = jb == j ? rval[b++] : 0.0;
                indices.push_back(j);
                values.push_back((pij + pji) * inv_2n);
            }
            indptr[i + 1] = (int64_t)indices.size();
            longest = std::max(longest, indptr[i + 1] - indptr[i]);
        }
        if (int rc = dev_upload(&t->indptr, indptr)) return rc;
        if (int rc = dev_upload(&t->indices, indices)) return rc;
        if (int rc = dev_upload(&t->values, values)) return rc;
        t->nnz = (int64_t)indices.size();
        t->max_row = longest;
        t->h_indptr.swap(indptr);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the pattern of %lld x %d neighbours", (long long)n, K);
    }
    dev_free(t->pcond);                                                        // P holds them now
    t->pcond = nullptr;
    t->att_grid = (int)((n + kTsneAttRows - 1) / kTsneAttRows);
    t->knn_ms[1] = ms_since(t0);
    return VBNMF_OK;
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
    if (t->K > 0) {
        HIPCHECK(hipEventCreate(&t->ev4));
        const size_t nk = (size_t)n * (size_t)t->K;
        if ((rc = dev_alloc(&t->nb_idx, nk)) || (rc = dev_alloc(&t->nb_dist, nk)) || (rc = dev_alloc(&t->pcond, nk))) return rc;
        hipError_t uerr = hipMemcpy(t->xt, xt.data(), (size_t)n * d * sizeof(double), hipMemcpyHostToDevice);
        tl_tsne_create_ms[1] = ms_since(t0);
        if (uerr != hipSuccess) return fail(VBNMF_ERR_HIP, "vbnmf_tsne_create_knn: %s", hipGetErrorString(uerr));
        if ((rc = tsne_knn_search(t, cus, 1, std::log(perplexity)))) return rc;
        if ((rc = tsne_knn_pattern(t))) return rc;
        tl_tsne_create_ms[2] = t->knn_ms[0];
        for (int k = 0; k < 3; k++) t->times_ms[k] = tl_tsne_create_ms[k];
        return VBNMF_OK;
    }
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

// neighbors < 0: the dense handle; 0: floor(3 perplexity) neighbours; else that many
static int tsne_create_any(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, int32_t neighbors,
                           vbnmf_tsne **handle)
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
    int32_t K = 0;
    if (neighbors >= 0) {
        const double want = neighbors > 0 ? (double)neighbors : std::floor(3.0 * perplexity);
        if (want > (double)kTsneKnnMax) return fail(VBNMF_ERR_BAD_ARG, "%.0f neighbours are more than the kernel's limit of %d", want, kTsneKnnMax);
        K = (int32_t)want;
        if (K < 1 || (int64_t)K > n - 1) return fail(VBNMF_ERR_BAD_ARG, "%d neighbours are outside [1, n - 1 = %lld]", K, (long long)(n - 1));
        if (!(perplexity < (double)K))
            return fail(VBNMF_ERR_BAD_ARG, "the perplexity %g needs more than %d neighbours: %d outcomes cannot carry its entropy", perplexity, K, K);
    }
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
        t->n = (int32_t)n; t->d = d; t->K = K;
        if (int rc = tsne_create(t.get(), device, xt, perplexity)) return rc;
        *handle = t.release();
        return VBNMF_OK;
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for %lld x %d points", (long long)n, d);
    }
}

int vbnmf_tsne_create(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, vbnmf_tsne **handle)
{
    return tsne_create_any(device, n, d, x, perplexity, normalize, -1, handle);
}

int vbnmf_tsne_create_knn(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, int32_t neighbors,
                          vbnmf_tsne **handle)
{
    if (neighbors < 0) {
        if (handle) *handle = nullptr;
        return fail(VBNMF_ERR_BAD_ARG, "neighbors = %d is negative", neighbors);
    }
    return tsne_create_any(device, n, d, x, perplexity, normalize, neighbors, handle);
}

int vbnmf_knn(int32_t device, int64_t n, int32_t d, const double *x, int32_t k, int32_t *idx, double *dist)
{
    if (!x || !idx || !dist) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (n < 2 || n > 2147481600ll) return fail(VBNMF_ERR_BAD_ARG, "n = %lld points is outside [2, 2^31 - 2048]", (long long)n);
    if (d < 1 || d > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "d = %d is outside [1, %d]", d, VBNMF_MAX_RANK);
    if (k < 1 || (int64_t)k > n - 1) return fail(VBNMF_ERR_BAD_ARG, "k = %d neighbours are outside [1, n - 1 = %lld]", k, (long long)(n - 1));
    if (k > kTsneKnnMax) return fail(VBNMF_ERR_BAD_ARG, "k = %d neighbours are more than the kernel's limit of %d", k, kTsneKnnMax);
    try {
        for (int64_t q = 0; q < n * d; q++)
            if (!std::isfinite(x[q])) return fail(VBNMF_ERR_BAD_ARG, "x[%lld, %lld] is not finite", (long long)(q / d), (long long)(q % d));
        std::vector<double> xt((size_t)n * d);
        for (int64_t i = 0; i < n; i++)
            for (int c = 0; c < d; c++) xt[(size_t)c * n + i] = x[i * d + c];
        if (int rc = check_device(device)) return rc;
        std::unique_ptr<vbnmf_tsne, void (*)(vbnmf_tsne *)> t(new vbnmf_tsne(), vbnmf_tsne_destroy);      // the search's buffers only
        t->n = (int32_t)n; t->d = d; t->K = k; t->device = device;
        HIPCHECK(hipSetDevice(device));
        int cus = 0;
        if (int rc = device_cus(device, cus)) return rc;
        HIPCHECK(hipStreamCreate(&t->stream));
        HIPCHECK(hipEventCreate(&t->ev0));
        HIPCHECK(hipEventCreate(&t->ev1));
        const size_t nk = (size_t)n * (size_t)k;
        int rc;
        if ((rc = dev_upload(&t->xt, xt)) || (rc = dev_alloc(&t->nb_idx, nk)) || (rc = dev_alloc(&t->nb_dist, nk))) return rc;
        if ((rc = tsne_knn_search(t.get(), cus, 0, 0.0))) return rc;
        HIPCHECK(hipMemcpy(idx, t->nb_idx, nk * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(dist, t->nb_dist, nk * sizeof(double), hipMemcpyDeviceToHost));
        return VBNMF_OK;
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for %lld x %d points", (long long)n, d);
    }
}

int vbnmf_tsne_neighbors(vbnmf_tsne *t, int32_t *idx, double *dist)
{
    if (int rc = tsne_use(t)) return rc;
    if (t->K <= 0) return fail(VBNMF_ERR_STATE, "a dense handle has no neighbour lists: create it with vbnmf_tsne_create_knn");
    const size_t nk = (size_t)t->n * (size_t)t->K;
    if (idx) HIPCHECK(hipMemcpy(idx, t->nb_idx, nk * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (dist) HIPCHECK(hipMemcpy(dist, t->nb_dist, nk * sizeof(double), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

int vbnmf_tsne_sparse_p(vbnmf_tsne *t, int64_t *nnz, int64_t *indptr, int32_t *indices, double *values)
{
    if (int rc = tsne_use(t)) return rc;
    if (t->K <= 0) return fail(VBNMF_ERR_STATE, "a dense handle stores no P: create it with vbnmf_tsne_create_knn");
    if (nnz) *nnz = t->nnz;
    if (indptr) std::copy(t->h_indptr.begin(), t->h_indptr.end(), indptr);
    if (indices) HIPCHECK(hipMemcpy(indices, t->indices, (size_t)t->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (indices && values) HIPCHECK(hipMemcpy(values, t->values, (size_t)t->nnz * sizeof(double), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

int vbnmf_tsne_knn_info(vbnmf_tsne *t, int64_t *ints, double *times_ms)
{
    if (ints) {
        const int64_t v[10] = {kTsneKnnMax, kTsneThreads, kTsneLdsRow, kTsneRepTile, kTsneIBlock, kTsneAttRows, t ? t->K : 0, t ? t->nnz : 0,
                               t ? t->max_row : 0, t ? t->att_grid : 0};
        for (int k = 0; k < 10; k++) ints[k] = v[k];
    }
    if (times_ms)
        for (int k = 0; k < 5; k++) times_ms[k] = t ? t->knn_ms[k] : (k == 0 ? tl_knn_search_ms : 0.0);
    return VBNMF_OK;
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
    dev_free(t->nb_idx); dev_free(t->nb_dist); dev_free(t->pcond); dev_free(t->indptr); dev_free(t->indices); dev_free(t->values);
    if (t->ev4) (void)hipEventDestroy(t->ev4);
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
        if (int rc = tsne_launch_force(t, cost, it == last ? t->ev4 : nullptr)) return rc;      // (ev4: a neighbour handle's, between its two launches)
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
    if (t->K > 0) {
        t->knn_ms[4] = ms;
        HIPCHECK(hipEventElapsedTime(&ms, t->ev2, t->ev4));
        t->knn_ms[2] = ms;
        HIPCHECK(hipEventElapsedTime(&ms, t->ev4, t->ev3));
        t->knn_ms[3] = ms;
    }
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
