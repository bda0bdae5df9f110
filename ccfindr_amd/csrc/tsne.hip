// tsne.hip -- the t-SNE map behind visualize_clusters (tsne.h): arguments are checked and x is normalised on the host, the
// affinities are one launch at creation, an iteration of the descent is a force launch and an update launch on the handle's
// stream.  The handle lives across calls and regrows one of its buffers (tsne_costs_reserve), so it frees what it owns in
// vbnmf_tsne_destroy and not through a DeviceCall.
// A neighbour handle (vbnmf_tsne_create_knn, tsne_knn.h) is the same handle: its creation is the search with the
// bisection in one launch and the sparse P's pattern built here on the host; its force stage is two launches.
// Both kinds and vbnmf_knn share one preparation of the points (tsne_points), one opening of a handle (tsne_open) and one
// launcher of the two row kernels (tsne_row_kernel); the slots of the two *_info calls are named by the enums below.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "device.h"
#include "tsne.h"
#include "tsne_knn.h"

using namespace vbnmf;

// The slots of what vbnmf_tsne_info and vbnmf_tsne_knn_info hand out, in the order include/vbnmf.h states them.
enum TsneInfoSlot : int { kInfoWave, kInfoThreads, kInfoIBlock, kInfoJTile, kInfoLdsRow, kInfoAffGrid, kInfoForceGrid, kInfoUpdThreads };
enum TsneTimeSlot : int { kTimeNormalise, kTimeUpload, kTimeAffinities, kTimeLoop, kTimeReadBack, kTimeLastForce, kTimeLastUpdate, kTsneTimeSlots };
constexpr int kTsneCreateTimes = kTimeAffinities + 1;                         // the create's part of them
enum TsneKnnInfoSlot : int { kKnnInfoLimit, kKnnInfoThreads, kKnnInfoLdsRow, kKnnInfoRepTile, kKnnInfoIBlock, kKnnInfoAttRows, kKnnInfoK, kKnnInfoNnz,
                             kKnnInfoLongest, kKnnInfoAttGrid };
enum TsneKnnTimeSlot : int { kKnnTimeSearch, kKnnTimePattern, kKnnTimeAttract, kKnnTimeRepulse, kKnnTimeUpdate, kTsneKnnTimeSlots };
// The handle's events: around a row kernel or a run's iterations; of a run's last iteration, in front of its force stage, between
// that stage's two launches (a neighbour handle's) and behind it.
enum TsneEvent : int { kEvBegin, kEvEnd, kEvLast, kEvLastMid, kEvLastForce, kTsneEvents };

struct vbnmf_tsne {
    int device = 0, cus = 0;
    int32_t n = 0, d = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[kTsneEvents] = {};
    double *xt = nullptr, *beta = nullptr, *sum_p = nullptr, *inv_s = nullptr;
    int32_t *trips = nullptr;
    double *state = nullptr;       // [6][n]: y0 y1 u0 u1 g0 g1
    double *sums = nullptr;        // [kTsneForceSums][n]
    double *cost_i = nullptr;      // [n]
    double *costs = nullptr;       // [costs_cap] the run's cost values
    int64_t costs_cap = 0;
    int aff_grid = 0, force_grid = 0;
    bool has_state = false;
    double times_ms[kTsneTimeSlots] = {};
    // a neighbour handle's (K > 0)
    int32_t K = 0;
    int32_t *nb_idx = nullptr;     // [n][K]
    double *nb_dist = nullptr;     // [n][K]
    double *pcond = nullptr;       // [n][K] p_{j|i}
    int64_t *indptr = nullptr;     // [n + 1]
    int32_t *indices = nullptr;    // [nnz]
    double *values = nullptr;      // [nnz]
    std::vector<int64_t> h_indptr;
    int64_t nnz = 0, max_row = 0;
    int att_grid = 0;
    double knn_ms[kTsneKnnTimeSlots] = {};
};

namespace {

thread_local double tl_tsne_create_ms[kTsneCreateTimes] = {};
thread_local double tl_knn_search_ms = 0.0;

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

int tsne_elapsed(vbnmf_tsne *t, TsneEvent from, TsneEvent to, double *ms)
{
    float f = 0.0f;
    HIPCHECK(hipEventElapsedTime(&f, t->ev[from], t->ev[to]));
    *ms = f;
    return VBNMF_OK;
}

// The device, its stream and events for a new handle.
int tsne_open(vbnmf_tsne *t, int32_t device)
{
    t->device = device;
    HIPCHECK(hipSetDevice(device));
    if (int rc = device_cus(device, t->cus)) return rc;
    HIPCHECK(hipStreamCreate(&t->stream));
    for (hipEvent_t &e : t->ev) HIPCHECK(hipEventCreate(&e));
    return VBNMF_OK;
}

// A row kernel (k_tsne_affinity, k_tsne_knn: one workgroup per point, in grid strides, a row of D each) over the handle's
// points: launch(grid, scratch) queues it on the stream, `scratch` being the workgroups' rows where LDS does not hold one;
// waits for it and leaves its device time in *ms.  `what` names the call in an error.
template <class Launch>
int tsne_row_kernel(vbnmf_tsne *t, const char *what, double *ms, Launch launch)
{
    const int64_t n = t->n;
    t->aff_grid = (int)std::min<int64_t>(n, (int64_t)t->cus * 4);
    double *scratch = nullptr;
    if (n > kTsneLdsRow) { if (int rc = dev_alloc(&scratch, (size_t)t->aff_grid * (size_t)n)) return rc; }
    hipError_t err = hipEventRecord(t->ev[kEvBegin], t->stream);
    launch(dim3((unsigned)t->aff_grid), scratch);
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipEventRecord(t->ev[kEvEnd], t->stream);
    const hipError_t serr = hipStreamSynchronize(t->stream);                  // scratch is free after this whatever happened
    dev_free(scratch);
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) return fail(VBNMF_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    return tsne_elapsed(t, kEvBegin, kEvEnd, ms);
}

// k_tsne_knn over the handle's xt into nb_idx, nb_dist (and, with `affinity`, beta, sum_p, inv_s, trips, pcond); waits for it
int tsne_knn_search(vbnmf_tsne *t, int affinity, double log_u)
{
    if (int rc = tsne_row_kernel(t, "the neighbour search", &t->knn_ms[kKnnTimeSearch], [&](dim3 grid, double *scratch) {
            TsneKnnArgs a;
            a.n = t->n; a.d = t->d; a.K = t->K; a.affinity = affinity; a.xt = t->xt; a.scratch = scratch; a.log_u = log_u;
            a.idx = t->nb_idx; a.dist = t->nb_dist; a.beta = t->beta; a.sum_p = t->sum_p; a.inv_s = t->inv_s; a.trips = t->trips; a.pcond = t->pcond;
            hipLaunchKernelGGL(k_tsne_knn, grid, dim3(kTsneThreads), 0, t->stream, a);
        }))
        return rc;
    tl_knn_search_ms = t->knn_ms[kKnnTimeSearch];
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
    t->knn_ms[kKnnTimePattern] = ms_since(t0);
    return VBNMF_OK;
}

// x, checked to be finite, as the device keeps it: xt[d][n]; the normalisation runs on that in a fixed order: column means,
// then the largest |value|
int tsne_points(int64_t n, int d, const double *x, int normalize, std::vector<double> &xt)
{
    for (int64_t q = 0; q < n * d; q++)
        if (!std::isfinite(x[q])) return fail(VBNMF_ERR_BAD_ARG, "x[%lld, %lld] is not finite", (long long)(q / d), (long long)(q % d));
    xt.resize((size_t)n * d);
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < d; k++) xt[(size_t)k * n + i] = x[i * d + k];
    if (!normalize) return VBNMF_OK;
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
    return VBNMF_OK;
}

int tsne_check_shape(int64_t n, int32_t d, int min_n)
{
    if (n < min_n || n > 2147481600ll)                                           // (int loop counters step by <= 1024)
        return fail(VBNMF_ERR_BAD_ARG, "n = %lld points is outside [%d, 2^31 - 2048]", (long long)n, min_n);
    if (d < 1 || d > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "d = %d is outside [1, %d]", d, VBNMF_MAX_RANK);
    return VBNMF_OK;
}

// open, allocate, upload, then the affinities: k_tsne_affinity, or the search with the bisection and the pattern
int tsne_create(vbnmf_tsne *t, int32_t device, const std::vector<double> &xt, double perplexity)
{
    const int64_t n = t->n;
    const size_t nk = (size_t)n * (size_t)t->K;
    const char *name = t->K > 0 ? "vbnmf_tsne_create_knn" : "vbnmf_tsne_create";
    const auto t0 = host_clock::now();
    int rc;
    if ((rc = tsne_open(t, device)) || (rc = dev_alloc(&t->xt, xt.size())) || (rc = dev_alloc(&t->beta, (size_t)n)) || (rc = dev_alloc(&t->sum_p, (size_t)n)) ||
        (rc = dev_alloc(&t->inv_s, (size_t)n)) || (rc = dev_alloc(&t->trips, (size_t)n)) || (rc = dev_alloc(&t->state, 6 * (size_t)n)) ||
        (rc = dev_alloc(&t->sums, (size_t)kTsneForceSums * n)) || (rc = dev_alloc(&t->cost_i, (size_t)n)))
        return rc;
    if (t->K > 0 && ((rc = dev_alloc(&t->nb_idx, nk)) || (rc = dev_alloc(&t->nb_dist, nk)) || (rc = dev_alloc(&t->pcond, nk)))) return rc;
    t->force_grid = (int)((n + kTsneIBlock - 1) / kTsneIBlock);
    const hipError_t uerr = hipMemcpy(t->xt, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice);
    tl_tsne_create_ms[kTimeUpload] = ms_since(t0);
    if (uerr != hipSuccess) return fail(VBNMF_ERR_HIP, "%s: %s", name, hipGetErrorString(uerr));
    const double log_u = std::log(perplexity);
    if (t->K > 0) {
        if ((rc = tsne_knn_search(t, 1, log_u)) || (rc = tsne_knn_pattern(t))) return rc;
        tl_tsne_create_ms[kTimeAffinities] = t->knn_ms[kKnnTimeSearch];
    } else {
        rc = tsne_row_kernel(t, name, &tl_tsne_create_ms[kTimeAffinities], [&](dim3 grid, double *scratch) {
            TsneAffArgs a;
            a.n = t->n; a.d = t->d; a.xt = t->xt; a.scratch = scratch; a.log_u = log_u;
            a.beta = t->beta; a.sum_p = t->sum_p; a.inv_s = t->inv_s; a.trips = t->trips;
            hipLaunchKernelGGL(k_tsne_affinity, grid, dim3(kTsneThreads), 0, t->stream, a);
        });
        if (rc) return rc;
    }
    for (int k = 0; k < kTsneCreateTimes; k++) t->times_ms[k] = tl_tsne_create_ms[k];
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
    if (int rc = tsne_check_shape(n, d, 1)) return rc;
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
        std::vector<double> xt;
        if (int rc = tsne_points(n, d, x, normalize, xt)) return rc;
        tl_tsne_create_ms[kTimeNormalise] = ms_since(t0);
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
    if (int rc = tsne_check_shape(n, d, 2)) return rc;
    if (k < 1 || (int64_t)k > n - 1) return fail(VBNMF_ERR_BAD_ARG, "k = %d neighbours are outside [1, n - 1 = %lld]", k, (long long)(n - 1));
    if (k > kTsneKnnMax) return fail(VBNMF_ERR_BAD_ARG, "k = %d neighbours are more than the kernel's limit of %d", k, kTsneKnnMax);
    try {
        std::vector<double> xt;
        int rc;
        if ((rc = tsne_points(n, d, x, 0, xt)) || (rc = check_device(device))) return rc;
        std::unique_ptr<vbnmf_tsne, void (*)(vbnmf_tsne *)> t(new vbnmf_tsne(), vbnmf_tsne_destroy);      // the search's buffers only
        t->n = (int32_t)n; t->d = d; t->K = k;
        const size_t nk = (size_t)n * (size_t)k;
        if ((rc = tsne_open(t.get(), device)) || (rc = dev_upload(&t->xt, xt)) || (rc = dev_alloc(&t->nb_idx, nk)) ||
            (rc = dev_alloc(&t->nb_dist, nk)) || (rc = tsne_knn_search(t.get(), 0, 0.0)))
            return rc;
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
        ints[kKnnInfoLimit] = kTsneKnnMax; ints[kKnnInfoThreads] = kTsneThreads; ints[kKnnInfoLdsRow] = kTsneLdsRow;
        ints[kKnnInfoRepTile] = kTsneRepTile; ints[kKnnInfoIBlock] = kTsneIBlock; ints[kKnnInfoAttRows] = kTsneAttRows;
        ints[kKnnInfoK] = t ? t->K : 0; ints[kKnnInfoNnz] = t ? t->nnz : 0; ints[kKnnInfoLongest] = t ? t->max_row : 0;
        ints[kKnnInfoAttGrid] = t ? t->att_grid : 0;
    }
    if (times_ms)
        for (int k = 0; k < kTsneKnnTimeSlots; k++) times_ms[k] = t ? t->knn_ms[k] : (k == kKnnTimeSearch ? tl_knn_search_ms : 0.0);
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
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
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
    HIPCHECK(hipEventRecord(t->ev[kEvBegin], t->stream));
    int32_t slot = 0;
    for (int32_t it = first_iter; it <= last; it++) {
        // the cost of the Y that iteration it - 1 left is formed by this iteration's force launch
        const int cost = it > first_iter && due(it - 1) ? 1 : 0;
        const double e = it <= stop_lying_iter ? exaggeration : 1.0, m = it <= mom_switch_iter ? momentum : final_momentum;
        if (it == last) HIPCHECK(hipEventRecord(t->ev[kEvLast], t->stream));    // the last iteration's two launches, each by itself
        if (int rc = tsne_launch_force(t, cost, it == last ? t->ev[kEvLastMid] : nullptr)) return rc;
        if (it == last) HIPCHECK(hipEventRecord(t->ev[kEvLastForce], t->stream));
        if (int rc = tsne_launch_update(t, 1, cost, e, m, eta, min_gain, t->costs + slot)) return rc;
        if (it == last) HIPCHECK(hipEventRecord(t->ev[kEvEnd], t->stream));
        if (cost) cost_iters[slot++] = it - 1;
    }
    if (int rc = tsne_launch_force(t, 1)) return rc;
    if (int rc = tsne_launch_update(t, 0, 1, 1.0, 0.0, 0.0, 0.0, t->costs + slot)) return rc;
    cost_iters[slot++] = last;
    HIPCHECK(hipStreamSynchronize(t->stream));
    int rc;
    if ((rc = tsne_elapsed(t, kEvBegin, kEvEnd, &t->times_ms[kTimeLoop])) ||       // the iterations, without the closing cost evaluation
        (rc = tsne_elapsed(t, kEvLast, kEvLastForce, &t->times_ms[kTimeLastForce])) ||
        (rc = tsne_elapsed(t, kEvLastForce, kEvEnd, &t->times_ms[kTimeLastUpdate])))
        return rc;
    if (t->K > 0) {
        t->knn_ms[kKnnTimeUpdate] = t->times_ms[kTimeLastUpdate];
        if ((rc = tsne_elapsed(t, kEvLast, kEvLastMid, &t->knn_ms[kKnnTimeAttract])) ||
            (rc = tsne_elapsed(t, kEvLastMid, kEvLastForce, &t->knn_ms[kKnnTimeRepulse])))
            return rc;
    }
    const auto t0 = host_clock::now();
    HIPCHECK(hipMemcpy(itercosts, t->costs, (size_t)slot * sizeof(double), hipMemcpyDeviceToHost));
    t->times_ms[kTimeReadBack] = ms_since(t0);
    *n_costs = slot;
    return VBNMF_OK;
}

int vbnmf_tsne_info(vbnmf_tsne *t, int32_t *ints, double *times_ms)
{
    if (ints) {
        ints[kInfoWave] = kTsneWave; ints[kInfoThreads] = kTsneThreads; ints[kInfoIBlock] = kTsneIBlock; ints[kInfoJTile] = kTsneJTile;
        ints[kInfoLdsRow] = kTsneLdsRow; ints[kInfoAffGrid] = t ? t->aff_grid : 0; ints[kInfoForceGrid] = t ? t->force_grid : 0;
        ints[kInfoUpdThreads] = kTsneUpdThreads;
    }
    if (times_ms)
        for (int k = 0; k < kTsneTimeSlots; k++) times_ms[k] = t ? t->times_ms[k] : (k < kTsneCreateTimes ? tl_tsne_create_ms[k] : 0.0);
    return VBNMF_OK;
}

}  // extern "C"
