// gsea.hip -- enrichment scores of assign_celltype's permutation loop (gsea.h): every argument is checked and the permutations
// are inverted on the host, the tables go up once, then one launch of k_gsea_perm per chunk of permutations (the identity
// first: the observed scores come from the same code) and one of k_gsea_count.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <new>

#include "device.h"
#include "gsea.h"

using namespace vbnmf;

namespace {

thread_local double tl_gsea_times_ms[4] = {0.0, 0.0, 0.0, 0.0};   // upload, kernels (device events), read-back, host checks + inversion

constexpr int64_t kGseaChunkBytes = 64ll << 20;                   // permutations of one upload: inverse + permutation rows within this

// permutations of one chunk for a table of N rows; VBNMF_GSEA_CHUNK_PERMS (>= 1) makes it smaller
int64_t gsea_chunk_perms(int64_t N)
{
    int64_t c = kGseaChunkBytes / (8 * std::max<int64_t>(N, 1));
    c = std::max<int64_t>(1, std::min<int64_t>(c, 1 << 20));
    if (const char *s = getenv("VBNMF_GSEA_CHUNK_PERMS")) {
        const long v = atol(s);
        if (v >= 1 && v < c) c = v;
    }
    return c;
}

// what the host derives from the checked arguments
struct GseaHost {
    std::vector<int32_t> M;            // [r x nS]
    std::vector<uint8_t> has_na;       // [r]
    std::unique_ptr<int32_t[]> inv;    // [nperm x N], every entry written by gsea_check
    bool any_na = false;
    int pad = 1;
};

int gsea_check(int64_t N, int32_t r, int32_t nS, const uint8_t *valid, const double *wp, const int64_t *hit_ptr, const int32_t *hit_row,
               const uint8_t *hit_is_miss, int64_t nperm, const int32_t *perms, GseaHost &H)
{
    const int64_t nks = (int64_t)r * nS;
    if (hit_ptr[0] != 0) return fail(VBNMF_ERR_BAD_ARG, "hit_ptr must start at 0");
    for (int64_t q = 0; q < nks; q++)
        if (hit_ptr[q + 1] < hit_ptr[q] || hit_ptr[q + 1] - hit_ptr[q] > N)
            return fail(VBNMF_ERR_BAD_ARG, "hit_ptr is not ascending, or a set has more hits than the table has rows (cluster %lld, set %lld)",
                        (long long)(q / nS), (long long)(q % nS));
    if (hit_ptr[nks] > 0 && (!hit_row || !hit_is_miss)) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    H.M.assign((size_t)nks, 0);
    H.has_na.assign((size_t)r, 0);
    int64_t maxT = 0;
    for (int32_t k = 0; k < r; k++) {
        const uint8_t *v = valid + (int64_t)k * N;
        int64_t nvalid = 0;
        for (int64_t i = 0; i < N; i++) nvalid += v[i] != 0;
        // x * gw^p of R/gsea.R:101 is NaN on a row that is no hit when its weight is not finite; the hits' walk would not see it
        for (int64_t i = 0; i < N; i++)
            if (v[i] && !std::isfinite(wp[(int64_t)k * N + i]))
                return fail(VBNMF_ERR_BAD_ARG, "cluster %d, row %lld: the weight gw^p is not finite", k, (long long)i);
        H.has_na[(size_t)k] = nvalid < N ? 1 : 0;
        H.any_na = H.any_na || nvalid < N;
        for (int32_t s = 0; s < nS; s++) {
            const int64_t q = (int64_t)k * nS + s;
            int64_t notmiss = 0, prev = -1;
            for (int64_t h = hit_ptr[q]; h < hit_ptr[q + 1]; h++) {
                const int64_t row = hit_row[h];
                if (row <= prev || row >= N)
                    return fail(VBNMF_ERR_BAD_ARG, "the hit rows of cluster %d, set %d are not ascending within [0, %lld)", k, s, (long long)N);
                if (!v[row]) return fail(VBNMF_ERR_BAD_ARG, "cluster %d, set %d: hit row %lld is an NA row (R/gsea.R:93 drops it before the overlap)", k, s, (long long)row);
                prev = row;
                notmiss += hit_is_miss[h] == 0;
            }
            const int64_t T = hit_ptr[q + 1] - hit_ptr[q], M = nvalid - notmiss;
            H.M[(size_t)q] = (int32_t)M;
            if (T > 0 && M > 0) {
                if (T > kGseaMaxSetHits)
                    return fail(VBNMF_ERR_BAD_ARG, "cluster %d, set %d has %lld hits; at most %d are sorted in LDS (vbnmf_gsea_info)", k, s, (long long)T, kGseaMaxSetHits);
                maxT = std::max(maxT, T);
            }
        }
    }
    while (H.pad < maxT) H.pad <<= 1;
    // the inverse of every permutation; a row that is none is found here
    H.inv.reset(new int32_t[std::max<size_t>((size_t)nperm * (size_t)N, 1)]);       // (not initialised: the workers' pages, below)
    std::atomic<int64_t> bad{-1};
    parallel_for(nperm, [&](int64_t b0, int64_t b1, int) {
        for (int64_t b = b0; b < b1; b++) {
            const int32_t *p = perms + b * N;
            int32_t *iv = H.inv.get() + b * N;
            // N entries inside [0, N) are a permutation iff none repeats; of a repeated row the last position stays in iv, so
            // an earlier one does not read itself back.  Then every entry of iv has been written.
            bool ok = true;
            for (int64_t i = 0; i < N && ok; i++) ok = p[i] >= 0 && p[i] < N;
            if (ok) {
                for (int64_t i = 0; i < N; i++) iv[p[i]] = (int32_t)i;
                for (int64_t i = 0; i < N && ok; i++) ok = iv[p[i]] == (int32_t)i;
            }
            if (!ok) { int64_t none = -1; bad.compare_exchange_strong(none, b); }
        }
    });
    if (bad.load() >= 0) return fail(VBNMF_ERR_BAD_ARG, "row %lld of perms is no permutation of 0 .. %lld", (long long)bad.load(), (long long)N - 1);
    return VBNMF_OK;
}

int gsea_grid(int cus) { return cus * (2048 / kGseaThreads); }

int gsea_run(int32_t device, int64_t N, int32_t r, int32_t nS, const uint8_t *valid, const double *wp, const int64_t *hit_ptr,
             const int32_t *hit_row, const uint8_t *hit_is_miss, int64_t nperm, const int32_t *perms, const GseaHost &H,
             double *es, int64_t *exceed, double *null_es)
{
    const int64_t nks = (int64_t)r * nS, nq = nks, nW = (N + 63) / 64;
    const int64_t chunk = std::min<int64_t>(gsea_chunk_perms(N), std::max<int64_t>(nperm, 1));
    DeviceCall D;
    if (int rc = D.enter(device)) return rc;
    int cus = 0;
    if (int rc = device_cus(device, cus)) return rc;
    const int64_t max_items = std::max<int64_t>(chunk, 1) * r;
    const unsigned grid_max = (unsigned)std::min<int64_t>(max_items, (int64_t)gsea_grid(cus));

    auto t0 = host_clock::now();
    const size_t nhits = (size_t)hit_ptr[nks];
    GseaArgs a;
    a.words = nullptr; a.prefix = nullptr;
    int32_t *d_inv = nullptr, *d_perms = nullptr;                 // one chunk of permutations: inverses, rows
    double *d_es = nullptr, *d_null = nullptr;                    // the observed scores, one chunk of null scores
    long long *d_exceed = nullptr;
    if (int rc = D.upload(&a.valid, valid, (size_t)r * N)) return rc;
    if (int rc = D.upload(&a.wp, wp, (size_t)r * N)) return rc;
    if (int rc = D.upload(&a.has_na, H.has_na.data(), (size_t)r)) return rc;
    if (int rc = D.upload(&a.hit_ptr, hit_ptr, (size_t)nks + 1)) return rc;
    if (int rc = D.upload(&a.hit_row, hit_row, nhits)) return rc;
    if (int rc = D.upload(&a.hit_is_miss, hit_is_miss, nhits)) return rc;
    if (int rc = D.upload(&a.M, H.M.data(), (size_t)nks)) return rc;
    if (int rc = D.alloc(&d_es, (size_t)nq)) return rc;
    if (int rc = D.alloc(&d_exceed, (size_t)nq)) return rc;
    if (nperm > 0) {
        if (int rc = D.alloc(&d_null, (size_t)chunk * nq)) return rc;
        if (int rc = D.alloc(&d_inv, (size_t)chunk * N)) return rc;
        if (H.any_na) { if (int rc = D.alloc(&d_perms, (size_t)chunk * N)) return rc; }
    }
    if (H.any_na) {
        if (int rc = D.alloc(&a.words, (size_t)grid_max * nW)) return rc;
        if (int rc = D.alloc(&a.prefix, (size_t)grid_max * nW)) return rc;
    }
    HIPCHECK(hipMemset(d_exceed, 0, (size_t)nq * sizeof(long long)));
    tl_gsea_times_ms[0] += ms_since(t0);
    a.N = N; a.r = r; a.nS = nS; a.pad = H.pad;
    const size_t lds = (size_t)kGseaLdsFixed + (size_t)kGseaLdsPerHit * (size_t)H.pad;
    float kms = 0.0f;

    // the observed scores: the identity permutation (R/gsea.R:57)
    a.nb = 1; a.inv = nullptr; a.perms = nullptr; a.out = d_es;
    HIPCHECK(hipEventRecord(D.ev0, nullptr));
    D.queued = true;
    hipLaunchKernelGGL(k_gsea_perm, dim3((unsigned)std::min<int64_t>(r, grid_max)), dim3(kGseaThreads), lds, nullptr, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(D.ev1, nullptr));
    HIPCHECK(hipEventSynchronize(D.ev1));
    HIPCHECK(hipEventElapsedTime(&kms, D.ev0, D.ev1));
    tl_gsea_times_ms[1] += kms;

    for (int64_t b0 = 0; b0 < nperm; b0 += chunk) {                                 // R/gsea.R:65-72
        const int64_t nb = std::min(chunk, nperm - b0);
        t0 = host_clock::now();
        HIPCHECK(hipMemcpy(d_inv, H.inv.get() + b0 * N, (size_t)nb * N * sizeof(int32_t), hipMemcpyHostToDevice));
        if (H.any_na) HIPCHECK(hipMemcpy(d_perms, perms + b0 * N, (size_t)nb * N * sizeof(int32_t), hipMemcpyHostToDevice));
        tl_gsea_times_ms[0] += ms_since(t0);
        a.nb = (int32_t)nb; a.inv = d_inv; a.perms = H.any_na ? d_perms : nullptr; a.out = d_null;
        HIPCHECK(hipEventRecord(D.ev0, nullptr));
        hipLaunchKernelGGL(k_gsea_perm, dim3((unsigned)std::min<int64_t>(nb * r, grid_max)), dim3(kGseaThreads), lds, nullptr, a);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(k_gsea_count, dim3((unsigned)((nq + kGseaThreads - 1) / kGseaThreads)), dim3(kGseaThreads), 0, nullptr,
                           d_es, d_null, (int32_t)nb, nq, d_exceed);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(D.ev1, nullptr));
        HIPCHECK(hipEventSynchronize(D.ev1));
        HIPCHECK(hipEventElapsedTime(&kms, D.ev0, D.ev1));
        tl_gsea_times_ms[1] += kms;
        if (null_es) {
            t0 = host_clock::now();
            HIPCHECK(hipMemcpy(null_es + b0 * nq, d_null, (size_t)nb * nq * sizeof(double), hipMemcpyDeviceToHost));
            tl_gsea_times_ms[2] += ms_since(t0);
        }
    }
    t0 = host_clock::now();
    HIPCHECK(hipMemcpy(es, d_es, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(exceed, d_exceed, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost));
    D.queued = false;
    for (int64_t q = 0; q < nq; q++)
        if (es[q] != es[q]) exceed[q] = -1;
    tl_gsea_times_ms[2] += ms_since(t0);
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int vbnmf_gsea_perm(int32_t device, int64_t N, int32_t r, int32_t nS, const uint8_t *valid, const double *wp, const int64_t *hit_ptr,
                    const int32_t *hit_row, const uint8_t *hit_is_miss, int64_t nperm, const int32_t *perms, double *es,
                    int64_t *exceed, double *null_es)
{
    for (double &v : tl_gsea_times_ms) v = 0.0;
    if (N < 1 || N > 2147483584ll) return fail(VBNMF_ERR_BAD_ARG, "N = %lld rows is outside [1, 2^31 - 64]", (long long)N);
    if (r < 1 || r > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", r, VBNMF_MAX_RANK);
    if (nS < 0 || nperm < 0) return fail(VBNMF_ERR_BAD_ARG, "negative number of sets or permutations");
    if (!valid || !wp || !hit_ptr || (nS > 0 && (!es || !exceed)) || (nperm > 0 && !perms)) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    try {
        const auto t0 = host_clock::now();
        GseaHost H;
        if (int rc = gsea_check(N, r, nS, valid, wp, hit_ptr, hit_row, hit_is_miss, nperm, perms, H)) return rc;
        tl_gsea_times_ms[3] = ms_since(t0);
        if (int rc = check_device(device)) return rc;
        if (nS == 0) return VBNMF_OK;
        return gsea_run(device, N, r, nS, valid, wp, hit_ptr, hit_row, hit_is_miss, nperm, perms, H, es, exceed, null_es);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory inverting %lld permutations of %lld rows", (long long)nperm, (long long)N);
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_HIP, "vbnmf_gsea_perm: %s", ex.what());
    }
}

int vbnmf_gsea_info(int64_t N, int32_t *wave_width, int32_t *workgroup_size, int32_t *max_set_hits, int64_t *chunk_perms, double *times_ms)
{
    if (wave_width) *wave_width = kGseaWave;
    if (workgroup_size) *workgroup_size = kGseaThreads;
    if (max_set_hits) *max_set_hits = kGseaMaxSetHits;
    if (chunk_perms) *chunk_perms = gsea_chunk_perms(N);
    if (times_ms)
        for (int k = 0; k < 4; k++) times_ms[k] = tl_gsea_times_ms[k];
    return VBNMF_OK;
}

}  // extern "C"
