// labels.hip -- the consensus accumulator (vbnmf_consensus_*, include/vbnmf.h; kernels: consensus.h): the arg-max labels of
// every run of a rank, from an engine's state or from the caller, and the sums the dispersion follows from.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "consensus.h"
#include "engine.h"

using namespace vbnmf;

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
