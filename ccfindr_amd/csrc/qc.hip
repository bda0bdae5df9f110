// qc.hip -- per-gene statistics for filter_genes (qc.h): the values grouped by gene and their row pointers go up once, one
// launch takes every row, the rows the kernel left undecided are finished on the host.
#include <algorithm>
#include <exception>
#include <new>

#include "device.h"
#include "qc.h"

using namespace vbnmf;

namespace {

thread_local double tl_qc_times_ms[4] = {0.0, 0.0, 0.0, 0.0};     // grouping by gene, upload, kernel (device events), host finish

// persistent workgroups of k_gene_stats on a device with `cus` compute units: as many as a CU holds threads for
int qc_grid(int cus) { return cus * (2048 / kQcThreads); }

int gene_stats_rows(const Matrix &M, int32_t device, int32_t bins, int64_t *nnz, double *sum, double *ss, int32_t *mode,
                    int64_t *host_finished)
{
    const int64_t n = M.n, m = M.m;
    for (double &v : tl_qc_times_ms) v = 0.0;
    DeviceCall D;
    if (int rc = D.enter(device)) return rc;
    // the values by gene, on the library's host threads (the cell numbers come with them and are dropped: no cell order, no cache)
    auto t0 = host_clock::now();
    std::vector<int64_t> rptr;
    BigVec<int32_t> ridx;
    BigVec<double> rval;
    transpose_compressed(m, n, M.colptr.data(), M.row.data(), M.val.data(), 0, rptr, ridx, rval, nullptr);
    BigVec<int32_t>().swap(ridx);
    tl_qc_times_ms[0] = ms_since(t0);

    t0 = host_clock::now();
    QcArgs a;
    if (int rc = D.upload(&a.rowptr, rptr.data(), (size_t)n + 1)) return rc;
    if (int rc = D.alloc(&a.nnz, (size_t)n)) return rc;
    if (int rc = D.alloc(&a.sum, (size_t)n)) return rc;
    if (int rc = D.alloc(&a.ss, (size_t)n)) return rc;
    if (int rc = D.alloc(&a.mode, (size_t)n)) return rc;
    if (int rc = D.alloc(&a.ticket, 1)) return rc;
    // the values go up as the doubles they are: packing integer counts into 2-byte words first cost more on the host than the
    // shorter copy saved, and the kernel's time did not change (profiles/qc_times.txt)
    if (int rc = D.upload(&a.val, rval.data(), rval.size())) return rc;
    HIPCHECK(hipMemsetAsync(a.ticket, 0, sizeof(unsigned int), nullptr));
    int cus = 0;
    if (int rc = device_cus(device, cus)) return rc;
    const int64_t tickets = (n + kQcTicketRows - 1) / kQcTicketRows;
    const unsigned grid = (unsigned)std::min<int64_t>(tickets, (int64_t)qc_grid(cus));
    tl_qc_times_ms[1] = ms_since(t0);
    a.n = n; a.m = m; a.bins = bins;
    HIPCHECK(hipEventRecord(D.ev0, nullptr));
    D.queued = true;
    hipLaunchKernelGGL(k_gene_stats, dim3(grid), dim3(kQcThreads), (size_t)kQcLdsFixed + 4 * (size_t)bins, nullptr, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(D.ev1, nullptr));
    HIPCHECK(hipMemcpy(nnz, a.nnz, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(sum, a.sum, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ss, a.ss, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(mode, a.mode, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    float kms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&kms, D.ev0, D.ev1));
    tl_qc_times_ms[2] = kms;

    // the rows the kernel left (a value that is no integer in [1, bins)): an exact sort-and-count each
    t0 = host_clock::now();
    std::vector<int64_t> left;
    for (int64_t i = 0; i < n; i++)
        if (mode[i] == 2) left.push_back(i);
    parallel_for((int64_t)left.size(), [&](int64_t b, int64_t e, int) {
        for (int64_t k = b; k < e; k++) {
            const int64_t i = left[(size_t)k];
            mode[i] = gene_mode_host(m, rptr[i + 1] - rptr[i], rval.data() + rptr[i]);
        }
    });
    if (host_finished) *host_finished = (int64_t)left.size();
    tl_qc_times_ms[3] = ms_since(t0);
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int vbnmf_matrix_gene_stats(const vbnmf_matrix *X, int32_t device, int32_t hist_bins, int64_t *nnz, double *sum, double *ss,
                            int32_t *mode, int64_t *host_finished)
{
    if (!X || !nnz || !sum || !ss || !mode) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (X->M.shell) return fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries");
    if (hist_bins == 0) hist_bins = kQcDefaultBins;
    if (hist_bins < 2 || hist_bins > kQcMaxBins)
        return fail(VBNMF_ERR_BAD_ARG, "hist_bins %d is outside [2, %d] (the occurrence table lives in LDS)", hist_bins, kQcMaxBins);
    if (int rc = check_device(device)) return rc;
    try {
        return gene_stats_rows(X->M, device, hist_bins, nnz, sum, ss, mode, host_finished);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory grouping the values by gene");
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_HIP, "vbnmf_matrix_gene_stats: %s", ex.what());
    }
}

int vbnmf_qc_info(int32_t *short_row_max, int32_t *pass_entries, int32_t *default_hist_bins, int32_t *grid_workgroups, double *times_ms)
{
    if (short_row_max) *short_row_max = kQcShortMax;
    if (pass_entries) *pass_entries = kQcPassEntries;
    if (default_hist_bins) *default_hist_bins = kQcDefaultBins;
    if (grid_workgroups) {
        int cnt = 0, cus = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0 || device_cus(0, cus) != VBNMF_OK) { (void)hipGetLastError(); *grid_workgroups = 0; }
        else *grid_workgroups = qc_grid(cus);
    }
    if (times_ms)
        for (int k = 0; k < 4; k++) times_ms[k] = tl_qc_times_ms[k];
    return VBNMF_OK;
}

}  // extern "C"
