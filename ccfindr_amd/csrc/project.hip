// project.hip -- projection of new cells onto a fitted basis (project.h): no layout, no engine -- the column range's compressed
// columns, the basis and the start go up once, one launch takes every cell to its own stop.  Then the same for a VB fit's
// posterior basis (vbproject.h), cell by cell and in the coupled form.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>

#include "device.h"
#include "project.h"
#include "rank.h"
#include "vbproject.h"

using namespace vbnmf;

namespace {

thread_local double tl_project_kernel_ms = 0.0;

// the persistent grid of the projection kernels: as many workgroups as a CU holds threads for (the kernels' few KB of LDS
// do not bound it), at most one per cell
int project_grid(int device, int64_t nc, unsigned &grid)
{
    int cus = 0;
    if (int rc = device_cus(device, cus)) return rc;
    grid = (unsigned)std::min<int64_t>(nc, (int64_t)cus * (2048 / kProjThreads));
    return VBNMF_OK;
}

int project_columns(const Matrix &M, int64_t cb, int64_t ce, int32_t r, const double *w, double *h, int32_t prior, double ga, double gb,
                    int32_t max_it, double tol, int32_t device, double *lk_cell, int32_t *it_cell, int32_t *reason_cell)
{
    const int64_t n = M.n, nc = ce - cb;
    const int R = padded_rank(r);
    DeviceCall D;
    if (int rc = D.enter(device)) return rc;
    // the basis by rows, R wide (what a cell gathers), colSums(w) (R/factorize.R:9; every column added gene by gene, in order)
    // and the start, cell by cell -- on the library's host threads
    std::vector<double> Wp((size_t)n * R, 0.0), cw((size_t)R, 0.0), Hp((size_t)nc * R, 0.0);
    parallel_for(n, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; i++)
            for (int k = 0; k < r; k++) Wp[(size_t)i * R + k] = w[(size_t)k * n + i];
    });
    parallel_for(r, [&](int64_t b, int64_t e, int) {
        for (int64_t k = b; k < e; k++) {
            double s = 0.0;
            for (int64_t i = 0; i < n; i++) s += w[(size_t)k * n + i];
            cw[k] = s;
        }
    });
    parallel_for(nc, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++)
            for (int k = 0; k < r; k++) Hp[(size_t)j * R + k] = h[(size_t)j * r + k];
    });
    const int64_t e0 = M.colptr[cb], ne = M.colptr[ce] - e0;

    ProjectArgs a;
    if (int rc = D.upload(&a.colptr, M.colptr.data() + cb, (size_t)nc + 1)) return rc;
    if (int rc = D.upload(&a.row, M.row.data() + e0, (size_t)ne)) return rc;
    if (int rc = D.upload(&a.val, M.val.data() + e0, (size_t)ne)) return rc;
    if (int rc = D.upload(&a.W, Wp.data(), Wp.size())) return rc;
    if (int rc = D.upload(&a.cw, cw.data(), cw.size())) return rc;
    if (int rc = D.upload(&a.H, Hp.data(), Hp.size())) return rc;
    if (int rc = D.alloc(&a.lk, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.it, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.reason, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.ticket, 1)) return rc;
    HIPCHECK(hipMemsetAsync(a.ticket, 0, sizeof(unsigned int), nullptr));
    a.base = e0; a.ncell = nc; a.r = r; a.prior = prior ? 1 : 0; a.max_it = max_it;
    a.ga = ga; a.gb = gb; a.tol = tol; a.eps = 2.220446049250313e-16;
    unsigned grid = 0;
    if (int rc = project_grid(device, nc, grid)) return rc;
    HIPCHECK(hipEventRecord(D.ev0, nullptr));
    D.queued = true;
    int rc = with_rank(R, [&](auto rt) {
        hipLaunchKernelGGL((k_project<rt()>), dim3(grid), dim3(kProjThreads), 0, nullptr, a);
        HIPCHECK(hipGetLastError());
        return (int)VBNMF_OK;
    });
    if (rc) return rc;
    HIPCHECK(hipEventRecord(D.ev1, nullptr));
    HIPCHECK(hipMemcpy(Hp.data(), a.H, Hp.size() * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    HIPCHECK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
    tl_project_kernel_ms = ms;
    parallel_for(nc, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++)
            for (int k = 0; k < r; k++) h[(size_t)j * r + k] = Hp[(size_t)j * R + k];
    });
    if (lk_cell) HIPCHECK(hipMemcpy(lk_cell, a.lk, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
    if (it_cell) HIPCHECK(hipMemcpy(it_cell, a.it, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (reason_cell) HIPCHECK(hipMemcpy(reason_cell, a.reason, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

// ---- the same for a VB fit's posterior basis (vbproject.h): the table lw | lw log lw by rows, colSums(ew) and the start go
// up once, one launch takes every cell to its own stop.
thread_local double tl_vb_project_kernel_ms = 0.0;

// What both VB projections put on the device (vbproject.h): per gene, 2 R wide, lw_i. | (lw log lw)_i. (R/bayesian.R:90; padding
// columns 0), colSums(ew) (:80; every column added gene by gene, in order), the start cell by cell -- formed on the library's host
// threads --, the cells' compressed columns, and room for eh, dh and the cell evidences.  Args: VbProjectArgs or VbpStepArgs,
// whose pointers of these names it fills.
template <class Args>
int vb_project_upload(const Matrix &M, int64_t cb, int64_t ce, int32_t r, const double *lw, const double *ew, const double *lh,
                      DeviceCall &D, Args &a)
{
    const int64_t n = M.n, nc = ce - cb;
    const int R = padded_rank(r);
    std::vector<double> Tp((size_t)n * 2 * R, 0.0), cew((size_t)R, 0.0), Hp((size_t)nc * R, 0.0);
    parallel_for(n, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; i++)
            for (int k = 0; k < r; k++) {
                const double v = lw[(size_t)k * n + i];
                Tp[(size_t)i * 2 * R + k] = v;
                Tp[(size_t)i * 2 * R + R + k] = v * std::log(v);
            }
    });
    parallel_for(r, [&](int64_t b, int64_t e, int) {
        for (int64_t k = b; k < e; k++) {
            double s = 0.0;
            for (int64_t i = 0; i < n; i++) s += ew[(size_t)k * n + i];
            cew[k] = s;
        }
    });
    parallel_for(nc, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++)
            for (int k = 0; k < r; k++) Hp[(size_t)j * R + k] = lh[(size_t)j * r + k];
    });
    const int64_t e0 = M.colptr[cb], ne = M.colptr[ce] - e0;

    if (int rc = D.upload(&a.colptr, M.colptr.data() + cb, (size_t)nc + 1)) return rc;
    if (int rc = D.upload(&a.row, M.row.data() + e0, (size_t)ne)) return rc;
    if (int rc = D.upload(&a.val, M.val.data() + e0, (size_t)ne)) return rc;
    if (int rc = D.upload(&a.T, Tp.data(), Tp.size())) return rc;
    if (int rc = D.upload(&a.cew, cew.data(), cew.size())) return rc;
    if (int rc = D.upload(&a.LH, Hp.data(), Hp.size())) return rc;
    if (int rc = D.alloc(&a.EH, Hp.size())) return rc;
    if (int rc = D.alloc(&a.DH, Hp.size())) return rc;
    if (int rc = D.alloc(&a.ev, (size_t)nc)) return rc;
    a.base = e0; a.ncell = nc; a.r = r;
    return VBNMF_OK;
}

// lh, eh, dh (each may be NULL) of the cells back into r x cells column-major arrays
template <class Args>
int vb_project_download(const Args &a, int64_t nc, int32_t r, double *lh, double *eh, double *dh)
{
    const int R = padded_rank(r);
    std::vector<double> back((size_t)nc * R);
    double *const outs[3] = {lh, eh, dh};
    const double *const srcs[3] = {a.LH, a.EH, a.DH};
    for (int q = 0; q < 3; q++) {
        if (!outs[q]) continue;
        HIPCHECK(hipMemcpy(back.data(), srcs[q], back.size() * sizeof(double), hipMemcpyDeviceToHost));
        double *out = outs[q];
        parallel_for(nc, [&](int64_t b, int64_t e, int) {
            for (int64_t j = b; j < e; j++)
                for (int k = 0; k < r; k++) out[(size_t)j * r + k] = back[(size_t)j * R + k];
        });
    }
    return VBNMF_OK;
}

int vb_project_columns(const Matrix &M, int64_t cb, int64_t ce, int32_t r, const double *lw, const double *ew, double ah, double bh,
                       double fudge, double *lh, double *eh, double *dh, int32_t max_it, double tol, int32_t device, double *ev_cell,
                       int32_t *it_cell, int32_t *reason_cell)
{
    const int64_t nc = ce - cb;
    const int R = padded_rank(r);
    DeviceCall D;
    if (int rc = D.enter(device)) return rc;
    VbProjectArgs a;
    if (int rc = vb_project_upload(M, cb, ce, r, lw, ew, lh, D, a)) return rc;
    if (int rc = D.alloc(&a.it, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.reason, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.ticket, 1)) return rc;
    HIPCHECK(hipMemsetAsync(a.ticket, 0, sizeof(unsigned int), nullptr));
    a.max_it = max_it; a.ah = ah; a.bh = bh; a.tol = tol; a.fudge = fudge;
    unsigned grid = 0;
    if (int rc = project_grid(device, nc, grid)) return rc;
    HIPCHECK(hipEventRecord(D.ev0, nullptr));
    D.queued = true;
    int rc = with_rank(R, [&](auto rt) {
        hipLaunchKernelGGL((k_vb_project<rt()>), dim3(grid), dim3(kProjThreads), 0, nullptr, a);
        HIPCHECK(hipGetLastError());
        return (int)VBNMF_OK;
    });
    if (rc) return rc;
    HIPCHECK(hipEventRecord(D.ev1, nullptr));
    if (int rc = vb_project_download(a, nc, r, lh, eh, dh)) return rc;
    float ms = 0.0f;
    HIPCHECK(hipEventSynchronize(D.ev1));
    HIPCHECK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
    tl_vb_project_kernel_ms = ms;
    if (ev_cell) HIPCHECK(hipMemcpy(ev_cell, a.ev, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
    if (it_cell) HIPCHECK(hipMemcpy(it_cell, a.it, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (reason_cell) HIPCHECK(hipMemcpy(reason_cell, a.reason, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

// ---- the coupled form (vbproject.h, k_vbp_step / k_vbp_control): the same upload plus what a cell carries between launches;
// (step, control) pairs are queued eight steps ahead, never past max_it, and the control block is read after each batch.
constexpr int kVbpBatch = 8;

int vb_project_coupled_columns(const Matrix &M, int64_t cb, int64_t ce, int32_t r, const double *lw, const double *ew, double *hyper,
                               const int32_t *flags, int32_t n0, int32_t dn, double fudge, double *lh, double *eh, double *dh,
                               int32_t max_it, double tol, int32_t device, double *ev_cell, int32_t *it_cell, int32_t *reason_cell,
                               int32_t *it_out, int32_t *reason_out, double *evidence, double *history, int64_t history_rows)
{
    const int64_t nc = ce - cb;
    const int R = padded_rank(r);
    DeviceCall D;
    if (int rc = D.enter(device)) return rc;
    const int64_t hrows = history ? std::min<int64_t>(std::max<int64_t>(history_rows, 0), max_it) : 0;
    VbpStepArgs a;
    double *hist = nullptr;
    if (int rc = vb_project_upload(M, cb, ce, r, lw, ew, lh, D, a)) return rc;
    if (int rc = D.alloc(&a.S, (size_t)nc * R)) return rc;
    if (int rc = D.alloc(&a.lgx, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.seh, (size_t)nc)) return rc;
    if (int rc = D.alloc(&a.sll, (size_t)nc)) return rc;
    if (int rc = D.alloc(&hist, (size_t)hrows * 5)) return rc;
    if (int rc = D.alloc(&a.ctl, 1)) return rc;
    a.fudge = fudge;
    VbpCtl c;
    std::memset(&c, 0, sizeof c);                            // it, stop, reason, lk0, the ticket: 0
    c.hyper[0] = 1.0; c.hyper[1] = 1.0; c.hyper[2] = hyper[0]; c.hyper[3] = hyper[1];
    c.tol = tol; c.max_it = max_it; c.n0 = n0; c.dn = dn;
    c.flags[2] = flags[0] ? 1 : 0; c.flags[3] = flags[1] ? 1 : 0;
    HIPCHECK(hipMemcpy(a.ctl, &c, sizeof c, hipMemcpyHostToDevice));
    unsigned grid = 0;
    if (int rc = project_grid(device, nc, grid)) return rc;
    HIPCHECK(hipEventRecord(D.ev0, nullptr));
    D.queued = true;
    int32_t queued = 0;
    while (!c.stop && queued < max_it) {
        const int32_t batch = std::min<int32_t>(kVbpBatch, max_it - queued);
        int rc = with_rank(R, [&](auto rt) {
            for (int32_t q = 0; q < batch; q++) {
                hipLaunchKernelGGL((k_vbp_step<rt()>), dim3(grid), dim3(kProjThreads), 0, nullptr, a);
                hipLaunchKernelGGL(k_vbp_control, dim3(1), dim3(1024), 0, nullptr, a.ev, a.seh, a.sll, nc, (int)r, a.ctl, hrows ? hist : nullptr,
                                   hrows);
            }
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        });
        if (rc) return rc;
        queued += batch;
        HIPCHECK(hipMemcpy(&c, a.ctl, sizeof c, hipMemcpyDeviceToHost));     // (waits for the batch)
    }
    if (!c.stop) return fail(VBNMF_ERR_HIP, "the coupled projection's device loop did not stop within max_it = %d steps", max_it);
    HIPCHECK(hipEventRecord(D.ev1, nullptr));
    if (int rc = vb_project_download(a, nc, r, lh, eh, dh)) return rc;
    float ms = 0.0f;
    HIPCHECK(hipEventSynchronize(D.ev1));
    HIPCHECK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
    tl_vb_project_kernel_ms = ms;
    if (ev_cell) HIPCHECK(hipMemcpy(ev_cell, a.ev, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
    if (it_cell) std::fill(it_cell, it_cell + nc, c.it);                     // one stop: every cell made the same steps
    if (reason_cell) std::fill(reason_cell, reason_cell + nc, c.reason);
    const int64_t rows = std::min<int64_t>(hrows, c.it);
    if (rows > 0) HIPCHECK(hipMemcpy(history, hist,(size_t)rows * 5 * sizeof(double), hipMemcpyDeviceToHost));
    hyper[0] = c.hyper[2]; hyper[1] = c.hyper[3];
    if (it_out) *it_out = c.it;
    if (reason_out) *reason_out = c.reason;
    if (evidence) *evidence = c.E;
    return VBNMF_OK;
}

// what the three projections ask of their matrix, rank, column range and step limit
int check_columns(const vbnmf_matrix *X, const char *who, int32_t r, int64_t col_begin, int64_t col_end, int32_t max_it)
{
    if (X->M.shell) return fail(VBNMF_ERR_BAD_ARG, "a shell matrix holds no entries: %s needs the compressed columns", who);
    if (r < 1 || r > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", r, VBNMF_MAX_RANK);
    if (col_begin < 0 || col_end > X->M.m || col_begin >= col_end)
        return fail(VBNMF_ERR_BAD_ARG, "column range [%lld, %lld) is empty or outside the matrix's %lld columns", (long long)col_begin,
                    (long long)col_end, (long long)X->M.m);
    if (max_it < 1) return fail(VBNMF_ERR_BAD_ARG, "max_it must be >= 1");
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int vbnmf_matrix_project(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r, const double *w, double *h,
                         int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol, int32_t device,
                         double *lk_cell, int32_t *it_cell, int32_t *reason_cell)
{
    if (!X || !w || !h) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_columns(X, "project", r, col_begin, col_end, max_it)) return rc;
    if (int rc = check_device(device)) return rc;
    try {
        return project_columns(X->M, col_begin, col_end, r, w, h, prior, gamma_a, gamma_b, max_it, tol, device, lk_cell, it_cell, reason_cell);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the projection's staging arrays");
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_HIP, "vbnmf_matrix_project: %s", ex.what());
    }
}

int vbnmf_project_info(int32_t r, int32_t *pass_entries, double *last_kernel_ms)
{
    if (r < 1 || r > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", r, VBNMF_MAX_RANK);
    if (pass_entries) *pass_entries = proj_pass_entries(padded_rank(r));
    if (last_kernel_ms) *last_kernel_ms = tl_project_kernel_ms;
    return VBNMF_OK;
}

int vbnmf_matrix_vb_project(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r, const double *lw, const double *ew,
                            double ah, double bh, double fudge, double *lh, double *eh, double *dh, int32_t max_it, double tol,
                            int32_t device, double *ev_cell, int32_t *it_cell, int32_t *reason_cell)
{
    if (!X || !lw || !ew || !lh) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_columns(X, "vb_project", r, col_begin, col_end, max_it)) return rc;
    if (!(ah > 0.0) || !(bh > 0.0)) return fail(VBNMF_ERR_BAD_ARG, "ah and bh must be > 0 (got %g, %g)", ah, bh);
    if (int rc = check_device(device)) return rc;
    try {
        return vb_project_columns(X->M, col_begin, col_end, r, lw, ew, ah, bh, fudge, lh, eh, dh, max_it, tol, device, ev_cell, it_cell,
                                  reason_cell);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the projection's staging arrays");
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_HIP, "vbnmf_matrix_vb_project: %s", ex.what());
    }
}

int vbnmf_matrix_vb_project_coupled(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r, const double *lw,
                                    const double *ew, double *hyper, const int32_t *flags, int32_t n0, int32_t dn, double fudge,
                                    double *lh, double *eh, double *dh, int32_t max_it, double tol, int32_t device, double *ev_cell,
                                    int32_t *it_cell, int32_t *reason_cell, int32_t *it, int32_t *reason, double *evidence,
                                    double *history, int64_t history_rows)
{
    if (!X || !lw || !ew || !lh || !hyper || !flags) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_columns(X, "vb_project", r, col_begin, col_end, max_it)) return rc;
    if (!(hyper[0] > 0.0) || !(hyper[1] > 0.0) || !std::isfinite(hyper[0]) || !std::isfinite(hyper[1]))
        return fail(VBNMF_ERR_BAD_ARG, "ah and bh must be > 0 and finite (got %g, %g)", hyper[0], hyper[1]);
    if (dn < 1) return fail(VBNMF_ERR_BAD_ARG, "dn must be >= 1");
    if (n0 < 0) return fail(VBNMF_ERR_BAD_ARG, "n0 must be >= 0");
    if (int rc = check_device(device)) return rc;
    try {
        return vb_project_coupled_columns(X->M, col_begin, col_end, r, lw, ew, hyper, flags, n0, dn, fudge, lh, eh, dh, max_it, tol, device,
                                          ev_cell, it_cell, reason_cell, it, reason, evidence, history, history_rows);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the projection's staging arrays");
    } catch (const std::exception &ex) {
        return fail(VBNMF_ERR_HIP, "vbnmf_matrix_vb_project_coupled: %s", ex.what());
    }
}

int vbnmf_vb_project_info(int32_t r, int32_t *pass_entries, double *last_kernel_ms)
{
    if (r < 1 || r > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", r, VBNMF_MAX_RANK);
    if (pass_entries) *pass_entries = proj_pass_entries(padded_rank(r));
    if (last_kernel_ms) *last_kernel_ms = tl_vb_project_kernel_ms;
    return VBNMF_OK;
}

}  // extern "C"
