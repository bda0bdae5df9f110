// svd.hip -- the sparse products on the tiled layout (k_spmm) and the truncated SVD of the resident X built on them (init.h:
// k_gram, k_small, k_apply, k_normal_init; the irlba of the svd2 initialiser), with the test hooks into its dense kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "engine.h"
#include "init.h"

using namespace vbnmf;

namespace {

int launch_spmm(vbnmf_engine *e, const SweepSide &a)
{
    return with_rank(e->R, [&](auto rt) {
        return with_sweep_shape<rt()>(e, [&](auto s) {
            return launch_lds_kernel<k_spmm<s.R, s.WIDE, s.NT, s.SP>>(e, dim3((unsigned)e->n_wg), s.NT, a);
        });
    });
}

// Sparse product with the resident X on operands that are ALREADY on the device: gene side C[n][R] = X B (B = the lh
// array, one row per cell), cell side C[m][R] = t(X) W (W = the lw array); the per-task partials are summed per
// major straight into `target`.
int spmm_device(vbnmf_engine *e, bool gene_side, double *target)
{
    SweepSide a = sweep_side_args(e, gene_side);
    a.logterm = 0;
    a.stop = nullptr;
    if (int rc = launch_spmm(e, a)) return rc;
    return launch_side_pack(e, gene_side, target);
}

// work space of the truncated SVD: [gram partials kGramBlocks * R*R | S (R*R) | S2 (R*R) | vals (R)]
struct SvdWs { double *gp, *S, *S2, *vals; };
SvdWs svd_ws(vbnmf_engine *e)
{
    const size_t RR = (size_t)e->R * e->R;
    SvdWs w;
    w.gp = e->svd_ws; w.S = w.gp + (size_t)kGramBlocks * RR; w.S2 = w.S + RR; w.vals = w.S2 + RR;
    return w;
}

int launch_gram(vbnmf_engine *e, const double *A, int64_t N)
{
    SvdWs w = svd_ws(e);
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_gram<rt()>>(e, dim3(kGramBlocks), 1024, 0, A, N, w.gp);
    });
}

int launch_small(vbnmf_engine *e, int mode, bool want_s2, double *vals_host, double seq)
{
    SvdWs w = svd_ws(e);
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_small<rt()>>(e, dim3(1), 1024, 0, w.gp, kGramBlocks, e->r, mode, w.S, want_s2 ? w.S2 : nullptr, w.vals,
                                            vals_host, seq, e->svd_status);
    });
}

int launch_apply(vbnmf_engine *e, const double *A, const double *S, int64_t N, double *B)
{
    return with_rank_up_to_64(e->R, [&](auto rt) {
        return launch_kernel<k_apply<rt()>>(e, dim3((unsigned)((N + 255) / 256)), 256, 0, A, S, N, B);
    });
}

// A <- orthonormal basis of range(A), A tall [N][R]: CholeskyQR twice (Gram matrix, its Cholesky factor's inverse,
// A times that) -- the second pass repairs the orthogonality the first loses to the condition number.  When `gram_ready`
// the block partials of t(A) A are already in the work space.
int orthonormalise(vbnmf_engine *e, double *A, int64_t N, bool gram_ready)
{
    SvdWs w = svd_ws(e);
    for (int pass = 0; pass < 2; pass++) {
        if (!(pass == 0 && gram_ready)) { if (int rc = launch_gram(e, A, N)) return rc; }
        if (int rc = launch_small(e, 0, false, nullptr, 0.0)) return rc;
        if (int rc = launch_apply(e, A, w.S, N, A)) return rc;
    }
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// Truncated SVD of the resident X by block subspace iteration, ENTIRELY on the device (the
// irlba::irlba(mat, rank) of the svd2 initialiser, reference R/bayesian.R:150-159): the subspace has k = the engine's
// rank columns (rank_out of them are returned); per iteration two sparse products (k_spmm), two CholeskyQR2
// orthonormalisations (k_gram / k_small / k_apply) and the k x k eigen-problem that yields the current singular values
// (k_small, Jacobi) -- the host only reads those k values from pinned memory for the stopping rule
// max |s - s_old| <= tol * s[0] over the leading rank_out.  No host <-> device copy inside the iteration.
// Outputs: u (n x rank_out, column-major), d (rank_out), vt (rank_out x m, column-major), iterations done.
int vbnmf_engine_svd(vbnmf_engine *e, int32_t rank_out, double tol, int32_t maxit, uint64_t seed, double *u, double *d,
                     double *vt, int32_t *iterations)
{
    if (!e || !u || !d || !vt) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (e->partitioned) return fail(VBNMF_ERR_STATE, "the truncated SVD needs an unpartitioned engine");
    if (rank_out < 1 || rank_out > e->r) return fail(VBNMF_ERR_BAD_ARG, "rank_out must be in [1, engine rank]");
    if (e->R > VBNMF_MAX_SVD_COLUMNS)
        return fail(VBNMF_ERR_BAD_ARG, "the device-resident SVD holds at most %d subspace columns (engine rank %d); use the sparse products (vbnmf_engine_spmm) with a host QR", VBNMF_MAX_SVD_COLUMNS, e->r);
    if (maxit < 1) return fail(VBNMF_ERR_BAD_ARG, "maxit must be >= 1");
    if (int rc = use_device(e)) return rc;
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false; e->ml_ready = false;
    const size_t RR = (size_t)e->R * e->R;
    if (!e->svd_ws) { if (int rc = dev_alloc(&e->svd_ws, (size_t)kGramBlocks * RR + 2 * RR + e->R)) return rc; }
    if (!e->svd_status) { if (int rc = dev_alloc(&e->svd_status, 1)) return rc; }
    HIPCHECK(hipMemsetAsync(e->svd_status, 0, sizeof(int32_t), e->stream));
    if (int rc = ensure_history(e, (size_t)e->R + 2)) return rc;             // pinned [R values | sequence number]
    SvdWs w = svd_ws(e);
    volatile double *hv = e->h_hist;
    hv[e->R] = 0.0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t nh = e->m * e->R;
    double *Q = e->lw, *Z = e->lh;                                           // n x k and m x k, index-major
    // range finder: Q = orth(X G), G standard normal m x k
    hipLaunchKernelGGL(k_normal_init, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, e->stream, Z, e->m, e->r, e->R, k0, k1);
    HIPCHECK(hipGetLastError());
    if (int rc = spmm_device(e, true, Q)) return rc;
    if (int rc = orthonormalise(e, Q, e->n, false)) return rc;
    std::vector<double> s_old;
    int it = 0;
    for (it = 1; it <= maxit; it++) {
        if (int rc = spmm_device(e, false, Z)) return rc;                    // Z = t(X) Q
        if (int rc = orthonormalise(e, Z, e->m, false)) return rc;
        if (int rc = spmm_device(e, true, Q)) return rc;                     // Y = X Z = Q Rm
        if (int rc = launch_gram(e, Q, e->n)) return rc;                     // t(Y) Y = t(Rm) Rm: eigenvalues = sigma^2
        if (int rc = launch_small(e, 1, false, e->h_hist_dev, (double)it)) return rc;
        if (int rc = orthonormalise(e, Q, e->n, true)) return rc;            // (the Gram partials are still in place)
        HIPCHECK(hipStreamSynchronize(e->stream));
        if (hv[e->R] != (double)it) return fail(VBNMF_ERR_HIP, "the singular values of iteration %d never arrived", it);
        std::vector<double> sv(rank_out);
        for (int q = 0; q < rank_out; q++) sv[q] = std::sqrt(std::max(0.0, (double)hv[q]));
        bool done = false;
        if (!s_old.empty()) {
            double dmax = 0.0;
            for (int q = 0; q < rank_out; q++) dmax = std::max(dmax, std::fabs(sv[q] - s_old[q]));
            done = dmax <= tol * sv[0];
        }
        s_old.swap(sv);
        if (done) break;
    }
    if (it > maxit) it = maxit;
    // B = t(Q) X = t(P), P = t(X) Q (m x k): B t(B) = t(P) P = Ub D^2 t(Ub); u = Q Ub, rows of vt = P Ub / D
    if (int rc = spmm_device(e, false, Z)) return rc;
    if (int rc = launch_gram(e, Z, e->m)) return rc;
    if (int rc = launch_small(e, 1, true, e->h_hist_dev, (double)(maxit + 1))) return rc;
    if (int rc = launch_apply(e, Q, w.S, e->n, e->ew)) return rc;
    if (int rc = launch_apply(e, Z, w.S2, e->m, e->eh)) return rc;
    HIPCHECK(hipStreamSynchronize(e->stream));
    int32_t status = 0;
    HIPCHECK(hipMemcpy(&status, e->svd_status, sizeof status, hipMemcpyDeviceToHost));
    if (status) return fail(VBNMF_ERR_STATE, "the subspace lost rank (a Gram matrix was not positive definite): fewer independent directions than the engine's rank");
    for (int q = 0; q < rank_out; q++) d[q] = std::sqrt(std::max(0.0, (double)hv[q]));
    try {
        std::vector<double> tmp((size_t)std::max(e->n, e->m) * e->R);
        HIPCHECK(hipMemcpy(tmp.data(), e->ew, (size_t)e->n * e->R * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < e->n; i++) for (int q = 0; q < rank_out; q++) u[i + (size_t)q * e->n] = tmp[(size_t)i * e->R + q];
        HIPCHECK(hipMemcpy(tmp.data(), e->eh, (size_t)e->m * e->R * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < e->m; j++) {
            const int64_t col = e->cell_perm.empty() ? j : e->cell_perm[j];
            for (int q = 0; q < rank_out; q++) vt[q + (size_t)col * rank_out] = tmp[(size_t)j * e->R + q];
        }
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the singular vectors");
    }
    if (iterations) *iterations = it;
    return VBNMF_OK;
}

// ---------------------------------------------------------------- sparse products (truncated SVD of the svd2 initialiser)
int vbnmf_engine_spmm(vbnmf_engine *e, int32_t transpose, const double *B, double *C)
{
    if (!e || !B || !C) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (e->partitioned) return fail(VBNMF_ERR_STATE, "spmm needs an unpartitioned engine");
    if (int rc = use_device(e)) return rc;
    // the factor arrays serve as operand storage: whatever state the engine held is gone
    e->has_state = false; e->stats_ready = false; e->step_pending = false; e->prime_pending = false; e->ml_ready = false;
    const bool gene_side = transpose == 0;             // C = X t(B): lanes own genes and gather rows of B (one per cell)
    const SideView out = side_view(e, gene_side), in = side_view(e, !gene_side);
    const int64_t n_in = in.nmaj, n_out = out.nmaj;
    double *operand = in.l;                            // gathered through LDS
    double *dense = out.e;                             // [n_out][R] result before the download
    try {
        std::vector<double> tmp;
        to_index_major(B, n_in, e->r, e->R, gene_side, tmp, gene_side ? &e->cell_perm : nullptr);     // B: one row per cell on the gene side
        HIPCHECK(hipMemcpyAsync(operand, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        if (int rc = spmm_device(e, gene_side, dense)) return rc;
        const int64_t cnt = n_out * e->R;
        tmp.resize((size_t)cnt);
        HIPCHECK(hipMemcpyAsync(tmp.data(), dense, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        from_index_major(tmp, n_out, e->r, e->R, !gene_side, C, gene_side ? nullptr : &e->cell_perm);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory staging the operands");
    }
    return VBNMF_OK;
}

}  // extern "C"

namespace {

// What a dense-SVD test hook holds on the device (DeviceCall's alloc / upload; never entered: use_device(0) chose the device)
// and pinned: released on every return path.
struct HookBuffers : DeviceCall {
    void *pinned = nullptr;
    ~HookBuffers() { if (pinned) (void)hipHostFree(pinned); }
};

int download(double *dst, const double *src, size_t count)
{
    HIPCHECK(hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

// R must be a width the dense kernels are instantiated for
int hook_width(int32_t R)
{
    return with_rank_up_to_64(R, [](auto) { return (int)VBNMF_OK; });
}

constexpr int64_t kHookMaxRows = (int64_t)1 << 24;           // 8 GB of doubles at R = 64: a test has no use for more

}  // namespace

extern "C" {

// ---- test hooks into the dense kernels of the truncated SVD (init.h), each with the launch geometry of
// vbnmf_engine_svd: upload, one launch of the product's kernel on the null stream, download
int vbnmf_test_svd_gram(int32_t R, int64_t N, const double *A, double *gp)
{
    if (!A || !gp || N < 1 || N > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or N outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dA = nullptr, *dgp = nullptr;
    const size_t RR = (size_t)R * R;
    if (int rc = hb.upload(&dA, A, (size_t)N * R)) return rc;
    if (int rc = hb.alloc(&dgp, (size_t)kGramBlocks * RR)) return rc;
    HIPCHECK(hipMemset(dgp, 0xFF, (size_t)kGramBlocks * RR * sizeof(double)));       // NaN: the kernel writes every partial
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_gram<rt()>, dim3(kGramBlocks), dim3(1024), 0, nullptr, (const double *)dA, N, dgp);
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    return download(gp, dgp, (size_t)kGramBlocks * RR);
}

int vbnmf_test_svd_small(int32_t R, int32_t k, int32_t mode, int32_t nb, const double *gp, double seq, double *S, double *S2,
                         double *vals, double *vals_host, int32_t *status)
{
    if (!gp || !S || !vals || !status) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (mode != 0 && mode != 1) return fail(VBNMF_ERR_BAD_ARG, "mode must be 0 (Cholesky) or 1 (Jacobi)");
    if (nb < 1 || nb > 65536) return fail(VBNMF_ERR_BAD_ARG, "nb must be in [1, 65536]");
    if (int rc = hook_width(R)) return rc;
    if (k < 1 || k > R) return fail(VBNMF_ERR_BAD_ARG, "k must be in [1, R]");
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    const size_t RR = (size_t)R * R;
    double *dgp = nullptr, *dS = nullptr, *dS2 = nullptr, *dvals = nullptr, *dstat = nullptr, *hv = nullptr, *hv_dev = nullptr;
    if (int rc = hb.upload(&dgp, gp, (size_t)nb * RR)) return rc;
    if (int rc = hb.alloc(&dS, RR)) return rc;
    if (S2) { if (int rc = hb.alloc(&dS2, RR)) return rc; }
    if (int rc = hb.alloc(&dvals, (size_t)R)) return rc;
    if (int rc = hb.alloc(&dstat, 1)) return rc;                               // (8 bytes: the status is its first 4)
    HIPCHECK(hipMemset(dS, 0xFF, RR * sizeof(double)));
    if (dS2) HIPCHECK(hipMemset(dS2, 0xFF, RR * sizeof(double)));
    HIPCHECK(hipMemset(dvals, 0, (size_t)R * sizeof(double)));
    HIPCHECK(hipMemset(dstat, 0, sizeof(double)));
    if (vals_host) {                                                           // pinned and device-visible, as the engine's history block
        hipError_t he = hipHostMalloc(&hb.pinned, ((size_t)R + 2) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
        if (he != hipSuccess) { (void)hipGetLastError(); hb.pinned = nullptr; return fail(VBNMF_ERR_OOM, "pinned values block: %s", hipGetErrorString(he)); }
        hv = static_cast<double *>(hb.pinned);
        for (int q = 0; q <= R; q++) hv[q] = 0.0;
        HIPCHECK(hipHostGetDevicePointer((void **)&hv_dev, hv, 0));
    }
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_small<rt()>, dim3(1), dim3(1024), 0, nullptr, (const double *)dgp, (int)nb, (int)k, (int)mode, dS, dS2, dvals,
                               hv_dev, seq, reinterpret_cast<int32_t *>(dstat));
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    HIPCHECK(hipDeviceSynchronize());
    if (int rc = download(S, dS, RR)) return rc;
    if (S2) { if (int rc = download(S2, dS2, RR)) return rc; }
    if (int rc = download(vals, dvals, (size_t)R)) return rc;
    HIPCHECK(hipMemcpy(status, dstat, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vals_host) { const volatile double *v = hv; for (int q = 0; q <= R; q++) vals_host[q] = v[q]; }
    return VBNMF_OK;
}

int vbnmf_test_svd_apply(int32_t R, int64_t N, const double *A, const double *S, int32_t in_place, double *B)
{
    if (!A || !S || !B || N < 1 || N > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or N outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dA = nullptr, *dS = nullptr, *dB = nullptr;
    if (int rc = hb.upload(&dA, A, (size_t)N * R)) return rc;
    if (int rc = hb.upload(&dS, S, (size_t)R * R)) return rc;
    if (in_place) dB = dA;
    else {
        if (int rc = hb.alloc(&dB, (size_t)N * R)) return rc;
        HIPCHECK(hipMemset(dB, 0xFF, (size_t)N * R * sizeof(double)));
    }
    if (int rc = with_rank_up_to_64(R, [&](auto rt) {
            hipLaunchKernelGGL(k_apply<rt()>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, (const double *)dA, (const double *)dS, N, dB);
            HIPCHECK(hipGetLastError());
            return (int)VBNMF_OK;
        })) return rc;
    return download(B, dB, (size_t)N * R);
}

int vbnmf_test_svd_normal(int64_t nmaj, int32_t r, int32_t R, uint64_t seed, double *g)
{
    if (!g || nmaj < 1 || nmaj > kHookMaxRows) return fail(VBNMF_ERR_BAD_ARG, "NULL argument or nmaj outside [1, 2^24]");
    if (int rc = hook_width(R)) return rc;
    if (r < 1 || r > R) return fail(VBNMF_ERR_BAD_ARG, "r must be in [1, R]");
    if (int rc = use_device(0)) return rc;
    HookBuffers hb;
    double *dg = nullptr;
    const int64_t cnt = nmaj * R;
    if (int rc = hb.alloc(&dg, (size_t)cnt)) return rc;
    HIPCHECK(hipMemset(dg, 0xFF, (size_t)cnt * sizeof(double)));
    hipLaunchKernelGGL(k_normal_init, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, nullptr, dg, nmaj, (int)r, (int)R, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
    HIPCHECK(hipGetLastError());
    return download(g, dg, (size_t)cnt);
}

}  // extern "C"
