// host.cpp -- host side of libvbnmf_hip.so: error plumbing, the fork-join over host threads, ingestion of X into the
// canonical CSC copy and the matrix handle's ABI.  The tiled layout is cut in layout.cpp, shared through node memory in
// blob.cpp.  No device code here.
//
// Reference behaviour this replaces: vb_iterate hands `as.matrix(bundle$mat)` to the
// native step on EVERY iteration (reference R/bayesian.R:339) and Rcpp copies it again
// into an Eigen::MatrixXd (reference src/RcppExports.cpp:15).  Here X is ingested once.
#include "common.h"

#include <algorithm>
#include <atomic>
#include <sched.h>

#include <chrono>
#include <system_error>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <new>

namespace vbnmf {

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char *last_error_cstr() { return g_err.c_str(); }

// ------------------------------------------------------------------ threads
static std::atomic<int> g_host_threads_override{0};         // vbnmf_set_host_threads (0: the default rule below)
void set_host_threads_override(int n) { g_host_threads_override.store(n > 0 ? std::min(n, 1024) : 0, std::memory_order_relaxed); }

int host_threads()
{
    const int forced = g_host_threads_override.load(std::memory_order_relaxed);
    if (forced > 0) return forced;
    static int n = [] {
        if (const char *s = getenv("VBNMF_HOST_THREADS")) {
            int v = atoi(s);
            if (v > 0) return v;
        }
        unsigned hc = std::thread::hardware_concurrency();
        int v = hc ? (int)hc : 1;
        cpu_set_t set;                                   // a rank pinned to a subset of the cores uses only those
        if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) v = std::min(v, CPU_COUNT(&set));
        return std::min(v, 32);
    }();
    return n;
}

// Fork-join over [0, count): every call starts and joins its own threads (~25 us apiece on the GPU box's host).  Round 5 built
// the alternative -- a pool of workers that outlives the call, the caller helping -- and measured it on the headline matrix's
// set-up (profiles/r05_setup_pool_ab.txt, r05_transpose_ab2.txt): the dispatch is cheaper, but the heavy phases run SLOWER on
// woken workers than on fresh threads (the fill of the gene side 0.07-0.09 s against 0.04-0.05 s, engine creation 0.30-0.36 s
// against 0.25-0.28 s): a new thread is placed on the idlest core of a 256-CPU host, a woken one near where it last ran or near
// its waker, and a phase of 40 ms is over before the balancer has spread them.  So: threads per call, and callers whose work is
// small ask for few of them (the state conversions of set_state / get_state, the cache key of the stateless entries).
static thread_local int tl_thread_share = 1;          // this host thread's calls use host_threads() / share threads by default
void set_thread_share(int share) { tl_thread_share = share > 1 ? share : 1; }
static int default_threads() { return std::max(1, host_threads() / tl_thread_share); }

void parallel_for(int64_t count, const std::function<void(int64_t, int64_t, int)> &fn, int max_threads)
{
    if (count <= 0) return;
    int nt = max_threads > 0 ? max_threads : default_threads();
    if ((int64_t)nt > count) nt = (int)count;
    if (nt <= 1) { fn(0, count, 0); return; }
    // An exception leaving a std::thread ends the process (std::terminate): a worker that runs out of memory hands its
    // exception to the calling thread instead, which rethrows it once every worker has been joined -- the C ABI's entry
    // points then turn it into VBNMF_ERR_OOM like any other allocation failure.
    std::exception_ptr first;
    std::mutex first_mu;
    auto guarded = [&](int64_t b, int64_t e, int t) {
        try {
            fn(b, e, t);
        } catch (...) {
            std::lock_guard<std::mutex> g(first_mu);
            if (!first) first = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int t = 1; t < nt; t++) {
        int64_t b = count * t / nt, e = count * (t + 1) / nt;
        try {
            th.emplace_back([&guarded, b, e, t] { guarded(b, e, t); });
        } catch (const std::system_error &) {            // thread limit reached: this piece runs here
            guarded(b, e, t);
        }
    }
    guarded(0, count / nt, 0);                           // (the caller takes the first piece instead of sleeping)
    for (auto &x : th) x.join();
    if (first) std::rethrow_exception(first);
}

// ------------------------------------------------------------------ ingestion
static void finish_matrix(Matrix &X)
{
    X.nnz = X.colptr[X.m];
    // one pass over the values on all host threads (it was a serial 5e7-element loop: 80 ms of the headline's ingestion)
    const int T = host_threads();
    std::vector<char> ints_t(T, 1);
    std::vector<double> mx_t(T, 0.0);
    parallel_for(X.nnz, [&](int64_t b, int64_t e, int tid) {
        bool ok = true;
        double m = 0.0;
        for (int64_t q = b; q < e; q++) {
            const double v = X.val[q];
            ok = ok && v >= 1.0 && v < 2147483648.0 && v == std::floor(v);
            m = std::max(m, v);
        }
        ints_t[tid] = ok ? 1 : 0; mx_t[tid] = m;
    }, T);
    bool ints = true;
    double mx = 0.0;
    for (int t = 0; t < T; t++) { ints = ints && ints_t[t]; mx = std::max(mx, mx_t[t]); }
    X.counts_int = ints;
    X.max_val = mx;
    X.counts_u16 = ints && mx <= kPackedCountMax;
}

const RowMajor &Matrix::row_major() const
{
    std::call_once(rm_cache->once, [&] {
        const std::vector<int32_t> &perm = cell_order();
        transpose_compressed(m, n, colptr.data(), row.data(), val.data(), 0, rm_cache->rm.ptr, rm_cache->rm.idx, rm_cache->rm.val,
                             perm.empty() ? nullptr : perm.data());
    });
    return rm_cache->rm;
}

static int matrix_from_dense(int64_t n, int64_t m, const double *A, Matrix &X)
{
    X.n = n; X.m = m;
    X.colptr.assign(m + 1, 0);
    parallel_for(m, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++) {
            const double *c = A + (size_t)j * n;
            int64_t k = 0;
            for (int64_t i = 0; i < n; i++) k += (c[i] != 0.0);
            X.colptr[j + 1] = k;
        }
    });
    for (int64_t j = 0; j < m; j++) X.colptr[j + 1] += X.colptr[j];
    int64_t nnz = X.colptr[m];
    X.row.resize(nnz);
    X.val.resize(nnz);
    parallel_for(m, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++) {
            const double *c = A + (size_t)j * n;
            int64_t o = X.colptr[j];
            for (int64_t i = 0; i < n; i++)
                if (c[i] != 0.0) { X.row[o] = (int32_t)i; X.val[o] = c[i]; o++; }
        }
    });
    finish_matrix(X);
    return VBNMF_OK;
}

// Compressed input with `nouter` outer vectors of inner indices < ninner.  Produces the
// canonical form in the same orientation (inner ascending, duplicates summed, zeros dropped).
static int canonicalise(int64_t nouter, int64_t ninner, const int32_t *p, const int32_t *idx, const double *x,
                        std::vector<int64_t> &optr, std::vector<int32_t> &oidx, std::vector<double> &oval)
{
    if (p[0] != 0) return fail(VBNMF_ERR_BAD_ARG, "pointer array must start at 0");
    for (int64_t j = 0; j < nouter; j++)
        if (p[j + 1] < p[j]) return fail(VBNMF_ERR_BAD_ARG, "pointer array is not non-decreasing at %lld", (long long)j);
    int64_t nin = p[nouter];
    {
        std::atomic<int64_t> bad{-1};                       // the first offending position any thread saw (smallest wins below)
        parallel_for(nin, [&](int64_t b, int64_t e, int) {
            for (int64_t q = b; q < e; q++)
                if (idx[q] < 0 || idx[q] >= ninner) {
                    int64_t cur = bad.load();
                    while ((cur < 0 || q < cur) && !bad.compare_exchange_weak(cur, q)) {}
                    break;
                }
        });
        const int64_t e = bad.load();
        if (e >= 0) return fail(VBNMF_ERR_BAD_ARG, "index %d at position %lld is outside [0, %lld)", idx[e], (long long)e, (long long)ninner);
    }
    optr.assign(nouter + 1, 0);
    std::vector<int64_t> kept(nouter, 0);
    // pass 1: per outer vector, sort a scratch copy and count surviving entries
    std::vector<int32_t> sidx(nin);
    std::vector<double> sval(nin);
    parallel_for(nouter, [&](int64_t b, int64_t e, int) {
        std::vector<std::pair<int32_t, double>> tmp;
        for (int64_t j = b; j < e; j++) {
            int64_t s = p[j], t = p[j + 1];
            bool sorted = true;
            for (int64_t q = s + 1; q < t; q++)
                if (idx[q] <= idx[q - 1]) { sorted = false; break; }
            int64_t o = s;
            if (sorted) {
                for (int64_t q = s; q < t; q++)
                    if (x[q] != 0.0) { sidx[o] = idx[q]; sval[o] = x[q]; o++; }
            } else {
                tmp.clear();
                for (int64_t q = s; q < t; q++) tmp.emplace_back(idx[q], x[q]);
                std::stable_sort(tmp.begin(), tmp.end(),
                                 [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &c) { return a.first < c.first; });
                size_t q = 0;
                while (q < tmp.size()) {
                    int32_t id = tmp[q].first;
                    double v = 0.0;
                    while (q < tmp.size() && tmp[q].first == id) { v += tmp[q].second; q++; }
                    if (v != 0.0) { sidx[o] = id; sval[o] = v; o++; }
                }
            }
            kept[j] = o - s;
        }
    });
    for (int64_t j = 0; j < nouter; j++) optr[j + 1] = optr[j] + kept[j];
    oidx.resize(optr[nouter]);
    oval.resize(optr[nouter]);
    parallel_for(nouter, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++) {
            int64_t s = p[j], o = optr[j];
            for (int64_t q = 0; q < kept[j]; q++) { oidx[o + q] = sidx[s + q]; oval[o + q] = sval[s + q]; }
        }
    });
    return VBNMF_OK;
}

int matrix_from_csc(int64_t n, int64_t m, const int32_t *p, const int32_t *i, const double *x, Matrix &X)
{
    X.n = n; X.m = m;
    int rc = canonicalise(m, n, p, i, x, X.colptr, X.row, X.val);
    if (rc) return rc;
    finish_matrix(X);
    return VBNMF_OK;
}

// Transpose a canonical compressed matrix (nouter x ninner) into the other orientation (inner indices of the
// result ascending).  The OUTPUT is what the threads divide: the inner indices are cut into ranges (a few hundred rows of the
// result each), and since every outer vector holds its inner indices in ascending order, the stretch of it that falls into a
// range is found by bisection (a table of nouter x (ranges + 1) offsets, one pass).  A thread then takes a range: it counts the
// range's entries per inner index, scans, and scatters them -- outer vectors in order, so the result is ascending -- with all its
// write cursors (a few hundred) and its output stretch in its own cache.  The earlier form divided the INPUT (one chunk of outer
// vectors per thread, a counter per (chunk, inner index), every thread scattering into all 20 000 rows of the result): 0.117 s
// for the headline matrix's 4.9e7 entries on the GPU box's host, most of it cache misses of the scatter; this one 0.06-0.08 s
// (profiles/r05_transpose_ab2.txt).  Round 5 also measured a two-level form (entries first into <= 256 buckets as 16-byte records,
// then a stable pass inside every bucket): 0.27 s -- the record buffer's fresh 800 MB cost more than the scattered cursors.
// The result does not depend on the thread count (each range's content and order are fixed by the input alone).
// perm (optional, nouter entries): outer vector p of the result's numbering is input vector perm[p].  VI / VD: vectors of
// int32_t / double (BigVec where the caller can take it: the 600 MB of the result are then first touched by the threads that
// write them instead of being zero-filled by the caller's one).
template <class VI, class VD>
void transpose_compressed(int64_t nouter, int64_t ninner, const int64_t *ptr, const int32_t *idx, const double *val,
                          int32_t idx_offset, std::vector<int64_t> &tptr, VI &tidx, VD &tval, const int32_t *perm)
{
    const int64_t s = ptr[0], t = ptr[nouter];
    const auto t_0 = std::chrono::steady_clock::now();
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(default_threads(), (t - s) / (1 << 18) + 1));
    auto src = [&](int64_t j) { return perm ? (int64_t)perm[j] : j; };          // input vector stored at position j
    tptr.assign(ninner + 1, 0);
    tidx.resize(t - s);
    tval.resize(t - s);
    if (ninner <= 0) return;
    // ranges of inner indices: a few per thread (they differ in entries; handed out through a counter), one when serial
    int64_t G = T == 1 ? 1 : std::min<int64_t>(ninner, 4 * (int64_t)T);
    while (G > 1 && nouter * (G + 1) > ((int64_t)1 << 26)) G /= 2;                 // (the table of offsets below: at most 256 MB)
    auto lo_of = [&](int64_t g) { return ninner * g / G; };
    // split[j * (G + 1) + g]: offset inside outer vector j (position order) of its first entry with inner index >= lo_of(g)
    std::vector<uint32_t> split((size_t)nouter * (size_t)(G + 1));
    std::vector<int64_t> tot_t((size_t)T * (size_t)G, 0);                       // entries per range, by thread
    parallel_for(nouter, [&](int64_t b, int64_t e, int tid) {
        int64_t *tot = &tot_t[(size_t)tid * (size_t)G];
        for (int64_t j = b; j < e; j++) {
            const int64_t c = src(j);
            const int32_t *first = idx + ptr[c], *last = idx + ptr[c + 1];
            uint32_t *sp = &split[(size_t)j * (size_t)(G + 1)];
            const int32_t *at = first;
            sp[0] = 0;
            for (int64_t g = 1; g < G; g++) {
                at = std::lower_bound(at, last, (int32_t)lo_of(g));
                sp[g] = (uint32_t)(at - first);
                tot[g - 1] += (int64_t)sp[g] - (int64_t)sp[g - 1];
            }
            sp[G] = (uint32_t)(last - first);
            tot[G - 1] += (int64_t)sp[G] - (int64_t)sp[G - 1];
        }
    }, T);
    static const bool tt = getenv("VBNMF_BUILD_TIMES") != nullptr;
    auto t_a = std::chrono::steady_clock::now();
    std::vector<int64_t> base((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; g++) {
        int64_t k = 0;
        for (int c = 0; c < T; c++) k += tot_t[(size_t)c * (size_t)G + (size_t)g];
        base[g + 1] = base[g] + k;
    }
    std::atomic<int64_t> next{0};
    parallel_for(T, [&](int64_t, int64_t, int) {
        std::vector<int64_t> cur;
        for (;;) {
            const int64_t g = next.fetch_add(1);
            if (g >= G) break;
            const int64_t lo = lo_of(g), hi = lo_of(g + 1);
            cur.assign((size_t)(hi - lo) + 1, 0);
            for (int64_t j = 0; j < nouter; j++) {
                const uint32_t *sp = &split[(size_t)j * (size_t)(G + 1) + (size_t)g];
                const int32_t *q = idx + ptr[src(j)];
                for (uint32_t u = sp[0]; u < sp[1]; u++) cur[(size_t)(q[u] - lo) + 1]++;
            }
            int64_t run = base[g];
            for (int64_t i = 0; i < hi - lo; i++) { const int64_t k = cur[(size_t)i + 1]; tptr[lo + i] = run; cur[(size_t)i] = run; run += k; }
            for (int64_t j = 0; j < nouter; j++) {
                const uint32_t *sp = &split[(size_t)j * (size_t)(G + 1) + (size_t)g];
                const int64_t c0 = ptr[src(j)];
                const int32_t *q = idx + c0;
                const double *v = val + c0;
                for (uint32_t u = sp[0]; u < sp[1]; u++) {
                    const int64_t o = cur[(size_t)(q[u] - lo)]++;
                    tidx[o] = (int32_t)(j - idx_offset);
                    tval[o] = v[u];
                }
            }
        }
    }, T);
    tptr[ninner] = t - s;
    if (tt) fprintf(stderr, "  transpose: T %d, G %lld, after the split table %.4f s, ranges %.4f s\n", T, (long long)G,
                    std::chrono::duration<double>(t_a - t_0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_a).count());
}

// the two pairs of vector types in use: the ingestion by rows, and the row-major copies (this file's and layout.cpp's)
template void transpose_compressed(int64_t, int64_t, const int64_t *, const int32_t *, const double *, int32_t, std::vector<int64_t> &,
                                   std::vector<int32_t> &, std::vector<double> &, const int32_t *);
template void transpose_compressed(int64_t, int64_t, const int64_t *, const int32_t *, const double *, int32_t, std::vector<int64_t> &,
                                   BigVec<int32_t> &, BigVec<double> &, const int32_t *);

static int matrix_from_csr(int64_t n, int64_t m, const int32_t *p, const int32_t *j, const double *x, Matrix &X)
{
    std::vector<int64_t> rptr;
    std::vector<int32_t> ridx;
    std::vector<double> rval;
    int rc = canonicalise(n, m, p, j, x, rptr, ridx, rval);
    if (rc) return rc;
    X.n = n; X.m = m;
    transpose_compressed(n, m, rptr.data(), ridx.data(), rval.data(), 0, X.colptr, X.row, X.val, nullptr);
    finish_matrix(X);
    return VBNMF_OK;
}

// Sum over the stored entries of columns [cb, ce) of f(x).  Per-column sums are formed independently and then added in
// column order, so the value does not depend on the host thread count.  Small integer counts go through a table of f.
template <class F>
static double sum_over_entries(const Matrix &X, int64_t cb, int64_t ce, F f)
{
    std::vector<double> table;
    if (X.counts_u16) {
        table.resize((size_t)X.max_val + 1);                // (the matrix's maximum bounds every column range's)
        for (size_t c = 0; c < table.size(); c++) table[c] = f((double)c);
    }
    std::vector<double> colsum(ce - cb, 0.0);
    parallel_for(ce - cb, [&](int64_t b, int64_t e, int) {
        for (int64_t j = b; j < e; j++) {
            double s = 0.0;
            for (int64_t q = X.colptr[cb + j]; q < X.colptr[cb + j + 1]; q++)
                s += X.counts_u16 ? table[(size_t)X.val[q]] : f(X.val[q]);
            colsum[j] = s;
        }
    });
    double s = 0.0;
    for (double v : colsum) s += v;
    return s;
}

// sum_ij lgamma(X_ij + 1) over stored entries (absent entries give lgamma(1) = 0): the
// iteration-invariant part of reference src/vbnmf_update.cpp:80-81.
double sum_lgamma_x1(const Matrix &X, int64_t cb, int64_t ce)
{
    return sum_over_entries(X, cb, ce, [](double v) { return std::lgamma(v + 1.0); });
}

// sum over stored entries of -x log x + x (reference R/factorize.R:46-47), columns [cb, ce), fixed order.
double sum_xlogx(const Matrix &X, int64_t cb, int64_t ce)
{
    return sum_over_entries(X, cb, ce, [](double v) { return v > 0.0 ? -v * std::log(v) + v : 0.0; });
}

int gene_mode_host(int64_t m, int64_t len, const double *values)
{
    std::vector<double> v(values, values + len);
    std::sort(v.begin(), v.end());
    const int64_t zeros = m - len;
    int64_t prev = 0;                                    // occurrences of the level before (0: there is none yet)
    bool zero_done = zeros <= 0;
    for (int64_t q = 0; q < len;) {
        if (!zero_done && v[q] > 0.0) {                  // the zeros' level sits between the negative and the positive values
            if (prev && prev < zeros) return 1;
            prev = zeros;
            zero_done = true;
        }
        int64_t e = q + 1;
        while (e < len && v[e] == v[q]) e++;
        if (prev && prev < e - q) return 1;
        prev = e - q;
        q = e;
    }
    if (!zero_done && prev && prev < zeros) return 1;    // (every stored value negative)
    return 0;
}

int check_dims(int64_t n, int64_t m)
{
    if (n <= 0 || m <= 0) return fail(VBNMF_ERR_BAD_ARG, "matrix dimensions must be positive (got %lld x %lld)", (long long)n, (long long)m);
    if (n > 0x7FFFFFFFLL - 64 || m > 0x7FFFFFFFLL - 64) return fail(VBNMF_ERR_BAD_ARG, "a matrix dimension exceeds 2^31-65");
    return VBNMF_OK;
}

}  // namespace vbnmf

// ====================================================================== C ABI (host-only part)
using namespace vbnmf;

extern "C" {

const char *vbnmf_last_error(void) { return vbnmf::last_error_cstr(); }
const char *vbnmf_version(void) { return "0.1.0"; }

}  // extern "C"

int vbnmf::new_matrix(vbnmf_matrix **out, const std::function<int(Matrix &)> &fill)
{
    if (!out) return fail(VBNMF_ERR_BAD_ARG, "out pointer is NULL");
    *out = nullptr;
    vbnmf_matrix *X = nullptr;
    try {
        X = new vbnmf_matrix();
        int rc = fill(X->M);
        if (rc) { delete X; return rc; }
        X->lgx = sum_lgamma_x1(X->M, 0, X->M.m);
    } catch (const std::bad_alloc &) {
        delete X;
        return fail(VBNMF_ERR_OOM, "out of host memory ingesting X");
    } catch (const std::exception &ex) {
        delete X;
        return fail(VBNMF_ERR_BAD_ARG, "ingesting X failed: %s", ex.what());
    }
    *out = X;
    return VBNMF_OK;
}

extern "C" {

int vbnmf_matrix_from_dense(int64_t n, int64_t m, const double *A, vbnmf_matrix **out)
{
    if (int rc = check_dims(n, m)) return rc;
    if (!A) return fail(VBNMF_ERR_BAD_ARG, "X is NULL");
    return new_matrix(out, [&](Matrix &M) { return matrix_from_dense(n, m, A, M); });
}

int vbnmf_matrix_from_csc(int64_t n, int64_t m, const int32_t *p, const int32_t *i, const double *x, vbnmf_matrix **out)
{
    if (int rc = check_dims(n, m)) return rc;
    if (!p || ((!i || !x) && p[m] > 0)) return fail(VBNMF_ERR_BAD_ARG, "a CSC slot pointer is NULL");
    return new_matrix(out, [&](Matrix &M) { return matrix_from_csc(n, m, p, i, x, M); });
}

int vbnmf_matrix_from_csr(int64_t n, int64_t m, const int32_t *p, const int32_t *j, const double *x, vbnmf_matrix **out)
{
    if (int rc = check_dims(n, m)) return rc;
    if (!p || ((!j || !x) && p[n] > 0)) return fail(VBNMF_ERR_BAD_ARG, "a CSR slot pointer is NULL");
    return new_matrix(out, [&](Matrix &M) { return matrix_from_csr(n, m, p, j, x, M); });
}

int vbnmf_matrix_info(const vbnmf_matrix *X, int64_t *n, int64_t *m, int64_t *nnz, double *lgx)
{
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (n) *n = X->M.n;
    if (m) *m = X->M.m;
    if (nnz) *nnz = X->M.nnz;
    if (lgx) *lgx = X->lgx;
    return VBNMF_OK;
}

int vbnmf_matrix_empty_counts(const vbnmf_matrix *X, int64_t *empty_rows, int64_t *empty_cols)
{
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (X->M.shell) return fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries");
    const Matrix &M = X->M;
    // rowSums(mat)==0 / colSums(mat)==0 of reference R/bayesian.R:244-245 (sums, not stored-entry counts).  Columns are
    // cut in chunks with their own row-sum arrays, added in chunk order (a fixed order: the test for == 0 must not
    // depend on the thread count); 0.15 s single-threaded at the headline size, once per vb_factorize call.
    int T = (int)std::max<int64_t>(1, std::min<int64_t>(64, M.nnz / (1 << 20) + 1));       // chunks: a function of X alone
    T = (int)std::max<int64_t>(1, std::min<int64_t>(T, ((int64_t)1 << 24) / std::max<int64_t>(1, M.n)));   // <= 128 MB of row sums in all
    std::vector<std::vector<double>> part(T);
    std::vector<int64_t> ecs(T, 0);
    // allocated HERE, where a failure is reported with its size: parallel_for would carry a worker's bad_alloc back to this
    // thread, and nothing in this entry catches it
    try {
        for (auto &rs : part) rs.assign(M.n, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory checking for empty rows (%d x %lld doubles)", T, (long long)M.n);
    }
    parallel_for(T, [&](int64_t b, int64_t e, int) {
        for (int64_t c = b; c < e; c++) {
            std::vector<double> &rs = part[c];
            for (int64_t j = M.m * c / T; j < M.m * (c + 1) / T; j++) {
                double cs = 0.0;
                for (int64_t q = M.colptr[j]; q < M.colptr[j + 1]; q++) { cs += M.val[q]; rs[M.row[q]] += M.val[q]; }
                ecs[c] += (cs == 0.0);
            }
        }
    });
    int64_t ec = 0, er = 0;
    for (int c = 0; c < T; c++) ec += ecs[c];
    for (int64_t i = 0; i < M.n; i++) {
        double v = 0.0;
        for (int c = 0; c < T; c++) v += part[c][i];
        er += (v == 0.0);
    }
    if (empty_rows) *empty_rows = er;
    if (empty_cols) *empty_cols = ec;
    return VBNMF_OK;
}

int vbnmf_matrix_col_sums(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, double *sums)
{
    if (!X || !sums) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (X->M.shell) return fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries");
    const Matrix &M = X->M;
    if (col_begin < 0 || col_end > M.m || col_begin > col_end)
        return fail(VBNMF_ERR_BAD_ARG, "column range [%lld, %lld) is outside the matrix's %lld columns", (long long)col_begin,
                    (long long)col_end, (long long)M.m);
    // Matrix::colSums (R/utils.R:81, :321): a sequential sum down each stored column, rows ascending
    parallel_for(col_end - col_begin, [&](int64_t b, int64_t e, int) {
        for (int64_t j = col_begin + b; j < col_begin + e; j++) {
            double s = 0.0;
            for (int64_t q = M.colptr[j]; q < M.colptr[j + 1]; q++) s += M.val[q];
            sums[j - col_begin] = s;
        }
    });
    return VBNMF_OK;
}

int vbnmf_test_gene_mode_host(int64_t m, int64_t len, const double *values, int32_t *out)
{
    if (!out || (!values && len > 0)) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (len < 0 || len > m) return fail(VBNMF_ERR_BAD_ARG, "a row of %lld cells cannot hold %lld stored values", (long long)m, (long long)len);
    try {
        *out = gene_mode_host(m, len, values);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory sorting a row of %lld values", (long long)len);
    }
    return VBNMF_OK;
}

void vbnmf_matrix_destroy(vbnmf_matrix *X) { delete X; }

int32_t vbnmf_padded_rank(int32_t r) { return (r < 1 || r > VBNMF_MAX_RANK) ? 0 : padded_rank(r); }
int32_t vbnmf_host_threads(void) { return host_threads(); }
int32_t vbnmf_set_host_threads(int32_t n)
{
    const int32_t before = host_threads();
    set_host_threads_override(n);
    return before;
}

}  // extern "C"
