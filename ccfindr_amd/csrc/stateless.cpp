// stateless.cpp -- the stateless forms of the C ABI (vbnmf_update_*, vbnmf_ml_update_*): one step on a matrix handed in with
// every call, behind a cache keyed by the matrix's content.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"

using namespace vbnmf;

namespace {

// The reference's caller hands the SAME X to every one of its thousands of calls (R/bayesian.R:339).  The stateless
// entries therefore keep the last ingested matrix and its engine alive, keyed by the CONTENT of X (dimensions + a
// 64-bit hash of every byte of the arrays handed in, formed by all host threads): a call with an X seen before costs
// the hash, the state upload, one step and the state download instead of ingestion + two layouts + an engine.
// VBNMF_STATELESS_CACHE=0 turns it off; vbnmf_stateless_cache_clear() releases what is held.
struct StatelessCache {
    std::mutex mu;                    // held for the whole call: stateless calls are serialised
    bool valid = false;
    int kind = 0;                     // 0 dense, 1 csc
    int64_t n = 0, m = 0, nnz = 0;
    uint64_t hash = 0, hash2 = 0;     // two independently seeded 64-bit hashes of the content: a 128-bit key
    std::vector<int32_t> colptr;      // csc: a copy of the pointer array, compared on a hit (not only hashed)
    std::vector<double> sample;       // dense: a strided sample of X (<= 4096 values), compared on a hit as well
    vbnmf_matrix *X = nullptr;
    vbnmf_engine *e = nullptr;
    int r = 0, device = 0;            // the engine's rank and device
    void drop()
    {
        vbnmf_engine_destroy(e); e = nullptr;
        vbnmf_matrix_destroy(X); X = nullptr;
        valid = false;
        colptr.clear();
        sample.clear();
    }
};
StatelessCache &stateless_cache() { static StatelessCache c; return c; }

// Two independently seeded hashes of the same bytes in ONE pass over them (the stateless cache's 128-bit key).  Per 4 MB chunk
// FOUR multiply-xorshift chains per seed, fed the chunk's 8-byte words in turn (word q goes to chain q mod 4), so eight independent
// chains are in flight and a thread hashes at memory speed instead of at one multiply latency per word (a 3.7 MB dense matrix
// -- the reference's shipped data set -- used to take 0.7 ms of every literal drop-in call); chains and chunks are combined in
// order: the value does not depend on the thread count.  The seed starts EVERY chain of every chunk (not only the final combine),
// so two seeds give two INDEPENDENT 64-bit hashes: contents that collide in a chain under one seed do not under the other
// (tests/test_node_shared_cpu.py).  Small inputs are hashed by few threads (a thread is worth starting for a chunk or more).
void hash_bytes2(const void *data, size_t bytes, uint64_t seed_a, uint64_t seed_b, uint64_t &out_a, uint64_t &out_b)
{
    const size_t chunk = (size_t)1 << 22;
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    std::vector<uint64_t> part_a(nchunks ? nchunks : 1, 0), part_b(nchunks ? nchunks : 1, 0);
    const unsigned char *p = static_cast<const unsigned char *>(data);
    constexpr uint64_t K = 0xFF51AFD7ED558CCDull, KL = 0xA24BAED4963EE407ull, KC = 0xC4CEB9FE1A85EC53ull;
    parallel_for((int64_t)nchunks, [&](int64_t b, int64_t e, int) {
        for (int64_t c = b; c < e; c++) {
            const size_t o = (size_t)c * chunk, len = std::min(chunk, bytes - o);
            const uint64_t salt = 0x9E3779B97F4A7C15ull ^ ((uint64_t)c * 0xD6E8FEB86659FD93ull);
            uint64_t ha[4], hb[4];
            for (int j = 0; j < 4; j++) { ha[j] = seed_a ^ salt ^ ((uint64_t)j * KL); hb[j] = seed_b ^ salt ^ ((uint64_t)j * KL); }
            size_t q = 0;
            for (; q + 32 <= len; q += 32) {
                uint64_t w[4];
                std::memcpy(w, p + o + q, 32);
                for (int j = 0; j < 4; j++) {
                    ha[j] = (ha[j] ^ w[j]) * K; hb[j] = (hb[j] ^ w[j]) * K;
                    ha[j] ^= ha[j] >> 32; hb[j] ^= hb[j] >> 32;
                }
            }
            for (int j = 0; q + 8 <= len; q += 8, j++) {
                uint64_t w;
                std::memcpy(&w, p + o + q, 8);
                ha[j] = (ha[j] ^ w) * K; hb[j] = (hb[j] ^ w) * K;
                ha[j] ^= ha[j] >> 32; hb[j] ^= hb[j] >> 32;
            }
            for (; q < len; q++) { ha[0] = (ha[0] ^ p[o + q]) * 0x100000001B3ull; hb[0] = (hb[0] ^ p[o + q]) * 0x100000001B3ull; }
            uint64_t da = ha[0], db = hb[0];
            for (int j = 1; j < 4; j++) { da = (da ^ ha[j]) * KC; da ^= da >> 29; db = (db ^ hb[j]) * KC; db ^= db >> 29; }
            part_a[c] = da; part_b[c] = db;
        }
    });
    uint64_t ha = seed_a, hb = seed_b;
    for (uint64_t v : part_a) { ha = (ha ^ v) * KC; ha ^= ha >> 29; }
    for (uint64_t v : part_b) { hb = (hb ^ v) * KC; hb ^= hb >> 29; }
    out_a = ha; out_b = hb;
}
uint64_t hash_bytes(const void *data, size_t bytes, uint64_t seed)
{
    uint64_t a, b;
    hash_bytes2(data, bytes, seed, ~seed, a, b);
    return a;
}

bool stateless_cache_enabled()
{
    const char *sv = getenv("VBNMF_STATELESS_CACHE");
    return !(sv && sv[0] == '0');
}

// The engine of rank r on the matrix with this key: from the cache, or ingested now through `ingest`.
int stateless_engine(int kind, int64_t n, int64_t m, int64_t nnz, uint64_t hash, uint64_t hash2, const int32_t *colptr, const double *dense, int32_t r,
                     const std::function<int(vbnmf_matrix **)> &ingest, vbnmf_engine **out)
{
    StatelessCache &C = stateless_cache();
    bool hit = C.valid && C.kind == kind && C.n == n && C.m == m && C.nnz == nnz && C.hash == hash && C.hash2 == hash2;
    if (hit && colptr) hit = C.colptr.size() == (size_t)m + 1 && std::memcmp(C.colptr.data(), colptr, ((size_t)m + 1) * sizeof(int32_t)) == 0;
    // dense: every 1/4096-th value (an odd stride, so the sample walks through all rows) beside the two hashes
    const size_t total = dense ? (size_t)n * (size_t)m : 0, stride = std::max<size_t>(1, total / 4096) | 1;
    if (hit && dense) {
        size_t q = 0;
        for (size_t o = 0; o < total && hit; o += stride, q++) hit = q < C.sample.size() && std::memcmp(&C.sample[q], dense + o, sizeof(double)) == 0;
        hit = hit && q == C.sample.size();
    }
    if (!hit) {
        C.drop();
        if (int rc = ingest(&C.X)) { C.X = nullptr; return rc; }
        C.kind = kind; C.n = n; C.m = m; C.nnz = nnz; C.hash = hash; C.hash2 = hash2; C.valid = true;
        if (colptr) C.colptr.assign(colptr, colptr + m + 1);
        if (dense) for (size_t o = 0; o < total; o += stride) C.sample.push_back(dense[o]);
    }
    // The stateless entries take no device argument (the reference's signature has none): VBNMF_DEVICE names it, read at
    // every call, so the slaves of Rmpi::mpi.applyLB (reference R/bayesian.R:262-263) that call the plain shim can each be
    // given their own GPU; default device 0.
    int device = 0;
    if (const char *dv = getenv("VBNMF_DEVICE")) device = atoi(dv);
    if (!C.e || C.r != r || C.device != device) {
        vbnmf_engine_destroy(C.e); C.e = nullptr;
        if (int rc = vbnmf_engine_create(C.X, r, device, &C.e)) { C.e = nullptr; return rc; }
        C.r = r; C.device = device;
    }
    *out = C.e;
    return VBNMF_OK;
}

int update_once(vbnmf_engine *e, const double *lw_in, const double *lh_in, const double *eh_in,
                double aw, double bw, double ah, double bh, double fudge,
                double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    int rc = vbnmf_engine_set_state(e, lw_in, lh_in, eh_in);
    if (!rc) rc = vbnmf_engine_step(e, aw, bw, ah, bh, fudge, lkh, nullptr);
    if (!rc) rc = vbnmf_engine_get_state(e, lw, lh, ew, eh, dw, dh);
    return rc;
}

int ml_update_once(vbnmf_engine *e, const double *w_in, const double *h_in, int32_t prior, double gamma_a, double gamma_b,
                   double *w, double *h, double *lk)
{
    int rc = vbnmf_engine_ml_set_state(e, w_in, h_in);
    if (!rc) rc = vbnmf_engine_ml_step(e, prior, gamma_a, gamma_b, lk);
    if (!rc) rc = vbnmf_engine_ml_get_state(e, w, h);
    return rc;
}

// dense / CSC front ends shared by the VB and ML stateless calls: `use(engine)` runs under the cache's lock
int with_dense(int64_t n, int64_t m, int32_t r, const double *X, const std::function<int(vbnmf_engine *)> &use)
{
    if (n <= 0 || m <= 0 || !X) return fail(VBNMF_ERR_BAD_ARG, "X is NULL or has a non-positive dimension");
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    const bool cache = stateless_cache_enabled();
    uint64_t h = 0, h2 = 0;
    if (cache) hash_bytes2(X, (size_t)n * (size_t)m * sizeof(double), 0x64656E7365ull, 0x3243F6A8885A308Dull, h, h2);
    if (!cache) C.drop();
    vbnmf_engine *e = nullptr;
    int rc = stateless_engine(0, n, m, 0, h, h2, nullptr, X, r, [&](vbnmf_matrix **M) { return vbnmf_matrix_from_dense(n, m, X, M); }, &e);
    if (!rc) rc = use(e);
    if (!cache || rc) C.drop();
    return rc;
}

int with_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
             const std::function<int(vbnmf_engine *)> &use)
{
    if (n <= 0 || m <= 0 || !p) return fail(VBNMF_ERR_BAD_ARG, "a CSC slot pointer is NULL or a dimension is non-positive");
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    const bool cache = stateless_cache_enabled();
    // the pointer array is checked BEFORE anything is read through it (the hash below walks nnz elements of i and x)
    if (p[0] != 0) return fail(VBNMF_ERR_BAD_ARG, "pointer array must start at 0");
    for (int64_t j = 0; j < m; j++)
        if (p[j + 1] < p[j]) return fail(VBNMF_ERR_BAD_ARG, "pointer array is not non-decreasing at %lld", (long long)j);
    const int64_t nnz = p[m];
    if (nnz > 0 && (!i || !x)) return fail(VBNMF_ERR_BAD_ARG, "a CSC slot pointer is NULL");
    uint64_t h = 0, h2 = 0;
    if (cache) {
        hash_bytes2(i, (size_t)nnz * sizeof(int32_t), 0x637363ull, 0x3243F6A8885A308Dull, h, h2);
        hash_bytes2(x, (size_t)nnz * sizeof(double), h, h2, h, h2);
    }
    if (!cache) C.drop();
    vbnmf_engine *e = nullptr;
    int rc = stateless_engine(1, n, m, nnz, h, h2, p, nullptr, r, [&](vbnmf_matrix **M) { return vbnmf_matrix_from_csc(n, m, p, i, x, M); }, &e);
    if (!rc) rc = use(e);
    if (!cache || rc) C.drop();
    return rc;
}

}  // namespace

extern "C" {

// Test hook (no device needed): the content hash of the stateless cache, for tests/test_cabi_symbols.py.
uint64_t vbnmf_test_hash_bytes(const void *data, int64_t bytes, uint64_t seed) { return (data && bytes >= 0) ? hash_bytes(data, (size_t)bytes, seed) : 0; }

void vbnmf_stateless_cache_clear(void)
{
    StatelessCache &C = stateless_cache();
    std::lock_guard<std::mutex> g(C.mu);
    C.drop();
}

int vbnmf_update_dense(int64_t n, int64_t m, int32_t r, const double *X, const double *lw_in, const double *lh_in,
                       const double *eh_in, double aw, double bw, double ah, double bh, double fudge,
                       double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    if (!lw_in || !lh_in || !eh_in) return fail(VBNMF_ERR_BAD_ARG, "a wh member is NULL");
    return with_dense(n, m, r, X, [&](vbnmf_engine *e) {
        return update_once(e, lw_in, lh_in, eh_in, aw, bw, ah, bh, fudge, lw, lh, ew, eh, dw, dh, lkh); });
}

int vbnmf_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
                     const double *lw_in, const double *lh_in, const double *eh_in,
                     double aw, double bw, double ah, double bh, double fudge,
                     double *lw, double *lh, double *ew, double *eh, double *dw, double *dh, double *lkh)
{
    if (!lw_in || !lh_in || !eh_in) return fail(VBNMF_ERR_BAD_ARG, "a wh member is NULL");
    return with_csc(n, m, r, p, i, x, [&](vbnmf_engine *e) {
        return update_once(e, lw_in, lh_in, eh_in, aw, bw, ah, bh, fudge, lw, lh, ew, eh, dw, dh, lkh); });
}

int vbnmf_ml_update_dense(int64_t n, int64_t m, int32_t r, const double *X, const double *w_in, const double *h_in,
                          int32_t prior, double gamma_a, double gamma_b, double *w, double *h, double *lk)
{
    if (!w_in || !h_in) return fail(VBNMF_ERR_BAD_ARG, "w or h is NULL");
    return with_dense(n, m, r, X, [&](vbnmf_engine *e) { return ml_update_once(e, w_in, h_in, prior, gamma_a, gamma_b, w, h, lk); });
}

int vbnmf_ml_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i, const double *x,
                        const double *w_in, const double *h_in, int32_t prior, double gamma_a, double gamma_b,
                        double *w, double *h, double *lk)
{
    if (!w_in || !h_in) return fail(VBNMF_ERR_BAD_ARG, "w or h is NULL");
    return with_csc(n, m, r, p, i, x, [&](vbnmf_engine *e) { return ml_update_once(e, w_in, h_in, prior, gamma_a, gamma_b, w, h, lk); });
}

}  // extern "C"
