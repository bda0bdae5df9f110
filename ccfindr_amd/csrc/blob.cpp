// blob.cpp -- node-shared layouts (one build per node, not per process): matrix shells, the layout blob, its export / import
// through a caller's buffer and its share / attach through a file in the node's shared memory.  Host code only.
//
// The reference ships the whole `bundle` -- the matrix included -- to every MPI slave (reference R/bayesian.R:252-263) and
// every slave densifies it again per iteration.  Here the processes of one node (one per GPU) share ONE ingestion and
// ONE pair of tiled layouts: the process that holds X exports a layout as a flat blob (into shared memory the caller
// maps), the others import it into a matrix SHELL -- a handle with X's metadata and no entries -- and upload it to their
// own GPU.  Blob = header (int64 words) + the layout's arrays, each 64-byte aligned, + a closing magic word.
#include "common.h"

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <fcntl.h>
#include <new>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/statvfs.h>
#include <system_error>
#include <unistd.h>

using namespace vbnmf;

namespace {

constexpr int64_t kBlobMagic = 0x56424E4D464C5930LL;      // "VBNMFLY0"
constexpr int64_t kBlobVersion = 3;                       // 3: the row index (row_ptr / row_task, n_rows, merge)
constexpr int kBlobHeaderWords = 56;
constexpr int kBlobArrays = 17;

// THE table of the blob's arrays, in blob order: whoever writes, sizes or reads a blob walks it through here.  The three
// ExtVec members are the big ones (the entry stream), which may live inside a mapping instead of the library's memory.
template <class LayoutT, class F>
void for_each_blob_array(LayoutT &L, F &&f)
{
    f(L.task_major); f(L.slice_width); f(L.slice_off); f(L.slice_block); f(L.slice_fast); f(L.block_start);
    f(L.seg_block); f(L.wg_seg0); f(L.seg_ptr); f(L.inv_ptr); f(L.inv_task);
    f(L.packed); f(L.wide_idx); f(L.wide_val);
    f(L.cell_perm);
    f(L.row_ptr); f(L.row_task);
}

struct BlobArray { const void *src; int64_t bytes; int64_t off; };

inline int64_t align64(int64_t v) { return (v + 63) & ~(int64_t)63; }

template <class V> int64_t vec_bytes(const V &v) { return (int64_t)v.size() * (int64_t)sizeof(typename V::value_type); }

// the arrays of a layout in blob order (pointers valid while L is; offsets from blob_size)
void blob_arrays(const Layout &L, BlobArray (&a)[kBlobArrays])
{
    int q = 0;
    for_each_blob_array(L, [&](const auto &v) { a[q++] = {v.data(), vec_bytes(v), 0}; });
}

// gives every array its offset inside the blob; returns the size of the whole blob
int64_t blob_size(BlobArray (&a)[kBlobArrays])
{
    int64_t off = kBlobHeaderWords * 8;
    for (int q = 0; q < kBlobArrays; q++) { off = align64(off); a[q].off = off; off += a[q].bytes; }
    return align64(off) + 8;
}

void parallel_copy(void *dst, const void *src, int64_t bytes)
{
    const int64_t chunk = (int64_t)4 << 20;
    const int64_t nchunks = (bytes + chunk - 1) / chunk;
    parallel_for(nchunks, [&](int64_t b, int64_t e, int) {
        for (int64_t c = b; c < e; c++) {
            const int64_t o = c * chunk, len = std::min(chunk, bytes - o);
            std::memcpy(static_cast<char *>(dst) + o, static_cast<const char *>(src) + o, (size_t)len);
        }
    });
}

void write_blob_header(int64_t *h, const Layout &L, const LayoutParams &lp, const vbnmf_matrix *X, int64_t total, const BlobArray (&a)[kBlobArrays])
{
    std::memset(h, 0, kBlobHeaderWords * 8);
    h[0] = kBlobMagic; h[1] = kBlobVersion; h[2] = total;
    h[3] = L.side; h[4] = L.wide ? 1 : 0; h[5] = L.n_major; h[6] = L.n_minor; h[7] = L.block_width; h[8] = L.n_blocks;
    h[9] = L.max_len; h[10] = L.n_wg; h[11] = L.row_slots; h[12] = L.n_tasks; h[13] = L.n_slices; h[14] = L.n_slots;
    h[15] = L.n_segs; h[16] = L.nnz;
    h[17] = lp.block_width; h[18] = lp.block_cap; h[19] = lp.max_len; h[20] = lp.n_wg; h[21] = lp.row_slots;
    h[22] = X->M.n; h[23] = X->M.m; h[24] = X->M.nnz;
    h[25] = L.n_rows; h[26] = L.merge ? 1 : 0; h[27] = lp.merge;
    for (int q = 0; q < kBlobArrays; q++) h[32 + q] = a[q].bytes;
}

// The whole blob of L into buf (blob_size bytes, all host threads): header, the arrays -- except those that live at their
// place in buf already (the big arrays of a layout that was built into this very mapping) -- and the closing word.
void write_blob(void *buf, const Layout &L, const LayoutParams &lp, const vbnmf_matrix *X)
{
    BlobArray a[kBlobArrays];
    blob_arrays(L, a);
    const int64_t total = blob_size(a);
    char *b = static_cast<char *>(buf);
    write_blob_header(reinterpret_cast<int64_t *>(b), L, lp, X, total, a);
    for (int q = 0; q < kBlobArrays; q++)
        if (a[q].src != b + a[q].off) parallel_copy(b + a[q].off, a[q].src, a[q].bytes);
    std::memcpy(b + total - 8, &kBlobMagic, 8);
}

// geometry of the whole-matrix layout of `side` that an engine of rank `geometry_rank` with n_wg workgroups uses
LayoutParams whole_matrix_params(const vbnmf_matrix *X, int side, int geometry_rank, int n_wg)
{
    const int R = padded_rank(geometry_rank);
    const int64_t nmaj = side == 0 ? X->M.n : X->M.m, nmin = side == 0 ? X->M.m : X->M.n;
    return default_layout_params(nmaj, nmin, R, n_wg, X->M.nnz);
}

struct ShmMap {
    void *base = nullptr;
    size_t bytes = 0;
    ~ShmMap() { if (base) munmap(base, bytes); }
};

// Creates path + ".part" (it must not exist), `bytes` long, mapped read-write.  A blob is built under that name and renamed
// when complete (publish_part), so a peer that sees `path` sees all of it.
int create_part(const std::string &path, int64_t bytes, std::shared_ptr<ShmMap> &map)
{
    {   // a memory file system that is full answers the WRITES with SIGBUS, not the ftruncate with an error: ask first
        std::string dir = path.substr(0, path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/'));
        if (dir.empty()) dir = ".";
        struct statvfs vs;
        if (statvfs(dir.c_str(), &vs) == 0 && (double)vs.f_bavail * (double)vs.f_frsize < (double)bytes)
            return fail(VBNMF_ERR_OOM, "%s has %.0f MB free, the layout needs %.0f MB", dir.c_str(),
                        (double)vs.f_bavail * (double)vs.f_frsize / 1e6, (double)bytes / 1e6);
    }
    const std::string part = path + ".part";
    const int fd = open(part.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) return fail(VBNMF_ERR_BAD_ARG, "cannot create %s: %s", part.c_str(), strerror(errno));
    if (ftruncate(fd, (off_t)bytes) != 0) { close(fd); unlink(part.c_str()); return fail(VBNMF_ERR_OOM, "cannot size %s to %lld bytes: %s", part.c_str(), (long long)bytes, strerror(errno)); }
    void *base = mmap(nullptr, (size_t)bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { unlink(part.c_str()); return fail(VBNMF_ERR_OOM, "cannot map %s: %s", part.c_str(), strerror(errno)); }
    map = std::make_shared<ShmMap>();
    map->base = base; map->bytes = (size_t)bytes;
    return VBNMF_OK;
}

int publish_part(const std::string &path)
{
    const std::string part = path + ".part";
    if (rename(part.c_str(), path.c_str()) != 0) { unlink(part.c_str()); return fail(VBNMF_ERR_BAD_ARG, "cannot rename %s: %s", part.c_str(), strerror(errno)); }
    return VBNMF_OK;
}

// The sink of vbnmf_matrix_share_layout: at the point where build_layout knows every size, create `path`.part with the
// whole blob's size and hand the layout its big arrays INSIDE the mapping.
struct ShmSink : LayoutSink {
    std::string path;
    std::shared_ptr<ShmMap> map;
    template <class T> static int64_t planned_bytes(const Layout &L, const ExtVec<T> &v)       // (not allocated yet: from n_slots)
    {
        const bool used = (static_cast<const void *>(&v) == static_cast<const void *>(&L.packed)) != L.wide;
        return used ? L.n_slots * (int64_t)sizeof(T) : 0;
    }
    template <class V> static int64_t planned_bytes(const Layout &, const V &v) { return vec_bytes(v); }
    template <class T> void adopt(ExtVec<T> &v, const BlobArray &a) { if (a.bytes) v.adopt(reinterpret_cast<T *>(static_cast<char *>(map->base) + a.off), (size_t)(a.bytes / (int64_t)sizeof(T)), map); }
    template <class V> void adopt(V &, const BlobArray &) {}
    int place(Layout &L) override
    {
        BlobArray a[kBlobArrays];
        int q = 0;
        for_each_blob_array(L, [&](const auto &v) { a[q++] = {nullptr, planned_bytes(L, v), 0}; });
        if (int rc = create_part(path, blob_size(a), map)) return rc;
        q = 0;
        for_each_blob_array(L, [&](auto &v) { adopt(v, a[q++]); });
        return VBNMF_OK;
    }
};

template <class T>
bool adopt_in_place(ExtVec<T> &v, const char *src, size_t count, const std::shared_ptr<void> &keep)
{
    if (!keep) return false;
    v.adopt(reinterpret_cast<T *>(const_cast<char *>(src)), count, keep);
    return true;
}
template <class V> bool adopt_in_place(V &, const char *, size_t, const std::shared_ptr<void> &) { return false; }

// A blob is outside input: what the header says and what the small arrays hold must be safe to index device memory by.
// Returns 0 or the error (message set).
int validate_layout(const Layout &L, const vbnmf_matrix *X)
{
    // the scalar fields must agree with the arrays they describe (the kernels index by them)
    const bool ok = (int64_t)L.task_major.size() == L.n_slices * kLanes && (int64_t)L.slice_width.size() == L.n_slices &&
                    (int64_t)L.slice_off.size() == L.n_slices && (int64_t)L.slice_fast.size() == L.n_slices &&
                    (int64_t)L.block_start.size() == (int64_t)L.n_blocks + 1 && (int64_t)L.seg_block.size() == L.n_segs &&
                    (int64_t)L.wg_seg0.size() == (int64_t)L.n_wg + 1 && (int64_t)L.seg_ptr.size() == L.n_segs + 1 &&
                    (int64_t)L.inv_ptr.size() == L.n_major + 1 && (int64_t)L.inv_task.size() == L.n_tasks &&
                    (int64_t)L.row_ptr.size() == L.n_major + 1 && (int64_t)L.row_task.size() == L.n_rows && L.n_rows <= L.n_tasks &&
                    (L.wide ? ((int64_t)L.wide_idx.size() == L.n_slots && (int64_t)L.wide_val.size() == L.n_slots)
                             : (int64_t)L.packed.size() == L.n_slots) &&
                    L.n_major == (L.side == 0 ? X->M.n : X->M.m) && L.n_minor == (L.side == 0 ? X->M.m : X->M.n) &&
                    L.wide == !X->M.counts_int;
    if (!ok) return fail(VBNMF_ERR_BAD_ARG, "layout blob: header and arrays disagree");
    // ... and the CONTENTS of the small arrays are what the kernels index device memory by: a blob from another build with
    // the same version word, or a half-overwritten mapping, must be an error here, not an out-of-bounds access on the GPU.
    // (The entry stream itself addresses LDS rows only: its offsets are masked to the staged block.)
    const char *bad = nullptr;
    const int64_t nsl = L.n_slices, nseg = L.n_segs;
    if (L.n_blocks < 1 || L.n_wg < 1 || L.row_slots < 1 || !(L.row_slots & 1) || L.max_len < 4 || L.block_width < 1) bad = "geometry";
    for (int64_t q = 0; !bad && q < nsl; q++) {
        const int64_t w = L.slice_width[q], o = L.slice_off[q];
        if (w < 4 || (w & 3) || w > L.max_len + 3 || o < 0 || (o & 255) || o + w * kLanes > L.n_slots) bad = "slice_off / slice_width";
        else if ((L.slice_fast[q] & 0xFFFF) > w || ((L.slice_fast[q] >> 16) & 0xFFFF) > w) bad = "slice_fast";
    }
    for (size_t q = 0; !bad && q < L.task_major.size(); q++)
        if (L.task_major[q] != kIdleLane && (int64_t)L.task_major[q] >= L.n_major) bad = "task_major";
    if (!bad && (L.block_start[0] != 0 || L.block_start[L.n_blocks] != L.n_minor)) bad = "block_start";
    for (int q = 0; !bad && q < L.n_blocks; q++) {
        const int64_t w = L.block_start[q + 1] - L.block_start[q];
        if (w < 1 || w > L.block_width) bad = "block_start";
    }
    for (int64_t q = 0; !bad && q < nseg; q++) if (L.seg_block[q] < 0 || L.seg_block[q] >= L.n_blocks) bad = "seg_block";
    if (!bad && (L.seg_ptr[0] != 0 || L.seg_ptr[nseg] != nsl)) bad = "seg_ptr";
    for (int64_t q = 0; !bad && q < nseg; q++) if (L.seg_ptr[q + 1] < L.seg_ptr[q]) bad = "seg_ptr";
    if (!bad && (L.wg_seg0[0] != 0 || L.wg_seg0[L.n_wg] != nseg)) bad = "wg_seg0";
    for (int q = 0; !bad && q < L.n_wg; q++) if (L.wg_seg0[q + 1] < L.wg_seg0[q]) bad = "wg_seg0";
    if (!bad && (L.inv_ptr[0] != 0 || L.inv_ptr[L.n_major] != L.n_tasks)) bad = "inv_ptr";
    for (int64_t q = 0; !bad && q < L.n_major; q++) if (L.inv_ptr[q + 1] < L.inv_ptr[q]) bad = "inv_ptr";
    for (int64_t q = 0; !bad && q < L.n_tasks; q++) if ((int64_t)L.inv_task[q] >= nsl * kLanes) bad = "inv_task";
    if (!bad && (L.row_ptr[0] != 0 || L.row_ptr[L.n_major] != L.n_rows)) bad = "row_ptr";
    for (int64_t q = 0; !bad && q < L.n_major; q++) if (L.row_ptr[q + 1] < L.row_ptr[q]) bad = "row_ptr";
    for (int64_t q = 0; !bad && q < L.n_rows; q++) if ((int64_t)L.row_task[q] >= nsl * kLanes) bad = "row_task";
    if (!bad && !L.merge && (L.row_ptr != L.inv_ptr || L.row_task != L.inv_task)) bad = "row_task";
    if (bad) return fail(VBNMF_ERR_BAD_ARG, "layout blob: the %s array is inconsistent (another build, or a damaged file?)", bad);
    return VBNMF_OK;
}

// Adds the layout in buf[0..bytes) (written by write_blob, this library version) to X's cache.
// keep == null: every array is copied out of the blob; otherwise the big arrays (entry stream) stay where they are --
// inside a mapping that `keep` holds for as long as the layout lives.
int load_blob(const vbnmf_matrix *X, const void *buf, int64_t bytes, std::shared_ptr<void> keep)
{
    if (!X || !buf) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (bytes < kBlobHeaderWords * 8 + 8) return fail(VBNMF_ERR_BAD_ARG, "layout blob is truncated (%lld bytes)", (long long)bytes);
    const int64_t *h = static_cast<const int64_t *>(buf);
    if (h[0] != kBlobMagic || h[1] != kBlobVersion) return fail(VBNMF_ERR_BAD_ARG, "not a layout blob of this library version");
    if (h[2] != bytes) return fail(VBNMF_ERR_BAD_ARG, "layout blob says %lld bytes, %lld were handed in", (long long)h[2], (long long)bytes);
    if (h[22] != X->M.n || h[23] != X->M.m || h[24] != X->M.nnz)
        return fail(VBNMF_ERR_BAD_ARG, "the layout blob was cut from a %lld x %lld matrix with %lld entries, this handle is %lld x %lld with %lld",
                    (long long)h[22], (long long)h[23], (long long)h[24], (long long)X->M.n, (long long)X->M.m, (long long)X->M.nnz);
    if (h[3] != 0 && h[3] != 1) return fail(VBNMF_ERR_BAD_ARG, "layout blob: bad side");
    int64_t off = kBlobHeaderWords * 8;
    for (int q = 0; q < kBlobArrays; q++) {
        if (h[32 + q] < 0) return fail(VBNMF_ERR_BAD_ARG, "layout blob: negative array size");
        off = align64(off) + h[32 + q];
        if (off > bytes) return fail(VBNMF_ERR_BAD_ARG, "layout blob: arrays run past the end");
    }
    off = align64(off);
    int64_t tail = 0;
    if (off + 8 != bytes) return fail(VBNMF_ERR_BAD_ARG, "layout blob: size does not match its array table");
    std::memcpy(&tail, static_cast<const char *>(buf) + off, 8);
    if (tail != kBlobMagic) return fail(VBNMF_ERR_BAD_ARG, "layout blob: closing word missing (a partial write?)");
    try {
        auto L = std::make_shared<Layout>();
        L->side = (int)h[3]; L->wide = h[4] != 0; L->n_major = h[5]; L->n_minor = h[6]; L->block_width = (int32_t)h[7];
        L->n_blocks = (int32_t)h[8]; L->max_len = (int32_t)h[9]; L->n_wg = (int32_t)h[10]; L->row_slots = (int32_t)h[11];
        L->n_tasks = h[12]; L->n_slices = h[13]; L->n_slots = h[14]; L->n_segs = h[15]; L->nnz = h[16];
        L->n_rows = h[25]; L->merge = h[26] != 0;
        LayoutParams lp;
        lp.block_width = (int32_t)h[17]; lp.block_cap = (int32_t)h[18]; lp.max_len = (int32_t)h[19]; lp.n_wg = (int32_t)h[20]; lp.row_slots = (int32_t)h[21];
        lp.merge = (int32_t)h[27];
        int q = 0;
        int64_t o = kBlobHeaderWords * 8;
        int rc = VBNMF_OK;
        for_each_blob_array(*L, [&](auto &v) {                 // copied; a big array is adopted in place when the blob is a kept mapping
            using T = typename std::remove_reference<decltype(v)>::type::value_type;
            o = align64(o);
            const int64_t nb = h[32 + q];
            const char *src = static_cast<const char *>(buf) + o;
            if (nb % (int64_t)sizeof(T)) rc = fail(VBNMF_ERR_BAD_ARG, "layout blob: array %d has a ragged size", q);
            else if (!adopt_in_place(v, src, (size_t)(nb / (int64_t)sizeof(T)), keep)) {
                v.resize((size_t)(nb / (int64_t)sizeof(T)));
                parallel_copy(v.data(), src, nb);
            }
            o += nb; q++;
        });
        if (rc) return rc;
        // the renumbering of the cells: a permutation, and the SAME one for every layout of this matrix (the engine's
        // cell-indexed arrays live in it); a shell adopts the first one it sees
        if (!L->cell_perm.empty()) {
            if ((int64_t)L->cell_perm.size() != X->M.m) return fail(VBNMF_ERR_BAD_ARG, "layout blob: cell order of the wrong length");
            std::vector<char> seen(X->M.m, 0);
            for (int32_t v : L->cell_perm) {
                if (v < 0 || v >= X->M.m || seen[v]) return fail(VBNMF_ERR_BAD_ARG, "layout blob: the cell order is not a permutation");
                seen[v] = 1;
            }
        }
        std::call_once(X->M.order_cache->once, [&] { X->M.order_cache->perm = L->cell_perm; });
        if (X->M.order_cache->perm != L->cell_perm)
            return fail(VBNMF_ERR_BAD_ARG, "layout blob: its cell order differs from the one this matrix handle already uses");
        if (int bad = validate_layout(*L, X)) return bad;
        cache_layout(X, L->side, lp, L);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory importing the layout");
    }
    return VBNMF_OK;
}

}  // namespace

extern "C" {

// meta[8] = n, m, stored entries, counts_int, counts_u16, max value, sum lgamma(x+1), sum(-x log x + x)
int vbnmf_matrix_get_meta(const vbnmf_matrix *X, double *meta)
{
    if (!X || !meta) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (!X->M.shell) std::call_once(X->xlx_once, [&] { X->xlx = sum_xlogx(X->M, 0, X->M.m); });
    meta[0] = (double)X->M.n; meta[1] = (double)X->M.m; meta[2] = (double)X->M.nnz;
    meta[3] = X->M.counts_int ? 1.0 : 0.0; meta[4] = X->M.counts_u16 ? 1.0 : 0.0; meta[5] = X->M.max_val;
    meta[6] = X->lgx; meta[7] = X->xlx;
    return VBNMF_OK;
}

int vbnmf_matrix_shell(const double *meta, vbnmf_matrix **out)
{
    if (!meta || !out) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *out = nullptr;
    const int64_t n = (int64_t)meta[0], m = (int64_t)meta[1], nnz = (int64_t)meta[2];
    if (int rc = check_dims(n, m)) return rc;
    if (nnz < 0) return fail(VBNMF_ERR_BAD_ARG, "negative entry count");
    vbnmf_matrix *X = new (std::nothrow) vbnmf_matrix();
    if (!X) return fail(VBNMF_ERR_OOM, "out of host memory");
    X->M.shell = true;
    X->M.n = n; X->M.m = m; X->M.nnz = nnz;
    X->M.counts_int = meta[3] != 0.0; X->M.counts_u16 = meta[4] != 0.0; X->M.max_val = meta[5];
    X->lgx = meta[6];
    std::call_once(X->xlx_once, [&] { X->xlx = meta[7]; });
    *out = X;
    return VBNMF_OK;
}

int vbnmf_matrix_is_shell(const vbnmf_matrix *X) { return X && X->M.shell ? 1 : 0; }

// The per-matrix work every whole-matrix layout starts from, done ahead of need (e.g. on a second host thread while the
// cell side is being cut): the order of the cells (order.cpp) and the row-major copy the gene side is cut from.
// The same on a background host thread owned by the handle (joined by vbnmf_matrix_prepare and by destroy): the call
// returns at once, and whoever needs the order or the row-major copy first simply waits for it (std::call_once).
int vbnmf_matrix_prepare_async(const vbnmf_matrix *X)
{
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (X->M.shell) return VBNMF_OK;
    std::lock_guard<std::mutex> g(X->prep_mu);
    if (X->prep.joinable()) return VBNMF_OK;                     // already under way (or done, not yet joined)
    try {
        X->prep = std::thread([X] {
            try { (void)X->M.cell_order(); (void)X->M.row_major(); } catch (...) { /* the consumer that needs them reports the failure */ }
        });
    } catch (const std::system_error &) {
        return fail(VBNMF_ERR_OOM, "could not start the background thread");
    }
    return VBNMF_OK;
}

int vbnmf_matrix_prepare(const vbnmf_matrix *X)
{
    if (!X) return fail(VBNMF_ERR_BAD_ARG, "matrix handle is NULL");
    if (X->M.shell) return VBNMF_OK;
    {
        std::lock_guard<std::mutex> g(X->prep_mu);
        if (X->prep.joinable()) X->prep.join();
    }
    try {
        (void)X->M.cell_order();
        (void)X->M.row_major();
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory preparing the matrix");
    }
    return VBNMF_OK;
}

// Blob of the whole-matrix layout of `side` in the geometry of rank `geometry_rank` for engines with n_wg sweep
// workgroups (vbnmf_device_sweep_workgroups).  buf == NULL: builds (and caches) the layout and returns its blob size in
// *bytes; otherwise writes the blob (all host threads) into buf[0..capacity).
int vbnmf_matrix_export_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg, void *buf,
                               int64_t capacity, int64_t *bytes)
{
    if (!X || !bytes) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_geometry_args(side, geometry_rank, n_wg)) return rc;
    std::shared_ptr<const Layout> L;
    LayoutParams lp;
    try {
        lp = whole_matrix_params(X, side, geometry_rank, n_wg);
        int rc = VBNMF_OK;
        L = shared_layout(X, side, lp, rc);
        if (rc) return rc;
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory building the layout");
    }
    BlobArray a[kBlobArrays];
    blob_arrays(*L, a);
    const int64_t total = blob_size(a);
    *bytes = total;
    if (!buf) return VBNMF_OK;
    if (capacity < total) return fail(VBNMF_ERR_BAD_ARG, "the buffer holds %lld bytes, the layout blob needs %lld", (long long)capacity, (long long)total);
    write_blob(buf, *L, lp, X);
    return VBNMF_OK;
}

// Adds the layout in buf[0..bytes) (written by vbnmf_matrix_export_layout, this library version) to X's cache: engines
// created afterwards in that geometry use it instead of cutting their own.  X: a shell or a full handle of the same matrix.
int vbnmf_matrix_import_layout(const vbnmf_matrix *X, const void *buf, int64_t bytes)
{
    return load_blob(X, buf, bytes, nullptr);
}

// The same layout, but living ONCE in the node's shared memory.  share: cuts the layout with its big arrays written
// straight into a new file `path` (a tmpfs path, e.g. under /dev/shm; built as path + ".part" and renamed when complete,
// so a peer that sees `path` sees all of it) and keeps that mapping as the layout's storage; a layout that is already
// cached in ordinary memory is copied into the file instead.  attach: maps `path` read-only and adopts the big arrays in
// place (the small index arrays are copied).  The file may be unlinked as soon as every process has attached.
int vbnmf_matrix_share_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg, const char *path)
{
    if (!X || !path) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_geometry_args(side, geometry_rank, n_wg)) return rc;
    try {
        const LayoutParams lp = whole_matrix_params(X, side, geometry_rank, n_wg);
        ShmSink sink;
        sink.path = path;
        int rc = VBNMF_OK;
        bool built = false;
        std::shared_ptr<const Layout> L = shared_layout(X, side, lp, rc, &sink, &built);
        if (rc) { if (sink.map) unlink((sink.path + ".part").c_str()); return rc; }
        std::shared_ptr<ShmMap> map = sink.map;             // the big arrays are in place already: header and small arrays around them
        if (!built || !map) {
            // already cached in ordinary memory: write a copy (the copying export into a fresh file)
            BlobArray a[kBlobArrays];
            blob_arrays(*L, a);
            if ((rc = create_part(path, blob_size(a), map))) return rc;
        }
        write_blob(map->base, *L, lp, X);
        map.reset();
        return publish_part(path);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory building the layout");
    }
}

int vbnmf_matrix_attach_layout(const vbnmf_matrix *X, const char *path)
{
    if (!X || !path) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(VBNMF_ERR_BAD_ARG, "cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < kBlobHeaderWords * 8 + 8) { close(fd); return fail(VBNMF_ERR_BAD_ARG, "%s is not a layout blob", path); }
    void *base = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) return fail(VBNMF_ERR_OOM, "cannot map %s: %s", path, strerror(errno));
    auto map = std::make_shared<ShmMap>();
    map->base = base; map->bytes = (size_t)st.st_size;
    return load_blob(X, base, (int64_t)st.st_size, map);
}

}  // extern "C"
