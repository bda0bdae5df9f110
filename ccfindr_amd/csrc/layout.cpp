// layout.cpp -- the builder of the tiled device layout (build_layout: a driver over the phases that VBNMF_BUILD_TIMES
// names), the per-matrix cache of whole-matrix layouts, the rank classes of a sweep, and vbnmf_layout_build.  Host code only.
#include "common.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <new>

namespace vbnmf {

int env_int(const char *name, int dflt)
{
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    return atoi(s);
}

int check_geometry_args(int side, int rank, int n_wg)
{
    if (side != 0 && side != 1) return fail(VBNMF_ERR_BAD_ARG, "side must be 0 or 1");
    if (rank < 1 || rank > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", rank, VBNMF_MAX_RANK);
    if (n_wg < 1) return fail(VBNMF_ERR_BAD_ARG, "n_wg must be positive");
    return VBNMF_OK;
}

LayoutParams default_layout_params(int64_t n_major, int64_t n_minor, int R, int n_wg, int64_t nnz)
{
    LayoutParams lp;
    // One minor block of the gathered factor must fit the workgroup's LDS: block_width * R * 8 bytes.
    int lds_kb = env_int("VBNMF_LDS_KB", 160);
    if (lds_kb < 8) lds_kb = 8;
    if (lds_kb > 160) lds_kb = 160;
    int64_t cmax = ((int64_t)lds_kb * 1024 - kLdsReserveBytes) / lds_row_bytes(R);
    if (n_wg <= 0) n_wg = env_int("VBNMF_NWG", 256);
    if (n_wg < 1) n_wg = 1;
    // Longest task.  A lane walks its task serially (~0.15 us per entry when its wave is alone on a SIMD), so on a
    // small matrix 256-entry tasks leave a handful of waves running for 40 us while the rest of the chip idles:
    // tasks are cut short enough that every wave of every workgroup can have work, up to the 256 that the
    // headline size wants (192 measures the same there and 128 slower with merged pieces, profiles/piece_merge_ab.txt).
    // VBNMF_MAX_LEN overrides.
    int ml = env_int("VBNMF_MAX_LEN", 0);
    if (ml <= 0) {
        const int64_t waves = (int64_t)n_wg * (sweep_threads(R) / kLanes);
        // measured on 1 000 x 450, 2 000 x 5 000, 5 000 x 10 000 and the headline matrix: best near two entries per lane
        // of every wave, not below 16
        ml = nnz > 0 ? (int)std::max<int64_t>(16, std::min<int64_t>(256, 2 * nnz / (kLanes * waves) + 1)) : 256;
    }
    if (ml < kWidthQuantum) ml = kWidthQuantum;
    ml = (ml + kWidthQuantum - 1) / kWidthQuantum * kWidthQuantum;
    // Dense-ish matrices: a (major, block) pair much longer than the longest task is cut into several tasks anyway, so a
    // narrower block costs no extra task and stages less.  About three tasks per pair at the matrix's mean density
    // (2 000 x 10 000, 75 % stored, rank 5: 78.1 us per step with 160 KB blocks, 76.7 with 80, 75.4 with 32 -- this rule --,
    // 81.8 with 16); never below 256 rows; at 5 % density the LDS capacity is the tighter bound by far.
    if (nnz > 0 && n_major > 0 && n_minor > 0 && env_int("VBNMF_LDS_KB", 0) == 0) {
        const double density = (double)nnz / ((double)n_major * (double)n_minor);
        const int64_t want = (int64_t)std::max(256.0, 3.0 * (double)ml / std::max(density, 1e-9));
        if (want < cmax) cmax = want;
    }
    cmax &= ~(int64_t)7;
    if (cmax > 65528) cmax = 65528;            // local minor index is 16 bits
    if (cmax < 8) cmax = 8;
    int64_t nb = (n_minor + cmax - 1) / cmax;
    int64_t c = (n_minor + nb - 1) / nb;       // equal-width blocks instead of a short last one
    c = (c + 7) & ~(int64_t)7;
    if (c > cmax) c = cmax;
    lp.block_width = (int32_t)c;
    lp.block_cap = (int32_t)cmax;
    lp.n_wg = n_wg;
    lp.max_len = ml;
    lp.row_slots = lds_row_bytes(R) / 16;
    // One lane per task of the sweep (ranks up to 32): the pieces of a cut pair are laid in neighbouring lanes and the wave
    // adds them up before anything is stored (cut_tasks).  VBNMF_MERGE_PIECES=0/1 forces it off / on.
    lp.merge = (rank_shares(R) == 1 && env_int("VBNMF_MERGE_PIECES", 1) != 0) ? 1 : 0;
    return lp;
}

// ------------------------------------------------------------------ the builder's phases
namespace {

// Major-compressed view of X[:, cb:ce): entries of major M are [pb[M], pe[M]) of idx / val.  Contiguous majors: pb = ptr,
// pe = ptr + 1; the cell side under a renumbering of the cells walks the columns in the new order through two index arrays
// instead (no copy of X).  The view owns whatever storage it needed; otherwise it points into X.
struct MajorView {
    int64_t n_major = 0, n_minor = 0;
    const int64_t *pb = nullptr, *pe = nullptr;
    const int32_t *idx = nullptr;
    const double *val = nullptr;
    std::vector<int64_t> ptr, end;          // offsets of a permuted cell side (begin, end), of a partial-range transpose or of the count split
    BigVec<int32_t> tidx;                   // the partial-range transpose
    BigVec<double> tval;
    std::vector<int32_t> xidx;              // the count split
    std::vector<double> xval;
    MajorView() = default;
    MajorView(const MajorView &) = delete;
    MajorView &operator=(const MajorView &) = delete;
};

void major_view(const Matrix &X, int64_t cb, int64_t ce, int side, const int32_t *perm, MajorView &V)
{
    if (side == 1) {
        V.n_major = ce - cb; V.n_minor = X.n;
        V.idx = X.row.data(); V.val = X.val.data();
        if (perm) {
            V.ptr.resize(ce - cb); V.end.resize(ce - cb);
            for (int64_t p = 0; p < ce - cb; p++) { V.ptr[p] = X.colptr[cb + perm[p]]; V.end[p] = X.colptr[cb + perm[p] + 1]; }
            V.pb = V.ptr.data(); V.pe = V.end.data();
        } else {
            V.pb = X.colptr.data() + cb; V.pe = V.pb + 1;
        }
        return;
    }
    V.n_major = X.n; V.n_minor = ce - cb;
    if (cb == 0 && ce == X.m) {
        const RowMajor &Rm = X.row_major();               // built once per matrix (in the matrix's cell order), shared by every engine on it
        V.pb = Rm.ptr.data(); V.idx = Rm.idx.data(); V.val = Rm.val.data();
    } else {
        transpose_compressed(ce - cb, X.n, X.colptr.data() + cb, X.row.data(), X.val.data(), 0, V.ptr, V.tidx, V.tval, perm);
        V.pb = V.ptr.data(); V.idx = V.tidx.data(); V.val = V.tval.data();
    }
    V.pe = V.pb + 1;
}

// integer counts above the packed range: the entry is stored as ceil(x / kPackedCountMax) entries of the same minor
void split_large_counts(MajorView &V)
{
    const int64_t nm = V.n_major;
    std::vector<int64_t> xptr(nm + 1, 0);
    for (int64_t M = 0; M < nm; M++) {
        int64_t c = 0;
        for (int64_t q = V.pb[M]; q < V.pe[M]; q++) c += (int64_t)std::ceil(V.val[q] / kPackedCountMax);
        xptr[M + 1] = xptr[M] + c;
    }
    V.xidx.resize(xptr[nm]); V.xval.resize(xptr[nm]);
    parallel_for(nm, [&](int64_t b, int64_t e, int) {
        for (int64_t M = b; M < e; M++) {
            int64_t o = xptr[M];
            for (int64_t q = V.pb[M]; q < V.pe[M]; q++) {
                double left = V.val[q];
                while (left > 0.0) {
                    const double piece = std::min(left, kPackedCountMax);
                    V.xidx[o] = V.idx[q]; V.xval[o] = piece; o++;
                    left -= piece;
                }
            }
        }
    });
    V.ptr.swap(xptr);                                     // (the view it was read through is not needed any more)
    V.pb = V.ptr.data(); V.pe = V.pb + 1; V.idx = V.xidx.data(); V.val = V.xval.data();
}

// Minor blocks.  Whole workgroups are handed to blocks (a workgroup stages ONE block per side), so a block whose
// cost is 9.8 workgroups' worth gets 10 or 9 of them -- and in the second case each of its workgroups carries 9 %
// more than the rest (measured on the headline matrix, gene side: 26 equal blocks, 22 with 10 workgroups and 4
// with 9: modelled cost max / mean 1.13, and the slowest workgroups took 100 us against a mean of 88).  The block
// boundaries are therefore put where the cumulative entry count reaches a whole number of workgroup quotas:
// every block is worth an integer G_b of them (G_b as equal as possible), no wider than the LDS allows.
// With more blocks than workgroups (huge matrices) the blocks stay equal and are bin-packed below (pack_blocks).
std::vector<int64_t> cut_blocks(const MajorView &V, const LayoutParams &lp)
{
    const int32_t wmax = lp.block_cap > 0 ? lp.block_cap : lp.block_width;
    std::vector<int64_t> bstart;
    std::vector<int64_t> mcount(V.n_minor + 1, 0);                     // entries per minor -> prefix sums
    {
        const int T = host_threads();
        std::vector<std::vector<int64_t>> part(T);
        parallel_for(V.n_major, [&](int64_t b, int64_t e, int tid) {
            std::vector<int64_t> &c = part[tid];
            c.assign(V.n_minor, 0);
            for (int64_t M = b; M < e; M++)
                for (int64_t q = V.pb[M]; q < V.pe[M]; q++) c[V.idx[q]]++;
        }, T);
        for (const auto &c : part)
            if (!c.empty()) for (int64_t j = 0; j < V.n_minor; j++) mcount[j + 1] += c[j];
    }
    for (int64_t j = 0; j < V.n_minor; j++) mcount[j + 1] += mcount[j];
    const int64_t total = mcount[V.n_minor];
    int64_t nb = (V.n_minor + wmax - 1) / wmax;
    const bool proportional = env_int("VBNMF_EQUAL_BLOCKS", 0) == 0 && total > 0;
    for (; proportional && nb <= lp.n_wg; nb++) {
        std::vector<int64_t> cand(nb + 1, 0);
        bool ok = true;
        int64_t gsum = 0;
        for (int64_t b = 0; b < nb && ok; b++) {
            gsum += lp.n_wg / nb + (b < lp.n_wg % nb ? 1 : 0);              // G_b: as equal as possible
            int64_t end = V.n_minor;
            if (b + 1 < nb) {
                const double target = (double)total * (double)gsum / (double)lp.n_wg;
                end = std::lower_bound(mcount.begin(), mcount.end(), (int64_t)std::llround(target)) - mcount.begin();
                end = std::min<int64_t>(std::max<int64_t>(end, cand[b] + 1), V.n_minor - (nb - 1 - b));
            }
            cand[b + 1] = end;
            ok = end - cand[b] <= wmax;
        }
        if (ok) { bstart.swap(cand); break; }
    }
    if (bstart.empty()) {                                                   // equal blocks
        nb = (V.n_minor + lp.block_width - 1) / lp.block_width;
        bstart.resize(nb + 1);
        for (int64_t b = 0; b <= nb; b++) bstart[b] = std::min<int64_t>(V.n_minor, b * (int64_t)lp.block_width);
    }
    return bstart;
}

// bpos[major][b] = position of the major's first entry whose minor is in block >= b
std::vector<int64_t> block_positions(const MajorView &V, const std::vector<int64_t> &bstart)
{
    const int32_t nblk = (int32_t)bstart.size() - 1;
    std::vector<int64_t> bpos((size_t)V.n_major * (nblk + 1));
    parallel_for(V.n_major, [&](int64_t b, int64_t e, int) {
        for (int64_t M = b; M < e; M++) {
            int64_t q = V.pb[M], t = V.pe[M];
            int64_t *bp = &bpos[(size_t)M * (nblk + 1)];
            for (int32_t blk = 0; blk <= nblk; blk++) {
                int64_t lim = bstart[blk];
                while (q < t && V.idx[q] < lim) q++;
                bp[blk] = q;
            }
        }
    });
    return bpos;
}

// phase 0 = the task's entries of value 1 (placed first, see cut_tasks), 1 = those of value 2, 2 = the others
// (every entry when the fast stretch is off)
constexpr int kPhases = 3;
inline int phase_of(double v, bool fast_ones) { return !fast_ones ? 2 : (v == 1.0 ? 0 : (v == 2.0 ? 1 : 2)); }

// A task: `len` entries of `major`; n1 / n2 of them have the value 1 / 2 (the fill places the ones first, then the twos).
// opos < 0: the entries are positions [pos, pos + len) of the view.  Otherwise the task is a piece of a cut pair whose
// entries were dealt over its pieces: entry u is position pos + ord[opos + u], pos the pair's first position.
// first: the smallest minor among its entries.
struct Task { uint32_t major; int32_t len; int64_t pos; int32_t n1, n2; int64_t opos; int32_t first; };
struct BlockTasks {
    std::vector<Task> tasks;
    std::vector<uint32_t> ord;          // the dealt pairs' entries, piece by piece, relative to the pair's first position
};

// tasks per block: (major, block) runs longer than max_len are cut in near-equal pieces
// n1 = the task's entries of value exactly 1: they are placed first in the task, so that the sweep can run the
// leading trips of a slice -- as far as EVERY lane still sits on such entries -- through a shorter loop (no
// count conversion, and on the gene side a running product in place of a logarithm per entry, kernels.h).
// Tasks are therefore grouped by padded length first and, within a length class, by n1: the 64 tasks of a slice
// then agree on how long that leading stretch is.
// merge: the pieces of a pair form a GROUP that is sorted as one unit and so lands in consecutive lanes; the sweep adds
// the pieces' statistics inside the wave and the pair costs one partial row (two where it straddles a slice border).
// The order of a pair's entries is free, so they are dealt round the pieces -- the ones first, then the twos, then the
// rest: the pieces' lengths, ones and ones-or-twos differ by at most one.  The number of pieces is raised until all of
// them fall in ONE padded length (a group whose pieces differed there could not be placed in a list sorted by it).
std::vector<BlockTasks> cut_tasks(const MajorView &V, const std::vector<int64_t> &bpos, int32_t nblk, int32_t max_len, bool fast_ones, bool merge)
{
    std::vector<BlockTasks> btasks(nblk);
    parallel_for(nblk, [&](int64_t b0, int64_t b1, int) {
        struct Unit { int32_t t0, cnt, pad, n1; };           // tasks [t0, t0 + cnt) of T: a group, or a task alone
        std::vector<Unit> units;
        std::vector<uint32_t> dealt;
        auto padded = [](int64_t len) { return (int32_t)((len + kWidthQuantum - 1) / kWidthQuantum); };
        for (int64_t blk = b0; blk < b1; blk++) {
            std::vector<Task> &T = btasks[blk].tasks;
            std::vector<uint32_t> &O = btasks[blk].ord;
            units.clear();
            for (int64_t M = 0; M < V.n_major; M++) {
                const int64_t *bp = &bpos[(size_t)M * (nblk + 1)];
                int64_t q0 = bp[blk], cnt = bp[blk + 1] - q0;
                if (cnt <= 0) continue;
                int64_t pieces = (cnt + max_len - 1) / max_len;
                if (!merge || pieces == 1) {
                    for (int64_t pc = 0; pc < pieces; pc++) {
                        int64_t s = cnt * pc / pieces, t = cnt * (pc + 1) / pieces;
                        int32_t n1 = 0, n2 = 0;
                        if (fast_ones) for (int64_t q = q0 + s; q < q0 + t; q++) { n1 += (V.val[q] == 1.0); n2 += (V.val[q] == 2.0); }
                        units.push_back({(int32_t)T.size(), 1, padded(t - s), n1});
                        T.push_back({(uint32_t)M, (int32_t)(t - s), q0 + s, n1, n2, -1, V.idx[q0 + s]});
                    }
                    continue;
                }
                // Every piece in one padded length: with P pieces of w quanta the lengths cnt / P (+ 1) must all lie in
                // (4 (w - 1), 4 w].  Among the counts from the fewest the cap allows to half as many again, the one that
                // costs least: its slots, padding included, plus six slots per piece (3 000 x 6 000 at a cap of 16: fewer,
                // longer pieces keep more of the leading stretch of ones, more, shorter ones pad less).  More pieces cost
                // no more rows.
                {
                    int64_t best = 0, best_cost = 0;
                    for (int64_t P = pieces; P <= std::min<int64_t>(cnt, pieces + pieces / 2 + 2) || !best; P++) {
                        const int64_t w = (cnt + kWidthQuantum * P - 1) / (kWidthQuantum * P);
                        if (cnt < P * (kWidthQuantum * (w - 1) + 1)) continue;
                        const int64_t cost = kWidthQuantum * w * P + 6 * P;
                        if (!best || cost < best_cost) { best = P; best_cost = cost; }
                    }
                    pieces = best;
                }
                dealt.clear();
                int64_t n1t = 0, n12t = 0;
                for (int ph = fast_ones ? 0 : 2; ph < kPhases; ph++) {
                    for (int64_t u = 0; u < cnt; u++) if (phase_of(V.val[q0 + u], fast_ones) == ph) dealt.push_back((uint32_t)u);
                    if (ph == 0) n1t = (int64_t)dealt.size();
                    if (ph == 1) n12t = (int64_t)dealt.size();
                }
                int32_t gmin1 = INT32_MAX;
                const int32_t t0 = (int32_t)T.size();
                for (int64_t pc = 0; pc < pieces; pc++) {                  // piece pc takes entries pc, pc + pieces, ... of the deal
                    const int64_t len = cnt / pieces + (pc < cnt % pieces ? 1 : 0);
                    const int32_t n1 = (int32_t)(n1t > pc ? (n1t - pc + pieces - 1) / pieces : 0);
                    const int32_t n12 = (int32_t)(n12t > pc ? (n12t - pc + pieces - 1) / pieces : 0);
                    const int64_t opos = (int64_t)O.size();
                    int32_t first = INT32_MAX;
                    for (int64_t j = 0; j < len; j++) {
                        const uint32_t u = dealt[pc + j * pieces];
                        O.push_back(u);
                        first = std::min(first, V.idx[q0 + u]);
                    }
                    gmin1 = std::min(gmin1, n1);
                    T.push_back({(uint32_t)M, (int32_t)len, q0, n1, n12 - n1, opos, first});
                }
                units.push_back({t0, (int32_t)pieces, padded(cnt / pieces + (cnt % pieces ? 1 : 0)), gmin1});
            }
            std::stable_sort(units.begin(), units.end(), [&](const Unit &a, const Unit &c2) {
                if (a.pad != c2.pad) return a.pad > c2.pad;
                // inside a length class by the number of ones -- descending in even classes, ascending in odd ones, so
                // that the slice that straddles two classes joins tasks with ALIKE counts (its leading stretch is the
                // minimum over its lanes): gene side of the headline matrix, stretch 48.0 -> 53.9 % of the slots
                return (a.pad & 1) ? a.n1 < c2.n1 : a.n1 > c2.n1;
            });
            std::vector<Task> sorted;
            sorted.reserve(T.size());
            for (const Unit &u : units) sorted.insert(sorted.end(), T.begin() + u.t0, T.begin() + u.t0 + u.cnt);
            T.swap(sorted);
        }
    });
    return btasks;
}

// out[s] = the `width` elements of in[order[s]]: the one permutation behind the renumbering of the slices
template <class V>
void permute_rows(V &v, const std::vector<int32_t> &order, size_t width)
{
    V out;
    out.reserve(v.size());                                // (filled by appending: no pass that zeroes it first)
    for (int32_t o : order) out.insert(out.end(), v.begin() + (size_t)o * width, v.begin() + ((size_t)o + 1) * width);
    v.swap(out);
}

// The tasks by columns, one row per lane of every slice (id = slice * kLanes + lane; idle lanes: major kIdleLane, everything
// else 0).  `major` is the layout's own task_major (the one column the device reads); the others serve the builder only.
struct TaskTable {
    std::vector<uint32_t> &major;
    std::vector<int64_t> pos, opos;
    std::vector<int32_t> len, n1, n2, first;
    BigVec<uint32_t> ord;                   // the dealt pairs' entries (Task::opos points in here), all blocks
    explicit TaskTable(Layout &L) : major(L.task_major) {}
    void assign(size_t rows)
    {
        major.assign(rows, kIdleLane); pos.assign(rows, 0); opos.assign(rows, -1); len.assign(rows, 0); n1.assign(rows, 0); n2.assign(rows, 0);
        first.assign(rows, 0);
    }
    void permute(const std::vector<int32_t> &order)
    {
        permute_rows(major, order, kLanes); permute_rows(pos, order, kLanes); permute_rows(opos, order, kLanes); permute_rows(len, order, kLanes);
        permute_rows(n1, order, kLanes); permute_rows(n2, order, kLanes); permute_rows(first, order, kLanes);
    }
    // position in the view of entry u of task id
    int64_t at(size_t id, int64_t u) const { return opos[id] < 0 ? pos[id] + u : pos[id] + (int64_t)ord[(size_t)(opos[id] + u)]; }
};

// slices: 64 consecutive tasks of a block; blocks in index order.  bslice0[b]: the first slice of block b.
int form_slices(const std::vector<BlockTasks> &btasks, Layout &L, TaskTable &tasks, std::vector<int64_t> &bslice0)
{
    const int32_t nblk = (int32_t)btasks.size();
    bslice0.assign(nblk + 1, 0);
    for (int32_t blk = 0; blk < nblk; blk++)
        bslice0[blk + 1] = bslice0[blk] + ((int64_t)btasks[blk].tasks.size() + kLanes - 1) / kLanes;
    L.n_slices = bslice0[nblk];
    if (L.n_slices > 0x7FFFFFF0LL / kLanes) return fail(VBNMF_ERR_BAD_ARG, "too many tasks for 32-bit task ids");
    tasks.assign((size_t)L.n_slices * kLanes);
    L.slice_width.assign(L.n_slices, 0);
    L.slice_block.assign(L.n_slices, 0);
    L.slice_fast.assign(L.n_slices, 0);
    L.n_tasks = 0;
    size_t nord = 0;
    for (int32_t blk = 0; blk < nblk; blk++) nord += btasks[blk].ord.size();
    tasks.ord.reserve(nord);
    for (int32_t blk = 0; blk < nblk; blk++) {
        const std::vector<Task> &T = btasks[blk].tasks;
        const int64_t ord0 = (int64_t)tasks.ord.size();
        tasks.ord.insert(tasks.ord.end(), btasks[blk].ord.begin(), btasks[blk].ord.end());
        L.n_tasks += (int64_t)T.size();
        for (size_t q = 0; q < T.size(); q++) {
            size_t id = (size_t)bslice0[blk] * kLanes + q;
            tasks.major[id] = T[q].major; tasks.pos[id] = T[q].pos; tasks.len[id] = T[q].len; tasks.n1[id] = T[q].n1; tasks.n2[id] = T[q].n2;
            tasks.opos[id] = T[q].opos < 0 ? -1 : ord0 + T[q].opos; tasks.first[id] = T[q].first;
        }
        for (int64_t s = bslice0[blk]; s < bslice0[blk + 1]; s++) {
            int32_t w = tasks.len[(size_t)s * kLanes];           // sorted by padded length: the first lane's is the largest
            L.slice_width[s] = (w + kWidthQuantum - 1) / kWidthQuantum * kWidthQuantum;
            L.slice_block[s] = blk;
            int32_t f = INT32_MAX;                               // leading entries that are ones in EVERY lane (idle lanes: none)
            int32_t f12 = INT32_MAX;                             // ... that are ones or twos in every lane (ones first, then twos)
            for (int l = 0; l < kLanes; l++) {
                f = std::min(f, tasks.n1[(size_t)s * kLanes + l]);
                f12 = std::min(f12, tasks.n1[(size_t)s * kLanes + l] + tasks.n2[(size_t)s * kLanes + l]);
            }
            const int32_t f1 = std::min<int32_t>(f / 8 * 8, 0x7FF8);   // whole loop trips (8 entries)
            const int32_t f2 = std::min<int32_t>(std::max(f1, f12 / 8 * 8), 0x7FF8);      // (sign bit of the word stays clear)
            L.slice_fast[s] = f1 | (f2 << 16);                   // low half: the stretch of ones; high half: of ones and twos
        }
    }
    return VBNMF_OK;
}

// Modelled cost of a slice in entry-equivalents: what the block costs and the deal below balance (nothing else uses it).
double slice_cost(const Layout &L, int64_t s)
{
    const double c0 = 10.0;                              // per-slice overhead in entry-equivalents
    // an entry of the leading stretch of ones costs the gene side (which carries the logarithm) ~0.6 and the cell
    // side ~0.9 of an ordinary entry (instruction counts of the two loops, kernels.h)
    const double fast_discount = L.side == 0 ? 0.4 : 0.1;
    // (the stretch of twos behind the ones saves the gene side's logarithm only: ~0.18 of an entry)
    const int32_t f1 = L.slice_fast[s] & 0xFFFF, f2 = L.slice_fast[s] >> 16;
    return (double)L.slice_width[s] - fast_discount * (double)f1 - (L.side == 0 ? 0.18 : 0.0) * (double)(f2 - f1) + c0;
}

using Segment = std::pair<int32_t, std::vector<int32_t>>;    // (block, its slices in this share)
using Shares = std::vector<std::vector<Segment>>;            // the segments of every workgroup

// Whole workgroups per live block in proportion to block cost (largest remainder); no block more than it has slices.
std::vector<int> apportion_workgroups(const std::vector<int32_t> &live, const std::vector<double> &bcost, double total,
                                      const std::vector<int64_t> &bslice0, int n_wg)
{
    std::vector<int> G(bcost.size(), 0);
    std::vector<std::pair<double, int32_t>> frac;
    auto slices_of = [&](int32_t blk) { return bslice0[blk + 1] - bslice0[blk]; };
    int used = 0;
    for (int32_t blk : live) {
        double quota = n_wg * bcost[blk] / total;
        int g = std::max(1, (int)std::floor(quota));
        g = (int)std::min<int64_t>(g, slices_of(blk));
        G[blk] = g; used += g;
        frac.emplace_back(quota - g, blk);
    }
    std::stable_sort(frac.begin(), frac.end(), [](const std::pair<double, int32_t> &x, const std::pair<double, int32_t> &y) { return x.first > y.first; });
    for (size_t q = 0; used < n_wg && !frac.empty(); q = (q + 1) % frac.size()) {   // hand out the spare workgroups
        int32_t blk = frac[q].second;
        if (G[blk] < slices_of(blk)) { G[blk]++; used++; }
        else if (q + 1 == frac.size()) { bool any = false; for (auto &f : frac) any |= G[f.second] < slices_of(f.second); if (!any) break; }
    }
    while (used > n_wg) {                                 // too many (each block needs at least one): shrink the most over-served
        int32_t worst = -1;
        for (int32_t blk : live) if (G[blk] > 1 && (worst < 0 || bcost[blk] / G[blk] < bcost[worst] / G[worst])) worst = blk;
        if (worst < 0) break;
        G[worst]--; used--;
    }
    return G;
}

// longest-processing-time deal of block blk's slices [s0, s1) to the g workgroups from `mine` on: slices by cost,
// descending (ties by id), each to the workgroup of the block with the least cost so far (ties to the lowest) -- equal
// cost AND, because the costly slices go round first, the same mix of long and short slices in every share
void deal_shares(const Layout &L, int32_t blk, int64_t s0, int64_t s1, int g, std::vector<Segment> *mine)
{
    for (int j = 0; j < g; j++) mine[j].emplace_back(blk, std::vector<int32_t>());
    std::vector<int32_t> by_cost;
    for (int64_t i = s0; i < s1; i++) by_cost.push_back((int32_t)i);
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](int32_t x, int32_t y) { return slice_cost(L, x) > slice_cost(L, y); });
    std::vector<double> load(g, 0.0);
    for (int32_t i : by_cost) {
        const size_t j = std::min_element(load.begin(), load.end()) - load.begin();          // (ties to the lowest)
        mine[j].back().second.push_back(i);
        load[j] += slice_cost(L, i);
    }
}

// more blocks than workgroups: whole blocks, costliest first, each onto the least loaded workgroup
void pack_blocks(const std::vector<int32_t> &live, const std::vector<double> &bcost, const std::vector<int64_t> &bslice0, Shares &shares)
{
    std::vector<int32_t> ord(live);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return bcost[x] > bcost[y]; });
    std::vector<double> load(shares.size(), 0.0);
    for (int32_t blk : ord) {
        const size_t best = std::min_element(load.begin(), load.end()) - load.begin();
        shares[best].emplace_back(blk, std::vector<int32_t>());
        for (int64_t i = bslice0[blk]; i < bslice0[blk + 1]; i++) shares[best].back().second.push_back((int32_t)i);
        load[best] += bcost[blk];
    }
    for (auto &sh : shares)
        std::stable_sort(sh.begin(), sh.end(), [](const Segment &x, const Segment &y) { return x.first < y.first; });
}

// persistent workgroups.  Shares are block-aligned so a workgroup stages one block per side:
// whole workgroups are apportioned to blocks in proportion to block cost (largest remainder);
// a block's slices are dealt to its workgroups longest-processing-time-first (equal cost,
// same mix of long and short slices); inside a share the waves pull the slices longest first at run
// time (see below).  With more blocks than workgroups, whole blocks are bin-packed onto workgroups instead.
// Sets wg_seg0 / seg_block / seg_ptr; returns the processing order: order[new slice id] = the id it has now.
std::vector<int32_t> share_out(Layout &L, const std::vector<int64_t> &bslice0)
{
    const int32_t nblk = L.n_blocks;
    std::vector<double> bcost(nblk, 0.0);
    double total = 0.0;
    for (int32_t blk = 0; blk < nblk; blk++) {
        for (int64_t s = bslice0[blk]; s < bslice0[blk + 1]; s++) bcost[blk] += slice_cost(L, s);
        total += bcost[blk];
    }
    Shares shares(L.n_wg);
    std::vector<int32_t> live;                            // blocks that have slices
    for (int32_t blk = 0; blk < nblk; blk++) if (bslice0[blk + 1] > bslice0[blk]) live.push_back(blk);
    if ((int64_t)live.size() <= L.n_wg && !live.empty()) {
        const std::vector<int> G = apportion_workgroups(live, bcost, total, bslice0, L.n_wg);
        int w = 0;
        for (int32_t blk : live) {
            deal_shares(L, blk, bslice0[blk], bslice0[blk + 1], G[blk], &shares[w]);
            w += G[blk];
        }
    } else {
        pack_blocks(live, bcost, bslice0, shares);
    }
    L.wg_seg0.assign(L.n_wg + 1, 0);
    L.seg_block.clear();
    L.seg_ptr.assign(1, 0);
    std::vector<int32_t> order;
    order.reserve(L.n_slices);
    // Inside a share the waves take slices DYNAMICALLY (an LDS ticket counter), longest first: the
    // hardware issues the oldest wave of a SIMD first, so equal static shares finish far apart
    // (measured: 50 / 75 / 99 us for the three waves of a SIMD) while greedy longest-first pulling
    // ends all waves within one slice of each other.  Which wave runs a slice does not change any
    // result (per-task partials; per-slice evidence partials summed in list order).
    for (int w = 0; w < L.n_wg; w++) {
        L.wg_seg0[w] = (int32_t)L.seg_block.size();
        for (auto &seg : shares[w]) {
            std::vector<int32_t> &sl = seg.second;
            std::stable_sort(sl.begin(), sl.end(), [&](int32_t x, int32_t y) { return L.slice_width[x] > L.slice_width[y]; });
            L.seg_block.push_back(seg.first);
            order.insert(order.end(), sl.begin(), sl.end());
            L.seg_ptr.push_back((int32_t)order.size());
        }
    }
    L.wg_seg0[L.n_wg] = (int32_t)L.seg_block.size();
    L.n_segs = (int64_t)L.seg_block.size();
    return order;
}

// Renumber the slices in processing order, so that list position == slice id: the kernel then finds
// a slice's width, offset, majors and partial rows directly from its ticket, with no indirection.
void renumber_slices(Layout &L, TaskTable &tasks, const std::vector<int32_t> &order)
{
    permute_rows(L.slice_width, order, 1); permute_rows(L.slice_block, order, 1); permute_rows(L.slice_fast, order, 1);
    tasks.permute(order);
    L.slice_off.assign(L.n_slices, 0);
    int64_t off = 0;
    for (int64_t s = 0; s < L.n_slices; s++) { L.slice_off[s] = off; off += (int64_t)L.slice_width[s] * kLanes; }
    L.n_slots = off;
}

// inverse index: the tasks of each major in (block, position) order -- the pieces of a dealt pair by their first minor --:
// the fixed order in which their partial statistics are summed (built once the slices have their final numbers)
void build_inverse(Layout &L, const TaskTable &tasks)
{
    const int64_t nmaj = L.n_major;
    L.inv_ptr.assign(nmaj + 1, 0);
    for (uint32_t M : tasks.major)
        if (M != kIdleLane) L.inv_ptr[M + 1]++;
    for (int64_t M = 0; M < nmaj; M++) L.inv_ptr[M + 1] += L.inv_ptr[M];
    L.inv_task.assign(L.n_tasks, 0);
    std::vector<int32_t> cur(L.inv_ptr.begin(), L.inv_ptr.end() - 1);
    std::vector<std::pair<int64_t, int32_t>> key(L.n_tasks);
    for (size_t id = 0; id < tasks.major.size(); id++) {
        uint32_t M = tasks.major[id];
        if (M == kIdleLane) continue;
        int32_t o = cur[M]++;
        L.inv_task[o] = (uint32_t)id; key[o] = {tasks.pos[id], tasks.first[id]};
    }
    parallel_for(nmaj, [&](int64_t b, int64_t e, int) {
        std::vector<std::pair<std::pair<int64_t, int32_t>, uint32_t>> t2;      // ((position, first minor), id) per major
        for (int64_t M = b; M < e; M++) {
            int32_t s = L.inv_ptr[M], t = L.inv_ptr[M + 1];
            if (t - s < 2) continue;
            t2.clear();
            for (int32_t q = s; q < t; q++) t2.emplace_back(key[q], L.inv_task[q]);
            std::sort(t2.begin(), t2.end());
            for (int32_t q = s; q < t; q++) L.inv_task[q] = t2[q - s].second;
        }
    });
}

// row index: the first lanes of the runs (common.h) of each major, in the inverse index's order
void build_rows(Layout &L)
{
    if (!L.merge) { L.row_ptr = L.inv_ptr; L.row_task = L.inv_task; L.n_rows = L.n_tasks; return; }
    const std::vector<uint32_t> &major = L.task_major;
    auto leads = [&](uint32_t id) { return (id % kLanes) == 0 || major[id] != major[id - 1]; };
    L.row_ptr.assign(L.n_major + 1, 0);
    L.row_task.clear();
    for (int64_t M = 0; M < L.n_major; M++) {
        for (int32_t q = L.inv_ptr[M]; q < L.inv_ptr[M + 1]; q++)
            if (leads(L.inv_task[q])) L.row_task.push_back(L.inv_task[q]);
        L.row_ptr[M + 1] = (int32_t)L.row_task.size();
    }
    L.n_rows = (int64_t)L.row_task.size();
}

// ---- fill: slot(t, lane) = off + (t/4)*256 + lane*4 + t%4 ; padding slots are {minor 0, value 0}.
inline int64_t slot_of(int64_t slice_off, int64_t t, int lane)
{
    return slice_off + (t / kUnroll) * (kLanes * kUnroll) + lane * kUnroll + (t % kUnroll);
}

// The entry stream of one slice: put() stores entry q of the view as entry t of a lane, pad() closes a lane from t0 on.
struct SliceWriter {
    Layout &L;
    const MajorView &V;
    int32_t m0;                 // first minor of the slice's block
    int64_t off;
    int32_t width;
    void put(int lane, int64_t t, int64_t q) const
    {
        const int64_t slot = slot_of(off, t, lane);
        uint32_t local = (uint32_t)(V.idx[q] - m0);
        if (L.wide) { L.wide_idx[slot] = local; L.wide_val[slot] = V.val[q]; }
        else L.packed[slot] = ((uint32_t)V.val[q] << kPackedCountShift) | ((local * (uint32_t)L.row_slots) << 4);
    }
    void pad(int lane, int64_t t0) const                  // the arrays are not zero-filled at allocation: the tail of every lane is
    {
        for (int64_t t = t0; t < width; t++) {
            const int64_t slot = slot_of(off, t, lane);
            if (L.wide) { L.wide_idx[slot] = 0u; L.wide_val[slot] = 0.0; } else L.packed[slot] = 0u;
        }
    }
};

// per worker thread, allocated once: the fill must not allocate per slice
struct GroupScratch {
    std::vector<int32_t> sorted[16];                   // per lane of the group: entry positions by (phase, residue, minor)
    std::vector<uint8_t> bucket_of;                    // (phase, residue) of every entry of the task at hand
};

// VBNMF_NO_BANK_SCHEDULE=1: every lane's entries in stored order, phase by phase
void fill_in_order(const MajorView &V, const TaskTable &tasks, int64_t s, bool fast_ones, const SliceWriter &out)
{
    for (int lane = 0; lane < kLanes; lane++) {
        const size_t id = (size_t)s * kLanes + lane;
        int64_t t = 0;
        if (tasks.major[id] != kIdleLane)
            for (int ph = 0; ph < kPhases; ph++)
                for (int64_t u = 0; u < tasks.len[id]; u++)
                    if (phase_of(V.val[tasks.at(id, u)], fast_ones) == ph) out.put(lane, t++, tasks.at(id, u));
        out.pad(lane, t);
    }
}

// The order of a task's entries is free (it only fixes the summation order), so it is chosen
// to keep the LDS gathers of the sweep conflict-free: a ds_read_b128 wave instruction is served
// in four fixed groups of 16 lanes, one LDS cycle per group when the 16 addresses fall in 16
// different 16-byte bank slots.  Rows of the staged factor are an odd number of slots long, so
// the slot of piece p of row `local` is (stride*local + p) mod 16: two lanes of a group collide
// exactly when their minors are congruent mod 16.  Step by step, the 16 lanes of a group choose in
// turn (the turn order rotates with the step): a lane takes, among the residues (local mod 16) it
// still has entries of and no earlier lane of this step took, the one it has most of; a lane that
// finds all its residues taken doubles up on the least used one.  Round 2 chose residue by residue
// (demand order, each to the lane with the fewest other residues left): twice the inner work plus
// a sort per step -- 85 % of the layout's build time -- for conflict rates this scheme undercuts
// (LDS cycles per group read on the headline matrix, gene / cell side: 1.70 / 1.86 then, 1.66 / 1.83 now).
//
// lanes[16]: the lanes of slice s that the hardware serves together; rides: VBNMF_NO_BANK_RIDES is not set.
void schedule_group(const MajorView &V, const TaskTable &tasks, int64_t s, const int (&lanes)[16], bool fast_ones, bool rides,
                    GroupScratch &scratch, const SliceWriter &out)
{
    const int32_t *idx = V.idx;
    const int32_t m0 = out.m0;
    // key[lane][phase][residue] = (entries left << 4) | (15 - residue): the largest key among a lane's candidates is
    // "most entries left, ties to the lowest residue" in one comparison
    uint32_t key[16][kPhases][16];
    int32_t nxt[16][kPhases][16];                   // where the next entry of that bucket sits in scratch.sorted[lane]
    int32_t nrow[16][kPhases][16];                  // ... and the local minor (row of the staged block) of that entry
    uint16_t avail[16][kPhases] = {};               // residues with entries left, as a bit mask
    int32_t rem[16][kPhases] = {}, step[16] = {};
    int64_t base[16];
    const uint32_t *dealt[16];                      // a piece of a dealt pair: its entries relative to base (TaskTable::at)
    auto at = [&](int j, int32_t t) { return dealt[j] ? base[j] + (int64_t)dealt[j][t] : base[j] + t; };
    int T = 0;
    for (int j = 0; j < 16; j++) {
        const size_t id = (size_t)s * kLanes + lanes[j];
        base[j] = 0; dealt[j] = nullptr;
        if (tasks.major[id] == kIdleLane) continue;
        const int64_t q0 = tasks.pos[id];
        const int32_t len = tasks.len[id];
        base[j] = q0;
        if (tasks.opos[id] >= 0) dealt[j] = tasks.ord.data() + tasks.opos[id];
        scratch.bucket_of.resize(len);
        int32_t cnt[kPhases * 16] = {};
        for (int32_t t = 0; t < len; t++) {    // one pass over the task: phase and residue of every entry
            const int b = phase_of(V.val[at(j, t)], fast_ones) * 16 + ((idx[at(j, t)] - m0) & 15);
            scratch.bucket_of[t] = (uint8_t)b;
            cnt[b]++;
        }
        int32_t o = 0, w[kPhases * 16];
        for (int ph = 0; ph < kPhases; ph++)
            for (int r = 0; r < 16; r++) {
                const int32_t c = cnt[ph * 16 + r];
                nxt[j][ph][r] = o; w[ph * 16 + r] = o; o += c;
                rem[j][ph] += c;
                key[j][ph][r] = ((uint32_t)c << 4) | (uint32_t)(15 - r);
                if (c) avail[j][ph] |= (uint16_t)(1u << r);
            }
        scratch.sorted[j].resize(len);
        for (int32_t t = 0; t < len; t++)      // stable: a bucket keeps its entries in ascending minor order
            scratch.sorted[j][w[scratch.bucket_of[t]]++] = t;
        for (int ph = 0; ph < kPhases; ph++)
            for (int r = 0; r < 16; r++)
                nrow[j][ph][r] = (key[j][ph][r] >> 4) ? (int32_t)(idx[at(j, scratch.sorted[j][nxt[j][ph][r]])] - m0) : -1;
        T = std::max(T, len);
    }
    for (int t = 0; t < T; t++) {
        uint32_t used = 0;                     // residues taken in this step
        uint8_t usedcnt[16] = {};
        int32_t row_of[16];                    // the row the FIRST taker of a residue reads in this step
        for (int q = 0; q < 16; q++) {
            const int j = (t + q) & 15;
            const int ph = rem[j][0] > 0 ? 0 : (rem[j][1] > 0 ? 1 : 2);
            if (rem[j][ph] == 0) continue;
            const uint32_t *k = key[j][ph];
            // A FREE RIDE first (round 5): lanes of a group that read the SAME row in a step share one address -- a
            // broadcast, not a conflict.  If the next entry of one of this lane's buckets is the very row an earlier
            // lane of the step reads, it goes now.  Neighbouring tasks share many minors -- the layout keeps similar
            // cells together, and a gene's cells recur from gene to gene --: LDS cycles per group read on the headline
            // matrix 1.33 -> 1.18 (gene side) and 1.76 -> 1.30 (cell side) by the CPU model that reproduces the counters
            // (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.345 before).
            int ride = -1;
            for (uint32_t a = rides ? (avail[j][ph] & used) : 0u; a; a &= a - 1) {
                const int r = __builtin_ctz(a);
                if (nrow[j][ph][r] == row_of[r]) { ride = r; break; }
            }
            uint32_t cand = avail[j][ph] & ~used;
            int best;
            if (ride >= 0) best = ride;
            else if (cand) {
                uint32_t bk = 0;
                best = 0;
                while (cand) {
                    const int r = __builtin_ctz(cand);
                    cand &= cand - 1;
                    if (k[r] > bk) { bk = k[r]; best = r; }
                }
            } else {                           // every residue it has is taken: the least used, then the fullest, then the lowest
                best = -1;
                for (uint32_t a = avail[j][ph]; a; a &= a - 1) {
                    const int r = __builtin_ctz(a);
                    if (best < 0 || usedcnt[r] < usedcnt[best] || (usedcnt[r] == usedcnt[best] && k[r] > k[best])) best = r;
                }
            }
            out.put(lanes[j], step[j]++, at(j, scratch.sorted[j][nxt[j][ph][best]++]));
            if (ride < 0) {
                if (!((used >> best) & 1u)) row_of[best] = nrow[j][ph][best];
                used |= 1u << best; usedcnt[best]++;
            }
            rem[j][ph]--;
            key[j][ph][best] -= 16;
            if ((key[j][ph][best] >> 4) == 0) { avail[j][ph] &= (uint16_t)~(1u << best); nrow[j][ph][best] = -1; }
            else nrow[j][ph][best] = (int32_t)(idx[at(j, scratch.sorted[j][nxt[j][ph][best]])] - m0);
        }
    }
    for (int j = 0; j < 16; j++) out.pad(lanes[j], step[j]);
}

// Writes every slot of the entry stream, padding included, on all host threads.
int fill_slices(const MajorView &V, const TaskTable &tasks, bool fast_ones, Layout &L)
{
    static const int kGroupOf[64] = {0,0,0,0,1,1,1,1,1,1,1,1,0,0,0,0,1,1,1,1,0,0,0,0,0,0,0,0,1,1,1,1,
                                     2,2,2,2,3,3,3,3,3,3,3,3,2,2,2,2,3,3,3,3,2,2,2,2,2,2,2,2,3,3,3,3};
    const bool schedule = env_int("VBNMF_NO_BANK_SCHEDULE", 0) == 0;
    const bool rides = env_int("VBNMF_NO_BANK_RIDES", 0) == 0;            // (A/B switch of round 5's broadcast rides, schedule_group)
    // Slices differ in cost by two orders of magnitude and lie sorted by width inside a segment: small chunks
    // handed out through a shared counter, not one contiguous range per thread.
    std::atomic<int64_t> next_chunk{0};
    // A worker that runs out of memory says so here and the others stop at their next chunk instead of filling a layout
    // that is lost already (parallel_for would carry its exception to this thread only after every worker had finished).
    std::atomic<bool> fill_oom{false};
    const int64_t kChunk = 16;
    parallel_for(host_threads(), [&](int64_t, int64_t, int) {
        try {
            GroupScratch scratch;
            for (;;) {
                const int64_t c0 = next_chunk.fetch_add(kChunk);
                if (c0 >= L.n_slices) break;
                for (int64_t s = c0; s < std::min<int64_t>(L.n_slices, c0 + kChunk); s++) {
                    const SliceWriter out{L, V, (int32_t)L.block_start[L.slice_block[s]], L.slice_off[s], L.slice_width[s]};
                    if (!schedule) { fill_in_order(V, tasks, s, fast_ones, out); continue; }
                    for (int g = 0; g < 4; g++) {
                        int lanes[16], nl = 0;
                        for (int lane = 0; lane < kLanes; lane++) if (kGroupOf[lane] == g) lanes[nl++] = lane;
                        schedule_group(V, tasks, s, lanes, fast_ones, rides, scratch, out);
                    }
                }
            }
        } catch (const std::bad_alloc &) {
            fill_oom.store(true);
            next_chunk.store(L.n_slices);
        }
    });
    if (fill_oom.load()) return fail(VBNMF_ERR_OOM, "out of host memory filling the tiled layout");
    return VBNMF_OK;
}

}  // namespace

// ------------------------------------------------------------------ the builder
int build_layout(const Matrix &X, int64_t cb, int64_t ce, int side, const LayoutParams &lp, const std::vector<int32_t> *perm_in, Layout &L,
                 LayoutSink *sink)
{
    const int32_t *perm = (perm_in && !perm_in->empty()) ? perm_in->data() : nullptr;
    if (perm && (int64_t)perm_in->size() != ce - cb) return fail(VBNMF_ERR_BAD_ARG, "cell order has %lld entries for %lld cells", (long long)perm_in->size(), (long long)(ce - cb));
    if (cb < 0 || ce > X.m || cb >= ce) return fail(VBNMF_ERR_BAD_ARG, "column range [%lld, %lld) is outside the matrix", (long long)cb, (long long)ce);
    // (max_len <= 0x7FF8: the two leading-stretch lengths of a slice share one int32, 15 + 16 bits -- slice_fast)
    if (lp.block_width <= 0 || lp.block_width > 65536 || lp.max_len <= 0 || lp.max_len > 0x7FF8 || lp.max_len % kWidthQuantum || lp.n_wg <= 0 || lp.row_slots <= 0 ||
        (int64_t)std::max(lp.block_width, lp.block_cap) * lp.row_slots > (int64_t)(kPackedOffsetMask >> 4) + 1)
        return fail(VBNMF_ERR_BAD_ARG, "bad layout parameters");

    auto T0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (getenv("VBNMF_BUILD_TIMES")) { auto t = std::chrono::steady_clock::now(); fprintf(stderr, "  layout side %d %-12s %.3f s\n", side, what, std::chrono::duration<double>(t - T0).count()); T0 = t; } };
    MajorView V;
    major_view(X, cb, ce, side, perm, V);
    if (perm) L.cell_perm.assign(perm, perm + (ce - cb));
    lap("transpose");
    L.side = side;
    L.wide = !X.counts_int;
    L.n_major = V.n_major; L.n_minor = V.n_minor;
    L.nnz = X.colptr[ce] - X.colptr[cb];                 // stored entries of X (before any splitting below)
    L.max_len = lp.max_len;
    L.n_wg = lp.n_wg;
    L.row_slots = lp.row_slots;
    L.merge = lp.merge != 0;
    if (!L.wide && X.max_val > kPackedCountMax) split_large_counts(V);

    L.block_start = cut_blocks(V, lp);
    L.n_blocks = (int32_t)L.block_start.size() - 1;
    L.block_width = 0;                                                      // the WIDEST block: what the LDS image is sized for
    for (int32_t b = 0; b < L.n_blocks; b++) L.block_width = std::max<int32_t>(L.block_width, (int32_t)(L.block_start[b + 1] - L.block_start[b]));
    lap("blocks");
    std::vector<int64_t> bpos = block_positions(V, L.block_start);
    lap("bpos");
    const bool fast_ones = !L.wide && env_int("VBNMF_NO_FAST_ONES", 0) == 0;
    std::vector<BlockTasks> btasks = cut_tasks(V, bpos, L.n_blocks, lp.max_len, fast_ones, L.merge);
    lap("tasks");
    TaskTable tasks(L);
    std::vector<int64_t> bslice0;
    if (int rc = form_slices(btasks, L, tasks, bslice0)) return rc;
    btasks.clear();
    lap("slices");
    renumber_slices(L, tasks, share_out(L, bslice0));
    lap("shares");
    build_inverse(L, tasks);
    build_rows(L);
    lap("inverse");
    try {
        // not zero-filled (the fill below writes every slot, padding included: first touch by the thread that fills)
        if (sink) { if (int rc = sink->place(L)) return rc; }
        else if (L.wide) { L.wide_idx.resize(L.n_slots); L.wide_val.resize(L.n_slots); }
        else L.packed.resize(L.n_slots);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory building the tiled layout (%lld slots)", (long long)L.n_slots);
    }
    lap("alloc");
    if (int rc = fill_slices(V, tasks, fast_ones, L)) return rc;
    lap("fill");
    return VBNMF_OK;
}

// ------------------------------------------------------------------ the per-matrix cache of whole-matrix layouts
static int cache_cap() { return 2 * std::max(0, env_int("VBNMF_LAYOUT_CACHE", 3)); }      // entries = pairs x 2 sides

// Drops the oldest entries down to `cap`; their device copies live on only in the engines that use them.
static void evict_oldest(LayoutCache &C, int cap)
{
    while ((int)C.entries.size() > cap) {
        const Layout *gone = C.entries.front().layout.get();
        C.entries.erase(C.entries.begin());
        for (size_t i = 0; i < C.copies.size();)
            if (C.copies[i].key == gone) C.copies.erase(C.copies.begin() + i); else i++;
    }
}

std::shared_ptr<const Layout> shared_layout(const vbnmf_matrix *X, int side, const LayoutParams &lp, int &rc, LayoutSink *sink, bool *built)
{
    rc = VBNMF_OK;
    if (built) *built = false;
    const int cap = cache_cap();
    LayoutCache &C = X->layouts;
    {
        std::lock_guard<std::mutex> g(C.mu);
        for (size_t i = 0; i < C.entries.size(); i++)
            if (C.entries[i].side == side && C.entries[i].lp == lp) {
                LayoutCache::Entry hit = C.entries[i];
                C.entries.erase(C.entries.begin() + i);
                C.entries.push_back(hit);                                  // most recently used last
                return hit.layout;
            }
    }
    if (X->M.shell) {
        rc = fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries and no imported layout of side %d "
                  "for this geometry (block %d, row stride %d slots, %d workgroups); import it with vbnmf_matrix_import_layout", side,
                  lp.block_width, lp.row_slots, lp.n_wg);
        return nullptr;
    }
    auto L = std::make_shared<Layout>();
    rc = build_layout(X->M, 0, X->M.m, side, lp, &X->M.cell_order(), *L, sink);
    if (rc) return nullptr;
    if (built) *built = true;
    if (cap > 0 || sink) {
        std::lock_guard<std::mutex> g(C.mu);
        C.entries.push_back({side, lp, L});
        evict_oldest(C, std::max(cap, 2));
    }
    return L;
}

void cache_layout(const vbnmf_matrix *X, int side, const LayoutParams &lp, std::shared_ptr<const Layout> L)
{
    LayoutCache &C = X->layouts;
    std::lock_guard<std::mutex> g(C.mu);
    for (size_t i = 0; i < C.entries.size();)
        if (C.entries[i].side == side && C.entries[i].lp == lp) C.entries.erase(C.entries.begin() + i); else i++;
    C.entries.push_back({side, lp, std::move(L)});
    // an imported layout is kept whatever VBNMF_LAYOUT_CACHE says (a shell cannot rebuild it); it counts towards the cap
    // (and a shell cannot cut an evicted layout again: it keeps them all)
    if (!X->M.shell) evict_oldest(C, std::max(2, cache_cap()));
}

std::shared_ptr<void> cached_device_copy(const vbnmf_matrix *X, const Layout *L, int device)
{
    LayoutCache &C = X->layouts;
    std::lock_guard<std::mutex> g(C.mu);
    for (const auto &c : C.copies)
        if (c.key == L && c.device == device) return c.arrays;
    return nullptr;
}

void store_device_copy(const vbnmf_matrix *X, const Layout *L, int device, std::shared_ptr<void> arrays)
{
    LayoutCache &C = X->layouts;
    std::lock_guard<std::mutex> g(C.mu);
    bool cached = false;
    for (const auto &q : C.entries) cached |= q.layout.get() == L;
    if (!cached) return;
    for (const auto &c : C.copies)
        if (c.key == L && c.device == device) return;         // another thread was first
    C.copies.push_back({L, device, std::move(arrays)});
}

// ------------------------------------------------------------------ rank classes
std::vector<int32_t> rank_classes(const int32_t *ranks, int32_t count, int32_t max_classes)
{
    std::vector<int32_t> padded;
    for (int32_t q = 0; q < count; q++) padded.push_back(padded_rank(ranks[q]));
    std::sort(padded.begin(), padded.end());
    padded.erase(std::unique(padded.begin(), padded.end()), padded.end());
    std::vector<int32_t> classes;
    if (!padded.empty()) {
        if (max_classes < 1) max_classes = 1;
        int32_t top = padded.back();
        classes.push_back(top);
        while ((int32_t)classes.size() < max_classes) {
            // the largest planned rank whose rows are at most half as wide as the current lowest class's
            int32_t next = 0;
            for (int32_t p : padded) if (lds_row_bytes(p) * 2 <= lds_row_bytes(top)) next = p;
            if (!next) break;
            classes.push_back(next);
            top = next;
        }
        std::sort(classes.begin(), classes.end());
    }
    return classes;
}

int plan_class(const vbnmf_matrix *X, int R)
{
    std::lock_guard<std::mutex> g(X->plan_mu);
    for (int32_t c : X->plan) if (c >= R) return c;
    return R;
}

static int check_ranks(const int32_t *ranks, int32_t count)
{
    for (int32_t q = 0; q < count; q++)
        if (ranks[q] < 1 || ranks[q] > VBNMF_MAX_RANK) return fail(VBNMF_ERR_BAD_ARG, "rank %d is outside [1, %d]", ranks[q], VBNMF_MAX_RANK);
    return VBNMF_OK;
}

}  // namespace vbnmf

// ====================================================================== C ABI (layouts and rank plans)
using namespace vbnmf;

extern "C" {

// Rank classes of a sweep over several ranks (reference R/bayesian.R:316: `for(rank in ranks)`, every rank on the same
// matrix).  The tiled layout depends on the rank only through the LDS row size; cutting one per row size costs more host
// time than the whole sweep spends on the device (BASELINE config C4: six geometries, 5 s, against 0.3 s of stepping).
// With a plan, every rank uses the geometry of the smallest class at or above it: narrower blocks than its own rows
// would allow (more, shorter tasks: a slower step), but cut once.  max_classes = 1: one class at the largest rank;
// k > 1: the k - 1 further classes halve the remaining range of row sizes each (largest first).  count = 0 clears it.
int vbnmf_matrix_plan_ranks(vbnmf_matrix *X, const int32_t *ranks, int32_t count, int32_t max_classes)
{
    if (!X || (count > 0 && !ranks) || count < 0) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_ranks(ranks, count)) return rc;
    std::vector<int32_t> classes = rank_classes(ranks, count, max_classes);
    std::lock_guard<std::mutex> g(X->plan_mu);
    X->plan.swap(classes);
    return VBNMF_OK;
}

// Rank classes of a sweep (see vbnmf_matrix_plan_ranks) WITHOUT touching a matrix: classes[0..n) = padded ranks, ascending.
int vbnmf_plan_classes(const int32_t *ranks, int32_t count, int32_t max_classes, int32_t *classes, int32_t *n_classes)
{
    if ((count > 0 && !ranks) || count < 0 || !classes || !n_classes) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_ranks(ranks, count)) return rc;
    const std::vector<int32_t> c = rank_classes(ranks, count, max_classes);
    for (size_t q = 0; q < c.size(); q++) classes[q] = c[q];       // at most `count` entries
    *n_classes = (int32_t)c.size();
    return VBNMF_OK;
}

int vbnmf_layout_build(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t side, int32_t r,
                       vbnmf_layout **out, vbnmf_layout_view *view)
{
    if (!X || !out || !view) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (int rc = check_geometry_args(side, r)) return rc;
    if (X->M.shell) return fail(VBNMF_ERR_STATE, "this matrix handle is a shell (vbnmf_matrix_shell): it holds no entries");
    *out = nullptr;
    vbnmf_layout *H = nullptr;
    try {
        H = new vbnmf_layout();
        int R = std::max(padded_rank(r), plan_class(X, padded_rank(r)));      // the geometry of the rank's class (plan_ranks)
        int64_t nmaj = side == 0 ? X->M.n : col_end - col_begin;
        int64_t nmin = side == 0 ? col_end - col_begin : X->M.n;
        const bool range_ok = col_begin >= 0 && col_end <= X->M.m && col_begin < col_end;      // build_layout reports a bad range
        LayoutParams lp = default_layout_params(nmaj, nmin, R, 0, range_ok ? X->M.colptr[col_end] - X->M.colptr[col_begin] : 0);
        // the cells in the order an engine on these columns uses (order.cpp): the matrix's for the whole matrix, the range's own otherwise
        std::vector<int32_t> own;
        const bool whole = col_begin == 0 && col_end == X->M.m;
        if (!whole && range_ok) own = compute_cell_order(X->M, col_begin, col_end);
        int rc = build_layout(X->M, col_begin, col_end, side, lp, whole ? &X->M.cell_order() : &own, H->L);
        if (rc) { delete H; return rc; }
    } catch (const std::bad_alloc &) {
        delete H;
        return fail(VBNMF_ERR_OOM, "out of host memory building the layout");
    }
    const Layout &L = H->L;
    view->side = L.side; view->wide = L.wide ? 1 : 0;
    view->n_major = L.n_major; view->n_minor = L.n_minor;
    view->block_width = L.block_width; view->n_blocks = L.n_blocks; view->max_len = L.max_len; view->n_wg = L.n_wg;
    view->n_tasks = L.n_tasks; view->n_slices = L.n_slices; view->n_slots = L.n_slots; view->n_segs = L.n_segs;
    view->task_major = L.task_major.data(); view->slice_width = L.slice_width.data();
    view->slice_off = L.slice_off.data(); view->slice_block = L.slice_block.data(); view->slice_fast = L.slice_fast.data();
    view->seg_block = L.seg_block.data(); view->wg_seg0 = L.wg_seg0.data();
    view->seg_ptr = L.seg_ptr.data(); view->row_slots = L.row_slots; view->block_start = L.block_start.data();
    view->inv_ptr = L.inv_ptr.data(); view->inv_task = L.inv_task.data();
    view->packed = L.wide ? nullptr : L.packed.data();
    view->wide_idx = L.wide ? L.wide_idx.data() : nullptr;
    view->wide_val = L.wide ? L.wide_val.data() : nullptr;
    view->cell_perm = L.cell_perm.empty() ? nullptr : L.cell_perm.data();
    view->n_rows = L.n_rows; view->row_ptr = L.row_ptr.data(); view->row_task = L.row_task.data(); view->merge = L.merge ? 1 : 0;
    *out = H;
    return VBNMF_OK;
}

void vbnmf_layout_destroy(vbnmf_layout *L) { delete L; }

}  // extern "C"
