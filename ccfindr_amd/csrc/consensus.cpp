// consensus.cpp -- the cophenetic correlation of factorize()'s consensus matrix (reference R/factorize.R:69-78:
// hclust / cophenetic / cor on 1 - conav) in grouped form, on the host.
//
// Cells that carry the same label in every run are at distance 0 from each other and at the same distance from every
// other cell; whatever the linkage, they are joined first, at height 0, in any order.  Above that level the dendrogram is
// the dendrogram of the G distinct label tuples ("groups"), weighted by the group sizes, with distance = Hamming distance
// of the tuples / runs.  The correlation runs over all m (m - 1) / 2 pairs of cells: a pair inside a group has distance
// and cophenetic distance 0, a pair between groups a, b counts size_a * size_b times.
//
// Agglomeration: nearest-neighbour chain (valid for the reducible linkages served here: average, single, complete), O(G^2)
// work on one G x G matrix of doubles.  Ties: the nearest neighbour of the chain's tip is the group the chain came from
// if that one is among the nearest, else the nearest with the lowest number; a merged cluster keeps the lower number of
// its two parts.  Under ties at positive heights 'average' and 'complete' return the coefficient of ONE valid dendrogram,
// not necessarily the one another scan order would build; 'single' does not depend on the choice.
//
// Past the host form's cap the same agglomeration runs on the device (cophenet.h): this file keeps its host glue --
// argument checks, buffers, the last step of the correlation -- free of HIP calls (common.h: coph_dev_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <unordered_map>

#include "common.h"

using namespace vbnmf;

namespace {

enum class Link { average, single, complete };

int parse_method(const char *method, Link &link)
{
    if (method && !std::strcmp(method, "average")) { link = Link::average; return VBNMF_OK; }
    if (method && !std::strcmp(method, "single")) { link = Link::single; return VBNMF_OK; }
    if (method && !std::strcmp(method, "complete")) { link = Link::complete; return VBNMF_OK; }
    return fail(VBNMF_ERR_BAD_ARG, "linkage '%s' is not served by the grouped cophenetic (average, single, complete)", method ? method : "(null)");
}

// What the correlation is formed from, on either path: the sums over all pairs of cells and the ranges of both sides.
struct PairSums {
    long double npair = 0, sd = 0, sdd = 0, sc = 0, scc = 0, sdc = 0;
    double dmin = 0, dmax = 0, cmin = 0, cmax = 0;
};

void correlation(const PairSums &p, double *coph)
{
    if (!(p.dmax > p.dmin) || !(p.cmax > p.cmin)) return;        // cor() of a constant: NA in the reference
    const long double vd = p.sdd - p.sd * p.sd / p.npair, vc = p.scc - p.sc * p.sc / p.npair;
    if (!(vd > 0) || !(vc > 0)) return;
    *coph = (double)((p.sdc - p.sd * p.sc / p.npair) / std::sqrt(vd * vc));
}

// One of the walk's five sums.  Up to kPlainSumGroups groups it is the plain long double sum it always was, so that no
// result at those sizes moves.  Above -- sizes the accumulator's entry answered with NaN until the device path came -- the
// rounding error of every addition is kept beside the sum (Neumaier): the walk then adds G^2 / 2 terms, 1.8e7 at 6000
// groups, and where the cophenetic distances have little variance the correlation magnifies what a plain sum loses a
// thousandfold (5999 groups of random labels, 'average': 1.8e-12 off the exact value with plain sums).
constexpr int64_t kPlainSumGroups = 4096;
struct WalkSum {
    long double s = 0, c = 0;
    bool compensated = false;
    void add(long double v)
    {
        if (!compensated) { s += v; return; }
        const long double t = s + v;
        c += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
        s = t;
    }
    long double value() const { return compensated ? s + c : s; }
};

// orig(i, j): distance of groups i != j.  Returns the correlation, NaN when distance or cophenetic distance has no variance.
// merges ([G-1][2]: the cluster kept, the cluster dropped) and heights ([G-1]) record the dendrogram when not null.
template <class Orig>
int cophenetic_core(int64_t G, const int64_t *sizes, Link link, Orig orig, double *coph, int64_t *merges = nullptr, double *heights = nullptr)
{
    *coph = std::numeric_limits<double>::quiet_NaN();
    long double cells = 0;
    bool inside = false;                       // some group holds a pair of cells: a pair with d = c = 0
    for (int64_t g = 0; g < G; g++) {
        if (sizes[g] < 1) return fail(VBNMF_ERR_BAD_ARG, "group %lld has size %lld", (long long)g, (long long)sizes[g]);
        cells += (long double)sizes[g];
        inside = inside || sizes[g] > 1;
    }
    const long double npair = cells * (cells - 1) / 2;
    if (G < 2) return VBNMF_OK;                // one group: every distance is 0
    std::vector<double> W;
    std::vector<int64_t> next, tail, chain;
    std::vector<double> weight;
    std::vector<char> active;
    try {
        W.resize((size_t)G * G);
        next.assign((size_t)G, -1); tail.resize((size_t)G); chain.reserve((size_t)G);
        weight.resize((size_t)G); active.assign((size_t)G, 1);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the %lld x %lld group distance matrix", (long long)G, (long long)G);
    }
    for (int64_t i = 0; i < G; i++) {
        tail[i] = i; weight[i] = (double)sizes[i];
        W[(size_t)i * G + i] = 0.0;
        for (int64_t j = i + 1; j < G; j++) W[(size_t)i * G + j] = W[(size_t)j * G + i] = orig(i, j);
    }
    WalkSum sd, sdd, sc, scc, sdc;
    sd.compensated = sdd.compensated = sc.compensated = scc.compensated = sdc.compensated = G > kPlainSumGroups;
    double dmin = inside ? 0.0 : HUGE_VAL, dmax = inside ? 0.0 : -HUGE_VAL, cmin = dmin, cmax = dmax;
    int64_t lowest = 0;                        // no active group below this number
    for (int64_t left = G; left > 1; left--) {
        if (chain.empty()) {
            while (!active[lowest]) lowest++;
            chain.push_back(lowest);
        }
        int64_t x, y;
        for (;;) {
            x = chain.back();
            const double *row = &W[(size_t)x * G];
            const int64_t prev = chain.size() >= 2 ? chain[chain.size() - 2] : -1;
            y = prev;
            double best = prev >= 0 ? row[prev] : HUGE_VAL;
            for (int64_t j = lowest; j < G; j++)
                if (active[j] && j != x && row[j] < best) { best = row[j]; y = j; }
            if (y < 0) return fail(VBNMF_ERR_BAD_ARG, "group distances must be finite");
            if (y == prev) break;              // reciprocal nearest neighbours
            chain.push_back(y);
        }
        chain.pop_back(); chain.pop_back();
        const double h = W[(size_t)x * G + y];
        // every pair of groups meets in exactly one merge: their cophenetic distance is its height
        for (int64_t i = x; i >= 0; i = next[i])
            for (int64_t j = y; j >= 0; j = next[j]) {
                const double d = orig(i, j);
                const long double w = (long double)sizes[i] * (long double)sizes[j];
                sd.add(w * d); sdd.add(w * d * d); sc.add(w * h); scc.add(w * h * h); sdc.add(w * d * h);
                dmin = std::min(dmin, d); dmax = std::max(dmax, d);
            }
        cmin = std::min(cmin, h); cmax = std::max(cmax, h);
        const int64_t keep = std::min(x, y), drop = std::max(x, y);
        if (merges) { merges[2 * (G - left)] = keep; merges[2 * (G - left) + 1] = drop; }
        if (heights) heights[G - left] = h;
        const double wk = weight[keep], wd = weight[drop];
        double *rk = &W[(size_t)keep * G];
        const double *rd = &W[(size_t)drop * G];
        for (int64_t k = lowest; k < G; k++) {
            if (!active[k] || k == keep || k == drop) continue;
            double v;
            switch (link) {
                case Link::single: v = std::min(rk[k], rd[k]); break;
                case Link::complete: v = std::max(rk[k], rd[k]); break;
                default: v = (wk * rk[k] + wd * rd[k]) / (wk + wd); break;
            }
            rk[k] = v; W[(size_t)k * G + keep] = v;
        }
        active[drop] = 0;
        weight[keep] = wk + wd;
        next[tail[keep]] = drop; tail[keep] = tail[drop];
    }
    PairSums p;
    p.npair = npair; p.sd = sd.value(); p.sdd = sdd.value(); p.sc = sc.value(); p.scc = scc.value(); p.sdc = sdc.value();
    p.dmin = dmin; p.dmax = dmax; p.cmin = cmin; p.cmax = cmax;
    correlation(p, coph);
    return VBNMF_OK;
}

// Device buffers of one call: whatever was allocated is freed on every return path.
struct DeviceBuffers {
    std::vector<void *> held;
    ~DeviceBuffers() { for (void *p : held) coph_dev_free(p); }
    template <class T>
    int get(T **p, size_t count, const char *what)
    {
        void *q = nullptr;
        if (int rc = coph_dev_alloc(&q, count * sizeof(T), what)) return rc;
        held.push_back(q);
        *p = static_cast<T *>(q);
        return VBNMF_OK;
    }
};

// The same coefficient with the agglomeration on device `device` (cophenet.h).  Exactly one of tuples ([G][R] labels) and
// dist ([G][G] distances, R = 1) is given.  Everything that can be refused is refused before the first launch.
int cophenetic_device(int device, int64_t G, int32_t R, const uint8_t *tuples, const double *dist, const int64_t *sizes, Link link,
                      double *coph, int64_t *merges, double *heights)
{
    *coph = std::numeric_limits<double>::quiet_NaN();
    long double cells = 0;
    bool inside = false;
    for (int64_t g = 0; g < G; g++) {
        if (sizes[g] < 1) return fail(VBNMF_ERR_BAD_ARG, "group %lld has size %lld", (long long)g, (long long)sizes[g]);
        cells += (long double)sizes[g];
        inside = inside || sizes[g] > 1;
    }
    // the weighted sums S are integer-valued doubles: exact below 2^53
    if (cells * cells * (long double)R / 2 >= 9007199254740992.0L)
        return fail(VBNMF_ERR_BAD_ARG, "cells^2 * runs / 2 must stay below 2^53 on the device path (%.0Lf cells, %d runs)", cells, R);
    if (dist)
        for (int64_t i = 0; i < G; i++)
            for (int64_t j = i + 1; j < G; j++)
                if (!std::isfinite(dist[(size_t)i * G + j])) return fail(VBNMF_ERR_BAD_ARG, "group distances must be finite");
    if (G < 2) return VBNMF_OK;                // one group: every distance is 0
    if (G > kCophMaxGroups)
        return fail(VBNMF_ERR_BAD_ARG, "the device path serves at most %lld groups (%lld given)", (long long)kCophMaxGroups, (long long)G);
    if (int rc = coph_dev_use(device)) return rc;

    const size_t g = (size_t)G, gg = g * g;
    DeviceBuffers dev;
    double *W = nullptr, *S = nullptr, *weight = nullptr, *rowsum = nullptr, *mm = nullptr, *d_heights = nullptr, *out = nullptr, *d_dist = nullptr;
    unsigned long long *isum = nullptr;
    uint8_t *d_tuples = nullptr;
    int64_t *d_sizes = nullptr;
    long long *d_merges = nullptr;
    int *chain = nullptr;
    if (int rc = dev.get(&W, gg, "the group distance matrix")) return rc;
    if (int rc = dev.get(&S, gg, "the weighted distance sums")) return rc;
    if (int rc = dev.get(&weight, g, "the cluster weights")) return rc;
    if (int rc = dev.get(&mm, 2 * g, "the row ranges")) return rc;
    if (int rc = dev.get(&d_sizes, g, "the group sizes")) return rc;
    if (int rc = dev.get(&chain, g, "the chain")) return rc;
    if (int rc = dev.get(&d_merges, 2 * (g - 1), "the merge list")) return rc;
    if (int rc = dev.get(&d_heights, g - 1, "the merge heights")) return rc;
    if (int rc = dev.get(&out, (size_t)kCophOut, "the result block")) return rc;
    if (int rc = coph_dev_upload(d_sizes, sizes, g * sizeof(int64_t))) return rc;
    std::vector<double> h_mm, h_fsum;
    std::vector<unsigned long long> h_isum;
    std::vector<long long> h_merges;
    try {
        h_mm.resize(2 * g);
        if (tuples) h_isum.resize(2 * g); else h_fsum.resize(2 * g);
        if (merges) h_merges.resize(2 * (g - 1));
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the row sums of %lld groups", (long long)G);
    }
    if (tuples) {
        if (int rc = dev.get(&d_tuples, g * (size_t)R, "the label tuples")) return rc;
        if (int rc = dev.get(&isum, 2 * g, "the row sums")) return rc;
        if (int rc = coph_dev_upload(d_tuples, tuples, g * (size_t)R)) return rc;
        if (int rc = coph_dev_setup_tuples(d_tuples, d_sizes, (int)G, R, W, S, weight, isum, mm)) return rc;
    } else {
        if (int rc = dev.get(&d_dist, gg, "the given distances")) return rc;
        if (int rc = dev.get(&rowsum, 2 * g, "the row sums")) return rc;
        if (int rc = coph_dev_upload(d_dist, dist, gg * sizeof(double))) return rc;
        if (int rc = coph_dev_setup_dist(d_dist, d_sizes, (int)G, W, S, weight, rowsum, mm)) return rc;
    }
    if (int rc = coph_dev_chain(W, S, weight, chain, (int)G, (int)link, d_merges, d_heights, out)) return rc;
    double res[kCophOut];
    if (int rc = coph_dev_download(res, out, sizeof res)) return rc;
    if (int rc = coph_dev_download(h_mm.data(), mm, 2 * g * sizeof(double))) return rc;
    if (tuples) { if (int rc = coph_dev_download(h_isum.data(), isum, 2 * g * sizeof(unsigned long long))) return rc; }
    else if (int rc = coph_dev_download(h_fsum.data(), rowsum, 2 * g * sizeof(double))) return rc;
    if ((int)res[8] == kCophNotFinite) return fail(VBNMF_ERR_BAD_ARG, "group distances must be finite");
    if ((int)res[8] != kCophOk || (int64_t)res[9] != G - 1)
        return fail(VBNMF_ERR_STATE, "the device agglomeration stopped at a loop bound after %lld of %lld merges", (long long)res[9], (long long)(G - 1));
    if (merges) {
        if (int rc = coph_dev_download(h_merges.data(), d_merges, 2 * (g - 1) * sizeof(long long))) return rc;
        for (size_t k = 0; k < 2 * (g - 1); k++) merges[k] = (int64_t)h_merges[k];
    }
    if (heights) if (int rc = coph_dev_download(heights, d_heights, (g - 1) * sizeof(double))) return rc;

    PairSums p;
    p.npair = cells * (cells - 1) / 2;
    p.dmin = inside ? 0.0 : HUGE_VAL; p.dmax = inside ? 0.0 : -HUGE_VAL;
    for (size_t i = 0; i < g; i++) {
        const long double si = (long double)sizes[i];
        if (tuples) { p.sd += si * (long double)h_isum[2 * i]; p.sdd += si * (long double)h_isum[2 * i + 1]; }
        else { p.sd += si * (long double)h_fsum[2 * i]; p.sdd += si * (long double)h_fsum[2 * i + 1]; }
        p.dmin = std::min(p.dmin, h_mm[2 * i]); p.dmax = std::max(p.dmax, h_mm[2 * i + 1]);
    }
    const long double runs = (long double)R;   // the integer sums count Hamming distances: d = ham / R
    p.sd /= runs; p.sdd /= runs * runs;
    p.sc = (long double)res[0] + (long double)res[1];
    p.scc = (long double)res[2] + (long double)res[3];
    p.sdc = ((long double)res[4] + (long double)res[5]) / runs;
    p.cmin = std::min(inside ? 0.0 : HUGE_VAL, res[6]); p.cmax = std::max(inside ? 0.0 : -HUGE_VAL, res[7]);
    correlation(p, coph);
    return VBNMF_OK;
}

int check_where(int32_t where)
{
    if (where < -1 || where > 1) return fail(VBNMF_ERR_BAD_ARG, "where must be 0 (host), 1 (device) or -1 (by size), not %d", where);
    return VBNMF_OK;
}

}  // namespace

extern "C" {

int vbnmf_cophenetic_grouped(int64_t G, int32_t R, const uint8_t *tuples, const int64_t *sizes, const char *method, double *coph)
{
    if (!tuples || !sizes || !coph) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (G < 1 || R < 1 || R > 65535) return fail(VBNMF_ERR_BAD_ARG, "grouped cophenetic needs G >= 1 groups and 1 <= R <= 65535 runs");
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    std::vector<uint16_t> ham;                 // Hamming distances of the tuples
    try { ham.resize((size_t)G * G); } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory for the %lld x %lld group distance matrix", (long long)G, (long long)G);
    }
    parallel_for(G, [&](int64_t g0, int64_t g1, int) {
        for (int64_t i = g0; i < g1; i++) {
            const uint8_t *ti = tuples + (size_t)i * R;
            for (int64_t j = 0; j < G; j++) {
                const uint8_t *tj = tuples + (size_t)j * R;
                int d = 0;
                for (int32_t a = 0; a < R; a++) d += ti[a] != tj[a];
                ham[(size_t)i * G + j] = (uint16_t)d;
            }
        }
    });
    const double runs = (double)R;
    return cophenetic_core(G, sizes, link, [&](int64_t i, int64_t j) { return (double)ham[(size_t)i * G + j] / runs; }, coph);
}

int vbnmf_cophenetic_grouped_device(int32_t device, int64_t G, int32_t R, const uint8_t *tuples, const int64_t *sizes, const char *method, double *coph)
{
    if (!tuples || !sizes || !coph) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (G < 1 || R < 1 || R > 65535) return fail(VBNMF_ERR_BAD_ARG, "grouped cophenetic needs G >= 1 groups and 1 <= R <= 65535 runs");
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    try {
        return cophenetic_device(device, G, R, tuples, nullptr, sizes, link, coph, nullptr, nullptr);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory in the device cophenetic");
    }
}

int vbnmf_test_cophenetic_trace(int32_t where, int32_t device, int64_t G, const double *dist, const int64_t *sizes, const char *method, double *coph,
                                int64_t *merges, double *heights)
{
    if (!dist || !sizes || !coph) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (G < 1) return fail(VBNMF_ERR_BAD_ARG, "grouped cophenetic needs G >= 1 groups");
    if (int rc = check_where(where)) return rc;
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    if (where == 0 || (where < 0 && G <= 4096))
        return cophenetic_core(G, sizes, link, [&](int64_t i, int64_t j) { return dist[(size_t)i * G + j]; }, coph, merges, heights);
    try {
        return cophenetic_device(device, G, 1, nullptr, dist, sizes, link, coph, merges, heights);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory in the device cophenetic");
    }
}

int vbnmf_test_cophenetic_dist(int64_t G, const double *dist, const int64_t *sizes, const char *method, double *coph)
{
    if (!dist || !sizes || !coph) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    if (G < 1) return fail(VBNMF_ERR_BAD_ARG, "grouped cophenetic needs G >= 1 groups");
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    return cophenetic_core(G, sizes, link, [&](int64_t i, int64_t j) { return dist[(size_t)i * G + j]; }, coph);
}

int vbnmf_consensus_cophenetic(vbnmf_consensus *c, const char *method, int64_t max_groups, double *coph, int64_t *groups)
{
    return vbnmf_consensus_cophenetic_on(c, method, max_groups, 0, coph, groups);
}

int vbnmf_consensus_cophenetic_on(vbnmf_consensus *c, const char *method, int64_t max_groups, int32_t where, double *coph, int64_t *groups)
{
    if (!c || !coph || !groups) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *coph = std::numeric_limits<double>::quiet_NaN();
    *groups = 0;
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    if (int rc = check_where(where)) return rc;
    const bool stated = max_groups > 0;        // an explicit cap holds on either path
    if (!stated) max_groups = where == 0 ? 4096 : kCophMaxGroups;
    std::vector<uint8_t> labels;
    int64_t m = 0;
    int32_t R = 0, unlabelled = 0, device = 0;
    if (int rc = consensus_download(c, labels, m, R, unlabelled, &device)) return rc;
    if (R < 1) return fail(VBNMF_ERR_STATE, "cophenetic before the first run was added");
    try {
        // distinct label tuples, numbered by their first cell
        std::unordered_map<std::string, int64_t> seen;
        std::vector<uint8_t> tuples;
        std::vector<int64_t> sizes;
        std::string key((size_t)R, '\0');
        for (int64_t j = 0; j < m; j++) {
            for (int32_t a = 0; a < R; a++) key[(size_t)a] = (char)labels[(size_t)a * m + j];
            auto it = seen.find(key);
            if (it == seen.end()) {
                seen.emplace(key, (int64_t)sizes.size());
                sizes.push_back(1);
                tuples.insert(tuples.end(), key.begin(), key.end());
            } else {
                sizes[(size_t)it->second]++;
            }
        }
        *groups = (int64_t)sizes.size();
        if (unlabelled || *groups > max_groups) return VBNMF_OK;         // NaN: a missing label, or past the stated cap
        if (where == 0 || (where < 0 && *groups <= 4096)) return vbnmf_cophenetic_grouped(*groups, R, tuples.data(), sizes.data(), method, coph);
        if (*groups > kCophMaxGroups) return VBNMF_OK;                   // NaN: past what the device path serves
        return vbnmf_cophenetic_grouped_device(device, *groups, R, tuples.data(), sizes.data(), method, coph);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory grouping the label tuples");
    }
}

}  // extern "C"
