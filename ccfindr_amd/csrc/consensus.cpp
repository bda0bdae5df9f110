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

// orig(i, j): distance of groups i != j.  Returns the correlation, NaN when distance or cophenetic distance has no variance.
template <class Orig>
int cophenetic_core(int64_t G, const int64_t *sizes, Link link, Orig orig, double *coph)
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
    long double sd = 0, sdd = 0, sc = 0, scc = 0, sdc = 0;
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
                sd += w * d; sdd += w * d * d; sc += w * h; scc += w * h * h; sdc += w * d * h;
                dmin = std::min(dmin, d); dmax = std::max(dmax, d);
            }
        cmin = std::min(cmin, h); cmax = std::max(cmax, h);
        const int64_t keep = std::min(x, y), drop = std::max(x, y);
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
    if (!(dmax > dmin) || !(cmax > cmin)) return VBNMF_OK;       // cor() of a constant: NA in the reference
    const long double vd = sdd - sd * sd / npair, vc = scc - sc * sc / npair;
    if (!(vd > 0) || !(vc > 0)) return VBNMF_OK;
    *coph = (double)((sdc - sd * sc / npair) / std::sqrt(vd * vc));
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
    if (!c || !coph || !groups) return fail(VBNMF_ERR_BAD_ARG, "NULL argument");
    *coph = std::numeric_limits<double>::quiet_NaN();
    *groups = 0;
    Link link;
    if (int rc = parse_method(method, link)) return rc;
    if (max_groups <= 0) max_groups = 4096;
    std::vector<uint8_t> labels;
    int64_t m = 0;
    int32_t R = 0, unlabelled = 0;
    if (int rc = consensus_download(c, labels, m, R, unlabelled)) return rc;
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
        return vbnmf_cophenetic_grouped(*groups, R, tuples.data(), sizes.data(), method, coph);
    } catch (const std::bad_alloc &) {
        return fail(VBNMF_ERR_OOM, "out of host memory grouping the label tuples");
    }
}

}  // extern "C"
