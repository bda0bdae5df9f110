// tests/asan_cophenet_host.cpp -- AddressSanitizer / UBSan pass over the HOST glue of the device cophenetic
// (ccfindr_amd/csrc/consensus.cpp: argument checks, the grouping of the label tuples, the allocation and free paths,
// the downloads and the last step of the correlation), as a CPU build with the device calls stubbed out.  A stand-alone
// program: nothing is loaded into Python and nothing touches a GPU.
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//         -o /tmp/asan_cophenet_host tests/asan_cophenet_host.cpp ccfindr_amd/csrc/consensus.cpp -pthread
//     /tmp/asan_cophenet_host
//
// The stubs below stand for common.h's coph_dev_*: "device" buffers are malloc blocks (so a size the glue gets wrong
// is a heap overflow the sanitizer sees, and a buffer it forgets is a leak), every stub writes or reads each buffer over
// the full extent the kernels use (cophenet.h), and allocation number `fail_at` fails, once for every position.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <random>

#include "../ccfindr_amd/csrc/common.h"

struct vbnmf_consensus {
    int64_t m = 0;
    int32_t runs = 0, unlabelled = 0;
    std::vector<uint8_t> labels;
};

namespace {
int g_allocs = 0, g_live = 0, g_fail_at = -1, g_chain_status = vbnmf::kCophOk;
char g_msg[512];
}

namespace vbnmf {

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}

void parallel_for(int64_t count, const std::function<void(int64_t, int64_t, int)> &fn, int) { if (count > 0) fn(0, count, 0); }

int consensus_download(vbnmf_consensus *c, std::vector<uint8_t> &labels, int64_t &m, int32_t &runs, int32_t &unlabelled, int32_t *device)
{
    labels = c->labels; m = c->m; runs = c->runs; unlabelled = c->unlabelled;
    if (device) *device = 0;
    return VBNMF_OK;
}

int coph_dev_use(int device) { return device == 0 ? VBNMF_OK : fail(VBNMF_ERR_BAD_ARG, "device %d is outside [0, 1)", device); }

int coph_dev_alloc(void **p, size_t bytes, const char *what)
{
    *p = nullptr;
    if (g_allocs++ == g_fail_at) return fail(VBNMF_ERR_OOM, "out of device memory: %zu bytes for %s", bytes, what);
    *p = std::malloc(bytes ? bytes : 1);
    g_live++;
    return VBNMF_OK;
}

void coph_dev_free(void *p)
{
    if (!p) return;
    std::free(p);
    g_live--;
}

int coph_dev_upload(void *dst, const void *src, size_t bytes) { std::memcpy(dst, src, bytes); return VBNMF_OK; }
int coph_dev_download(void *dst, const void *src, size_t bytes) { std::memcpy(dst, src, bytes); return VBNMF_OK; }

static void fill_common(size_t G, const int64_t *sizes, double *W, double *S, double *weight, double *mm)
{
    for (size_t k = 0; k < G * G; k++) { W[k] = 0.5; S[k] = 1.0; }
    for (size_t i = 0; i < G; i++) { weight[i] = (double)sizes[i]; mm[2 * i] = 0.25; mm[2 * i + 1] = 0.75; }
}

int coph_dev_setup_tuples(const uint8_t *tuples, const int64_t *sizes, int G, int R, double *W, double *S, double *weight, unsigned long long *isum, double *mm)
{
    unsigned long long sum = 0;
    for (size_t k = 0; k < (size_t)G * R; k++) sum += tuples[k];
    fill_common((size_t)G, sizes, W, S, weight, mm);
    for (size_t i = 0; i < (size_t)G; i++) { isum[2 * i] = sum % 7 + i; isum[2 * i + 1] = 3 * i + 1; }
    return VBNMF_OK;
}

int coph_dev_setup_dist(const double *dist, const int64_t *sizes, int G, double *W, double *S, double *weight, double *fsum, double *mm)
{
    double sum = 0;
    for (size_t k = 0; k < (size_t)G * G; k++) sum += dist[k];
    fill_common((size_t)G, sizes, W, S, weight, mm);
    for (size_t i = 0; i < (size_t)G; i++) { fsum[2 * i] = sum; fsum[2 * i + 1] = sum * 0.5; }
    return VBNMF_OK;
}

int coph_dev_chain(double *W, double *S, double *weight, int *chain, int G, int link, long long *merges, double *heights, double *out)
{
    (void)link;
    for (int i = 0; i < G; i++) { chain[i] = i; weight[i] += W[(size_t)i * G + G - 1] + S[(size_t)(G - 1) * G + i]; }
    for (int k = 0; k < G - 1; k++) { merges[2 * k] = 0; merges[2 * k + 1] = k + 1; heights[k] = 0.1 * (k + 1); }
    for (int k = 0; k < kCophOut; k++) out[k] = 1.0 + k;
    out[6] = 0.1; out[7] = 0.1 * (G - 1);
    out[8] = (double)g_chain_status; out[9] = (double)(G - 1);
    return VBNMF_OK;
}

}  // namespace vbnmf

#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_msg); return 1; } \
    } while (0)

int main()
{
    std::mt19937_64 rng(5);
    double coph = 0;
    for (int G : {1, 2, 3, 17, 130}) {
        for (int R : {1, 5, 20}) {
            std::vector<uint8_t> tuples((size_t)G * R);
            std::vector<int64_t> sizes((size_t)G);
            std::vector<double> dist((size_t)G * G, 0.0);
            for (auto &t : tuples) t = (uint8_t)(1 + rng() % 3);
            for (auto &s : sizes) s = (int64_t)(1 + rng() % 50);
            for (int i = 0; i < G; i++)
                for (int j = i + 1; j < G; j++) dist[(size_t)i * G + j] = dist[(size_t)j * G + i] = 0.1 + (double)(rng() % 1000) / 1000.0;
            std::vector<int64_t> merges((size_t)(G > 1 ? 2 * (G - 1) : 0));
            std::vector<double> heights((size_t)(G > 1 ? G - 1 : 0));
            // every return path: success, then a failure at each allocation in turn
            for (int fail_at = -1; fail_at < 16; fail_at++) {
                g_fail_at = fail_at;
                g_allocs = 0;
                int rc = vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "average", &coph);
                EXPECT(g_live == 0);
                EXPECT(rc == VBNMF_OK || (rc == VBNMF_ERR_OOM && fail_at >= 0 && fail_at < g_allocs));
                EXPECT(rc != VBNMF_OK || G == 1 || fail_at < 0 || fail_at >= g_allocs);
                g_allocs = 0;
                rc = vbnmf_test_cophenetic_trace(1, 0, G, dist.data(), sizes.data(), "complete", &coph, merges.data(), heights.data());
                EXPECT(g_live == 0);
                EXPECT(rc == VBNMF_OK || rc == VBNMF_ERR_OOM);
                EXPECT(rc != VBNMF_OK || G == 1 || (merges[1] == 1 && heights[(size_t)G - 2] > 0));
            }
            g_fail_at = -1;
            // the host core's trace, and outputs left out
            EXPECT(vbnmf_test_cophenetic_trace(0, 0, G, dist.data(), sizes.data(), "single", &coph, merges.data(), heights.data()) == VBNMF_OK);
            EXPECT(vbnmf_test_cophenetic_trace(0, 0, G, dist.data(), sizes.data(), "average", &coph, nullptr, nullptr) == VBNMF_OK);
            EXPECT(vbnmf_test_cophenetic_trace(1, 0, G, dist.data(), sizes.data(), "average", &coph, nullptr, nullptr) == VBNMF_OK);
            EXPECT(vbnmf_test_cophenetic_trace(-1, 0, G, dist.data(), sizes.data(), "average", &coph, merges.data(), nullptr) == VBNMF_OK);
            // the kernel's status words
            if (G > 1) {
                g_chain_status = vbnmf::kCophNotFinite;
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "single", &coph) == VBNMF_ERR_BAD_ARG);
                g_chain_status = vbnmf::kCophBound;
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "single", &coph) == VBNMF_ERR_STATE);
                g_chain_status = vbnmf::kCophOk;
                EXPECT(g_live == 0 && std::isnan(coph));
                // refused before any allocation
                g_allocs = 0;
                dist[1] = INFINITY;
                EXPECT(vbnmf_test_cophenetic_trace(1, 0, G, dist.data(), sizes.data(), "average", &coph, nullptr, nullptr) == VBNMF_ERR_BAD_ARG);
                sizes[0] = 0;
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                sizes[0] = 200000000; sizes[1] = 200000000;
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                sizes[0] = sizes[1] = 1;
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, tuples.data(), sizes.data(), "ward", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_cophenetic_grouped_device(3, G, R, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, 0, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, 65536, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_cophenetic_grouped_device(0, 0, R, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_cophenetic_grouped_device(0, G, R, nullptr, sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
                EXPECT(vbnmf_test_cophenetic_trace(2, 0, G, dist.data(), sizes.data(), "average", &coph, nullptr, nullptr) == VBNMF_ERR_BAD_ARG);
                EXPECT(g_allocs == 0 && g_live == 0);
            }
        }
    }
    // more groups than the kernel's flags hold: refused from the sizes alone
    {
        const int64_t G = vbnmf::kCophMaxGroups + 1;
        std::vector<uint8_t> tuples((size_t)G, 1);
        std::vector<int64_t> sizes((size_t)G, 1);
        g_allocs = 0;
        EXPECT(vbnmf_cophenetic_grouped_device(0, G, 1, tuples.data(), sizes.data(), "average", &coph) == VBNMF_ERR_BAD_ARG);
        EXPECT(g_allocs == 0);
    }
    // the accumulator's entry: grouping of the downloaded labels, the caps, the choice of the place
    for (int m : {1, 7, 300, 5000}) {
        for (int R : {1, 4, 12}) {
            vbnmf_consensus c;
            c.m = m; c.runs = R;
            c.labels.resize((size_t)m * R);
            for (auto &l : c.labels) l = (uint8_t)(1 + rng() % 4);
            int64_t groups = 0, g2 = 0;
            double host = 0;
            EXPECT(vbnmf_consensus_cophenetic(&c, "average", 1 << 20, &host, &groups) == VBNMF_OK);
            EXPECT(groups >= 1 && groups <= m);
            for (int where : {-1, 0, 1}) {
                for (int fail_at = -1; fail_at < 14; fail_at++) {
                    g_fail_at = fail_at;
                    g_allocs = 0;
                    const int rc = vbnmf_consensus_cophenetic_on(&c, "average", 0, where, &coph, &g2);
                    EXPECT(g_live == 0 && g2 == groups);
                    EXPECT(rc == VBNMF_OK || rc == VBNMF_ERR_OOM);
                    if (where == 0 || (where < 0 && groups <= 4096)) EXPECT(rc == VBNMF_OK && g_allocs == 0);
                    if (where == 0 && groups > 4096) EXPECT(std::isnan(coph));
                }
                g_fail_at = -1;
                EXPECT(vbnmf_consensus_cophenetic_on(&c, "average", groups - 1 > 0 ? groups - 1 : -1, where, &coph, &g2) == VBNMF_OK);
                EXPECT(groups == 1 || std::isnan(coph));
            }
            c.unlabelled = 1;
            EXPECT(vbnmf_consensus_cophenetic_on(&c, "single", 0, 1, &coph, &g2) == VBNMF_OK && std::isnan(coph));
            EXPECT(vbnmf_consensus_cophenetic_on(&c, "single", 0, 5, &coph, &g2) == VBNMF_ERR_BAD_ARG);
            EXPECT(vbnmf_consensus_cophenetic_on(&c, "ward", 0, 1, &coph, &g2) == VBNMF_ERR_BAD_ARG);
        }
    }
    EXPECT(g_live == 0);
    std::printf("asan cophenet host ok\n");
    return 0;
}
