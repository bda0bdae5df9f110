// device.hip -- the definitions behind device.h: the library's one device buffer pool and the device checks.  No kernels.
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "device.h"

namespace vbnmf {

// ---- device buffer pool.  An engine owns ~25 device buffers (state, partial rows up to 100 MB a side, reduce buffers);
// a rank sweep creates and destroys an engine per (run, rank) unit, and every hipFree synchronises the whole device --
// including the streams of other engines of the process (vb_factorize(concurrent = K)).  Freed buffers therefore go to a
// per-process free list and the next engine takes the smallest one that fits (within 1.5 x of the request); the list holds
// at most VBNMF_POOL_MB (default 4096) and gives the oldest buffers back to the driver beyond that.  Measured on the C4
// sweep (19 engines in a row): engine creation + destruction 0.5 s -> 0.1 s (profiles/r04_c4_sweep.json).
struct PoolBuf { void *p; size_t bytes; int device; };
struct DevicePool {
    std::mutex mu;
    std::vector<PoolBuf> free_list;                  // oldest first
    std::vector<PoolBuf> live;                       // buffers handed out (size and device of every pointer)
    size_t held = 0;
    size_t cap = [] { const char *s = getenv("VBNMF_POOL_MB"); long v = s ? atol(s) : 4096; return (size_t)(v < 0 ? 0 : v) << 20; }();
};
DevicePool &device_pool() { static DevicePool *P = new DevicePool(); return *P; }      // (never destroyed: no HIP calls at exit)

// every buffer on the free list goes back to the driver
void pool_drop(DevicePool &P)
{
    std::vector<PoolBuf> drop;
    { std::lock_guard<std::mutex> g(P.mu); drop.swap(P.free_list); P.held = 0; }
    for (const PoolBuf &b : drop) (void)hipFree(b.p);
}

int pool_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (bytes == 0) bytes = 8;
    int device = 0;
    (void)hipGetDevice(&device);
    DevicePool &P = device_pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        int best = -1;
        for (int q = 0; q < (int)P.free_list.size(); q++) {
            const PoolBuf &b = P.free_list[q];
            if (b.device == device && b.bytes >= bytes && b.bytes <= bytes + bytes / 2 + 4096 && (best < 0 || b.bytes < P.free_list[best].bytes)) best = q;
        }
        if (best >= 0) {
            PoolBuf b = P.free_list[best];
            P.free_list.erase(P.free_list.begin() + best);
            P.held -= b.bytes;
            P.live.push_back(b);
            *p = b.p;
            return VBNMF_OK;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {                  // give the pooled buffers back and try once more
        (void)hipGetLastError();
        pool_drop(P);
        e = hipMalloc(p, bytes);
    }
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(VBNMF_ERR_OOM, "out of device memory (%zu bytes)", bytes); }
    if (e != hipSuccess) return fail(VBNMF_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> g(P.mu);
    P.live.push_back({*p, bytes, device});
    return VBNMF_OK;
}

// The caller guarantees that no queued work still uses the buffer (engines synchronise their streams before they free).
void dev_free(void *p)
{
    if (!p) return;
    DevicePool &P = device_pool();
    std::vector<PoolBuf> drop;
    {
        std::lock_guard<std::mutex> g(P.mu);
        PoolBuf b{p, 0, 0};
        bool known = false;
        for (size_t q = 0; q < P.live.size(); q++)
            if (P.live[q].p == p) { b = P.live[q]; P.live.erase(P.live.begin() + q); known = true; break; }
        if (!known || P.cap == 0 || b.bytes > P.cap) { drop.push_back(b); }
        else {
            P.free_list.push_back(b);
            P.held += b.bytes;
            while (P.held > P.cap && !P.free_list.empty()) {
                drop.push_back(P.free_list.front());
                P.held -= P.free_list.front().bytes;
                P.free_list.erase(P.free_list.begin());
            }
        }
    }
    for (const PoolBuf &b : drop) (void)hipFree(b.p);
}

int check_device(int device)
{
    int cnt = 0;
    hipError_t err = hipGetDeviceCount(&cnt);
    if (err != hipSuccess || cnt <= 0) {
        (void)hipGetLastError();
        return fail(VBNMF_ERR_NO_DEVICE, "no HIP device is available (%s); this library has no CPU fallback",
                    err != hipSuccess ? hipGetErrorString(err) : "device count is 0");
    }
    if (device < 0 || device >= cnt) return fail(VBNMF_ERR_BAD_ARG, "device %d is outside [0, %d)", device, cnt);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VBNMF_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device, prop.gcnArchName);
    return VBNMF_OK;
}

int use_device(int device)
{
    if (int rc = check_device(device)) return rc;
    HIPCHECK(hipSetDevice(device));
    return VBNMF_OK;
}

int device_cus(int device, int &cus)
{
    cus = 0;
    HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus <= 0) cus = 256;
    return VBNMF_OK;
}

}  // namespace vbnmf

// Gives every device buffer the pool holds back to the driver (buffers in use by live engines are not touched).
extern "C" void vbnmf_pool_trim(void) { vbnmf::pool_drop(vbnmf::device_pool()); }
