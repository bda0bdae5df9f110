// device.h -- the host side's device runtime, shared by every .hip unit: the error macro, the device buffer pool's interface
// (defined once, in device.hip: the library holds ONE pool), the device checks, and DeviceCall, the owner of what a library
// call holds on a device while it runs.  Nothing here has state of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <type_traits>
#include <vector>

#include "common.h"

#define HIPCHECK(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return fail(VBNMF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace vbnmf {

int pool_alloc(void **p, size_t bytes);      // a buffer of the current device, from the pool or the driver
void dev_free(void *p);                      // back to the pool; no queued work may still use it
int check_device(int device);                // the device exists and is a gfx950
int use_device(int device);                  // ... and is current
int device_cus(int device, int &cus);        // its compute units (256 where the runtime reports none)

using host_clock = std::chrono::steady_clock;      // the host-side split times the *_info calls report
inline double ms_since(host_clock::time_point t0) { return std::chrono::duration<double, std::milli>(host_clock::now() - t0).count(); }

template <typename T>
int dev_alloc(T **p, size_t count)
{
    return pool_alloc((void **)p, (count ? count : 1) * sizeof(T));
}

template <typename T>
int dev_upload(T **p, const T *src, size_t count)
{
    if (int rc = dev_alloc(p, count)) return rc;
    if (count) HIPCHECK(hipMemcpy((void *)*p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return VBNMF_OK;
}
template <typename T, typename V>            // V: ExtVec<T> or a std::vector of T
int dev_upload(T **p, const V &v) { return dev_upload(p, v.data(), v.size()); }

// A library call's stay on a device: enter() makes the device current, alloc() / upload() hand out pool buffers (into the
// caller's typed pointers; `const T *` too) and remember them, ev0 / ev1 time the kernels on the null stream.  The
// destructor waits for the null stream if `queued` says work may still run, returns the buffers, destroys the events and
// makes the caller's device current again -- on every path out of the call.
struct DeviceCall {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool queued = false;

    DeviceCall() = default;
    DeviceCall(const DeviceCall &) = delete;
    int enter(int device)
    {
        (void)hipGetDevice(&caller_device);
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(hipEventCreate(&ev0));
        HIPCHECK(hipEventCreate(&ev1));
        return VBNMF_OK;
    }
    template <typename T>
    int alloc(T **p, size_t count)
    {
        bufs.push_back(nullptr);                 // (room first: a buffer is never handed out unregistered)
        if (int rc = dev_alloc(p, count)) return rc;
        bufs.back() = (void *)*p;
        return VBNMF_OK;
    }
    template <typename T>
    int upload(T **p, const std::remove_const_t<T> *src, size_t count)
    {
        if (int rc = alloc(p, count)) return rc;
        if (count) HIPCHECK(hipMemcpy((void *)*p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return VBNMF_OK;
    }
    ~DeviceCall()
    {
        if (queued) (void)hipStreamSynchronize(nullptr);
        for (void *p : bufs) dev_free(p);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (caller_device >= 0) (void)hipSetDevice(caller_device);
    }

private:
    std::vector<void *> bufs;
    int caller_device = -1;      // the device that was current when the call came in
};

}  // namespace vbnmf
