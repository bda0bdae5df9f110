// cophenet.hip -- the host's handle on the grouped cophenetic's kernels (cophenet.h), as common.h declares it; consensus.cpp
// holds the glue and stays free of HIP calls.
#include "cophenet.h"
#include "device.h"

namespace vbnmf {

int coph_dev_use(int device) { return use_device(device); }

int coph_dev_alloc(void **p, size_t bytes, const char *what)
{
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e == hipSuccess) return VBNMF_OK;
    (void)hipGetLastError();
    *p = nullptr;
    if (e == hipErrorOutOfMemory) return fail(VBNMF_ERR_OOM, "out of device memory: %zu bytes for %s", bytes, what);
    return fail(VBNMF_ERR_HIP, "hipMalloc of %zu bytes for %s failed: %s", bytes, what, hipGetErrorString(e));
}

void coph_dev_free(void *p)
{
    if (p) (void)hipFree(p);
}

int coph_dev_upload(void *dst, const void *src, size_t bytes)
{
    if (bytes) HIPCHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return VBNMF_OK;
}

int coph_dev_download(void *dst, const void *src, size_t bytes)
{
    if (bytes) HIPCHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return VBNMF_OK;
}

int coph_dev_setup_tuples(const uint8_t *tuples, const int64_t *sizes, int G, int R, double *W, double *S, double *weight, unsigned long long *isum, double *mm)
{
    hipLaunchKernelGGL(k_coph_setup_tuples, dim3((unsigned)G), dim3(kCophSetupThreads), 0, 0, tuples, sizes, G, R, W, S, weight, isum, mm);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int coph_dev_setup_dist(const double *dist, const int64_t *sizes, int G, double *W, double *S, double *weight, double *fsum, double *mm)
{
    hipLaunchKernelGGL(k_coph_setup_dist, dim3((unsigned)G), dim3(kCophSetupThreads), 0, 0, dist, sizes, G, W, S, weight, fsum, mm);
    HIPCHECK(hipGetLastError());
    return VBNMF_OK;
}

int coph_dev_chain(double *W, double *S, double *weight, int *chain, int G, int link, long long *merges, double *heights, double *out)
{
    hipLaunchKernelGGL(k_coph_chain, dim3(1), dim3(kCophChainThreads), 0, 0, W, S, weight, chain, G, link, merges, heights, out);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    return VBNMF_OK;
}

}  // namespace vbnmf
