// philox.h -- counter-based random numbers on the device: Philox4x32-10, a 53-bit uniform, and the Gamma variate of the
// 'random' initial state.  The draws are a function of (seed, factor, element) only, so they do not depend on the launch
// geometry, the device or the rank count of a partitioned run.  (R's RNG stream cannot be matched outside R.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vbnmf {

// ---------------------------------------------------------------- Philox4x32-10
struct Philox {
    uint32_t c[4], k[2];
};
__host__ __device__ __forceinline__ void philox_round(uint32_t (&c)[4], const uint32_t (&k)[2])
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
// 4 x 32 random bits for counter (i0, i1, i2, i3) under key (k0, k1)
__host__ __device__ __forceinline__ void philox4x32(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t k0, uint32_t k1,
                                                    uint32_t (&out)[4])
{
    uint32_t c[4] = {i0, i1, i2, i3}, k[2] = {k0, k1};
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox_round(c, k);
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}
// uniform in (0, 1): 53 bits, never 0 or 1
__host__ __device__ __forceinline__ double u53(uint32_t hi, uint32_t lo)
{
    const uint64_t v = ((uint64_t)hi << 21) ^ (uint64_t)(lo >> 11);              // 53 bits
    return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}

// One Gamma(shape a, scale s) variate for stream (element, factor) of key seed.  Marsaglia & Tsang (2000): for a >= 1,
// d = a - 1/3, c = 1/sqrt(9d): x ~ N(0,1), v = (1 + c x)^3, accept if v > 0 and log u < x^2/2 + d - d v + d log v;
// a < 1: Gamma(a + 1) u^(1/a).  Attempt t of the stream uses counter (element lo, element hi, factor, t).
__device__ inline double gamma_draw(double a, double scale, uint64_t element, uint32_t factor, uint32_t k0, uint32_t k1)
{
    const double a1 = a < 1.0 ? a + 1.0 : a;
    const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = 0.0;
    uint32_t r[4];
    for (uint32_t t = 0; t < 64; t++) {                       // acceptance > 0.95 per attempt: 64 never runs out in practice
        philox4x32((uint32_t)element, (uint32_t)(element >> 32), factor, 2 * t, k0, k1, r);
        const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);     // Box-Muller
        philox4x32((uint32_t)element, (uint32_t)(element >> 32), factor, 2 * t + 1, k0, k1, r);
        const double u = u53(r[0], r[1]);
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = v1 * v1 * v1;
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) {
            g = d * v;
            if (a < 1.0) g *= pow(u53(r[2], r[3]), 1.0 / a);
            break;
        }
    }
    return g * scale;
}

}  // namespace vbnmf
