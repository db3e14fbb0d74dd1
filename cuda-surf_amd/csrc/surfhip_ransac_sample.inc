// surfhip_ransac_sample.inc -- the sampler of both RANSAC kernels (included by
// surfhip_ransac.inc, inside an anonymous namespace): K distinct candidate
// ranks from a counter hash of (seed, hypothesis, n).  __host__ __device__, so
// that tests/host/fundamental_math_main.cpp runs the very same draw.
// surfhip_fundamental_math.inc includes it too: once per translation unit.
#pragma once

__host__ __device__ __forceinline__ uint32_t fd_fmix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// K distinct indices below n (n >= K): draw j picks among the n - j indices
// not taken yet, in ascending order of those
template <int K>
__host__ __device__ __forceinline__ void fd_sample(uint32_t seed, uint32_t hyp, int n, int (&idx)[K])
{
    int s[K];                               // the picks so far, ascending
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t r = fd_fmix32(seed ^ (0x9E3779B9u * ((uint32_t)K * hyp + (uint32_t)j + 1u)));
        int d = (int)(r % (uint32_t)(n - j));
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (i < j && d >= s[i]) ++d;
        idx[j] = d;
        int cur = d;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < j) {
                const int lo = min(s[i], cur), hi = max(s[i], cur);
                s[i] = lo;
                cur = hi;
            }
            if (i == j) s[i] = cur;
        }
    }
}
