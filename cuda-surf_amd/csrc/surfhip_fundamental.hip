// surfhip_fundamental.hip -- batched RANSAC fundamental matrices
// (surfhip_fundamental_batch) for gfx950.  No reference counterpart: main.cpp
// only draws the matches.
//
// The epipolar model of the RANSAC driver in surfhip_ransac.inc, which
// describes the input, the phases and why a pair's result is bit-identical
// from run to run.  What is the fundamental matrix's own (its arithmetic is
// surfhip_fundamental_math.inc):
//   distance: the squared Sampson distance, fp32.
//   hypothesis: eight candidates, the Hartley-normalised 8-point solve in
//      fp64 registers, Frobenius norm 1, not rank-2 projected.
//   refit: normalised 8-point least squares over the current inliers (the 36
//      distinct moments of the 9 x 9 normal matrix), then cyclic Jacobi in
//      LDS for the smallest eigenvector (each rotation's nine rows on nine
//      threads), rank-2 projection, de-normalisation, Frobenius norm 1, sign,
//      fp32.
//   failure: the zero matrix.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surfhip_internal.h"

namespace surfhip {

namespace {

#include "surfhip_ransac.inc"
#include "surfhip_fundamental_math.inc"

// fd_refit_solve's cooperating threads: the block
struct FdBlock {
    int first, step;
    __device__ void sync() const { __syncthreads(); }
};

struct FdModel {
    using Record = surfhip_fundamental;
    static constexpr int kMin = 8;
    static constexpr int kMoments = 36;
    struct Work {
        double ws[180];                     // fd_refit_solve's matrices
    };

    static __device__ __forceinline__ float* matrix(Record& r) { return r.f; }

    static __device__ __forceinline__ void failed(float* F)
    {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = 0.0f;
    }

    static __device__ __forceinline__ float err2(const float* F, const float4& c)
    {
        return fd_sampson2(F, c.x, c.y, c.z, c.w);
    }

    static __device__ __forceinline__ void hypothesis(const double (&x)[8], const double (&y)[8],
                                                      const double (&u)[8], const double (&v)[8], float* out)
    {
        float f[9];
        const bool ok = fd_eight_point(x, y, u, v, f);
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = ok ? f[i] : 0.0f;
    }

    // sum of qq_i pp_j, qq = (uu uv u vv v 1), pp = (xx xy x yy y 1)
    static __device__ __forceinline__ void moments(double x, double y, double u, double v, double (&m)[36])
    {
        const double pp[6] = {x * x, x * y, x, y * y, y, 1.0};
        const double qq[6] = {u * u, u * v, u, v * v, v, 1.0};
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int t = 0; t < 6; ++t) m[6 * q + t] += qq[q] * pp[t];
    }

    // The unit vector that minimises the sum of the squared epipolar residuals
    // in the normalised coordinates, made rank 2: by the whole block, rows of
    // the Jacobi rotations spread over its first threads.
    static __device__ __forceinline__ int solve(const double (&m)[36], double cx, double cy, double s1, double cu,
                                                double cv, double s2, Work& w, float* cur)
    {
        float out[9];
        const bool ok = fd_refit_solve(m, cx, cy, s1, cu, cv, s2, w.ws, out, FdBlock{(int)threadIdx.x, kRsThreads});
        if (ok && threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) cur[i] = out[i];
        }
        __syncthreads();
        return ok ? kRsOk : kRsDegenerate;
    }
};

__global__ __launch_bounds__(kRsThreads) void k_fundamental(const surfhip_point* __restrict__ pts,
                                                            const int* __restrict__ counts, int slots,
                                                            float max_amb, float thr2, int nhyp, uint32_t seed,
                                                            surfhip_fundamental* __restrict__ out,
                                                            uint8_t* __restrict__ inlier)
{
    __shared__ RsShared<FdModel> sh;
    ransac_pair<FdModel>(sh, pts, counts, slots, max_amb, thr2, nhyp, seed, out, inlier);
}

}  // namespace

hipError_t launch_fundamental_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                    float thresh, int nhyp, uint32_t seed, surfhip_fundamental* out, uint8_t* inlier,
                                    hipStream_t s)
{
    return ransac_launch(k_fundamental, pts, counts, slots, npairs, max_amb, thresh, nhyp, seed, out, inlier, s);
}

}  // namespace surfhip
