// surfhip_homography.hip -- batched RANSAC homographies (surfhip_homography_batch)
// for gfx950.  No reference counterpart: main.cpp only draws the matches.
//
// The projective model of the RANSAC driver in surfhip_ransac.inc, which
// describes the input, the phases and why a pair's result is bit-identical
// from run to run.  What is the homography's own:
//   distance: the one-way squared transfer error in image 2, fp32.
//   hypothesis: four candidates, the closed-form unit-square -> quadrilateral
//      maps of both images in fp64, H = Q2 adj(Q1), scaled to h33 = 1.
//   refit: inhomogeneous Hartley-normalised DLT over the current inliers (the
//      24 moments the 8 x 8 normal equations consist of), Cholesky by one
//      thread, de-normalised, scaled to h33 = 1, stored as fp32.
//   failure: the identity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surfhip_internal.h"

namespace surfhip {

namespace {

#include "surfhip_ransac.inc"

constexpr double kHgCollinear = 1e-3;       // a triangle is degenerate when |cross| <= this * (longest side)^2
constexpr double kHgTinyH33 = 1e-12;        // |h33| <= this * ||H||_F: no usable scale
constexpr double kHgTinyPivot = 1e-12;      // Cholesky pivot <= this * its diagonal entry: singular
constexpr float kHgFar = 3.0e38f;           // fp32 entries of a usable H stay below this

__device__ __forceinline__ bool tri_degenerate(double ax, double ay, double bx, double by, double cx, double cy)
{
    const double abx = bx - ax, aby = by - ay, acx = cx - ax, acy = cy - ay, bcx = cx - bx, bcy = cy - by;
    const double cross = abx * acy - aby * acx;
    const double l2 = fmax(fmax(abx * abx + aby * aby, acx * acx + acy * acy), bcx * bcx + bcy * bcy);
    return !(fabs(cross) > kHgCollinear * l2);
}

__device__ __forceinline__ bool quad_degenerate(const double (&x)[4], const double (&y)[4])
{
    return tri_degenerate(x[0], y[0], x[1], y[1], x[2], y[2]) || tri_degenerate(x[0], y[0], x[1], y[1], x[3], y[3]) ||
           tri_degenerate(x[0], y[0], x[2], y[2], x[3], y[3]) || tri_degenerate(x[1], y[1], x[2], y[2], x[3], y[3]);
}

// unit square (0,0) (1,0) (1,1) (0,1) -> the quadrilateral (Heckbert 1989)
__device__ __forceinline__ void square_to_quad(const double (&x)[4], const double (&y)[4], double (&M)[9])
{
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], sx = x[0] - x[1] + x[2] - x[3];
    const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], sy = y[0] - y[1] + y[2] - y[3];
    const double den = dx1 * dy2 - dy1 * dx2;
    const double g = (sx * dy2 - sy * dx2) / den, h = (dx1 * sy - dy1 * sx) / den;
    M[0] = x[1] - x[0] + g * x[1]; M[1] = x[3] - x[0] + h * x[3]; M[2] = x[0];
    M[3] = y[1] - y[0] + g * y[1]; M[4] = y[3] - y[0] + h * y[3]; M[5] = y[0];
    M[6] = g; M[7] = h; M[8] = 1.0;
}

// H scaled to h33 = 1 as fp32; false when it has no usable scale or is not finite
__device__ __forceinline__ bool scale_to_f32(const double (&H)[9], float* out)
{
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) n2 += H[i] * H[i];
    if (!(fabs(H[8]) > kHgTinyH33 * sqrt(n2)) || !(n2 < 1e300)) return false;
    const double inv = 1.0 / H[8];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float v = (float)(H[i] * inv);
        ok = ok && fabsf(v) < kHgFar;
        out[i] = v;
    }
    out[8] = 1.0f;
    return ok;
}

struct HgModel {
    using Record = surfhip_homography;
    static constexpr int kMin = 4;
    static constexpr int kMoments = 24;
    struct Work {
        double sol[8][9];
        int status;
    };

    static __device__ __forceinline__ float* matrix(Record& r) { return r.h; }

    static __device__ __forceinline__ void failed(float* H)
    {
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = i % 4 == 0 ? 1.0f : 0.0f;
    }

    // one-way squared transfer error in image 2 (fp32); w <= 0 (or NaN) is infinitely far
    static __device__ __forceinline__ float err2(const float* H, const float4& c)
    {
        const float X = H[0] * c.x + H[1] * c.y + H[2];
        const float Y = H[3] * c.x + H[4] * c.y + H[5];
        const float W = H[6] * c.x + H[7] * c.y + H[8];
        if (!(W > 0.0f)) return __builtin_inff();
        const float iw = 1.0f / W;
        const float dx = X * iw - c.z, dy = Y * iw - c.w;
        return dx * dx + dy * dy;
    }

    static __device__ __forceinline__ void hypothesis(const double (&x)[4], const double (&y)[4],
                                                      const double (&u)[4], const double (&v)[4], float* out)
    {
        bool ok = !quad_degenerate(x, y) && !quad_degenerate(u, v);
        if (ok) {
            double A[9], B[9], H[9];
            square_to_quad(x, y, A);
            square_to_quad(u, v, B);
            const double adj[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                                   A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                                   A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    H[3 * r + c] = B[3 * r] * adj[c] + B[3 * r + 1] * adj[3 + c] + B[3 * r + 2] * adj[6 + c];
            ok = scale_to_f32(H, out);
        }
        if (!ok) {
#pragma unroll
            for (int i = 0; i < 9; ++i) out[i] = 0.0f;
        }
    }

    // sum of w * p p^T (upper triangle xx xy x yy y 1) for w = 1, u~, v~, u~^2 + v~^2
    static __device__ __forceinline__ void moments(double x, double y, double u, double v, double (&m)[24])
    {
        const double pp[6] = {x * x, x * y, x, y * y, y, 1.0};
        const double q = u * u + v * v;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            m[t] += pp[t];
            m[6 + t] += u * pp[t];
            m[12 + t] += v * pp[t];
            m[18 + t] += q * pp[t];
        }
    }

    // Minimises, over h33~ = 1, the sum of the squared DLT residuals (x~ h1 +
    // y~ h2 + h3 - u~ (x~ h7 + y~ h8) - u~)^2 + (the same with v~, h4..h6) in
    // the normalised coordinates: by one thread.
    static __device__ __forceinline__ int solve(const double (&m)[24], double cx, double cy, double s1, double cu,
                                                double cv, double s2, Work& w, float* cur)
    {
        if (threadIdx.x == 0) {
            // [P 0 -Pu; 0 P -Pv; . . Pq] h = [Pu e3; Pv e3; -Pq e3] (8 unknowns), by Cholesky
            constexpr int S[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            double (&M)[8][9] = w.sol;
            for (int i = 0; i < 8; ++i)
                for (int j = 0; j < 9; ++j) M[i][j] = 0.0;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) M[i][j] = M[3 + i][3 + j] = m[S[i][j]];
                for (int j = 0; j < 2; ++j) {
                    M[i][6 + j] = M[6 + j][i] = -m[6 + S[i][j]];
                    M[3 + i][6 + j] = M[6 + j][3 + i] = -m[12 + S[i][j]];
                }
                M[i][8] = m[6 + S[i][2]];
                M[3 + i][8] = m[12 + S[i][2]];
            }
            for (int i = 0; i < 2; ++i) {
                for (int j = 0; j < 2; ++j) M[6 + i][6 + j] = m[18 + S[i][j]];
                M[6 + i][8] = -m[18 + S[i][2]];
            }
            bool ok = true;
            for (int j = 0; j < 8 && ok; ++j) {                 // M = L L^T in the lower triangle
                const double diag = M[j][j];
                double s = diag;
                for (int k = 0; k < j; ++k) s -= M[j][k] * M[j][k];
                if (!(s > kHgTinyPivot * diag)) { ok = false; break; }
                const double l = sqrt(s);
                M[j][j] = l;
                for (int i = j + 1; i < 8; ++i) {
                    double t = M[i][j];
                    for (int k = 0; k < j; ++k) t -= M[i][k] * M[j][k];
                    M[i][j] = t / l;
                }
            }
            int st = kRsDegenerate;
            if (ok) {
                for (int i = 0; i < 8; ++i) {                   // L z = b
                    double t = M[i][8];
                    for (int k = 0; k < i; ++k) t -= M[i][k] * M[k][8];
                    M[i][8] = t / M[i][i];
                }
                for (int i = 7; i >= 0; --i) {                  // L^T h = z
                    double t = M[i][8];
                    for (int k = i + 1; k < 8; ++k) t -= M[k][i] * M[k][8];
                    M[i][8] = t / M[i][i];
                }
                const double h[9] = {M[0][8], M[1][8], M[2][8], M[3][8], M[4][8], M[5][8], M[6][8], M[7][8], 1.0};
                // G = H~ T1, then T2^-1 G
                double G[9], Hd[9];
                for (int r = 0; r < 3; ++r) {
                    G[3 * r] = s1 * h[3 * r];
                    G[3 * r + 1] = s1 * h[3 * r + 1];
                    G[3 * r + 2] = h[3 * r + 2] - s1 * cx * h[3 * r] - s1 * cy * h[3 * r + 1];
                }
                for (int c = 0; c < 3; ++c) {
                    Hd[c] = G[c] / s2 + cu * G[6 + c];
                    Hd[3 + c] = G[3 + c] / s2 + cv * G[6 + c];
                    Hd[6 + c] = G[6 + c];
                }
                float out[9];
                if (scale_to_f32(Hd, out)) {
                    for (int i = 0; i < 9; ++i) cur[i] = out[i];
                    st = kRsOk;
                }
            }
            w.status = st;
        }
        __syncthreads();
        const int st = w.status;
        __syncthreads();
        return st;
    }
};

__global__ __launch_bounds__(kRsThreads) void k_homography(const surfhip_point* __restrict__ pts,
                                                           const int* __restrict__ counts, int slots,
                                                           float max_amb, float thr2, int nhyp, uint32_t seed,
                                                           surfhip_homography* __restrict__ out,
                                                           uint8_t* __restrict__ inlier)
{
    __shared__ RsShared<HgModel> sh;
    ransac_pair<HgModel>(sh, pts, counts, slots, max_amb, thr2, nhyp, seed, out, inlier);
}

}  // namespace

hipError_t launch_homography_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                   float thresh, int nhyp, uint32_t seed, surfhip_homography* out, uint8_t* inlier,
                                   hipStream_t s)
{
    return ransac_launch(k_homography, pts, counts, slots, npairs, max_amb, thresh, nhyp, seed, out, inlier, s);
}

}  // namespace surfhip
