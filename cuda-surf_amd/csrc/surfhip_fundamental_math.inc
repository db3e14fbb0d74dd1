// surfhip_fundamental_math.inc -- the per-thread arithmetic of
// surfhip_fundamental.hip (included there, inside its anonymous namespace):
// the Sampson distance, the 8-point solver of one hypothesis and the tail of
// a refit (9 x 9 and 3 x 3 cyclic Jacobi, rank-2 projection,
// de-normalisation).  Nothing here touches threadIdx or LDS by
// name; the functions are __host__ __device__ so that a host program can run
// the very same arithmetic against a float64 reference.  The sampler of the
// hypotheses, which the homography kernel shares, is pulled in from its own
// file, so that this one include still gives a host program all of it.

#include "surfhip_ransac_sample.inc"

constexpr double kFdRankTol = 1e-7;         // a sample is degenerate when |last pivot| <= this * |first pivot|
constexpr double kFdEigTol = 1e-12;         // a refit is degenerate when its second smallest eigenvalue <= this * the largest
constexpr double kFdTinyNorm = 1e-150;      // ||F||_F at or below this: no usable scale
constexpr int kFdSweeps = 16;               // most Jacobi sweeps; a sweep without a rotation ends it earlier
constexpr double kFdSqrt2 = 1.4142135623730951;

// squared Sampson distance of (x, y) -> (u, v) under row-major F, fp32, one
// rounding per written operation; d == 0 gives inf or NaN, which no
// `< thr2` passes
__host__ __device__ __forceinline__ float fd_sampson2(const float* f, float x, float y, float u, float v)
{
    const float a = (f[0] * x + f[1] * y) + f[2];
    const float b = (f[3] * x + f[4] * y) + f[5];
    const float c = (f[6] * x + f[7] * y) + f[8];
    const float a2 = (f[0] * u + f[3] * v) + f[6];
    const float b2 = (f[1] * u + f[4] * v) + f[7];
    const float r = (u * a + v * b) + c;
    const float d = (a * a + b * b) + (a2 * a2 + b2 * b2);
    return (r * r) / d;
}

__host__ __device__ __forceinline__ void fd_cswap(bool c, double& a, double& b)
{
    const double t = a;
    a = c ? b : a;
    b = c ? t : b;
}

// T2^T Fn T1 for the similarities T = [s 0 -s cx; 0 s -s cy; 0 0 1], scaled
// to Frobenius norm 1 and rounded to fp32; false when the norm vanishes or
// anything is not finite
__host__ __device__ __forceinline__ bool fd_denormalise(const double (&fn)[9], double cx, double cy, double s1,
                                                        double cu, double cv, double s2, float* out)
{
    double g[9], f[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        g[3 * r] = s1 * fn[3 * r];
        g[3 * r + 1] = s1 * fn[3 * r + 1];
        g[3 * r + 2] = (fn[3 * r + 2] - (s1 * cx) * fn[3 * r]) - (s1 * cy) * fn[3 * r + 1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f[c] = s2 * g[c];
        f[3 + c] = s2 * g[3 + c];
        f[6 + c] = (g[6 + c] - (s2 * cu) * g[c]) - (s2 * cv) * g[3 + c];
    }
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) n2 += f[i] * f[i];
    if (!(n2 > kFdTinyNorm * kFdTinyNorm) || !(n2 < 1e300)) return false;
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = (float)(f[i] * inv);
    return true;
}

// The fundamental matrix through 8 correspondences into out[9]: Hartley
// normalisation of both octets, the 8 x 9 epipolar system, its null vector by
// Gaussian elimination with full pivoting (every index a compile-time
// constant: the system stays in registers), de-normalised, Frobenius norm 1.
// false: coincident points or a null space that is not one-dimensional.
__host__ __device__ __forceinline__ bool fd_eight_point(const double (&x)[8], const double (&y)[8],
                                                        const double (&u)[8], const double (&v)[8], float* out)
{
    double cx = 0.0, cy = 0.0, cu = 0.0, cv = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { cx += x[i]; cy += y[i]; cu += u[i]; cv += v[i]; }
    cx *= 0.125; cy *= 0.125; cu *= 0.125; cv *= 0.125;
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double ex = x[i] - cx, ey = y[i] - cy, eu = u[i] - cu, ev = v[i] - cv;
        m1 += sqrt(ex * ex + ey * ey);
        m2 += sqrt(eu * eu + ev * ev);
    }
    m1 *= 0.125; m2 *= 0.125;
    if (!(m1 > 0.0) || !(m2 > 0.0)) return false;
    const double s1 = kFdSqrt2 / m1, s2 = kFdSqrt2 / m2;
    double a[8][9];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double xn = (x[i] - cx) * s1, yn = (y[i] - cy) * s1, un = (u[i] - cu) * s2, vn = (v[i] - cv) * s2;
        a[i][0] = un * xn; a[i][1] = un * yn; a[i][2] = un;
        a[i][3] = vn * xn; a[i][4] = vn * yn; a[i][5] = vn;
        a[i][6] = xn; a[i][7] = yn; a[i][8] = 1.0;
    }
    int perm[9];                            // column c of the system holds unknown perm[c]
#pragma unroll
    for (int c = 0; c < 9; ++c) perm[c] = c;
    double inv[8];
    double first = 0.0, last = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // the column whose largest entry at or below row k is largest (the first on a tie) comes to k
        double cm[9];
#pragma unroll
        for (int c = k; c < 9; ++c) {
            double m = 0.0;
#pragma unroll
            for (int p = k; p < 8; ++p) m = fmax(m, fabs(a[p][c]));
            cm[c] = m;
        }
#pragma unroll
        for (int c = k + 1; c < 9; ++c) {
            const bool sw = cm[c] > cm[k];
#pragma unroll
            for (int p = 0; p < 8; ++p) fd_cswap(sw, a[p][k], a[p][c]);
            fd_cswap(sw, cm[k], cm[c]);
            const int t = perm[k];
            perm[k] = sw ? perm[c] : perm[k];
            perm[c] = sw ? t : perm[c];
        }
        // ... then the row with that entry (the first on a tie)
#pragma unroll
        for (int p = k + 1; p < 8; ++p) {
            const bool sw = fabs(a[p][k]) > fabs(a[k][k]);
#pragma unroll
            for (int c = k; c < 9; ++c) fd_cswap(sw, a[k][c], a[p][c]);
        }
        const double piv = a[k][k];
        if (k == 0) first = fabs(piv);
        if (k == 7) last = fabs(piv);
        inv[k] = piv != 0.0 ? 1.0 / piv : 0.0;
#pragma unroll
        for (int p = k + 1; p < 8; ++p) {
            const double m = a[p][k] * inv[k];
#pragma unroll
            for (int c = k + 1; c < 9; ++c) a[p][c] -= m * a[k][c];
        }
    }
    if (!(last > kFdRankTol * first)) return false;
    double z[9];
    z[8] = 1.0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        double s = 0.0;
#pragma unroll
        for (int c = k + 1; c < 9; ++c) s += a[k][c] * z[c];
        z[k] = -(s * inv[k]);
    }
    double fn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) t = perm[c] == i ? z[c] : t;
        fn[i] = t;
    }
    return fd_denormalise(fn, cx, cy, s1, cu, cv, s2, out);
}

// Who runs the tail of a refit.  Its loops over matrix rows are spread over
// `step` cooperating threads (this one takes first, first + step, ...) that
// all follow the same control flow on the same values and meet in sync()
// between a write and a dependent read; each element is computed by one
// thread with the arithmetic a single thread would use, so the result does
// not depend on how many cooperate.  On the host: one thread, no sync.
struct FdSolo {
    int first = 0, step = 1;
    __host__ __device__ void sync() const {}
};

// Cyclic Jacobi on the symmetric n x n matrix A (row-major, both triangles
// kept): A becomes diagonal, the columns of V its eigenvectors.  Pairs in
// the order (0,1) (0,2) .. (n-2,n-1); a pair is skipped when a_pq^2 <=
// 1e-36 |a_pp a_qq| (and when a_pq == 0); at most kFdSweeps sweeps, ending
// with the first sweep that rotates nothing.  A and V lie in LDS: every
// index here is a run-time one.
template <class CTX>
__host__ __device__ inline void fd_jacobi(double* A, double* V, int n, const CTX& ctx)
{
    for (int i = ctx.first; i < n * n; i += ctx.step) V[i] = i / n == i % n ? 1.0 : 0.0;
    ctx.sync();
    for (int sweep = 0; sweep < kFdSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
                if (apq == 0.0 || !(apq * apq > 1e-36 * fabs(app * aqq))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                ctx.sync();                             // everyone has read a_pq, a_pp, a_qq
                for (int k = ctx.first; k < n; k += ctx.step) {     // columns p, q
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
                ctx.sync();
                for (int k = ctx.first; k < n; k += ctx.step) {     // rows p, q
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = k == q ? 0.0 : c * apk - s * aqk;
                    A[q * n + k] = k == p ? 0.0 : s * apk + c * aqk;
                }
                ctx.sync();
            }
        }
        if (!rotated) break;
    }
}

// index of the smallest diagonal entry of the n x n matrix A (the first on a tie)
__host__ __device__ inline int fd_smallest(const double* A, int n)
{
    int best = 0;
    for (int i = 1; i < n; ++i)
        if (A[i * n + i] < A[best * n + best]) best = i;
    return best;
}

// The tail of a refit, run by every thread of ctx with the same arguments;
// all of them return the same out and flag.  m[6 i + j] = sum of qq_i pp_j
// over the inliers, qq = (uu, uv, u, vv, v, 1) and pp = (xx, xy, x, yy, y, 1)
// in normalised coordinates: the 36 distinct sums among the 45 moments of the
// 9 x 9 matrix A^T A of the rows (ux, uy, u, vx, vy, v, x, y, 1).  ws is
// 2 * 81 + 2 * 9 doubles of work space (LDS).  Smallest eigenvector by
// Jacobi, rank-2 projection through the Jacobi eigenvectors of Fn^T Fn,
// de-normalised, Frobenius norm 1, fp32, the entry of largest magnitude (the
// first on a tie) positive.  false: degenerate.
template <class CTX>
__host__ __device__ inline bool fd_refit_solve(const double (&m)[36], double cx, double cy, double s1, double cu,
                                               double cv, double s2, double* ws, float* out, const CTX& ctx)
{
    double* A = ws;
    double* V = ws + 81;
    double* B = ws + 162;
    double* W = ws + 171;
    ctx.sync();                                         // the work space is free
#pragma unroll
    for (int i = 0; i < 6; ++i) {                       // A[(3 a + c)][(3 b + d)] = m[6 S(a, b) + S(c, d)]
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            // S = {{0 1 2} {1 3 4} {2 4 5}}: sum i is (ra, rb), sum j is (rc, rd)
            const int ra = i < 3 ? 0 : (i < 5 ? 1 : 2), rb = i < 3 ? i : (i < 5 ? i - 2 : 2);
            const int rc = j < 3 ? 0 : (j < 5 ? 1 : 2), rd = j < 3 ? j : (j < 5 ? j - 2 : 2);
            if (ctx.first == 0) {
                A[(3 * ra + rc) * 9 + 3 * rb + rd] = m[6 * i + j];
                A[(3 * ra + rd) * 9 + 3 * rb + rc] = m[6 * i + j];
                A[(3 * rb + rc) * 9 + 3 * ra + rd] = m[6 * i + j];
                A[(3 * rb + rd) * 9 + 3 * ra + rc] = m[6 * i + j];
            }
        }
    }
    ctx.sync();
    fd_jacobi(A, V, 9, ctx);
    const int e = fd_smallest(A, 9);
    double lmax = 0.0, second = 1e300;
    for (int i = 0; i < 9; ++i) {
        lmax = fmax(lmax, A[i * 9 + i]);
        if (i != e) second = fmin(second, A[i * 9 + i]);
    }
    if (!(second > kFdEigTol * lmax)) return false;
    double fn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) fn[i] = V[i * 9 + e];
    if (ctx.first == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                B[3 * i + j] = (fn[i] * fn[j] + fn[3 + i] * fn[3 + j]) + fn[6 + i] * fn[6 + j];
    }
    ctx.sync();
    fd_jacobi(B, W, 3, ctx);
    const int z = fd_smallest(B, 3);
    const double w0 = W[z], w1 = W[3 + z], w2 = W[6 + z];
    double pr[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double d = (fn[3 * r] * w0 + fn[3 * r + 1] * w1) + fn[3 * r + 2] * w2;
        pr[3 * r] = fn[3 * r] - d * w0;
        pr[3 * r + 1] = fn[3 * r + 1] - d * w1;
        pr[3 * r + 2] = fn[3 * r + 2] - d * w2;
    }
    if (!fd_denormalise(pr, cx, cy, s1, cu, cv, s2, out)) return false;
    float big = 0.0f, at = 0.0f;                        // the entry of largest magnitude, the first on a tie
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const bool more = fabsf(out[i]) > big;
        at = more ? out[i] : at;
        big = more ? fabsf(out[i]) : big;
    }
    if (at < 0.0f) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = -out[i];
    }
    return true;
}
