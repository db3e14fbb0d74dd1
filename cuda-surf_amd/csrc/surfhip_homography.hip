// surfhip_homography.hip -- batched RANSAC homographies (surfhip_homography_batch)
// for gfx950.  No reference counterpart: main.cpp only draws the matches.
//
// Input is what surfhip_match_batch leaves in the set-1 SurfPoint slots: a
// point whose match >= 0 and ambiguity <= max_ambiguity is a candidate
// correspondence (x, y) -> (match_x, match_y).  One 256-thread workgroup
// estimates one pair's homography, start to finish, with nothing but LDS
// between its phases:
//   1. compact: the pair's candidates go to LDS as float4 (x, y, u, v) in
//      ascending point index (wave ballot + prefix counts).  The first
//      kHomogCap fit; for the rest the kernel goes back to the point array
//      (a table of candidate ranks per 256 points finds the k-th candidate, a
//      loop over the points past the last resident one scores them): slower,
//      never truncated.
//   2. search: 256 hypotheses at a time, lane = hypothesis: four distinct
//      candidates from a counter hash of (seed, hypothesis, ncand), the
//      closed-form unit-square -> quadrilateral maps of both images in fp64,
//      H = Q2 adj(Q1), scaled to h33 = 1 and parked in LDS as fp32.  Then
//      lane = candidate: every wave walks the parked matrices (LDS broadcast
//      reads), counts the inliers of its 64 candidates with ballot +
//      popcount, lane j & 63 keeps the count of hypothesis j.  The counts of
//      the four waves are added and each thread keeps the best (count, lowest
//      index) of the hypotheses it generated; one integer max over the block
//      at the end.
//   3. refine, twice: inhomogeneous Hartley-normalised DLT over the current
//      inliers (centroids, mean distances, then the 24 moments the 8 x 8
//      normal equations consist of, all in fp64, per thread in ascending
//      candidate order and combined in a fixed tree), Cholesky by one thread,
//      de-normalised, scaled to h33 = 1, stored as fp32; recount.
//   4. write the 64-B result and the pair's row of the inlier mask.
// Every sum has a fixed order and nothing depends on the pair's position in
// the batch, so a pair's result is bit-identical from run to run and from
// batch to batch.  Only integer reductions cross lanes for the selection; no
// atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surfhip_internal.h"

namespace surfhip {

namespace {

constexpr int kHgThreads = 256;
constexpr int kHgWaves = kHgThreads / 64;
constexpr int kHgChunk = 256;               // hypotheses generated and scored per round (one per thread)
constexpr int kHgTab = 512;                 // candidate-rank checkpoints: one per 256 points
constexpr int kHgRed = 24;                  // widest block sum (the moments)
constexpr double kHgCollinear = 1e-3;       // a triangle is degenerate when |cross| <= this * (longest side)^2
constexpr double kHgTinyH33 = 1e-12;        // |h33| <= this * ||H||_F: no usable scale
constexpr double kHgTinyPivot = 1e-12;      // Cholesky pivot <= this * its diagonal entry: singular
constexpr float kHgFar = 3.0e38f;           // fp32 entries of a usable H stay below this

struct HgShared {
    float4 cand[kHomogCap];
    float hyp[kHgChunk][12];                // 9 used; 48-B rows for 16-B broadcast reads
    int cnt[kHgWaves][kHgChunk];
    int tab[kHgTab];
    double red[kHgWaves][kHgRed];
    double sol[8][9];
    unsigned long long wkey[kHgWaves];
    float curH[12];
    int wcount[kHgWaves];
    int tail;                               // point index of the candidate of rank kHomogCap
    int status;
};

struct HgPair {
    const surfhip_point* pts;
    int n;                                  // clamped count
    int ncand;
    int nlds;                               // min(ncand, kHomogCap)
    float max_amb;
};

// the six fields the stage may read, and the candidate filter
__device__ __forceinline__ bool load_cand(const surfhip_point* p, float max_amb, float4& c)
{
    const int m = p->match;
    const float a = p->ambiguity;
    c = make_float4(p->x, p->y, p->match_x, p->match_y);
    return m >= 0 && a <= max_amb;
}

// one-way squared transfer error in image 2 (fp32); w <= 0 (or NaN) is infinitely far
__device__ __forceinline__ float transfer_err2(const float* H, const float4& c)
{
    const float X = H[0] * c.x + H[1] * c.y + H[2];
    const float Y = H[3] * c.x + H[4] * c.y + H[5];
    const float W = H[6] * c.x + H[7] * c.y + H[8];
    if (!(W > 0.0f)) return __builtin_inff();
    const float iw = 1.0f / W;
    const float dx = X * iw - c.z, dy = Y * iw - c.w;
    return dx * dx + dy * dy;
}

// f(candidate) for this thread's candidates, ascending: the LDS-resident ones
// strided by the block, then (above the capacity) the points past them
template <class F>
__device__ __forceinline__ void for_each_cand(const HgPair& P, const HgShared& sh, F f)
{
    for (int k = threadIdx.x; k < P.nlds; k += kHgThreads) f(sh.cand[k]);
    if (P.ncand > kHomogCap) {
        for (int i = sh.tail + threadIdx.x; i < P.n; i += kHgThreads) {
            float4 q;
            if (load_cand(P.pts + i, P.max_amb, q)) f(q);
        }
    }
}

// sum of v[0..N) over the block, the same bits in every thread: xor butterfly
// inside a wave, then the four waves in order
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], HgShared& sh)
{
    static_assert(N <= kHgRed, "block_sum width");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
        if (lane == 0) sh.red[wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((sh.red[0][i] + sh.red[1][i]) + sh.red[2][i]) + sh.red[3][i];
    __syncthreads();
}

// the candidate of rank k (sampling only)
__device__ float4 get_cand(const HgPair& P, const HgShared& sh, int k)
{
    if (k < kHomogCap) return sh.cand[k];
    const int nt = min((P.n + 255) >> 8, kHgTab);
    int lo = 0, hi = nt - 1;
    while (lo < hi) {                       // last checkpoint at or below k
        const int mid = (lo + hi + 1) >> 1;
        if (sh.tab[mid] <= k) lo = mid; else hi = mid - 1;
    }
    int r = sh.tab[lo];
    float4 q;
    for (int i = lo << 8; i < P.n; ++i) {
        if (load_cand(P.pts + i, P.max_amb, q)) {
            if (r == k) return q;
            ++r;
        }
    }
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ uint32_t hg_hash(uint32_t seed, uint32_t hyp, uint32_t j)
{
    uint32_t x = seed ^ (0x9E3779B9u * (4u * hyp + j + 1u));
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// four distinct indices below n (n >= 4): draw j picks among the n - j
// indices not taken yet, in ascending order of those
__device__ __forceinline__ void hg_sample(uint32_t seed, uint32_t hyp, int n, int (&idx)[4])
{
    int s0 = 0, s1 = 0, s2 = 0;             // the picks so far, ascending
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int d = (int)(hg_hash(seed, hyp, (uint32_t)j) % (uint32_t)(n - j));
        if (j >= 1 && d >= s0) ++d;
        if (j >= 2 && d >= s1) ++d;
        if (j >= 3 && d >= s2) ++d;
        idx[j] = d;
        if (j == 0) s0 = d;
        if (j == 1) { s1 = max(s0, d); s0 = min(s0, d); }
        if (j == 2) {
            const int a = min(s0, d), b = max(s0, d);
            s0 = a; s2 = max(s1, b); s1 = min(s1, b);
        }
    }
}

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

// hypothesis `hyp` of this pair into out[9]; a degenerate sample gives the
// zero matrix, under which every point is an outlier
__device__ void make_hypothesis(const HgPair& P, const HgShared& sh, uint32_t seed, int hyp, float* out)
{
    int idx[4];
    hg_sample(seed, (uint32_t)hyp, P.ncand, idx);
    double x[4], y[4], u[4], v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 c = get_cand(P, sh, idx[j]);
        x[j] = c.x; y[j] = c.y; u[j] = c.z; v[j] = c.w;
    }
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

// inliers of `j`-th parked hypothesis among this lane's candidate, added to
// the count kept by lane j & 63
__device__ __forceinline__ void score_tile(const HgShared& sh, const float4& c, bool valid, float thr2, int nh,
                                           int lane, int (&acc)[kHgChunk / 64])
{
#pragma unroll
    for (int q = 0; q < kHgChunk / 64; ++q) {
        const int jend = min(64, nh - 64 * q);
        for (int jj = 0; jj < jend; ++jj) {
            const float* H = sh.hyp[64 * q + jj];
            const bool in = valid && transfer_err2(H, c) < thr2;
            const int n = __popcll(__ballot(in));
            acc[q] += (lane == jj) ? n : 0;
        }
    }
}

// (inliers under sh.curH, sum of their squared errors), the same in every thread
__device__ void recount(const HgPair& P, HgShared& sh, float thr2, int& ninl, double& sum2)
{
    float H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = sh.curH[i];
    double a[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        const float e = transfer_err2(H, c);
        if (e < thr2) { a[0] += 1.0; a[1] += (double)e; }
    });
    block_sum(a, sh);
    ninl = (int)a[0];
    sum2 = a[1];
}

// One refit of sh.curH over its own inliers: minimises, over h33~ = 1, the sum
// of the squared DLT residuals (x~ h1 + y~ h2 + h3 - u~ (x~ h7 + y~ h8) - u~)^2 +
// (the same with v~, h4..h6) in Hartley-normalised coordinates.  Returns the
// status, the same in every thread.
__device__ int refit(const HgPair& P, HgShared& sh, float thr2)
{
    float H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = sh.curH[i];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (transfer_err2(H, c) < thr2) {
            a[0] += 1.0; a[1] += (double)c.x; a[2] += (double)c.y; a[3] += (double)c.z; a[4] += (double)c.w;
        }
    });
    block_sum(a, sh);
    if (a[0] < 4.0) return SURFHIP_HOMOG_DEGENERATE;
    const double inv = 1.0 / a[0];
    const double cx = a[1] * inv, cy = a[2] * inv, cu = a[3] * inv, cv = a[4] * inv;
    double d[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (transfer_err2(H, c) < thr2) {
            const double ex = c.x - cx, ey = c.y - cy, eu = c.z - cu, ev = c.w - cv;
            d[0] += sqrt(ex * ex + ey * ey);
            d[1] += sqrt(eu * eu + ev * ev);
        }
    });
    block_sum(d, sh);
    const double m1 = d[0] * inv, m2 = d[1] * inv;
    if (!(m1 > 0.0) || !(m2 > 0.0)) return SURFHIP_HOMOG_DEGENERATE;      // all inliers coincident
    const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
    // moments: sum of w * p p^T (upper triangle xx xy x yy y 1) for w = 1, u~, v~, u~^2 + v~^2
    double m[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) m[i] = 0.0;
    for_each_cand(P, sh, [&](const float4& c) {
        if (transfer_err2(H, c) < thr2) {
            const double x = (c.x - cx) * s1, y = (c.y - cy) * s1, u = (c.z - cu) * s2, v = (c.w - cv) * s2;
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
    });
    block_sum(m, sh);
    if (threadIdx.x == 0) {
        // [P 0 -Pu; 0 P -Pv; . . Pq] h = [Pu e3; Pv e3; -Pq e3] (8 unknowns), by Cholesky
        constexpr int S[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
        double (&M)[8][9] = sh.sol;
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
        int st = SURFHIP_HOMOG_DEGENERATE;
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
                for (int i = 0; i < 9; ++i) sh.curH[i] = out[i];
                st = SURFHIP_HOMOG_OK;
            }
        }
        sh.status = st;
    }
    __syncthreads();
    const int st = sh.status;
    __syncthreads();
    return st;
}

__global__ __launch_bounds__(kHgThreads) void k_homography(const surfhip_point* __restrict__ pts,
                                                           const int* __restrict__ counts, int slots,
                                                           float max_amb, float thr2, int nhyp, uint32_t seed,
                                                           surfhip_homography* __restrict__ out,
                                                           uint8_t* __restrict__ inlier)
{
    __shared__ HgShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x;
    HgPair P;
    P.pts = pts + pair * (size_t)slots;
    P.n = min(max(counts[pair], 0), slots);
    P.max_amb = max_amb;

    // ---- 1. compact the candidates, ascending
    int running = 0;
    for (int base = 0; base < P.n; base += kHgThreads) {
        const int i = base + tid;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool is = i < P.n && load_cand(P.pts + i, max_amb, c);
        const unsigned long long b = __ballot(is);
        if (lane == 0) sh.wcount[wave] = __popcll(b);
        if (tid == 0 && (base >> 8) < kHgTab) sh.tab[base >> 8] = running;
        __syncthreads();
        int before = running, total = running;
#pragma unroll
        for (int w = 0; w < kHgWaves; ++w) {
            const int n = sh.wcount[w];
            before += (w < wave) ? n : 0;
            total += n;
        }
        if (is) {
            const int pos = before + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < kHomogCap) sh.cand[pos] = c;
            if (pos == kHomogCap) sh.tail = i;
        }
        running = total;
        __syncthreads();
    }
    P.ncand = running;
    P.nlds = min(running, kHomogCap);

    int status = SURFHIP_HOMOG_OK, ninl = 0;
    double sum2 = 0.0;
    if (P.ncand < 4) {
        status = SURFHIP_HOMOG_TOO_FEW;
    } else {
        // ---- 2. search
        unsigned long long best = 0;        // (count << 32) | ~hypothesis: most inliers, then lowest index
        float bestH[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) bestH[i] = 0.0f;
        for (int h0 = 0; h0 < nhyp; h0 += kHgChunk) {
            const int nh = min(kHgChunk, nhyp - h0);
            float mine[9];
            if (tid < nh) {
                make_hypothesis(P, sh, seed, h0 + tid, mine);
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.hyp[tid][i] = mine[i];
            }
            __syncthreads();
            int acc[kHgChunk / 64];
#pragma unroll
            for (int q = 0; q < kHgChunk / 64; ++q) acc[q] = 0;
            for (int k0 = wave * 64; k0 < P.nlds; k0 += kHgThreads) {
                const int k = k0 + lane;
                const bool valid = k < P.nlds;
                const float4 c = sh.cand[valid ? k : 0];
                score_tile(sh, c, valid, thr2, nh, lane, acc);
            }
            if (P.ncand > kHomogCap) {
                for (int i0 = sh.tail + wave * 64; i0 < P.n; i0 += kHgThreads) {
                    const int i = i0 + lane;
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    const bool valid = i < P.n && load_cand(P.pts + i, max_amb, c);
                    score_tile(sh, c, valid, thr2, nh, lane, acc);
                }
            }
#pragma unroll
            for (int q = 0; q < kHgChunk / 64; ++q) sh.cnt[wave][64 * q + lane] = acc[q];
            __syncthreads();
            if (tid < nh) {
                const int n = sh.cnt[0][tid] + sh.cnt[1][tid] + sh.cnt[2][tid] + sh.cnt[3][tid];
                const unsigned long long key = ((unsigned long long)(uint32_t)n << 32) | (uint32_t)~(uint32_t)(h0 + tid);
                if (n > 0 && key > best) {
                    best = key;
#pragma unroll
                    for (int i = 0; i < 9; ++i) bestH[i] = mine[i];
                }
            }
            __syncthreads();                // hyp and cnt are rewritten by the next round
        }
        unsigned long long top = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(top, off, 64);
            top = o > top ? o : top;
        }
        if (lane == 0) sh.wkey[wave] = top;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kHgWaves; ++w) top = sh.wkey[w] > top ? sh.wkey[w] : top;
        if ((int)(top >> 32) < 4) {
            status = SURFHIP_HOMOG_DEGENERATE;
        } else {
            if (best == top) {              // one thread: hypothesis indices are distinct
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.curH[i] = bestH[i];
            }
            __syncthreads();
            // ---- 3. two rounds of refit + recount
            for (int round = 0; round < 2 && status == SURFHIP_HOMOG_OK; ++round) {
                status = refit(P, sh, thr2);
                if (status == SURFHIP_HOMOG_OK) {
                    recount(P, sh, thr2, ninl, sum2);
                    if (ninl < 4) status = SURFHIP_HOMOG_DEGENERATE;
                }
            }
        }
    }

    // ---- 4. results
    float H[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (status == SURFHIP_HOMOG_OK) {
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = sh.curH[i];
    } else {
        ninl = 0;
        sum2 = 0.0;
    }
    if (tid == 0) {
        surfhip_homography r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.h[i] = H[i];
        r.status = status;
        r.ncand = P.ncand;
        r.ninliers = ninl;
        r.rms = ninl > 0 ? (float)sqrt(sum2 / (double)ninl) : 0.0f;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        out[pair] = r;
    }
    if (inlier) {
        uint8_t* row = inlier + pair * (size_t)slots;
        for (int i = tid; i < slots; i += kHgThreads) {
            uint8_t v = 0;
            float4 c;
            if (status == SURFHIP_HOMOG_OK && i < P.n && load_cand(P.pts + i, max_amb, c))
                v = transfer_err2(H, c) < thr2 ? 1 : 0;
            row[i] = v;
        }
    }
}

}  // namespace

hipError_t launch_homography_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                   float thresh, int nhyp, uint32_t seed, surfhip_homography* out, uint8_t* inlier,
                                   hipStream_t s)
{
    constexpr int kMaxGrid = 65535;                         // pairs per launch, as launch_match_batch
    for (int p0 = 0; p0 < npairs; p0 += kMaxGrid) {
        const int np = npairs - p0 < kMaxGrid ? npairs - p0 : kMaxGrid;
        k_homography<<<np, kHgThreads, 0, s>>>(pts + (size_t)p0 * slots, counts + p0, slots, max_amb,
                                               thresh * thresh, nhyp, seed, out + p0,
                                               inlier ? inlier + (size_t)p0 * slots : nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace surfhip
