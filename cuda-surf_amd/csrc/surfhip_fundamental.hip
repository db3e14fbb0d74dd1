// surfhip_fundamental.hip -- batched RANSAC fundamental matrices
// (surfhip_fundamental_batch) for gfx950.  No reference counterpart: main.cpp
// only draws the matches.
//
// The epipolar sibling of surfhip_homography.hip, with the same input (the
// match fields surfhip_match_batch leaves in the set-1 SurfPoint slots; a
// point whose match >= 0 and ambiguity <= max_ambiguity is a candidate
// correspondence (x, y) -> (match_x, match_y)) and the same phases, one
// 256-thread workgroup per pair with nothing but LDS between them:
//   1. compact: the pair's candidates go to LDS as float4 (x, y, u, v) in
//      ascending point index; the first kFundCap fit, the rest is re-read
//      from the point array (never truncated).
//   2. search: 256 hypotheses at a time, lane = hypothesis: eight distinct
//      candidates from a counter hash of (seed, hypothesis, ncand), the
//      Hartley-normalised 8-point solve in fp64 registers
//      (surfhip_fundamental_math.inc), Frobenius norm 1, parked in LDS as
//      fp32, not rank-2 projected.  Then lane = candidate: every wave walks
//      the parked matrices, counts the inliers (squared Sampson distance
//      below thr^2) of its 64 candidates with ballot + popcount.  Most
//      inliers wins, the lowest hypothesis index on a tie.
//   3. refine, twice: normalised 8-point least squares over the current
//      inliers (centroids, mean distances, then the 36 distinct moments of
//      the 9 x 9 normal matrix, all in fp64, per thread in ascending
//      candidate order and combined in a fixed tree), then cyclic Jacobi in
//      LDS for the smallest eigenvector (each rotation's nine rows on nine
//      threads), rank-2 projection, de-normalisation, Frobenius norm 1, sign,
//      fp32; recount.
//   4. write the 64-B result and the pair's row of the inlier mask.
// Every sum has a fixed order and nothing depends on the pair's position in
// the batch, so a pair's result is bit-identical from run to run and from
// batch to batch.  Only integer reductions cross lanes for the selection; no
// atomics anywhere.
//
// The compaction, for_each_cand, block_sum, get_cand and the key reduction
// are copies of their surfhip_homography.hip namesakes (that file is left
// as it was, so k_homography's code object cannot have changed).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surfhip_internal.h"

namespace surfhip {

namespace {

#include "surfhip_fundamental_math.inc"

constexpr int kFdThreads = 256;
constexpr int kFdWaves = kFdThreads / 64;
constexpr int kFdChunk = 256;               // hypotheses generated and scored per round (one per thread)
constexpr int kFdTab = 512;                 // candidate-rank checkpoints: one per 256 points
constexpr int kFdRed = 36;                  // widest block sum (the moments)
constexpr int kFdMin = 8;                   // correspondences a model needs

struct FdShared {
    float4 cand[kFundCap];
    float hyp[kFdChunk][12];                // 9 used; 48-B rows for 16-B broadcast reads
    int cnt[kFdWaves][kFdChunk];
    int tab[kFdTab];
    double red[kFdWaves][kFdRed];
    double ws[180];                         // fd_refit_solve's matrices
    unsigned long long wkey[kFdWaves];
    float curF[12];
    int wcount[kFdWaves];
    int tail;                               // point index of the candidate of rank kFundCap
};

// fd_refit_solve's cooperating threads: the block
struct FdBlock {
    int first, step;
    __device__ void sync() const { __syncthreads(); }
};

struct FdPair {
    const surfhip_point* pts;
    int n;                                  // clamped count
    int ncand;
    int nlds;                               // min(ncand, kFundCap)
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

__device__ __forceinline__ float sampson2(const float* F, const float4& c)
{
    return fd_sampson2(F, c.x, c.y, c.z, c.w);
}

// f(candidate) for this thread's candidates, ascending: the LDS-resident ones
// strided by the block, then (above the capacity) the points past them
template <class F>
__device__ __forceinline__ void for_each_cand(const FdPair& P, const FdShared& sh, F f)
{
    for (int k = threadIdx.x; k < P.nlds; k += kFdThreads) f(sh.cand[k]);
    if (P.ncand > kFundCap) {
        for (int i = sh.tail + threadIdx.x; i < P.n; i += kFdThreads) {
            float4 q;
            if (load_cand(P.pts + i, P.max_amb, q)) f(q);
        }
    }
}

// sum of v[0..N) over the block, the same bits in every thread: xor butterfly
// inside a wave, then the four waves in order
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], FdShared& sh)
{
    static_assert(N <= kFdRed, "block_sum width");
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
__device__ float4 get_cand(const FdPair& P, const FdShared& sh, int k)
{
    if (k < kFundCap) return sh.cand[k];
    const int nt = min((P.n + 255) >> 8, kFdTab);
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

// hypothesis `hyp` of this pair into out[9]; a degenerate sample gives the
// zero matrix, under which every point is an outlier
__device__ void make_hypothesis(const FdPair& P, const FdShared& sh, uint32_t seed, int hyp, float* out)
{
    int idx[kFdMin];
    fd_sample<kFdMin>(seed, (uint32_t)hyp, P.ncand, idx);
    double x[kFdMin], y[kFdMin], u[kFdMin], v[kFdMin];
#pragma unroll
    for (int j = 0; j < kFdMin; ++j) {
        const float4 c = get_cand(P, sh, idx[j]);
        x[j] = c.x; y[j] = c.y; u[j] = c.z; v[j] = c.w;
    }
    float f[9];
    const bool ok = fd_eight_point(x, y, u, v, f);
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? f[i] : 0.0f;
}

// inliers of `j`-th parked hypothesis among this lane's candidate, added to
// the count kept by lane j & 63
__device__ __forceinline__ void score_tile(const FdShared& sh, const float4& c, bool valid, float thr2, int nh,
                                           int lane, int (&acc)[kFdChunk / 64])
{
#pragma unroll
    for (int q = 0; q < kFdChunk / 64; ++q) {
        const int jend = min(64, nh - 64 * q);
        for (int jj = 0; jj < jend; ++jj) {
            const float* F = sh.hyp[64 * q + jj];
            const bool in = valid && sampson2(F, c) < thr2;
            const int n = __popcll(__ballot(in));
            acc[q] += (lane == jj) ? n : 0;
        }
    }
}

// (inliers under sh.curF, sum of their squared distances), the same in every thread
__device__ void recount(const FdPair& P, FdShared& sh, float thr2, int& ninl, double& sum2)
{
    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = sh.curF[i];
    double a[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        const float e = sampson2(F, c);
        if (e < thr2) { a[0] += 1.0; a[1] += (double)e; }
    });
    block_sum(a, sh);
    ninl = (int)a[0];
    sum2 = a[1];
}

// One refit of sh.curF over its own inliers: the unit vector that minimises
// the sum of the squared epipolar residuals in Hartley-normalised
// coordinates, made rank 2.  Returns the status, the same in every thread.
__device__ int refit(const FdPair& P, FdShared& sh, float thr2)
{
    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = sh.curF[i];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (sampson2(F, c) < thr2) {
            a[0] += 1.0; a[1] += (double)c.x; a[2] += (double)c.y; a[3] += (double)c.z; a[4] += (double)c.w;
        }
    });
    block_sum(a, sh);
    if (a[0] < (double)kFdMin) return SURFHIP_FUND_DEGENERATE;
    const double inv = 1.0 / a[0];
    const double cx = a[1] * inv, cy = a[2] * inv, cu = a[3] * inv, cv = a[4] * inv;
    double d[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (sampson2(F, c) < thr2) {
            const double ex = c.x - cx, ey = c.y - cy, eu = c.z - cu, ev = c.w - cv;
            d[0] += sqrt(ex * ex + ey * ey);
            d[1] += sqrt(eu * eu + ev * ev);
        }
    });
    block_sum(d, sh);
    const double m1 = d[0] * inv, m2 = d[1] * inv;
    if (!(m1 > 0.0) || !(m2 > 0.0)) return SURFHIP_FUND_DEGENERATE;       // all inliers coincident
    const double s1 = kFdSqrt2 / m1, s2 = kFdSqrt2 / m2;
    // moments: sum of qq_i pp_j, qq = (uu uv u vv v 1), pp = (xx xy x yy y 1)
    double m[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) m[i] = 0.0;
    for_each_cand(P, sh, [&](const float4& c) {
        if (sampson2(F, c) < thr2) {
            const double x = (c.x - cx) * s1, y = (c.y - cy) * s1, u = (c.z - cu) * s2, v = (c.w - cv) * s2;
            const double pp[6] = {x * x, x * y, x, y * y, y, 1.0};
            const double qq[6] = {u * u, u * v, u, v * v, v, 1.0};
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int t = 0; t < 6; ++t) m[6 * q + t] += qq[q] * pp[t];
        }
    });
    block_sum(m, sh);
    // the tail, by the whole block: rows of the Jacobi rotations spread over its first threads
    float out[9];
    const bool ok = fd_refit_solve(m, cx, cy, s1, cu, cv, s2, sh.ws, out, FdBlock{(int)threadIdx.x, kFdThreads});
    if (ok && threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sh.curF[i] = out[i];
    }
    __syncthreads();
    return ok ? SURFHIP_FUND_OK : SURFHIP_FUND_DEGENERATE;
}

__global__ __launch_bounds__(kFdThreads) void k_fundamental(const surfhip_point* __restrict__ pts,
                                                            const int* __restrict__ counts, int slots,
                                                            float max_amb, float thr2, int nhyp, uint32_t seed,
                                                            surfhip_fundamental* __restrict__ out,
                                                            uint8_t* __restrict__ inlier)
{
    __shared__ FdShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x;
    FdPair P;
    P.pts = pts + pair * (size_t)slots;
    P.n = min(max(counts[pair], 0), slots);
    P.max_amb = max_amb;

    // ---- 1. compact the candidates, ascending
    int running = 0;
    for (int base = 0; base < P.n; base += kFdThreads) {
        const int i = base + tid;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool is = i < P.n && load_cand(P.pts + i, max_amb, c);
        const unsigned long long b = __ballot(is);
        if (lane == 0) sh.wcount[wave] = __popcll(b);
        if (tid == 0 && (base >> 8) < kFdTab) sh.tab[base >> 8] = running;
        __syncthreads();
        int before = running, total = running;
#pragma unroll
        for (int w = 0; w < kFdWaves; ++w) {
            const int n = sh.wcount[w];
            before += (w < wave) ? n : 0;
            total += n;
        }
        if (is) {
            const int pos = before + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < kFundCap) sh.cand[pos] = c;
            if (pos == kFundCap) sh.tail = i;
        }
        running = total;
        __syncthreads();
    }
    P.ncand = running;
    P.nlds = min(running, kFundCap);

    int status = SURFHIP_FUND_OK, ninl = 0;
    double sum2 = 0.0;
    if (P.ncand < kFdMin) {
        status = SURFHIP_FUND_TOO_FEW;
    } else {
        // ---- 2. search
        unsigned long long best = 0;        // (count << 32) | ~hypothesis: most inliers, then lowest index
        float bestF[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) bestF[i] = 0.0f;
        for (int h0 = 0; h0 < nhyp; h0 += kFdChunk) {
            const int nh = min(kFdChunk, nhyp - h0);
            float mine[9];
            if (tid < nh) {
                make_hypothesis(P, sh, seed, h0 + tid, mine);
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.hyp[tid][i] = mine[i];
            }
            __syncthreads();
            int acc[kFdChunk / 64];
#pragma unroll
            for (int q = 0; q < kFdChunk / 64; ++q) acc[q] = 0;
            for (int k0 = wave * 64; k0 < P.nlds; k0 += kFdThreads) {
                const int k = k0 + lane;
                const bool valid = k < P.nlds;
                const float4 c = sh.cand[valid ? k : 0];
                score_tile(sh, c, valid, thr2, nh, lane, acc);
            }
            if (P.ncand > kFundCap) {
                for (int i0 = sh.tail + wave * 64; i0 < P.n; i0 += kFdThreads) {
                    const int i = i0 + lane;
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    const bool valid = i < P.n && load_cand(P.pts + i, max_amb, c);
                    score_tile(sh, c, valid, thr2, nh, lane, acc);
                }
            }
#pragma unroll
            for (int q = 0; q < kFdChunk / 64; ++q) sh.cnt[wave][64 * q + lane] = acc[q];
            __syncthreads();
            if (tid < nh) {
                const int n = sh.cnt[0][tid] + sh.cnt[1][tid] + sh.cnt[2][tid] + sh.cnt[3][tid];
                const unsigned long long key = ((unsigned long long)(uint32_t)n << 32) | (uint32_t)~(uint32_t)(h0 + tid);
                if (n > 0 && key > best) {
                    best = key;
#pragma unroll
                    for (int i = 0; i < 9; ++i) bestF[i] = mine[i];
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
        for (int w = 0; w < kFdWaves; ++w) top = sh.wkey[w] > top ? sh.wkey[w] : top;
        if ((int)(top >> 32) < kFdMin) {
            status = SURFHIP_FUND_DEGENERATE;
        } else {
            if (best == top) {              // one thread: hypothesis indices are distinct
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.curF[i] = bestF[i];
            }
            __syncthreads();
            // ---- 3. two rounds of refit + recount
            for (int round = 0; round < 2 && status == SURFHIP_FUND_OK; ++round) {
                status = refit(P, sh, thr2);
                if (status == SURFHIP_FUND_OK) {
                    recount(P, sh, thr2, ninl, sum2);
                    if (ninl < kFdMin) status = SURFHIP_FUND_DEGENERATE;
                }
            }
        }
    }

    // ---- 4. results
    float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (status == SURFHIP_FUND_OK) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = sh.curF[i];
    } else {
        ninl = 0;
        sum2 = 0.0;
    }
    if (tid == 0) {
        surfhip_fundamental r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.f[i] = F[i];
        r.status = status;
        r.ncand = P.ncand;
        r.ninliers = ninl;
        r.rms = ninl > 0 ? (float)sqrt(sum2 / (double)ninl) : 0.0f;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        out[pair] = r;
    }
    if (inlier) {
        uint8_t* row = inlier + pair * (size_t)slots;
        for (int i = tid; i < slots; i += kFdThreads) {
            uint8_t v = 0;
            float4 c;
            if (status == SURFHIP_FUND_OK && i < P.n && load_cand(P.pts + i, max_amb, c))
                v = sampson2(F, c) < thr2 ? 1 : 0;
            row[i] = v;
        }
    }
}

}  // namespace

hipError_t launch_fundamental_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                    float thresh, int nhyp, uint32_t seed, surfhip_fundamental* out, uint8_t* inlier,
                                    hipStream_t s)
{
    constexpr int kMaxGrid = 65535;                         // pairs per launch, as launch_match_batch
    for (int p0 = 0; p0 < npairs; p0 += kMaxGrid) {
        const int np = npairs - p0 < kMaxGrid ? npairs - p0 : kMaxGrid;
        k_fundamental<<<np, kFdThreads, 0, s>>>(pts + (size_t)p0 * slots, counts + p0, slots, max_amb,
                                                thresh * thresh, nhyp, seed, out + p0,
                                                inlier ? inlier + (size_t)p0 * slots : nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace surfhip
