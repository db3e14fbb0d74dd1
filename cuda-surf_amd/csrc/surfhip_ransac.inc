// surfhip_ransac.inc -- the RANSAC driver of k_homography and k_fundamental
// (included by surfhip_homography.hip and surfhip_fundamental.hip, inside
// their anonymous namespaces, before the model is defined).
//
// Input is what surfhip_match_batch leaves in the set-1 SurfPoint slots: a
// point whose match >= 0 and ambiguity <= max_ambiguity is a candidate
// correspondence (x, y) -> (match_x, match_y).  One 256-thread workgroup
// estimates one pair's 3 x 3 model, start to finish, with nothing but LDS
// between its phases:
//   1. compact: the pair's candidates go to LDS as float4 (x, y, u, v) in
//      ascending point index (wave ballot + prefix counts).  The first
//      kRansacCap fit; for the rest the kernel goes back to the point array
//      (a table of candidate ranks per 256 points finds the k-th candidate, a
//      loop over the points past the last resident one scores them): slower,
//      never truncated.
//   2. search: 256 hypotheses at a time, lane = hypothesis: M::kMin distinct
//      candidates from a counter hash of (seed, hypothesis, ncand), the
//      model's solver, the matrix parked in LDS as fp32.  Then lane =
//      candidate: every wave walks the parked matrices (LDS broadcast reads),
//      counts the inliers of its 64 candidates with ballot + popcount, lane
//      j & 63 keeps the count of hypothesis j.  The counts of the four waves
//      are added and each thread keeps the best (count, lowest index) of the
//      hypotheses it generated; one integer max over the block at the end.
//   3. refine, twice: centroids and mean distances of the current inliers
//      (Hartley normalisation), then the model's moments, all in fp64, per
//      thread in ascending candidate order and combined in a fixed tree; the
//      model's solve; recount.
//   4. write the 64-B result and the pair's row of the inlier mask.
// Every sum has a fixed order and nothing depends on the pair's position in
// the batch, so a pair's result is bit-identical from run to run and from
// batch to batch.  Only integer reductions cross lanes for the selection; no
// atomics anywhere.
//
// The model M is a struct of constants and static functions:
//   Record                    the public 64-B result
//   kMin                      correspondences a hypothesis needs
//   kMoments                  sums a refit accumulates (the widest block sum)
//   Work                      the LDS its solve needs
//   err2(m, c)                squared fp32 distance of candidate c under m[9]
//   hypothesis(x, y, u, v, out)   m[9] through kMin correspondences; a degenerate
//                             sample gives the zero matrix, under which every
//                             point is an outlier
//   moments(x, y, u, v, m)    one normalised inlier added to the kMoments sums
//   solve(m, cx, cy, s1, cu, cv, s2, work, cur)   by the whole block: cur[9]
//                             from the summed moments; the status, the same in
//                             every thread, cur untouched unless it is OK
//   failed(m)                 the matrix returned with a status other than OK
//   matrix(r)                 the nine floats of a Record

#include "surfhip_ransac_sample.inc"

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsChunk = 256;               // hypotheses generated and scored per round (one per thread)
constexpr int kRsTab = 512;                 // candidate-rank checkpoints: one per 256 points

enum : int { kRsOk = 0, kRsTooFew = 1, kRsDegenerate = 2 };
static_assert(SURFHIP_HOMOG_OK == kRsOk && SURFHIP_HOMOG_TOO_FEW == kRsTooFew &&
                  SURFHIP_HOMOG_DEGENERATE == kRsDegenerate && SURFHIP_FUND_OK == kRsOk &&
                  SURFHIP_FUND_TOO_FEW == kRsTooFew && SURFHIP_FUND_DEGENERATE == kRsDegenerate,
              "both families share the driver's status values");

template <class M>
struct RsShared {
    float4 cand[kRansacCap];
    float hyp[kRsChunk][12];                // 9 used; 48-B rows for 16-B broadcast reads
    int cnt[kRsWaves][kRsChunk];
    int tab[kRsTab];
    double red[kRsWaves][M::kMoments];
    typename M::Work work;
    unsigned long long wkey[kRsWaves];
    float cur[12];
    int wcount[kRsWaves];
    int tail;                               // point index of the candidate of rank kRansacCap
};

struct RsPair {
    const surfhip_point* pts;
    int n;                                  // clamped count
    int ncand;
    int nlds;                               // min(ncand, kRansacCap)
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

// f(candidate) for this thread's candidates, ascending: the LDS-resident ones
// strided by the block, then (above the capacity) the points past them
template <class M, class F>
__device__ __forceinline__ void for_each_cand(const RsPair& P, const RsShared<M>& sh, F f)
{
    for (int k = threadIdx.x; k < P.nlds; k += kRsThreads) f(sh.cand[k]);
    if (P.ncand > kRansacCap) {
        for (int i = sh.tail + threadIdx.x; i < P.n; i += kRsThreads) {
            float4 q;
            if (load_cand(P.pts + i, P.max_amb, q)) f(q);
        }
    }
}

// sum of v[0..N) over the block, the same bits in every thread: xor butterfly
// inside a wave, then the four waves in order
template <class M, int N>
__device__ __forceinline__ void block_sum(double (&v)[N], RsShared<M>& sh)
{
    static_assert(N <= M::kMoments, "block_sum width");
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
template <class M>
__device__ float4 get_cand(const RsPair& P, const RsShared<M>& sh, int k)
{
    if (k < kRansacCap) return sh.cand[k];
    const int nt = min((P.n + 255) >> 8, kRsTab);
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

// hypothesis `hyp` of this pair into out[9]
template <class M>
__device__ void make_hypothesis(const RsPair& P, const RsShared<M>& sh, uint32_t seed, int hyp, float* out)
{
    int idx[M::kMin];
    fd_sample<M::kMin>(seed, (uint32_t)hyp, P.ncand, idx);
    double x[M::kMin], y[M::kMin], u[M::kMin], v[M::kMin];
#pragma unroll
    for (int j = 0; j < M::kMin; ++j) {
        const float4 c = get_cand(P, sh, idx[j]);
        x[j] = c.x; y[j] = c.y; u[j] = c.z; v[j] = c.w;
    }
    M::hypothesis(x, y, u, v, out);
}

// inliers of `j`-th parked hypothesis among this lane's candidate, added to
// the count kept by lane j & 63
template <class M>
__device__ __forceinline__ void score_tile(const RsShared<M>& sh, const float4& c, bool valid, float thr2, int nh,
                                           int lane, int (&acc)[kRsChunk / 64])
{
#pragma unroll
    for (int q = 0; q < kRsChunk / 64; ++q) {
        const int jend = min(64, nh - 64 * q);
        for (int jj = 0; jj < jend; ++jj) {
            const bool in = valid && M::err2(sh.hyp[64 * q + jj], c) < thr2;
            const int n = __popcll(__ballot(in));
            acc[q] += (lane == jj) ? n : 0;
        }
    }
}

// (inliers under sh.cur, sum of their squared distances), the same in every thread
template <class M>
__device__ void recount(const RsPair& P, RsShared<M>& sh, float thr2, int& ninl, double& sum2)
{
    float cur[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) cur[i] = sh.cur[i];
    double a[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        const float e = M::err2(cur, c);
        if (e < thr2) { a[0] += 1.0; a[1] += (double)e; }
    });
    block_sum(a, sh);
    ninl = (int)a[0];
    sum2 = a[1];
}

// One refit of sh.cur over its own inliers, in Hartley-normalised coordinates
// (both point sets moved to their centroids and scaled to mean distance
// sqrt 2).  Returns the status, the same in every thread.
template <class M>
__device__ int refit(const RsPair& P, RsShared<M>& sh, float thr2)
{
    float cur[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) cur[i] = sh.cur[i];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (M::err2(cur, c) < thr2) {
            a[0] += 1.0; a[1] += (double)c.x; a[2] += (double)c.y; a[3] += (double)c.z; a[4] += (double)c.w;
        }
    });
    block_sum(a, sh);
    if (a[0] < (double)M::kMin) return kRsDegenerate;
    const double inv = 1.0 / a[0];
    const double cx = a[1] * inv, cy = a[2] * inv, cu = a[3] * inv, cv = a[4] * inv;
    double d[2] = {0.0, 0.0};
    for_each_cand(P, sh, [&](const float4& c) {
        if (M::err2(cur, c) < thr2) {
            const double ex = c.x - cx, ey = c.y - cy, eu = c.z - cu, ev = c.w - cv;
            d[0] += sqrt(ex * ex + ey * ey);
            d[1] += sqrt(eu * eu + ev * ev);
        }
    });
    block_sum(d, sh);
    const double m1 = d[0] * inv, m2 = d[1] * inv;
    if (!(m1 > 0.0) || !(m2 > 0.0)) return kRsDegenerate;                 // all inliers coincident
    const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
    double m[M::kMoments];
#pragma unroll
    for (int i = 0; i < M::kMoments; ++i) m[i] = 0.0;
    for_each_cand(P, sh, [&](const float4& c) {
        if (M::err2(cur, c) < thr2)
            M::moments((c.x - cx) * s1, (c.y - cy) * s1, (c.z - cu) * s2, (c.w - cv) * s2, m);
    });
    block_sum(m, sh);
    return M::solve(m, cx, cy, s1, cu, cv, s2, sh.work, sh.cur);
}

// one pair, by its workgroup
template <class M>
__device__ __forceinline__ void ransac_pair(RsShared<M>& sh, const surfhip_point* __restrict__ pts,
                                            const int* __restrict__ counts, int slots, float max_amb, float thr2,
                                            int nhyp, uint32_t seed, typename M::Record* __restrict__ out,
                                            uint8_t* __restrict__ inlier)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x;
    RsPair P;
    P.pts = pts + pair * (size_t)slots;
    P.n = min(max(counts[pair], 0), slots);
    P.max_amb = max_amb;

    // ---- 1. compact the candidates, ascending
    int running = 0;
    for (int base = 0; base < P.n; base += kRsThreads) {
        const int i = base + tid;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool is = i < P.n && load_cand(P.pts + i, max_amb, c);
        const unsigned long long b = __ballot(is);
        if (lane == 0) sh.wcount[wave] = __popcll(b);
        if (tid == 0 && (base >> 8) < kRsTab) sh.tab[base >> 8] = running;
        __syncthreads();
        int before = running, total = running;
#pragma unroll
        for (int w = 0; w < kRsWaves; ++w) {
            const int n = sh.wcount[w];
            before += (w < wave) ? n : 0;
            total += n;
        }
        if (is) {
            const int pos = before + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < kRansacCap) sh.cand[pos] = c;
            if (pos == kRansacCap) sh.tail = i;
        }
        running = total;
        __syncthreads();
    }
    P.ncand = running;
    P.nlds = min(running, kRansacCap);

    int status = kRsOk, ninl = 0;
    double sum2 = 0.0;
    if (P.ncand < M::kMin) {
        status = kRsTooFew;
    } else {
        // ---- 2. search
        unsigned long long best = 0;        // (count << 32) | ~hypothesis: most inliers, then lowest index
        float bestm[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) bestm[i] = 0.0f;
        for (int h0 = 0; h0 < nhyp; h0 += kRsChunk) {
            const int nh = min(kRsChunk, nhyp - h0);
            float mine[9];
            if (tid < nh) {
                make_hypothesis(P, sh, seed, h0 + tid, mine);
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.hyp[tid][i] = mine[i];
            }
            __syncthreads();
            int acc[kRsChunk / 64];
#pragma unroll
            for (int q = 0; q < kRsChunk / 64; ++q) acc[q] = 0;
            for (int k0 = wave * 64; k0 < P.nlds; k0 += kRsThreads) {
                const int k = k0 + lane;
                const bool valid = k < P.nlds;
                const float4 c = sh.cand[valid ? k : 0];
                score_tile(sh, c, valid, thr2, nh, lane, acc);
            }
            if (P.ncand > kRansacCap) {
                for (int i0 = sh.tail + wave * 64; i0 < P.n; i0 += kRsThreads) {
                    const int i = i0 + lane;
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    const bool valid = i < P.n && load_cand(P.pts + i, max_amb, c);
                    score_tile(sh, c, valid, thr2, nh, lane, acc);
                }
            }
#pragma unroll
            for (int q = 0; q < kRsChunk / 64; ++q) sh.cnt[wave][64 * q + lane] = acc[q];
            __syncthreads();
            if (tid < nh) {
                const int n = sh.cnt[0][tid] + sh.cnt[1][tid] + sh.cnt[2][tid] + sh.cnt[3][tid];
                const unsigned long long key = ((unsigned long long)(uint32_t)n << 32) | (uint32_t)~(uint32_t)(h0 + tid);
                if (n > 0 && key > best) {
                    best = key;
#pragma unroll
                    for (int i = 0; i < 9; ++i) bestm[i] = mine[i];
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
        for (int w = 0; w < kRsWaves; ++w) top = sh.wkey[w] > top ? sh.wkey[w] : top;
        if ((int)(top >> 32) < M::kMin) {
            status = kRsDegenerate;
        } else {
            if (best == top) {              // one thread: hypothesis indices are distinct
#pragma unroll
                for (int i = 0; i < 9; ++i) sh.cur[i] = bestm[i];
            }
            __syncthreads();
            // ---- 3. two rounds of refit + recount
            for (int round = 0; round < 2 && status == kRsOk; ++round) {
                status = refit(P, sh, thr2);
                if (status == kRsOk) {
                    recount(P, sh, thr2, ninl, sum2);
                    if (ninl < M::kMin) status = kRsDegenerate;
                }
            }
        }
    }

    // ---- 4. results
    float m[9];
    M::failed(m);
    if (status == kRsOk) {
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = sh.cur[i];
    } else {
        ninl = 0;
        sum2 = 0.0;
    }
    if (tid == 0) {
        typename M::Record r;
#pragma unroll
        for (int i = 0; i < 9; ++i) M::matrix(r)[i] = m[i];
        r.status = status;
        r.ncand = P.ncand;
        r.ninliers = ninl;
        r.rms = ninl > 0 ? (float)sqrt(sum2 / (double)ninl) : 0.0f;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        out[pair] = r;
    }
    if (inlier) {
        uint8_t* row = inlier + pair * (size_t)slots;
        for (int i = tid; i < slots; i += kRsThreads) {
            uint8_t v = 0;
            float4 c;
            if (status == kRsOk && i < P.n && load_cand(P.pts + i, max_amb, c))
                v = M::err2(m, c) < thr2 ? 1 : 0;
            row[i] = v;
        }
    }
}

// `kernel` (a __global__ around ransac_pair) over npairs pairs, 65,535 a launch
template <class R>
hipError_t ransac_launch(void (*kernel)(const surfhip_point*, const int*, int, float, float, int, uint32_t, R*,
                                        uint8_t*),
                         const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                         float thresh, int nhyp, uint32_t seed, R* out, uint8_t* inlier, hipStream_t s)
{
    constexpr int kMaxGrid = 65535;                         // pairs per launch, as launch_match_batch
    for (int p0 = 0; p0 < npairs; p0 += kMaxGrid) {
        const int np = npairs - p0 < kMaxGrid ? npairs - p0 : kMaxGrid;
        kernel<<<np, kRsThreads, 0, s>>>(pts + (size_t)p0 * slots, counts + p0, slots, max_amb, thresh * thresh,
                                         nhyp, seed, out + p0, inlier ? inlier + (size_t)p0 * slots : nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
