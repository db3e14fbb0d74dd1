// surfhip_match.hip -- descriptor matching (Surfor::match) for gfx950.
//
// Reference: Surfor::match (surf.cpp:418-428) -> cuFindMaxCorr
// (surfd.cu:3554-3566) -> findMaxCorr (surfd.cu:2530-2656).  For every
// point p1 of set 1 the reference keeps, per thread row ty = 0..7 of its
// block, the (max, second, index) of the scores against the set-2 points p2
// with (p2 % 32) / 4 == ty of every FULL 32-point tile (surfd.cu:2569 drops
// the last partial tile), then merges row 0 with rows 1..7 in order
// (surfd.cu:2638-2655).  A score is one fp32 FMA chain over the descriptor
// in index order (nvcc contracts `score += a * b`, surfd.cu:2596-2601).
//
// The same result, laid out for CDNA4 instead of a 32x8 CUDA block:
//   * k_match_part: lane = p1 (its descriptor lives in VGPRs), the wave walks
//     a chunk of set-2 tiles with the p2 descriptor wave-uniform (scalar
//     loads, an SGPR operand of every v_fma_f32), one FMA chain per score,
//     the 8 row states (max, second, index) in registers -- the tile position
//     j of an unrolled 32-step loop fixes the row, j / 4.  grid.y splits set
//     2 into chunks so that a few thousand points fill the 256 CUs.
//   * k_match_merge: one thread per (p1, row): the chunk states of the row
//     are combined in chunk order (top-2 of a concatenation, earlier index on
//     a tie: exactly the sequential scan's result); the row-0 lane then does
//     the reference's row merge over lane shuffles and writes the five
//     SurfPoint fields.
// These two kernels run the chains on the VALU; at ~3k x 3k x 64 they cost
// tens of microseconds per pair.
//
// Batched matching (surfhip_match_batch), pair i = frame i of set 1 against
// frame i of set 2 in the surfhip_detect_batch layout, runs the same chains
// on the matrix cores.  On gfx950 v_mfma_f32_32x32x2_f32 is bit-for-bit a
// k-ordered fmaf chain (one rounding per product, no wider accumulation), so
// chaining its k-steps s = 0, 1, .. into one accumulator that starts at 0,
// with descriptor element 2 s on lanes 0-31 and 2 s + 1 on lanes 32-63, is
// the reference's score, not a re-associated sum.
//   * k_match_batch: grid (point tiles of set 1, pairs).  A wave owns 32
//     set-1 points as the B operand (lane l: point l & 31, elements of
//     parity l >> 5; resident in VGPRs for nf = 64 / 128), the pair's set-2
//     tiles of 32 points are the A operand, staged once per block in LDS
//     (even and odd elements of a row apart, so a lane reads its k-steps
//     with 16-B loads; double-buffered, one barrier per tile).  The
//     accumulator D[p2][p1] has p1 on the lane and tile positions
//     8 q + 4 h + 0..3 (h = lane >> 5) in registers 4 q .. 4 q + 3: exactly
//     thread row 2 q + h, in ascending order, so each lane keeps four row
//     states and updates them from the accumulator registers.  After the
//     last tile lanes l and l ^ 32 exchange (max, index) of their rows and
//     the h = 0 lane does the row merge and writes the point.  The counts
//     are read on the device: no scratch, no host sync, one launch.
//   * k_match_batch_any: other descriptor lengths, both operands reloaded
//     from memory at every k-step.
//
// Mutual-best matching (surfhip_match_batch_cross) keeps a forward match
// (p1 -> p2) only when p1 is also the best set-1 point of p2.  fmaf(a, b, c)
// == fmaf(b, a, c), so the back direction's scores are the tile D[p2][p1]
// the forward kernels already hold: their CROSS instantiations reduce each
// tile's columns over the lanes (the maximum positive score, the lowest p1
// on a tie), combine the block's waves in LDS and send one 64-bit integer
// atomic max per (block, p2) to a caller-provided word per set-2 slot -- no
// second score pass, and an integer maximum does not depend on arrival
// order.  k_match_cross_filter then clears the matches that are not mutual.
//
// Windowed matching (surfhip_match_batch_window) offers p2 to p1 only inside
// a search window around p1.  surfhip_detect_batch writes keypoints in the
// order octave, level, row, column, so 32 consecutive points cover a narrow
// band of rows: k_match_tile_boxes writes the bounding box of every set-2
// tile, and the WIN instantiations of the batch kernels run their loop over
// the tiles whose box can hold a partner of the block's points (a wave skips
// the MFMAs of the tiles that cannot hold one of its own 32), with the window
// test beside the Laplace test in the scan.  A skipped tile holds no offered
// pair, so the result does not depend on the order of the points; the speed
// does.
//
// Guided matching (surfhip_match_batch_guided) measures the window from the
// point's predicted position H (x1, y1) instead, H the pair's 3 x 3 matrix in
// device memory: the GUIDED instantiations project every set-1 point once,
// ahead of the tile loop, and from there on the prediction (u, v) stands where
// the window kernels have (x1, y1) -- in the boxes, the kept-tile list and the
// scan's test.
//
// Epipolar matching (surfhip_match_batch_epipolar) keeps the window around the
// raw (x1, y1) and adds a band along the point's epipolar line under the
// pair's fundamental matrix F: every set-1 point computes its line (a, b, c)
// and lim = band^2 (a^2 + b^2) once, ahead of the tile loop, and the scan
// offers (x2, y2) when r = (x2 a + y2 b) + c has r r <= lim -- no division, no
// square root.  The tile boxes are the window call's; a line is tested against
// a box through r at the box's four corners (every fp32 operation of r is
// monotone in x2 and in y2, so r over the box lies between the smallest and
// the largest corner value): a wave skips the MFMAs of a staged tile that
// none of its lines can reach, and the block's kept-tile list drops a tile
// that none of the block's lines can reach.  The boxes of detected keypoints
// are wide and low (a band of rows over the frame's width), so this prunes
// for lines that run along the rows -- a stereo rig; a steep line crosses
// every such box and only the window prunes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surfhip_internal.h"

namespace surfhip {

namespace {

constexpr int kMatchThreads = 256;
constexpr int kTilesPerChunk = 2;   // 64 set-2 points per chunk (2 waves / SIMD at 3k x 3k)

// The set-2 points a match scans: the full 32-point tiles of n2 (surfd.cu:2569),
// or all of them.
__host__ __device__ __forceinline__ int scanned(int n2, int flags)
{
    return (flags & SURFHIP_MATCH_FULL_TAIL) ? n2 : 32 * (n2 / 32);
}

// Sequential (max, second, index) update with strict '>' (surfd.cu:2611-2620),
// branch-free (selects, no divergent control flow around the state).
__device__ __forceinline__ void scan_update(float s, int p2, float& mx, float& sc, int& ix)
{
    const bool gt = s > mx;
    const bool gt2 = s > sc;
    sc = gt ? mx : (gt2 ? s : sc);
    mx = gt ? s : mx;
    ix = gt ? p2 : ix;
}

// The reference's row merge (surfd.cu:2638-2655) and the write of the five
// match fields.  (M, S, I): row 0's state, which starts the merge; row(r, rm,
// ri) gives (max, index) of row r = 1 .. 7, in order -- the rows' second scores
// are not used, equal indices are skipped.  write: this lane writes pts1[p1].
template <class Row>
__device__ __forceinline__ void merge_rows_write(surfhip_point* pts1, const surfhip_point* pts2, int p1, bool write,
                                                 float M, float S, int I, Row row)
{
#pragma unroll
    for (int r = 1; r < 8; ++r) {
        float rm;
        int ri;
        row(r, rm, ri);
        if (I != ri) {
            if (rm > M) {
                S = fmaxf(M, S);
                M = rm;
                I = ri;
            } else if (rm > S) {
                S = rm;
            }
        }
    }
    if (!write) return;
    surfhip_point& q = pts1[p1];
    q.score = M;
    q.match = I;
    q.match_x = I >= 0 ? pts2[I].x : 0.0f;
    q.match_y = I >= 0 ? pts2[I].y : 0.0f;
    q.ambiguity = S / (M + 1e-6f);
}

// NF 64 / 128: the lane's descriptor in VGPRs, unrolled chains.  NF 0: any
// descriptor length nf (a multiple of 4, <= 1024), runtime trip count.
template <int NF>
__global__ __launch_bounds__(kMatchThreads) void k_match_part(const float* __restrict__ f1,
                                                              const float* __restrict__ f2, int n1, int nscan,
                                                              int ntile, float* __restrict__ pmx,
                                                              float* __restrict__ psc, int* __restrict__ pix, int nf)
{
    const int p1 = blockIdx.x * kMatchThreads + threadIdx.x;
    const int q1 = p1 < n1 ? p1 : n1 - 1;
    const int len = NF ? NF : nf;
    const float* ar = f1 + (size_t)q1 * len;
    float a[NF ? NF : 1];
    if constexpr (NF != 0) {
        const float4* ap = reinterpret_cast<const float4*>(ar);
#pragma unroll
        for (int d = 0; d < NF / 4; ++d) {
            const float4 v = ap[d];
            a[4 * d] = v.x;
            a[4 * d + 1] = v.y;
            a[4 * d + 2] = v.z;
            a[4 * d + 3] = v.w;
        }
    }
    float mx[8], sc[8];
    int ix[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        mx[g] = 0.0f;
        sc[g] = 0.0f;
        ix[g] = -1;
    }
    const int t0 = blockIdx.y * kTilesPerChunk;
    const int t1 = min(t0 + kTilesPerChunk, ntile);
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int p2 = 32 * t + j;
            if (p2 < nscan) {
                const float* b = f2 + (size_t)p2 * len;
                float s = 0.0f;
                if constexpr (NF != 0) {
#pragma unroll
                    for (int d = 0; d < NF; ++d) s = __builtin_fmaf(a[d], b[d], s);
                } else {
                    for (int d = 0; d < nf; ++d) s = __builtin_fmaf(ar[d], b[d], s);
                }
                scan_update(s, p2, mx[j >> 2], sc[j >> 2], ix[j >> 2]);
            }
        }
    }
    if (p1 < n1) {
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const size_t o = ((size_t)blockIdx.y * n1 + p1) * 8 + g;
            pmx[o] = mx[g];
            psc[o] = sc[g];
            pix[o] = ix[g];
        }
    }
}

// One thread per (p1, row g): lanes 8 q .. 8 q + 7 of a wave hold the 8 rows
// of one p1; the row-0 lane then merges the others in row order.
__global__ __launch_bounds__(256) void k_match_merge(surfhip_point* __restrict__ pts1,
                                                     const surfhip_point* __restrict__ pts2, int n1, int nchunk,
                                                     const float* __restrict__ pmx, const float* __restrict__ psc,
                                                     const int* __restrict__ pix)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int p1 = tid >> 3, g = tid & 7;
    const bool live = p1 < n1;
    // Row g over all chunks, in chunk (= p2) order: top-2 of the
    // concatenated sequences, the earlier index kept on a tie.
    float mx = 0.0f, sc = 0.0f;
    int ix = -1;
    if (live) {
#pragma unroll 8
        for (int c = 0; c < nchunk; ++c) {
            const size_t o = ((size_t)c * n1 + p1) * 8 + g;
            const float bm = pmx[o], bs = psc[o];
            const int bi = pix[o];
            const bool gt = bm > mx;
            sc = gt ? fmaxf(mx, bs) : fmaxf(sc, bm);
            mx = gt ? bm : mx;
            ix = gt ? bi : ix;
        }
    }
    merge_rows_write(pts1, pts2, p1, live && g == 0, mx, sc, ix, [&](int r, float& rm, int& ri) {
        rm = __shfl(mx, (threadIdx.x & ~7) + r);
        ri = __shfl(ix, (threadIdx.x & ~7) + r);
    });
}

// ---- batched matching on the f32 MFMA ----------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBatchWaves = 4;                      // one per SIMD; each owns 32 set-1 points
constexpr int kBatchThreads = 64 * kBatchWaves;
constexpr int kBatchPts = 32 * kBatchWaves;         // set-1 points per block

__device__ __forceinline__ int clamp_count(int c, int slots) { return c < 0 ? 0 : (c > slots ? slots : c); }

enum { WIN_OFF = 0, WIN_LDS = 1, WIN_SHFL = 2 };

// The predicted position of (x, y) under the row-major 3 x 3 matrix m, in the
// operation order of transfer_err2 (surfhip_homography.hip), one fp32
// rounding per written operation and IEEE quotients.  W > 0 false (W <= 0 or
// NaN): (NaN, NaN), which no window test and no box takes.
__device__ __forceinline__ void guided_predict(const float* __restrict__ m, float x, float y, float& u, float& v)
{
    const float X = (m[0] * x + m[1] * y) + m[2];
    const float Y = (m[3] * x + m[4] * y) + m[5];
    const float W = (m[6] * x + m[7] * y) + m[8];
    const bool front = W > 0.0f;
    u = front ? X / W : __builtin_nanf("");
    v = front ? Y / W : __builtin_nanf("");
}

// A set-1 point's epipolar line under the row-major 3 x 3 matrix f, (x2, y2,
// 1) f (x1, y1, 1)^T = 0, as (a, b, c) (the Sampson a, b, c of
// surfhip_fundamental.hip), and lim = band^2 (a^2 + b^2): (x2, y2) lies within
// band pixels of the line when r = (x2 a + y2 b) + c has r r <= lim.  One fp32
// rounding per written operation; nothing is special-cased: an all-zero f
// gives 0 <= 0 everywhere, a NaN in f a NaN lim, which no r r is below.
struct EpiLine {
    float a, b, c, lim;
};

__device__ __forceinline__ EpiLine epipolar_line(const float* __restrict__ f, float x, float y, float band)
{
    EpiLine l;
    l.a = (f[0] * x + f[1] * y) + f[2];
    l.b = (f[3] * x + f[4] * y) + f[5];
    l.c = (f[6] * x + f[7] * y) + f[8];
    l.lim = (band * band) * (l.a * l.a + l.b * l.b);
    return l;
}

__device__ __forceinline__ bool epipolar_offered(const EpiLine& l, float x2, float y2)
{
    const float r = (x2 * l.a + y2 * l.b) + l.c;
    return r * r <= l.lim;
}

// May the line offer a point of the box b = (xmin, xmax, ymin, ymax)?  Never
// false for a box that holds an offered point: each operation of r is monotone
// in x2 and in y2, so r over the box lies between the smallest and the largest
// of its four corner values, computed with the same expression; squaring is
// monotone on either side of 0.  So nothing is offered when all four corners
// lie on one side of 0 with r r > lim.  A NaN corner or a NaN lim fails its
// comparisons, which keeps the tile.
__device__ __forceinline__ bool line_may_offer(const EpiLine& l, const float4& b)
{
    const float xa0 = b.x * l.a, xa1 = b.y * l.a, yb0 = b.z * l.b, yb1 = b.w * l.b;
    const float r0 = (xa0 + yb0) + l.c, r1 = (xa1 + yb0) + l.c, r2 = (xa0 + yb1) + l.c, r3 = (xa1 + yb1) + l.c;
    const bool far = r0 * r0 > l.lim && r1 * r1 > l.lim && r2 * r2 > l.lim && r3 * r3 > l.lim;
    const bool above = r0 > 0.0f && r1 > 0.0f && r2 > 0.0f && r3 > 0.0f;
    const bool below = r0 < 0.0f && r1 < 0.0f && r2 < 0.0f && r3 < 0.0f;
    return !(far && (above || below));
}

// One 32 x 32 score tile D[p2][p1] into the lane's four row states: register
// 4 q + r holds tile position 8 q + 4 h + r, i.e. thread row 2 q + h, r
// ascending.  lap2: the laplace of tile position (lane & 31), LAP only.
// CROSS: ks[4 q + r] also gets the score's bits where the pair (p1, p2) counts
// for the back direction (p2 offered, p1 live, score > 0 -- never a NaN), 0
// elsewhere; positive floats order like their bits.
// WIN (surfhip_match_batch_window): the pair also has to lie in the search
// window w around the lane's point (x1, y1).  WIN_LDS: xy2 holds the tile's
// 32 x then 32 y (16-B aligned), a lane reads its four positions of a q at
// once; WIN_SHFL: x2, y2 are those of tile position (lane & 31).  A NaN
// difference fails every comparison: not offered.
// EPI (surfhip_match_batch_epipolar): and in the band along the lane's line ep.
// (The kernels call it through scan_lane_tile, which has these in two structs:
// with the structs read in here, or with cross_reduce behind the same call,
// the CROSS kernels' registers are allocated differently.)
template <bool LAP, bool CROSS, int WIN, bool EPI = false>
__device__ __forceinline__ void scan_tile(const f32x16& acc, int t, int h, int nscan, int lap1, int lap2,
                                          float (&mx)[4], float (&sc)[4], int (&ix)[4], bool live1, uint32_t* ks,
                                          const surfhip_match_window* w, float x1, float y1, const float* xy2,
                                          float x2, float y2, const EpiLine* ep = nullptr)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 qx = {0, 0, 0, 0}, qy = {0, 0, 0, 0};
        if constexpr (WIN == WIN_LDS) {
            qx = *reinterpret_cast<const float4*>(xy2 + 8 * q + 4 * h);
            qy = *reinterpret_cast<const float4*>(xy2 + 32 + 8 * q + 4 * h);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 8 * q + 4 * h + r;
            const int p2 = 32 * t + j;
            bool ok = p2 < nscan;
            if (LAP) {
                const int l2 = __shfl(lap2, j);
                ok = ok && l2 == lap1;
            }
            if constexpr (WIN != WIN_OFF) {
                const float xr = r == 0 ? qx.x : r == 1 ? qx.y : r == 2 ? qx.z : qx.w;
                const float yr = r == 0 ? qy.x : r == 1 ? qy.y : r == 2 ? qy.z : qy.w;
                if constexpr (!EPI) {
                    const float dx = (WIN == WIN_LDS ? xr : __shfl(x2, j)) - x1;
                    const float dy = (WIN == WIN_LDS ? yr : __shfl(y2, j)) - y1;
                    ok = ok && dx >= w->dx_min && dx <= w->dx_max && dy >= w->dy_min && dy <= w->dy_max;
                } else {
                    const float xj = WIN == WIN_LDS ? xr : __shfl(x2, j), yj = WIN == WIN_LDS ? yr : __shfl(y2, j);
                    const float dx = xj - x1, dy = yj - y1;
                    ok = ok && dx >= w->dx_min && dx <= w->dx_max && dy >= w->dy_min && dy <= w->dy_max &&
                         epipolar_offered(*ep, xj, yj);
                }
            }
            if (ok) scan_update(acc[4 * q + r], p2, mx[q], sc[q], ix[q]);
            if constexpr (CROSS) {
                const float s = acc[4 * q + r];
                ks[4 * q + r] = (ok && live1 && s > 0.0f) ? __float_as_uint(s) : 0u;
            }
        }
    }
}

// ---- mutual-best matching: the back direction's column maxima ------------
// A key is (score bits << 32) | ~p1: the integer maximum is the largest
// positive score and, among equal scores, the lowest p1; 0 means "none".
typedef unsigned long long u64;

// The value of lane (lane ^ X), X < 32: DPP inside a quad, the LDS crossbar
// (ds_swizzle, bit mode: and 0x1f, or 0, xor X) beyond it.
template <int X>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v)
{
    if constexpr (X == 1)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    else if constexpr (X == 2)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    else
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F);
}

// One step of a transposing reduction over lane bit X: the lane keeps the
// entries 2 k + (its bit X) of N and takes its partner's maxima for them, so
// N entries become N / 2 that cover twice the lanes.
template <int N, int X>
__device__ __forceinline__ void cross_fold(uint32_t (&ks)[16], uint32_t (&ki)[16], bool up)
{
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const uint32_t keep_s = up ? ks[2 * k + 1] : ks[2 * k], keep_i = up ? ki[2 * k + 1] : ki[2 * k];
        const uint32_t send_s = up ? ks[2 * k] : ks[2 * k + 1], send_i = up ? ki[2 * k] : ki[2 * k + 1];
        const uint32_t rs = lane_xor<X>(send_s), ri = lane_xor<X>(send_i);
        const bool take = (((u64)rs << 32) | ri) > (((u64)keep_s << 32) | keep_i);
        ks[k] = take ? rs : keep_s;
        ki[k] = take ? ri : keep_i;
    }
}

// The 32 column maxima of a wave's 32 x 32 tile: ks as scan_tile's CROSS left
// it.  Returns, on the lanes with (lane & 31) < 16, the key of tile position
// j (also returned) over the wave's 32 set-1 points: lane (h, c) ends with
// register c of half h, position 8 (c >> 2) + 4 h + (c & 3).
__device__ __forceinline__ u64 cross_reduce(uint32_t (&ks)[16], int p1, int h, int c, int& j)
{
    uint32_t ki[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ki[i] = ~(uint32_t)p1;
    cross_fold<16, 1>(ks, ki, c & 1);
    cross_fold<8, 2>(ks, ki, c & 2);
    cross_fold<4, 4>(ks, ki, c & 4);
    cross_fold<2, 8>(ks, ki, c & 8);
    const uint32_t rs = lane_xor<16>(ks[0]), ri = lane_xor<16>(ki[0]);
    const u64 mine = ((u64)ks[0] << 32) | ki[0], other = ((u64)rs << 32) | ri;
    j = 8 * ((c >> 2) & 3) + 4 * h + (c & 3);
    const u64 key = other > mine ? other : mine;
    return (key >> 32) ? key : 0;
}

// scan_tile's arguments by name.  The set-1 side, the same for every tile of a
// lane: h, lap1 (LAP), live1 (CROSS), and w, x1, y1 (WIN).
struct ScanLane {
    int h, lap1;
    bool live1;
    float x1, y1;
    const surfhip_match_window* w;
};

// The set-2 side: tile t, lap2 (LAP), xy2 (WIN_LDS), x2 and y2 (WIN_SHFL).
struct ScanTile {
    int t, lap2;
    const float* xy2 = nullptr;
    float x2 = 0.0f, y2 = 0.0f;
};

template <bool LAP, bool CROSS, int WIN>
__device__ __forceinline__ void scan_lane_tile(const f32x16& acc, int nscan, const ScanLane& me, const ScanTile& tl,
                                               float (&mx)[4], float (&sc)[4], int (&ix)[4], uint32_t* ks)
{
    scan_tile<LAP, CROSS, WIN>(acc, tl.t, me.h, nscan, me.lap1, tl.lap2, mx, sc, ix, me.live1, ks, me.w, me.x1, me.y1,
                               tl.xy2, tl.x2, tl.y2);
}

// The same with the band along the lane's epipolar line (its own call: the
// line inside ScanLane moves the registers of the kernels that have none).
template <bool LAP, bool CROSS, int WIN>
__device__ __forceinline__ void scan_lane_tile_epi(const f32x16& acc, int nscan, const ScanLane& me,
                                                   const EpiLine& ln, const ScanTile& tl, float (&mx)[4],
                                                   float (&sc)[4], int (&ix)[4], uint32_t* ks)
{
    scan_tile<LAP, CROSS, WIN, true>(acc, tl.t, me.h, nscan, me.lap1, tl.lap2, mx, sc, ix, me.live1, ks, me.w, me.x1,
                                     me.y1, tl.xy2, tl.x2, tl.y2, &ln);
}

// Lanes l and l ^ 32 hold rows (0, 2, 4, 6) and (1, 3, 5, 7) of point p1;
// the h = 0 lane merges them as k_match_merge does and writes the point.
__device__ __forceinline__ void batch_finish(surfhip_point* pts1, const surfhip_point* pts2, int p1, int n1, int h,
                                             const float (&mx)[4], const float (&sc)[4], const int (&ix)[4])
{
    float omx[4];
    int oix[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        omx[q] = __shfl_xor(mx[q], 32);
        oix[q] = __shfl_xor(ix[q], 32);
    }
    if (h != 0 || p1 >= n1) return;
    merge_rows_write(pts1, pts2, p1, true, mx[0], sc[0], ix[0], [&](int r, float& rm, int& ri) {
        rm = (r & 1) ? omx[r >> 1] : mx[r >> 1];
        ri = (r & 1) ? oix[r >> 1] : ix[r >> 1];
    });
}

// ---- windowed matching: boxes --------------------------------------------
// A box is (xmin, xmax, ymin, ymax) of some points' finite-or-infinite
// coordinates; fminf / fmaxf drop NaN, and a box of no point is
// (+inf, -inf, +inf, -inf).
constexpr int kWinChunk = kBatchThreads;            // tile boxes a block tests at a time, one per thread

// The box of the points of 32 consecutive lanes (x, y; live: the lane has
// one), on every one of those lanes.
__device__ __forceinline__ float4 box_of_32(float x, float y, bool live)
{
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    x = live ? x : nan;
    y = live ? y : nan;
    float4 b = make_float4(fminf(inf, x), fmaxf(-inf, x), fminf(inf, y), fmaxf(-inf, y));
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
        b.x = fminf(b.x, __shfl_xor(b.x, m));
        b.y = fmaxf(b.y, __shfl_xor(b.y, m));
        b.z = fminf(b.z, __shfl_xor(b.z, m));
        b.w = fmaxf(b.w, __shfl_xor(b.w, m));
    }
    return b;
}

__device__ __forceinline__ float4 box_union(const float4& a, const float4& b)
{
    return make_float4(fminf(a.x, b.x), fmaxf(a.y, b.y), fminf(a.z, b.z), fmaxf(a.w, b.w));
}

// May a set-1 point of box a be offered a set-2 point of box b?  Never false
// for boxes that hold an offered pair: x2 - x1 lies between the two
// differences tested here and fp32 subtraction is monotone; a NaN (inf - inf)
// fails both comparisons, which keeps the tile.
__device__ __forceinline__ bool box_may_offer(const float4& a, const float4& b, const surfhip_match_window& w)
{
    return !(b.x - a.y > w.dx_max) && !(b.y - a.x < w.dx_min) && !(b.z - a.w > w.dy_max) &&
           !(b.w - a.z < w.dy_min);
}

// boxes[pair][tiles]: the box of every scanned 32-point tile of set 2 (the
// tiles at or past ntile are not written and not read).
__global__ __launch_bounds__(256) void k_match_tile_boxes(const MatchBatch mb)
{
    const int* __restrict__ counts2 = mb.counts2;
    float4* __restrict__ boxes = mb.boxes;
    const int pair = blockIdx.y;
    const int n2 = clamp_count(counts2[pair], mb.slots2);
    const int nscan = scanned(n2, mb.flags);
    const int t = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int p2 = 32 * t + (threadIdx.x & 31);
    const bool live = p2 < nscan;
    const surfhip_point* q = mb.pts2 + (size_t)pair * mb.slots2 + (live ? p2 : 0);
    const float4 b = box_of_32(q->x, q->y, live);
    if ((threadIdx.x & 31) == 0 && 32 * t < nscan) boxes[(size_t)pair * mb.tiles + t] = b;
}

// pts1 / pts2 may overlap (consecutive frames of one batch): no __restrict__
// on them; only the five match fields of pts1 are written and only x, y,
// laplace of pts2 (WIN: and x, y of pts1) are read.
// CROSS (surfhip_match_batch_cross): the tile's column maxima, which the
// forward scan throws away, also go to back[pair][p2] as keys: the four
// waves' maxima meet in LDS (ds_max_u64), and one tile later wave 0 sends the
// block's 32 keys with one 256-B atomic-max instruction.
// WIN (surfhip_match_batch_window): the block keeps, in ascending order, the
// tiles whose box (boxes[pair][tiles], k_match_tile_boxes) can hold a partner
// of one of its live points, and runs the same loop over that list; a wave
// whose own 32 points cannot have one in the staged tile only stages and
// waits.  A skipped tile holds no offered pair, so no row state, no key and
// no bit of the result depends on the skipping.
// GUIDED (surfhip_match_batch_guided): WIN around the lane's prediction under
// the pair's matrix, the nine floats at hm + pair * h_stride.
// EPIPOLAR (surfhip_match_batch_epipolar): WIN around the raw point, and the
// band along the lane's line under that matrix.  The block's lines lie in LDS;
// the thread that tests a tile's box for the list also walks the lines of the
// block's live points until one can reach the box, and a wave scores a staged
// tile only when one of its own lines can.
template <int NF, bool LAP, bool CROSS, int MODE = MATCH_PLAIN>
__global__ __launch_bounds__(kBatchThreads) void k_match_batch(const MatchBatch mb)
{
    constexpr bool WIN = MODE != MATCH_PLAIN;
    constexpr bool EPI = MODE == MATCH_EPIPOLAR;
    constexpr int RS = NF + 4;                             // LDS row: NF / 2 even, NF / 2 odd elements, pad
    constexpr int C4 = NF / 4;                              // float4 per descriptor
    constexpr int NV = 32 * C4 / kBatchThreads;             // float4 per thread per tile
    static_assert(32 * C4 % kBatchThreads == 0, "tile staging");
    __shared__ __attribute__((aligned(16))) float tile[2][32 * RS];
    __shared__ u64 colmax[CROSS ? 2 : 1][32];               // CROSS: the block's keys of tiles t and t + 1
    // WIN: the staged tiles' x[32], y[32]; the waves' boxes and kept-tile
    // counts; one chunk of the kept-tile list with the tiles' boxes
    __shared__ __attribute__((aligned(16))) float xy2[WIN ? 2 : 1][64];
    __shared__ float4 wbox[WIN ? kBatchWaves : 1];
    __shared__ int wcnt[WIN ? kBatchWaves : 1];
    __shared__ int tlist[WIN ? kWinChunk : 1];
    __shared__ float4 tbox[WIN ? kWinChunk : 1];

    const int pair = blockIdx.y, slots1 = mb.slots1, slots2 = mb.slots2;
    const int* __restrict__ counts1 = mb.counts1;
    const int* __restrict__ counts2 = mb.counts2;
    const int n1 = clamp_count(counts1[pair], slots1);
    // WIN: workgroups go to the 8 XCDs round-robin by their linear index, and
    // with an even grid.x the blocks that keep most tiles (the small, tall
    // (octave, level) groups at the end of every frame) would all meet on the
    // same XCDs: rotate the point blocks by the pair
    const int bx = WIN ? (blockIdx.x + blockIdx.y) % gridDim.x : blockIdx.x;
    const int base = bx * kBatchPts;
    if (base >= n1) return;
    const int n2 = clamp_count(counts2[pair], slots2);
    const int nscan = scanned(n2, mb.flags);
    const int ntile = (nscan + 31) / 32;
    surfhip_point* pts1 = mb.pts1 + (size_t)pair * slots1;
    const surfhip_point* pts2 = mb.pts2 + (size_t)pair * slots2;
    const float* __restrict__ f1 = mb.f1 + (size_t)pair * slots1 * NF;
    const float* __restrict__ f2 = mb.f2 + (size_t)pair * slots2 * NF;
    u64* __restrict__ back = CROSS ? mb.back + (size_t)pair * slots2 : nullptr;
    const surfhip_match_window& win = mb.win;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int p1 = base + 32 * wave + c;
    const bool wlive = base + 32 * wave < n1;               // a dead wave of a live block only stages tiles
    const int q1 = p1 < n1 ? p1 : n1 - 1;

    float b[NF / 2];                                        // b[s] = f1[p1][2 s + h]
    {
        const float4* bp = reinterpret_cast<const float4*>(f1 + (size_t)q1 * NF);
#pragma unroll
        for (int d = 0; d < C4; ++d) {
            const float4 v = bp[d];
            b[2 * d] = h ? v.y : v.x;
            b[2 * d + 1] = h ? v.w : v.z;
        }
    }
    const int lap1 = LAP ? pts1[q1].laplace : 0;

    float mx[4], sc[4];
    int ix[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mx[q] = 0.0f;
        sc[q] = 0.0f;
        ix[q] = -1;
    }

    float4 v[NV];
    int lap2 = 0, lapn = 0;
    float xn = 0.0f, yn = 0.0f;                             // WIN: x, y of the prefetched tile's position c
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + kBatchThreads * i;
            const int row = idx / C4, col = idx % C4;
            const int p2 = min(32 * t + row, nscan - 1);    // rows past nscan: any valid row (never scanned)
            v[i] = reinterpret_cast<const float4*>(f2 + (size_t)p2 * NF)[col];
        }
        if (LAP) lapn = pts2[min(32 * t + c, nscan - 1)].laplace;
        if constexpr (WIN) {
            xn = pts2[min(32 * t + c, nscan - 1)].x;
            yn = pts2[min(32 * t + c, nscan - 1)].y;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + kBatchThreads * i;
            const int row = idx / C4, col = idx % C4;
            float* dst = &tile[buf][row * RS + 2 * col];
            *reinterpret_cast<float2*>(dst) = make_float2(v[i].x, v[i].z);
            *reinterpret_cast<float2*>(dst + NF / 2) = make_float2(v[i].y, v[i].w);
        }
        if constexpr (WIN) {
            if (tid < 32) {
                xy2[buf][tid] = xn;
                xy2[buf][32 + tid] = yn;
            }
        }
    };
    // WIN: the score tile D[p2][p1] of the wave's points against the staged
    // tile (the WIN = false loop spells the same out: through this lambda its
    // registers are allocated differently, and its code is meant to stay put)
    auto score_tile = [&](int buf) {
        const float4* ap = reinterpret_cast<const float4*>(&tile[buf][c * RS + h * (NF / 2)]);
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NF / 8; ++k) {
            const float4 a = ap[k];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * k], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * k + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * k + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * k + 3], acc, 0, 0, 0);
        }
        return acc;
    };

    // CROSS: the keys of tile u, the slot-th of the loop, leave colmax[slot & 1],
    // which is zero again two tiles on (a key of 0 is "none": nothing to send,
    // and a sent key has 32 u + lane < nscan)
    auto send_keys = [&](int slot, int u) {
        if (tid < 32) {
            const u64 key = colmax[slot & 1][tid];
            colmax[slot & 1][tid] = 0;
            if (key) __hip_atomic_fetch_max(back + 32 * u + tid, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if constexpr (CROSS) {
        if (tid < 64) colmax[tid >> 5][tid & 31] = 0;
    }

    if constexpr (!WIN) {
        const ScanLane me = {h, lap1, p1 < n1, 0.0f, 0.0f, nullptr};
        if (ntile > 0) {
            load_tile(0);
            store_tile(0);
            lap2 = lapn;
        }
        __syncthreads();
        for (int t = 0; t < ntile; ++t) {
            const int cur = t & 1;
            const bool more = t + 1 < ntile;
            // unconditional (rows are clamped to valid ones; the last prefetch is
            // unused): in a branch the loads' wait would end that branch, ahead
            // of the MFMAs they are meant to run under
            load_tile(t + 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (CROSS) {
                // ahead of the MFMAs, which cover the atomics' latency
                if (wave == 0 && t > 0) send_keys(t - 1, t - 1);
            }
            if (wlive) {
                const float4* ap = reinterpret_cast<const float4*>(&tile[cur][c * RS + h * (NF / 2)]);
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < NF / 8; ++k) {
                    const float4 a = ap[k];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * k], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * k + 1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * k + 2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * k + 3], acc, 0, 0, 0);
                }
                uint32_t ks[16];
                scan_lane_tile<LAP, CROSS, WIN_OFF>(acc, nscan, me, {t, lap2}, mx, sc, ix, ks);
                if constexpr (CROSS) {
                    int j;
                    const u64 key = cross_reduce(ks, p1, h, c, j);
                    if (c < 16 && key)
                        __hip_atomic_fetch_max(&colmax[cur][j], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more) store_tile(cur ^ 1);
            lap2 = lapn;
            __syncthreads();
        }
        if constexpr (CROSS) {
            if (wave == 0 && ntile > 0) send_keys(ntile - 1, ntile - 1);
        }
    } else {
        const float4* __restrict__ boxes = mb.boxes + (size_t)pair * mb.tiles;
        float x1 = pts1[q1].x, y1 = pts1[q1].y;
        if constexpr (MODE == MATCH_GUIDED) guided_predict(mb.hm + (size_t)pair * mb.h_stride, x1, y1, x1, y1);
        const ScanLane me = {h, lap1, p1 < n1, x1, y1, &win};
        const float4 mybox = box_of_32(x1, y1, p1 < n1);    // the wave's live points (none: a dead wave)
        if (lane == 0) wbox[wave] = mybox;
        // EPI: the lane's line (a lane past n1 has that of point n1 - 1, one of its
        // wave's), and the block's lines, of which the first n1 - base are live
        EpiLine ln = {0.0f, 0.0f, 0.0f, 0.0f};
        const float4* lines = nullptr;
        if constexpr (EPI) {
            __shared__ float4 eline[kBatchPts];
            ln = epipolar_line(mb.hm + (size_t)pair * mb.h_stride, x1, y1, mb.band);
            if (h == 0) eline[32 * wave + c] = make_float4(ln.a, ln.b, ln.c, ln.lim);
            lines = eline;
        }
        const int nline = min(kBatchPts, n1 - base);
        __syncthreads();
        float4 blockbox = wbox[0];
#pragma unroll
        for (int w = 1; w < kBatchWaves; ++w) blockbox = box_union(blockbox, wbox[w]);

        for (int t0 = 0; t0 < ntile; t0 += kWinChunk) {
            // the kept tiles of [t0, t0 + kWinChunk), ascending: thread tid
            // tests tile t0 + tid, ballots and the waves' counts place it
            const int tt = t0 + tid;
            const float4 bb = boxes[min(tt, ntile - 1)];
            bool keep = tt < ntile && box_may_offer(blockbox, bb, win);
            if constexpr (EPI) {
                if (keep) {
                    bool any = false;
                    for (int k = 0; k < nline && !any; ++k) {
                        const float4 l = lines[k];
                        any = line_may_offer({l.x, l.y, l.z, l.w}, bb);
                    }
                    keep = any;
                }
            }
            const u64 kept = __ballot(keep);
            if (lane == 0) wcnt[wave] = __popcll(kept);
            __syncthreads();
            int first = 0, nl = 0;
#pragma unroll
            for (int w = 0; w < kBatchWaves; ++w) {
                const int n = wcnt[w];
                first += w < wave ? n : 0;
                nl += n;
            }
            if (keep) {
                const int pos = first + __popcll(kept & ((1ull << lane) - 1));
                tlist[pos] = tt;
                tbox[pos] = bb;
            }
            __syncthreads();
            nl = __builtin_amdgcn_readfirstlane(nl);

            // the loop above over the list; its tiles' keys leave before the
            // next chunk's barriers, so both colmax slots are zero again there
            if (nl > 0) {
                load_tile(__builtin_amdgcn_readfirstlane(tlist[0]));
                store_tile(0);
                lap2 = lapn;
            }
            __syncthreads();
            for (int i = 0; i < nl; ++i) {
                const int cur = i & 1;
                const bool more = i + 1 < nl;
                const int t = __builtin_amdgcn_readfirstlane(tlist[i]);
                load_tile(__builtin_amdgcn_readfirstlane(tlist[more ? i + 1 : i]));
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (CROSS) {
                    if (wave == 0 && i > 0) send_keys(i - 1, __builtin_amdgcn_readfirstlane(tlist[i - 1]));
                }
                // the wave's own box: a block over two (octave, level) groups is
                // tall, its waves are not
                bool mine = wlive && __builtin_amdgcn_readfirstlane(box_may_offer(mybox, tbox[i], win));
                if constexpr (EPI) mine = mine && __ballot(line_may_offer(ln, tbox[i])) != 0;
                if (mine) {
                    const f32x16 acc = score_tile(cur);
                    uint32_t ks[16];
                    if constexpr (EPI)
                        scan_lane_tile_epi<LAP, CROSS, WIN_LDS>(acc, nscan, me, ln, {t, lap2, xy2[cur]}, mx, sc, ix,
                                                                ks);
                    else
                        scan_lane_tile<LAP, CROSS, WIN_LDS>(acc, nscan, me, {t, lap2, xy2[cur]}, mx, sc, ix, ks);
                    if constexpr (CROSS) {
                        int j;
                        const u64 key = cross_reduce(ks, p1, h, c, j);
                        if (c < 16 && key)
                            __hip_atomic_fetch_max(&colmax[cur][j], key, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (more) store_tile(cur ^ 1);
                lap2 = lapn;
                __syncthreads();
            }
            if constexpr (CROSS) {
                if (wave == 0 && nl > 0) send_keys(nl - 1, __builtin_amdgcn_readfirstlane(tlist[nl - 1]));
            }
        }
    }
    if (wlive) batch_finish(pts1, pts2, p1, n1, h, mx, sc, ix);
}

// Any descriptor length (a multiple of 4, <= 1024): both operands come from
// memory at every k-step; no LDS, so a wave past n1 exits at once.
// CROSS: every wave sends its own 32 keys per tile.
// WIN: a wave walks all tile boxes and skips the tiles its own box misses.
// GUIDED: as in k_match_batch.
// EPIPOLAR: ... and the tiles none of its own lines can reach.
template <bool LAP, bool CROSS, int MODE = MATCH_PLAIN>
__global__ __launch_bounds__(kBatchThreads) void k_match_batch_any(const MatchBatch mb)
{
    constexpr bool WIN = MODE != MATCH_PLAIN;
    constexpr bool EPI = MODE == MATCH_EPIPOLAR;
    const int pair = blockIdx.y, slots1 = mb.slots1, slots2 = mb.slots2, nf = mb.nf;
    const int* __restrict__ counts1 = mb.counts1;
    const int* __restrict__ counts2 = mb.counts2;
    const int n1 = clamp_count(counts1[pair], slots1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = WIN ? (blockIdx.x + blockIdx.y) % gridDim.x : blockIdx.x;    // (as in k_match_batch)
    const int base = bx * kBatchPts + 32 * wave;
    if (base >= n1) return;
    const int n2 = clamp_count(counts2[pair], slots2);
    const int nscan = scanned(n2, mb.flags);
    const int ntile = (nscan + 31) / 32;
    surfhip_point* pts1 = mb.pts1 + (size_t)pair * slots1;
    const surfhip_point* pts2 = mb.pts2 + (size_t)pair * slots2;
    const float* __restrict__ f1 = mb.f1 + (size_t)pair * slots1 * nf;
    const float* __restrict__ f2 = mb.f2 + (size_t)pair * slots2 * nf;
    u64* __restrict__ back = CROSS ? mb.back + (size_t)pair * slots2 : nullptr;
    const float4* __restrict__ boxes = WIN ? mb.boxes + (size_t)pair * mb.tiles : nullptr;
    const surfhip_match_window& win = mb.win;
    const int h = lane >> 5, c = lane & 31;
    const int p1 = base + c;
    const int q1 = p1 < n1 ? p1 : n1 - 1;
    const float* r1 = f1 + (size_t)q1 * nf + h;
    const int lap1 = LAP ? pts1[q1].laplace : 0;
    float mx[4], sc[4];
    int ix[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mx[q] = 0.0f;
        sc[q] = 0.0f;
        ix[q] = -1;
    }
    float x1 = 0.0f, y1 = 0.0f;
    float4 mybox = {0, 0, 0, 0};
    if constexpr (WIN) {
        x1 = pts1[q1].x;
        y1 = pts1[q1].y;
        if constexpr (MODE == MATCH_GUIDED) guided_predict(mb.hm + (size_t)pair * mb.h_stride, x1, y1, x1, y1);
        mybox = box_of_32(x1, y1, p1 < n1);
    }
    EpiLine ln = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (EPI) ln = epipolar_line(mb.hm + (size_t)pair * mb.h_stride, x1, y1, mb.band);
    const ScanLane me = {h, lap1, p1 < n1, x1, y1, &win};
    constexpr int W = WIN ? WIN_SHFL : WIN_OFF;
    for (int t = 0; t < ntile; ++t) {
        if constexpr (WIN) {
            if (!__builtin_amdgcn_readfirstlane(box_may_offer(mybox, boxes[t], win))) continue;
        }
        if constexpr (EPI) {
            if (__ballot(line_may_offer(ln, boxes[t])) == 0) continue;
        }
        const int q2 = min(32 * t + c, nscan - 1);
        const float* r2 = f2 + (size_t)q2 * nf + h;
        const int lap2 = LAP ? pts2[q2].laplace : 0;
        const float x2 = WIN ? pts2[q2].x : 0.0f, y2 = WIN ? pts2[q2].y : 0.0f;
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < nf; d += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(r2[d], r1[d], acc, 0, 0, 0);
        uint32_t ks[16];
        if constexpr (EPI)
            scan_lane_tile_epi<LAP, CROSS, W>(acc, nscan, me, ln, {t, lap2, nullptr, x2, y2}, mx, sc, ix, ks);
        else
            scan_lane_tile<LAP, CROSS, W>(acc, nscan, me, {t, lap2, nullptr, x2, y2}, mx, sc, ix, ks);
        if constexpr (CROSS) {
            int j;
            const u64 key = cross_reduce(ks, p1, h, c, j);
            if (c < 16 && key)                              // a key: 32 t + j < nscan
                __hip_atomic_fetch_max(back + 32 * t + j, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    batch_finish(pts1, pts2, p1, n1, h, mx, sc, ix);
}

// The mutual-best filter, one thread per set-1 point below n1: a match whose
// set-2 point has another back best (the key's low word is not ~p1) is
// cleared; score and ambiguity stay the forward values.
__global__ __launch_bounds__(256) void k_match_cross_filter(const MatchBatch mb)
{
    const int* __restrict__ counts1 = mb.counts1;
    const u64* __restrict__ back = mb.back;
    const int pair = blockIdx.y, slots1 = mb.slots1, slots2 = mb.slots2;
    const int p1 = blockIdx.x * 256 + threadIdx.x;
    if (p1 >= clamp_count(counts1[pair], slots1)) return;
    surfhip_point& q = mb.pts1[(size_t)pair * slots1 + p1];
    const int m = q.match;
    if (m < 0 || m >= slots2) return;                       // (the forward pass writes -1 or an index below n2)
    if ((uint32_t)back[(size_t)pair * slots2 + m] == ~(uint32_t)p1) return;
    q.match = -1;
    q.match_x = 0.0f;
    q.match_y = 0.0f;
}

}  // namespace

// The chunks k_match_part's grid.y splits n2 set-2 points into.
static int match_chunks(int n2, int flags)
{
    const int ntile = (scanned(n2, flags) + 31) / 32;
    return (ntile + kTilesPerChunk - 1) / kTilesPerChunk;
}

size_t match_scratch_bytes(int n1, int n2, int flags)
{
    return (size_t)match_chunks(n2, flags) * 8 * (size_t)n1 * 12;
}

hipError_t launch_match(surfhip_point* pts1, const surfhip_point* pts2, const float* f1, const float* f2, int n1,
                        int n2, int nf, int flags, void* scratch, hipStream_t s)
{
    const int nscan = scanned(n2, flags);
    const int ntile = (nscan + 31) / 32;
    const int nchunk = match_chunks(n2, flags);
    float* pmx = static_cast<float*>(scratch);
    float* psc = pmx + (size_t)nchunk * 8 * n1;
    int* pix = reinterpret_cast<int*>(psc + (size_t)nchunk * 8 * n1);
    if (nchunk > 0) {
        const dim3 grid((n1 + kMatchThreads - 1) / kMatchThreads, nchunk);
        const auto part = nf == 64 ? k_match_part<64> : nf == 128 ? k_match_part<128> : k_match_part<0>;
        part<<<grid, kMatchThreads, 0, s>>>(f1, f2, n1, nscan, ntile, pmx, psc, pix, nf);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    k_match_merge<<<(8 * n1 + 255) / 256, 256, 0, s>>>(pts1, pts2, n1, nchunk, pmx, psc, pix);
    return hipGetLastError();
}

// The batch kernel of (mode, mutual, same laplace, nf): the template axes from
// the run-time values, one per step.
using BatchKernel = void (*)(MatchBatch);
template <int MODE = -1, int CROSS = -1, int LAP = -1>
static BatchKernel batch_kernel(int mode, bool cross, bool lap, int nf)
{
    if constexpr (MODE < 0)
        return mode == MATCH_PLAIN    ? batch_kernel<MATCH_PLAIN>(mode, cross, lap, nf)
               : mode == MATCH_WINDOW ? batch_kernel<MATCH_WINDOW>(mode, cross, lap, nf)
               : mode == MATCH_GUIDED ? batch_kernel<MATCH_GUIDED>(mode, cross, lap, nf)
                                      : batch_kernel<MATCH_EPIPOLAR>(mode, cross, lap, nf);
    else if constexpr (CROSS < 0)
        return cross ? batch_kernel<MODE, 1>(mode, cross, lap, nf) : batch_kernel<MODE, 0>(mode, cross, lap, nf);
    else if constexpr (LAP < 0)
        return lap ? batch_kernel<MODE, CROSS, 1>(mode, cross, lap, nf)
                   : batch_kernel<MODE, CROSS, 0>(mode, cross, lap, nf);
    else
        return nf == 64    ? k_match_batch<64, LAP != 0, CROSS != 0, MODE>
               : nf == 128 ? k_match_batch<128, LAP != 0, CROSS != 0, MODE>
                           : k_match_batch_any<LAP != 0, CROSS != 0, MODE>;
}

// The scratch of a batched match: the tile boxes (not MATCH_PLAIN), then the
// keys (SURFHIP_MATCH_MUTUAL).
static int match_window_tiles(int slots2) { return (slots2 + 31) / 32; }

static size_t match_box_bytes(int mode, int npairs, int slots2)
{
    return mode != MATCH_PLAIN ? sizeof(float4) * (size_t)npairs * (size_t)match_window_tiles(slots2) : 0;
}

static size_t match_key_bytes(int npairs, int slots2, int flags)
{
    return (flags & SURFHIP_MATCH_MUTUAL) ? sizeof(u64) * (size_t)npairs * (size_t)slots2 : 0;
}

size_t match_batch_scratch_bytes(int mode, int npairs, int slots2, int flags)
{
    if (npairs <= 0 || slots2 <= 0) return 0;
    return match_box_bytes(mode, npairs, slots2) + match_key_bytes(npairs, slots2, flags);
}

// Per launch of up to 65,535 pairs (grid.y): the boxes of set 2's tiles (not
// MATCH_PLAIN; in any state on entry), the batch kernel, and with
// SURFHIP_MATCH_MUTUAL the filter pass over the keys the batch kernel left (the
// kernel boundary makes them visible to it; zero on entry).
hipError_t launch_match_batch(const MatchBatch& in, int mode, void* scratch, hipStream_t s)
{
    const bool cross = (in.flags & SURFHIP_MATCH_MUTUAL) != 0, win = mode != MATCH_PLAIN;
    MatchBatch all = in;
    all.tiles = match_window_tiles(in.slots2);
    all.boxes = win ? static_cast<float4*>(scratch) : nullptr;
    all.back = nullptr;
    if (cross) {
        all.back = reinterpret_cast<u64*>(static_cast<char*>(scratch) + match_box_bytes(mode, in.npairs, in.slots2));
        const hipError_t e = hipMemsetAsync(all.back, 0, match_key_bytes(in.npairs, in.slots2, in.flags), s);
        if (e != hipSuccess) return e;
    }
    const BatchKernel kernel = batch_kernel(mode, cross, (in.flags & SURFHIP_MATCH_SAME_LAPLACE) != 0, in.nf);
    constexpr int kMaxGridY = 65535;
    for (int p0 = 0; p0 < in.npairs; p0 += kMaxGridY) {
        const MatchBatch b = all.from(p0);
        const int np = b.npairs < kMaxGridY ? b.npairs : kMaxGridY;
        hipError_t e = hipSuccess;
        if (win) {
            k_match_tile_boxes<<<dim3((b.tiles + 7) / 8, np), 256, 0, s>>>(b);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            kernel<<<dim3((b.slots1 + kBatchPts - 1) / kBatchPts, np), kBatchThreads, 0, s>>>(b);
            e = hipGetLastError();
        }
        if (e == hipSuccess && cross) {
            k_match_cross_filter<<<dim3((b.slots1 + 255) / 256, np), 256, 0, s>>>(b);
            e = hipGetLastError();
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace surfhip
