// surfhip_kernels.hip -- gfx950 kernels of the SURF detect+describe path: one
// translation unit, the stages in .inc files included in pipeline order (the
// order is part of the build: k_hess_w's place in the code object matters).
// This file keeps the shared device helpers, make_plan / hessian_plan_text,
// the row-sum and generic Hessian kernels with the Hessian launchers,
// k_worklist, choose_describe / launch_describe and k_pack.
//
// Stage map (reference file:line -> file -> kernels):
//   integralRow/integralCol    surfd.cu:129-165, 2683-2704 -> surfhip_integral.inc -> k_ii_bandsum, k_ii_bandscan,
//                              k_ii_fill(_w); or written by the Hessian kernels (plan.iiw)
//   calcHessianMultiConst      surfd.cu:445-481, 2829-2894 -> surfhip_hess_p0.inc -> k_hess_p0 (octave 0);
//                              surfhip_hess_w.inc -> k_hess_w (octaves 1-3); surfhip_hess_q0.inc / _q1.inc ->
//                              k_hess_q0 / q1 / q01, and here k_hessian(_t0) (other plans), k_ii_rowseg,
//                              k_rowsum_p0 (the integral writers' row sums)
//   halfImage                  surfd.cu:321-331            -> surfhip_nms.inc -> virtual planes (OctView)
//   findMaximumWithInterp      surfd.cu:676-832, 3058-3079 -> surfhip_nms.inc -> k_nms_scan, k_scan_*, k_nms_fit
//   (atomicInc emission order) surfd.cu:825-830            -> surfhip_sort.inc -> k_sort / k_sort_rank (canonical
//                              order + per-frame cap), k_offsets; surfhip_keep.inc -> k_keep_strongest (the
//                              n strongest of a frame ahead of the sort: surfhip_detector_set_keep)
//   assignOrientationApprox    surfd.cu:1711-1960          -> surfhip_desc.inc -> orientation_wave in k_describe,
//                              k_describe_rot
//   describe*WithoutNormalization + normalize
//                              surfd.cu:1566-1615, 2391-2493 -> surfhip_desc_u2.inc -> k_describe_u2 (upright,
//                              wsz 4; k_worklist here); surfhip_desc_ur.inc -> k_describe_ur (upright, small
//                              batches); surfhip_desc.inc -> k_describe_rot (rotated, wsz 4), k_describe (the rest)
//   (result slab)                                          -> here -> k_pack
//
// Numerics: this file is compiled with -ffp-contract=off and the pragma
// below, so each written float operation rounds once (the oracle's
// semantics); explicit fmaf() only where the reference wrote __fmaf_rn.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <string.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>

#include "surfhip_internal.h"

namespace surfhip {

#define INV255 0.003921568627f          // surfd.cu:356
#define H_PI_F 1.5707963267948966f      // cuda_utils.h:8
#define SEP_ANGLE_F 0.08726646259971647f
#define WINDOW_F 1.0471975511965976f
#define M_PI_D 3.14159265358979323846

__constant__ Tables c_tab;

hipError_t set_tables(const Tables& t)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &t, sizeof(Tables), 0, hipMemcpyHostToDevice);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember
// per (kernel, device) that it was set (a process may drive several GPUs,
// from several threads)
hipError_t set_max_lds(const void* fn, int bytes)
{
    constexpr int kFns = 8, kDevs = 64;
    static const void* fns[kFns] = {};
    static std::atomic<unsigned long long> done[kFns];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kDevs) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    static std::mutex mu;
    int slot = -1;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (int i = 0; i < kFns && slot < 0; i++)
            if (fns[i] == fn || fns[i] == nullptr) {
                fns[i] = fn;
                slot = i;
            }
    }
    if (slot < 0) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const unsigned long long bit = 1ull << dev;
    if (done[slot].load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[slot].fetch_or(bit, std::memory_order_release);
    return e;
}

__device__ __forceinline__ int f2i_rn(float v) { return (int)__builtin_rintf(v); }
__device__ __forceinline__ int f2i_rz(float v) { return (int)v; }

// Where a keypoint is described: a doubled detector's integral image is of
// the 2x frame, so the reference samples it at (2x, 2y) with 3.3 * scale
// for the descriptor (surfd.cu:1581-1592, 2406-2417) and 2 * scale for the
// orientation (surfd.cu:1734-1745); otherwise (x, y) and 1.65 * scale.
struct DescAt {
    float x, y, scale;
};
template <typename PT>
__device__ __forceinline__ DescAt desc_at(int doubled, const PT& p)
{
    return doubled ? DescAt{p.x + p.x, p.y + p.y, 3.3f * p.scale} : DescAt{p.x, p.y, 1.65f * p.scale};
}
template <typename PT>
__device__ __forceinline__ DescAt ori_at(int doubled, const PT& p)
{
    return doubled ? DescAt{p.x + p.x, p.y + p.y, p.scale + p.scale} : DescAt{p.x, p.y, p.scale};
}

__device__ __forceinline__ unsigned lane_id()
{
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Buffer (SRD) memory ops.  A raw buffer load past num_records returns 0 and
// a store past it is dropped, so loads and stores at image edges need no
// branch: a branch around a load makes hipcc wait for it (vmcnt(0)) right
// there, which serialises a prefetch pipeline, and a store under a divergent
// branch makes the outstanding-op count unknown, so the next counted wait
// becomes vmcnt(0) too.  Descriptors are built from wave-uniform values only.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
typedef uint32_t v2u32 __attribute__((ext_vector_type(2)));
typedef float v2f32 __attribute__((ext_vector_type(2)));
// 3 x mod 2^32 as one full-rate v_lshl_add_u32: LLVM lowers `3u * x` to
// the quarter-rate v_mul_lo_u32 / v_mad_u64_u32, which made up about a
// quarter of the Hessian kernels' VALU issue time
__device__ __forceinline__ uint32_t mul3(uint32_t x)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(r) : "v"(x));
    return r;
}
constexpr uint32_t kOOB = 0x80000000u;          // byte offset past every buffer here

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, long long bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_ld4(rsrc_t r, uint32_t off)
{
    const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// streaming store (nt): response planes are read back only by the NMS pass
__device__ __forceinline__ void buf_st_nt(rsrc_t r, uint32_t off, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, off, 0, 2);
}

// compile-time loop: fn(std::integral_constant<int, K>) for K = 0 .. N-1
template <typename Fn, int... Ks>
__device__ __forceinline__ void static_for_seq(Fn&& fn, std::integer_sequence<int, Ks...>)
{
    (fn(std::integral_constant<int, Ks>{}), ...);
}
template <int N, typename Fn>
__device__ __forceinline__ void static_for(Fn&& fn)
{
    static_for_seq(fn, std::make_integer_sequence<int, N>{});
}

// LDS ordering between the lanes of one wave, no wait: the LDS executes one
// wave's DS instructions in issue order, so a ds_read issued after a
// ds_write of the same wave sees it (and a later write cannot overtake an
// earlier read); only the compiler must keep the order.
__device__ __forceinline__ void lds_order()
{
    asm volatile("" ::: "memory");
}

// LDS visibility between the lanes of one wave
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#include "surfhip_integral.inc"

// ======================================================================
// Hessian determinant (calcHessianMultiConst, surfd.cu:445-481; getHessian
// surfd.cu:353-366).  One thread per response sample of one octave, all
// scales of the octave; cells outside a scale's valid window are written 0
// (the reference's cudaMemset, surf.cpp:348).  Planes 0/1 of octaves > 0
// (the reference's halfImage copies, surfd.cu:321-331) are never
// materialised: the NMS kernels read them from the previous octave's planes
// 2/4 (OctView).
// ======================================================================

// getSum (surfd.cu:334-343): inclusive rect [x2..x1] x [y2..y1].
__device__ __forceinline__ uint32_t box(const uint32_t* __restrict__ I, int ip, int x1, int y1, int x2, int y2)
{
    const int yp1 = (y1 + 1) * ip;
    const int yp2 = y2 * ip;
    return I[yp1 + x1 + 1] + I[yp2 + x2] - I[yp2 + x1 + 1] - I[yp1 + x2];
}

__device__ __forceinline__ float hessian_at(const uint32_t* __restrict__ I, int ip, int x0, int y0,
                                            int m, int x2, int x3, int x4)
{
    const int xp = x0 + m, xm = x0 - m, yp = y0 + m, ym = y0 - m;
    const int32_t sxx = (int32_t)(box(I, ip, xp + x2, y0 + x3, xm - x2, y0 - x3)
                                  - 3u * box(I, ip, x0 + x2, y0 + x3, x0 - x2, y0 - x3));
    const int32_t syy = (int32_t)(box(I, ip, x0 + x3, yp + x2, x0 - x3, ym - x2)
                                  - 3u * box(I, ip, x0 + x3, y0 + x2, x0 - x3, y0 - x2));
    const int32_t sxy = (int32_t)(box(I, ip, x0 + x4, y0, x0, y0 - x4)
                                  + box(I, ip, x0, y0 + x4, x0 - x4, y0)
                                  - box(I, ip, x0 + x4, y0 + x4, x0, y0)
                                  - box(I, ip, x0, y0, x0 - x4, y0 - x4));
    const float rr = INV255 * INV255;
    const float dxx = (float)sxx;
    const float dyy = (float)syy;
    const float dxy = 0.6f * (float)sxy;
    const float a = dxx * dyy;
    const float b = dxy * dxy;
    return rr * (a - b);
}

#include "surfhip_hess_q0.inc"
#include "surfhip_hess_q1.inc"
#include "surfhip_hess_p0.inc"
#include "surfhip_hess_w.inc"

// The row sums the integral writer's strips add to their local integral
// (plan.iiw): strip k's local integral starts at its halo column cs_k = ST k
// - HALO (k_hess_w: 480 k - 144; k_hess_p0: 128 k - 16), so the image's
// integral is L_k(R, c) + II(R, cs_k), and II(R, cs_k) is the running sum
// over pixel rows r < R of S_k(r) = the sum of row r over columns [0, cs_k).
// One wave per pixel row: a wave scan of the row's dword sums, chunk by chunk
// with a running carry; the lane holding the last dword before cs_k stores
// S_k(r).  Reads columns [0, cs_{ns-1}) of the frame once (1,296 of 1,920 at
// 1080p for k_hess_w's strips).
// (16 VGPRs: its waves fit beside k_describe_u2's, which leave 20 of a SIMD
// lane's 512 free, so the pass of the next batch runs inside describe)
template <int ST, int HALO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(16))) void k_ii_rowseg(
    const uint8_t* __restrict__ frames, int pitch, long long fstride, int H, int ns, int rs_rows,
    uint32_t* __restrict__ rowseg)
{
    static_assert(ST % 4 == 0 && HALO % 4 == 0, "strip boundaries on dword boundaries");
    const int f = blockIdx.y;
    const int r = blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= H) return;
    const int lane = (int)lane_id();
    const int nd = (ST * (ns - 1) - HALO) / 4;                // dwords below the last boundary
    // the row's dwords [0, nd): a buffer load past them returns 0
    const rsrc_t R = make_rsrc(frames + (size_t)f * fstride + (size_t)r * pitch, (long long)nd * 4);
    uint32_t* out = rowseg + (size_t)f * ns * rs_rows + r;
    uint32_t carry = 0u;
    constexpr int KC = 6;                                      // loads in flight per lane
    for (int d0 = 0; d0 < nd; d0 += 64 * KC) {
        uint32_t v[KC];
#pragma unroll
        for (int i = 0; i < KC; i++)
            v[i] = __builtin_amdgcn_raw_buffer_load_b32(R, (uint32_t)(d0 + 64 * i + lane) * 4u, 0, 0);
#pragma unroll
        for (int i = 0; i < KC; i++) {
            const int d = d0 + 64 * i + lane;
            const uint32_t x = __builtin_amdgcn_udot4(v[i], 0x01010101u, 0u, false);
            uint32_t tot;
            const uint32_t inc = carry + wave_excl_scan(x, tot) + x;
            carry += tot;
            // dword d ends at column 4 d + 3: the last one below cs_k when
            // 4 (d + 1) = ST k - HALO, i.e. d + 1 + HALO / 4 = (ST / 4) k
            constexpr int DO = 1 + HALO / 4;
            if (d < nd && (d + DO) % (ST / 4) == 0) out[(size_t)((d + DO) / (ST / 4)) * rs_rows] = inc;
        }
    }
}

// plan.rsum: the same buffer from the sums k_hess_p0's producers left per
// 128-column strip and pixel row (own | left << 16, p0_producer RS), no pass
// over the frames: S_k(r) = the own-column sums of the strips entirely left
// of X_k = ST k - HALO plus the left-of-X sum of the strip that holds X_k.
// One thread per frame and pixel row walks the strips once (a wave's loads
// are 64 consecutive rows of a slab); writes exactly what
// k_ii_rowseg<ST, HALO> writes: slabs 1 .. ns - 1, rows < H.
static_assert(p0::XST == hw::ST && p0::XHALO == hw::H, "k_hess_p0 prepares k_hess_w's strips' row sums");
template <int ST, int HALO>
__global__ __launch_bounds__(256) void k_rowsum_p0(const uint32_t* __restrict__ psum, int H, int np, int ns,
                                                   int rs_rows, uint32_t* __restrict__ rowseg)
{
    const int f = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    if (r >= H) return;
    const uint32_t* in = psum + (size_t)f * np * rs_rows + r;
    uint32_t* out = rowseg + (size_t)f * ns * rs_rows + r;
    uint32_t run = 0u;
    int sp = 0;
    for (int k = 1; k < ns; k++) {
        const int sx = (ST * k - HALO) >> 7;                   // the 128-column strip holding X_k
        if (sx >= np) break;                                   // (never: X_k < W)
        for (; sp < sx; sp++) run += in[(size_t)sp * rs_rows] & 0xffffu;
        out[(size_t)k * rs_rows] = run + (in[(size_t)sx * rs_rows] >> 16);
    }
}

hipError_t launch_rowseg(const FrameBatch& b, const FrameParams& P, const LaunchPlan& plan, uint32_t* rowseg,
                         hipStream_t s)
{
    // (plan.rsum: launch_hess_oct0 makes them)
    if (!plan.iiw || plan.rs_nstrips < 2 || plan.rsum) return hipSuccess;
    const dim3 g((P.H + 3) / 4, b.n);
    if (plan.iiw == 2)
        k_ii_rowseg<128, 16><<<g, 256, 0, s>>>(b.frames, b.pitch, b.stride, P.H, plan.rs_nstrips, plan.rs_rows, rowseg);
    else
        k_ii_rowseg<hw::ST, hw::H><<<g, 256, 0, s>>>(b.frames, b.pitch, b.stride, P.H, plan.rs_nstrips, plan.rs_rows,
                                                     rowseg);
    return hipGetLastError();
}

// Octave 1 on k_hess_q1 (only when k_hess_w is off: 2-octave detectors or
// SURFHIP_HESS_W=0) needs the geometry compiled into it (sampling 2, lobes
// 15/19/23).
static bool q1_ok(const FrameParams& P, const OctaveParams& q)
{
    static const int masks[3] = {15, 19, 23};
    if (P.sampling != 2 || q.delta != 4 || q.nscale != 3 || q.init_scale != 2) return false;
    for (int i = 0; i < 3; i++)
        if (q.mask[i] != masks[i] || q.x2[i] != masks[i] / 2 || q.x3[i] != 2 * (masks[i] / 2) ||
            q.x4[i] != 3 * (masks[i] / 2))
            return false;
    return true;
}

// Octave 0 on k_hess_q0 when its geometry is the one compiled into it
// (sampling 2, lobes 3/5/7/9/11).
static bool q0_ok(const FrameParams& P, const OctaveParams& q)
{
    static const int masks[5] = {3, 5, 7, 9, 11};
    if (P.sampling != 2 || q.delta != 2 || q.nscale != 5 || q.init_scale != 0) return false;
    for (int i = 0; i < 5; i++)
        if (q.mask[i] != masks[i] || q.x2[i] != masks[i] / 2 || q.x3[i] != 2 * (masks[i] / 2) ||
            q.x4[i] != 3 * (masks[i] / 2))
            return false;
    return true;
}

// k_hessian_t0 (octave 0 of the gather plan from LDS tiles): sample rows per
// workgroup and the corners' reach it stages (16 for init mask 9: lobe 11,
// m + x2 = 16)
constexpr int kT0BY = 8;
constexpr int kT0Halo = 16;

// Octaves 1 .. n of the default geometry (sampling 2, init mask 9: lobes
// 15/19/23, 31/39/47, 63/79/95) on k_hess_w; returns n (2 or 3) or 0.
static int hw_octaves(const FrameParams& P, const OctaveParams* oct)
{
    if (P.sampling != 2 || P.noct < 3) return 0;
    int n = 0;
    for (int o = 1; o <= 3 && o < P.noct; o++) {
        const OctaveParams& q = oct[o];
        bool ok = q.delta == (2 << o) && q.nscale == 3 && q.init_scale == 2;
        for (int i = 0; ok && i < 3; i++) {
            const int K = hw::kof(o, i);
            ok = q.mask[i] == 2 * K + 1 && q.x2[i] == K && q.x3[i] == 2 * K && q.x4[i] == 3 * K;
        }
        if (!ok) break;
        n = o;
    }
    return n >= 2 ? n : 0;
}

// Which kernel computes each octave's planes:
//   octave 0      k_hess_q0 (u8 frame; default geometry, batches > kGatherBatch)
//   octaves 1-3   k_hess_w (u8 frame; default geometry, 3+ octaves)
//   octave 1      k_hess_q1 when k_hess_w is off (2 octaves, or SURFHIP_HESS_W=0);
//                 k_hess_q0 + k_hess_q1 in one launch (k_hess_q01) unless SURFHIP_Q01=0
//   the rest      k_hessian, one thread per sample over the integral image
//                 (every octave for batches <= kGatherBatch or SURFHIP_HESS_GATHER=1)
// (sw: the detector's switches, read when it was created)
void make_plan(const FrameParams& P, const OctaveParams* oct, const Switches& sw, LaunchPlan& plan, int max_batch)
{
    plan = LaunchPlan{};
    int hb = 0, nb = 0;
    const bool gather = sw.hess_gather >= 0 ? sw.hess_gather != 0 : max_batch <= kGatherBatch;
    plan.hw_n = (!gather && sw.hess_w) ? hw_octaves(P, oct) : 0;
    plan.hw_nstrips = (P.W + hw::ST - 1) / hw::ST;
    plan.hw_nblk = ((P.H / 4 + 1 + hw::U - 1) / hw::U) * hw::U;
    plan.q0 = !gather && P.noct > 0 && q0_ok(P, oct[0]);
    plan.q0_strips = (oct[0].sw + 63) / 64;
    plan.q1 = !gather && P.noct > 1 && plan.hw_n == 0 && q1_ok(P, oct[1]);
    plan.q1_strips = P.noct > 1 ? (oct[1].sw + 63) / 64 : 0;
    plan.q01 = plan.q0 && plan.q1 && sw.q01;
    // octave 0 on k_hess_p0 unless SURFHIP_P0=0; SURFHIP_P0=BG (value 10 B + G)
    // picks its barrier interval B (steps) and consumer waves G
    plan.p0 = (plan.q0 && !plan.q01) ? sw.p0 : 0;
    // the gather plan's octave 0 from LDS tiles (k_hessian_t0) when its
    // corners reach at most kT0Halo integral samples from the sample and the
    // sampling step is 2 (the default geometry); SURFHIP_HESS_T0=0 disables
    {
        const OctaveParams& q = oct[0];
        int reach = 0;
        for (int i = 0; i < q.nscale; i++) reach = std::max(reach, std::max(q.mask[i] + q.x2[i], q.x4[i]));
        plan.t0 = gather && P.noct > 0 && q.delta == 2 && reach <= kT0Halo && sw.hess_t0;
        plan.t0_nbx = (q.sw + 63) / 64;
        plan.t0_nby = (q.sh + kT0BY - 1) / kT0BY;
    }
    for (int o = 0; o < kMaxOct; o++) {
        plan.hess_start[o] = hb;
        plan.nms_start[o] = nb;
        if (o < P.noct) {
            const OctaveParams& q = oct[o];
            plan.hess_nbx[o] = (q.sw + 63) / 64;
            const bool on_u8 = (o == 0 && plan.q0) || (o == 1 && plan.q1) || (o >= 1 && o <= plan.hw_n);
            if (!on_u8 && !(o == 0 && plan.t0)) hb += plan.hess_nbx[o] * ((q.sh + 3) / 4);
            plan.nms_nbx[o] = (q.nms_gx + 63) / 64;
            plan.nms_nby[o] = (q.nms_gy + kScanRows - 1) / kScanRows;
            nb += ((P.max_scale - 1) / 2) * plan.nms_nbx[o] * plan.nms_nby[o];   // levels k = 1, 3, .. < max_scale - 1
        } else {
            plan.hess_nbx[o] = plan.nms_nbx[o] = plan.nms_nby[o] = 1;
        }
    }
    plan.hess_start[kMaxOct] = hb;
    plan.nms_start[kMaxOct] = nb;
    // the integral image from k_hess_w (SURFHIP_II_FUSE=0 disables, =2 moves
    // it to k_hess_p0's producer): octave 0 on k_hess_p0 and octaves 1-3 on
    // k_hess_w; octaves past 3 (k_hessian) then read the integral written,
    // after them on the same stream
    {
        const bool on = plan.hw_n >= 2 && plan.p0 != 0 && !plan.t0 && sw.ii_fuse != 0;
        plan.iiw = !on ? 0 : (sw.ii_fuse == 2 && plan.p0 == 93) ? 2 : 1;
        plan.rs_rows = 4 * plan.hw_nblk;
        plan.rs_nstrips = plan.iiw == 2 ? plan.q0_strips : plan.hw_nstrips;
        // k_hess_w's row sums from k_hess_p0's producers instead of
        // k_ii_rowseg's pass over the frames: k_hess_w writes the integral,
        // octave 0 runs on the default k_hess_p0 (the RS instantiation) and
        // there is more than one k_hess_w strip; SURFHIP_ROWSUM=rowseg keeps
        // the pass (A/B), =p0 is the default
        plan.rsum = plan.iiw == 1 && plan.p0 == 93 && plan.rs_nstrips >= 2 && !sw.rowsum_rowseg;
    }
}

std::string hessian_plan_text(const LaunchPlan& plan, const FrameParams& P)
{
    std::string t;
    auto add = [&](const char* k, int o0, int o1) {
        if (o1 < o0) return;
        if (!t.empty()) t += " + ";
        t += k;
        t += o0 == o1 ? " (octave " + std::to_string(o0) + ")"
                      : " (octaves " + std::to_string(o0) + "-" + std::to_string(o1) + ")";
    };
    if (plan.q01) {
        add("k_hess_q01", 0, 1);
    } else {
        if (plan.p0) add("k_hess_p0", 0, 0);
        else if (plan.q0) add("k_hess_q0", 0, 0);
        if (plan.q1) add("k_hess_q1", 1, 1);
    }
    if (plan.t0) add("k_hessian_t0", 0, 0);
    if (plan.hw_n > 0) add("k_hess_w", 1, plan.hw_n);
    // (the row-sum pass runs before the stage: beside the previous batch's
    // NMS when pipelined, like the integral passes it replaces)
    if (plan.iiw) t += plan.iiw == 2 ? ", writing the integral image (k_hess_p0)" : ", writing the integral image";
    // the writer's row sums: from k_hess_p0's producers (plan.rsum), or the
    // pass over the frames (a single strip needs none)
    if (plan.iiw && plan.rs_nstrips >= 2)
        t += plan.rsum ? ", row sums from k_hess_p0 + k_rowsum_p0" : ", row sums from k_ii_rowseg";
    if (plan.hess_start[kMaxOct] > 0) {
        int lo = -1, hi = -1;
        for (int o = 0; o < P.noct; o++)
            if (plan.hess_start[o + 1] > plan.hess_start[o]) { if (lo < 0) lo = o; hi = o; }
        if (lo >= 0) add("k_hessian", lo, hi);
    }
    return t;
}

__device__ __forceinline__ int octave_of(const int* start, int noct, int b)
{
    int o = 0;
    while (o + 1 < noct && b >= start[o + 1]) o++;
    return o;
}

// 1-D grid of nf8 * per workgroups, XCD-aware: the workgroups of XCD x
// (blockIdx % 8) take frames x, x + 8, ..., each frame's `per` workgroups
// together, so a frame's integral image / response planes are fetched into
// one XCD's L2 instead of all eight.
// Batches of fewer than 8 frames spread each frame's workgroups over all
// XCDs instead (one frame per XCD would leave the others idle); the grid is
// frame_grid(nframes) * per.
__device__ __forceinline__ bool xcd_frame_block(int per, int nframes, int& f, int& lb)
{
    if (nframes < 8) {
        f = blockIdx.x / per;
        lb = blockIdx.x - f * per;
        return f < nframes;
    }
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    f = (k / per) * 8 + xcd;
    lb = k - (k / per) * per;
    return f < nframes;
}
static inline int frame_grid(int nframes) { return nframes < 8 ? nframes : (nframes + 7) & ~7; }

// All octaves (not on an LDS ring) of a frame in one launch: the local block
// index walks the octaves' sample grids (64 x 4 samples per block).
__global__ __launch_bounds__(256) void k_hessian(const int32_t* __restrict__ ii, float* __restrict__ resp,
                                                 FrameParams P, const OctaveParams* __restrict__ oct,
                                                 LaunchPlan plan, int nframes)
{
    int f, gb;
    if (!xcd_frame_block(plan.hess_start[kMaxOct], nframes, f, gb)) return;
    const int o = octave_of(plan.hess_start, P.noct, gb);
    const OctaveParams& q = oct[o];
    const int lb = gb - plan.hess_start[o];
    const int nbx = plan.hess_nbx[o];
    const int ix = (lb % nbx) * 64 + (threadIdx.x & 63);
    const int iy = (lb / nbx) * 4 + (threadIdx.x >> 6);
    if (ix >= q.sw || iy >= q.sh) return;
    const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
    float* R = resp + (size_t)f * P.resp_stride + q.ooff + (size_t)iy * q.sp + ix;
    const int x0 = q.delta * ix, y0 = q.delta * iy;
    const int ns = q.nscale;
#pragma unroll
    for (int i = 0; i < kMaxScale; i++) {
        if (i >= ns) break;
        const int b1 = q.b1[i];
        float v = 0.f;
        if (ix >= b1 && ix < q.sw - b1 && iy >= b1 && iy < q.sh - b1)
            v = hessian_at(I, P.ip, x0, y0, q.mask[i], q.x2[i], q.x3[i], q.x4[i]) * q.norm[i];
        R[(size_t)(q.init_scale + i) * q.osize] = v;
    }
}

// Octave 0 of the gather plan (few frames, config #2) from LDS tiles: a
// workgroup loads the integral-image tile under its 64 x kT0BY samples (the
// samples' span plus every corner's reach, kT0Halo on each side) with
// coalesced row loads, then each thread computes its samples' scales with
// hessian_at reading the tile -- the 32 corners of a response are LDS reads
// instead of global gathers (k_hessian: 32 dependent-latency gathers per
// response, 55 us for one 1080p frame's four octaves, 80 % of the responses
// in octave 0).  Same integer box sums and float ops as k_hessian, so the
// planes are bit-identical.
template <int HALO>
__global__ __launch_bounds__(256) void k_hessian_t0(const int32_t* __restrict__ ii, float* __restrict__ resp,
                                                    FrameParams P, OctaveParams q, int nbx, int nby, int nframes)
{
    constexpr int TW = 2 * 63 + 2 * HALO + 2;           // tile columns: integral x in [2 ix0 - HALO, ..]
    constexpr int TH = 2 * (kT0BY - 1) + 2 * HALO + 2;  // tile rows
    __shared__ uint32_t T[TH * TW];
    int f, lb;
    if (!xcd_frame_block(nbx * nby, nframes, f, lb)) return;
    const int by = lb / nbx, bx = lb - by * nbx;
    const int ix0 = bx * 64, iy0 = by * kT0BY;
    const int tx0 = 2 * ix0 - HALO, ty0 = 2 * iy0 - HALO;
    const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    // rows by wave, columns by lane (coalesced); coordinates outside the
    // image are clamped -- only samples outside the borders, which are not
    // computed, would read them
    for (int r = wv; r < TH; r += 4) {
        const int gy = min(max(ty0 + r, 0), P.iH - 1);
        const uint32_t* row = I + (size_t)gy * P.ip;
#pragma unroll
        for (int c0 = 0; c0 < TW; c0 += 64) {
            const int c = c0 + lane;
            if (c < TW) T[r * TW + c] = row[min(max(tx0 + c, 0), P.ip - 1)];
        }
    }
    __syncthreads();
    const int ix = ix0 + lane;
    for (int k = wv; k < kT0BY; k += 4) {
        const int iy = iy0 + k;
        if (ix >= q.sw || iy >= q.sh) continue;
        float* R = resp + (size_t)f * P.resp_stride + q.ooff + (size_t)iy * q.sp + ix;
        const int lx = 2 * lane + HALO, ly = 2 * k + HALO;          // (x0, y0) in the tile
#pragma unroll
        for (int i = 0; i < kMaxScale; i++) {
            if (i >= q.nscale) break;
            const int b1 = q.b1[i];
            float v = 0.f;
            if (ix >= b1 && ix < q.sw - b1 && iy >= b1 && iy < q.sh - b1)
                v = hessian_at(T, TW, lx, ly, q.mask[i], q.x2[i], q.x3[i], q.x4[i]) * q.norm[i];
            R[(size_t)(q.init_scale + i) * q.osize] = v;
        }
    }
}

// (ahead of launch_hess_oct0: k_hess_w keeps its place ahead of k_hess_p0 in the code object)
hipError_t launch_hess_w(const HessianArgs& a, hipStream_t s)
{
    const LaunchPlan& plan = *a.plan;
    const FrameBatch& b = a.b;
    if (!b.frames && plan_reads_frames(plan)) return hipErrorInvalidValue;
    if (plan.hw_n == 0) return hipSuccess;
    const dim3 g(((b.n + 7) & ~7) * plan.hw_nstrips);
    const OctaveParams& q3 = a.h_oct[plan.hw_n >= 3 ? 3 : 2];
    const bool wr = plan.iiw == 1 && a.ii_out && a.rowseg;
#define HW_LAUNCH(NO, IIW)                                                                                       \
    k_hess_w<NO, IIW><<<g, hw::THREADS, 0, s>>>(b.frames, b.pitch, b.stride, a.resp, *a.P, a.h_oct[1], a.h_oct[2], \
                                                q3, plan.hw_nstrips, b.n, plan.hw_nblk, a.rowseg, a.ii_out,      \
                                                plan.rs_rows)
    if (plan.hw_n >= 3) {
        if (wr) HW_LAUNCH(3, true);
        else HW_LAUNCH(3, false);
    } else {
        if (wr) HW_LAUNCH(2, true);
        else HW_LAUNCH(2, false);
    }
#undef HW_LAUNCH
    return hipGetLastError();
}

hipError_t launch_hess_oct0(const HessianArgs& a, hipStream_t s)
{
    const LaunchPlan& plan = *a.plan;
    const FrameParams& P = *a.P;
    const FrameBatch& b = a.b;
    if (!b.frames && plan_reads_frames(plan)) return hipErrorInvalidValue;
    const int nf8 = (b.n + 7) & ~7;
    const int nb0 = 8 * (((nf8 / 8) * plan.q0_strips + q0::WAVES - 1) / q0::WAVES);
    const int nb1 = 8 * (((nf8 / 8) * plan.q1_strips + q1::WAVES - 1) / q1::WAVES);
    if (plan.q01) {
        k_hess_q01<<<dim3(nb0 + nb1), q0::THREADS, 0, s>>>(b.frames, b.pitch, b.stride, a.resp, P, a.h_oct[0],
                                                           a.h_oct[1], plan.q0_strips, plan.q1_strips, nb0, b.n);
        return hipGetLastError();
    }
    const dim3 gp(nf8 * plan.q0_strips);
    const int pb = plan.p0 / 10, pg = plan.p0 % 10;      // interval, consumer waves
    // (iiw 2, only with the default 93: this launch writes the integral)
    const bool wr0 = plan.iiw == 2 && a.ii_out && a.rowseg;
#define P0_CASE(BB, GG)                                                                                          \
    else if (pb == BB && pg == GG) k_hess_p0<BB, GG, p0::PLANE_NT, false><<<gp, 64 * (1 + GG), 0, s>>>(            \
        b.frames, b.pitch, b.stride, a.resp, P, a.h_oct[0], plan.q0_strips, b.n, nullptr, nullptr, 0, nullptr, 0);
    // (rsum, only with the default 93 and k_hess_w writing the integral: this
    // launch also leaves its strips' row sums in psum, k_rowsum_p0 adds them
    // up into rowseg for the k_hess_w launch that follows on this stream)
    const bool rs0 = plan.rsum && plan.iiw == 1 && a.ii_out && a.rowseg && a.psum;
    if (wr0 && pb == 9 && pg == 3)
        k_hess_p0<9, 3, p0::PLANE_NT, true><<<gp, 64 * 4, 0, s>>>(b.frames, b.pitch, b.stride, a.resp, P,
                                                                  a.h_oct[0], plan.q0_strips, b.n, a.rowseg,
                                                                  a.ii_out, plan.rs_rows, nullptr, 0);
    else if (rs0 && pb == 9 && pg == 3) {
        k_hess_p0<9, 3, p0::PLANE_NT, false, true><<<gp, 64 * 4, 0, s>>>(
            b.frames, b.pitch, b.stride, a.resp, P, a.h_oct[0], plan.q0_strips, b.n, nullptr, nullptr, plan.rs_rows,
            a.psum, plan.hw_nstrips);
        k_rowsum_p0<hw::ST, hw::H><<<dim3((P.H + 255) / 256, b.n), 256, 0, s>>>(
            a.psum, P.H, plan.q0_strips, plan.rs_nstrips, plan.rs_rows, a.rowseg);
    }
    P0_CASE(9, 5) P0_CASE(9, 3) P0_CASE(9, 2) P0_CASE(9, 1) P0_CASE(3, 2)
#undef P0_CASE
    else if (plan.q0)
        k_hess_q0<4, 1, 2><<<dim3(nb0), q0::THREADS, 0, s>>>(b.frames, b.pitch, b.stride, a.resp, P, a.h_oct[0],
                                                             plan.q0_strips, b.n);
    if (plan.q1)
        k_hess_q1<2><<<dim3(nb1), q1::THREADS, 0, s>>>(b.frames, b.pitch, b.stride, a.resp, P, a.h_oct[1],
                                                       plan.q1_strips, b.n);
    return hipGetLastError();
}

hipError_t launch_hess_ii(const HessianArgs& a, hipStream_t s)
{
    const LaunchPlan& plan = *a.plan;
    if (plan.t0)
        k_hessian_t0<kT0Halo><<<dim3(frame_grid(a.b.n) * plan.t0_nbx * plan.t0_nby), 256, 0, s>>>(
            a.ii, a.resp, *a.P, a.h_oct[0], plan.t0_nbx, plan.t0_nby, a.b.n);
    if (plan.hess_start[kMaxOct] > 0)
        k_hessian<<<dim3(frame_grid(a.b.n) * plan.hess_start[kMaxOct]), 256, 0, s>>>(a.ii, a.resp, *a.P, a.d_oct, plan,
                                                                                     a.b.n);
    return hipGetLastError();
}

#include "surfhip_nms.inc"
#include "surfhip_keep.inc"
#include "surfhip_sort.inc"
#include "surfhip_desc.inc"
#include "surfhip_desc_ur.inc"
#include "surfhip_desc_u2.inc"

// The describe schedule flattened for k_describe_u2: entry offsets[f] + i =
// keypoint order[f][i]'s {x, y, scale, f * max_pts + kp}, so the describe
// loop reaches a keypoint in one load after its queue atomic (order[] and
// pts[] were two dependent loads, and the frame a search over offsets[]).
__global__ __launch_bounds__(256) void k_worklist(const surfhip_point* __restrict__ pts, int max_pts,
                                                  const int* __restrict__ counts, const int* __restrict__ offsets,
                                                  const int* __restrict__ order, float4* __restrict__ work,
                                                  FrameParams P)
{
    // a frame's entries over gridDim.x workgroups, strided (most of a
    // max_pts-sized grid would find nothing to do).  Entry = three float4:
    // the keypoint's window geometry, the describe kernel's per-keypoint
    // set-up moved here (surfd.cu:1581-1596, the upright branch of describe),
    // then the point's laplace / ori words (getTrace's inputs when the fit
    // left it to the describe, nms_fit_point):
    //   {dx, dy, spacing, f}  {ix, iy, step | hs << 10 | iradius << 22, f * max_pts + kp}
    //   {laplace, ori, 1 / spacing, 0}
    // (10 / 12 / 9 bits, iradius below the int's sign: choose_describe takes this path
    // only when the largest window of the detector's octaves fits, worklist_fits)
    const int f = blockIdx.y, n = counts[f], o = offsets[f];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int idx = f * max_pts + order[(size_t)f * max_pts + i];
        const surfhip_point p = pts[idx];
        const DescAt at = desc_at(P.doubled, p);
        const float scale = at.scale;
        const int step = max(f2i_rn(scale * 0.5f), 1);
        const int ix = f2i_rn(at.x), iy = f2i_rn(at.y);
        const float spacing = scale * (float)P.mag;
        const int hs = f2i_rz(scale);
        const int iradius = f2i_rn(((spacing * (float)(P.wsz + 1)) * 0.5f) / (float)step);
        float4* e = work + kWorkF4 * (size_t)(o + i);
        e[0] = make_float4(at.x - (float)ix, at.y - (float)iy, spacing, __int_as_float(f));
        e[1] = make_float4(__int_as_float(ix), __int_as_float(iy), __int_as_float(step | (hs << 10) | (iradius << 22)),
                           __int_as_float(idx));
        e[2] = make_float4(__int_as_float(p.laplace), p.ori, 1.f / spacing, 0.f);
    }
}

// Whether k_worklist's packed fields hold every keypoint window of this
// detector: the largest keypoint scale is makePoint's 1.2 ns
// divisor (surfd.cu:1001-1022) at the top octave with s + off <= max_scale -
// 1 + 1.5 (the fit's limits); describe uses 1.65 x (3.3 x doubled) of it
// (surfd.cu:1581-1592); step = rn(S / 2) < 2^10, hs = rz(S) < 2^12, iradius
// = rn(spacing (wsz + 1) / 2 / step) < 2^9: it sits in bits 22-31 of a signed
// int that k_describe_u2 decodes with an arithmetic shift.  The iradius bound
// decides nothing: the path needs wsz 4, hence mag 3 and iradius = 7.5 S /
// step + 1 with step = max(floor(S / 2 + 0.5), 1), below 24 for every S.
static bool worklist_fits(const FrameParams& P)
{
    const float oct = (float)(1 << (P.noct - 1));
    const float ns = ((float)P.init_lobe + (oct - 1.f) * (float)P.max_scale + ((float)P.max_scale + 0.5f) * 2.f * oct) / 3.f;
    const float S = (P.doubled ? 3.3f : 1.65f) * 1.2f * ns * P.divisor;
    const float step = std::max(std::floor(S * 0.5f + 0.5f), 1.f);
    const float iradius = S * (float)P.mag * (float)(P.wsz + 1) * 0.5f / step + 1.f;
    return S * 0.5f + 1.f < 1024.f && S + 1.f < 4096.f && iradius < 512.f;
}

DescribeChoice choose_describe(const Switches& sw, const FrameParams& P, int nframes)
{
    // SURFHIP_DESC_UR=1 / 0 forces k_describe_ur / k_describe_u2; default:
    // k_describe_ur for batches of <= kGatherBatch frames, where a wave gets
    // about one keypoint and the ring's fill latency is not amortised -- one
    // 1080p frame's describe 0.032 -> 0.030 ms
    const bool want_u2 = sw.desc_ur >= 0 ? sw.desc_ur == 0 : nframes > kGatherBatch;
    if (P.upright && P.wsz == 4) {
        if (!(want_u2 && worklist_fits(P))) return {kDescUr, false};
        // the fit's stash holds the box centre as two int16 (nms_fit_point,
        // decoded signed in k_describe_u2): from integral row / column 32768 on
        // the sign stays in the fit (trace_sign), whatever the switch says
        const bool fits16 = P.iH < 32768 && P.W + 1 < 32768;
        return {kDescU2, sw.trace_desc && fits16};
    }
    // windows past 4 x 4 x 8 (desc_wsz 5..7: up to 392 features)
    if (P.nfeat > 128) return {kDescWide, false};
    if (P.upright) return {kDescUpright, false};
    return {P.wsz == 4 && !sw.rot_atomic ? kDescRot : kDescRotAtomic, false};
}

hipError_t launch_describe(const int32_t* ii, const FrameParams& P, const PointSlots& p, const DescribeSchedule& sch,
                           int nframes, float* desc, hipStream_t s, bool beside, int cus, const Switches& sw,
                           DescribeChoice how)
{
    if (P.nfeat > 512) return hipErrorInvalidValue;
    // the describe kernels are persistent (per-XCD keypoint queues): 2,048
    // workgroups fill every CU; with another stream's kernels beside them
    // (SURFHIP_DESC_BESIDE workgroups per CU, default 3) a slot stays free
    if (cus <= 0) cus = 256;
    const int grid = (beside && sw.desc_beside > 0) ? ((sw.desc_beside * cus + 7) & ~7) : 2048;
    hipError_t e = hipMemsetAsync(sch.queue, 0, kDescQueueBytes, s);
    if (e != hipSuccess) return e;
    auto counted = [&](auto* k) {       // k_describe reads the counts, the others only their prefix
        k<<<grid, 256, 0, s>>>(ii, P, p.pts, p.max_pts, p.counts, sch.offsets, sch.order, nframes, desc, sch.queue);
    };
    auto plain = [&](auto* k) {
        k<<<grid, 256, 0, s>>>(ii, P, p.pts, p.max_pts, sch.offsets, sch.order, nframes, desc, sch.queue);
    };
    switch (how.kernel) {
        case kDescU2: {         // the LDS-DMA ring
            k_worklist<<<dim3(std::min(8, (p.max_pts + 255) / 256), nframes), 256, 0, s>>>(
                p.pts, p.max_pts, p.counts, sch.offsets, sch.order, sch.work, P);
            // (diagnostic: SURFHIP_U2_LDSPAD bytes of unused dynamic LDS per workgroup)
            auto* k = P.extend ? &k_describe_u2<true> : &k_describe_u2<false>;
            k<<<grid, 256, sw.u2_ldspad, s>>>(ii, P, sch.work, p.max_pts, sch.offsets, nframes, desc, sch.queue, p.pts,
                                              how.trace ? 1 : 0);
            break;
        }
        case kDescUr: plain(P.extend ? &k_describe_ur<true> : &k_describe_ur<false>); break;    // round 3's kernel
        case kDescWide: counted(P.upright ? &k_describe<true, 512> : &k_describe<false, 512>); break;
        case kDescUpright: counted(&k_describe<true, 128>); break;
        case kDescRot: plain(P.osz == 8 ? &k_describe_rot<8> : &k_describe_rot<4>); break;
        case kDescRotAtomic: counted(&k_describe<false, 128>); break;
    }
    return hipGetLastError();
}

// ======================================================================
// Result slab for the multi-GPU all-gather, compacted:
//   int32 header[4] = {nframes, total, nfeatures, 0}
//   int32 counts[nframes] (padded to 16 B)
//   SurfPoint points[total]            frame-major, canonical order
//   float     desc[total][nfeatures]   (absent when desc == nullptr)
// offsets[] is the exclusive prefix of counts written by k_offsets.
// ======================================================================
__global__ __launch_bounds__(256) void k_pack(const surfhip_point* __restrict__ pts, const float* __restrict__ desc,
                                              const int* __restrict__ counts, const int* __restrict__ offsets,
                                              int nframes, int max_pts, int nfeat, const int* __restrict__ status,
                                              size_t cap_bytes, uint8_t* __restrict__ slab)
{
    const int f = blockIdx.y;
    const int total = offsets[nframes];
    const size_t head = 16 + (((size_t)nframes * 4 + 15) & ~(size_t)15);
    const size_t need = head + (size_t)total * (sizeof(surfhip_point) + (desc ? 4 * (size_t)nfeat : 0));
    const bool fits = need <= cap_bytes;
    int* hdr = reinterpret_cast<int*>(slab);
    if (f == 0 && blockIdx.x == 0) {
        // hdr[3] bit 0: a frame of this batch was truncated at the candidate
        // capacity; bit 1: the slab did not fit cap_bytes (payload not written)
        if (threadIdx.x == 0) {
            hdr[0] = nframes;
            hdr[1] = total;
            hdr[2] = desc ? nfeat : 0;
            hdr[3] = (status ? (*status & 1) : 0) | (fits ? 0 : 2);
        }
        const int npad = (nframes + 3) & ~3;          // counts padded to 16 B with zeros (stable file bytes)
        for (int i = threadIdx.x; i < npad; i += 256) hdr[4 + i] = i < nframes ? counts[i] : 0;
    }
    if (!fits) return;
    surfhip_point* pout = reinterpret_cast<surfhip_point*>(slab + head);
    float* dout = reinterpret_cast<float*>(slab + head + (size_t)total * sizeof(surfhip_point));
    const int cnt = counts[f], off = offsets[f];
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t t = tid; t < (size_t)cnt; t += stride) pout[off + t] = pts[(size_t)f * max_pts + t];
    if (desc) {
        const float* src = desc + (size_t)f * max_pts * nfeat;
        float* dst = dout + (size_t)off * nfeat;
        const size_t n4 = (size_t)cnt * nfeat / 4;          // nfeat is 64 or 128
        for (size_t t = tid; t < n4; t += stride)
            reinterpret_cast<float4*>(dst)[t] = reinterpret_cast<const float4*>(src)[t];
    }
}

hipError_t launch_pack(const surfhip_point* pts, const float* desc, const int* counts, const DescribeSchedule& sch,
                       int nframes, int max_pts, int nfeat, const int* status, size_t cap_bytes, uint8_t* slab,
                       hipStream_t s)
{
    k_pack<<<dim3(16, nframes), 256, 0, s>>>(pts, desc, counts, sch.offsets, nframes, max_pts, nfeat, status,
                                             cap_bytes, slab);
    return hipGetLastError();
}

// surfhip_run_describe's schedule (launch_plant).  A template, instantiated
// here at the end of the file, so that it is the code object's last kernel:
// the other kernels keep their places relative to each other.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_plant(const int* __restrict__ counts, int max_pts,
                                                   int* __restrict__ clamped, int* __restrict__ order)
{
    const int f = blockIdx.y, n = min(max(counts[f], 0), max_pts);
    if (blockIdx.x == 0 && threadIdx.x == 0) clamped[f] = n;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < n; i += gridDim.x * THREADS)
        order[(size_t)f * max_pts + i] = i;
}

hipError_t launch_plant(const int* counts, int nframes, const PointSlots& pts, const DescribeSchedule& sch,
                        hipStream_t s)
{
    k_plant<256><<<dim3(std::min(8, (pts.max_pts + 255) / 256), nframes), 256, 0, s>>>(counts, pts.max_pts, pts.counts,
                                                                                       sch.order);
    k_offsets<<<1, 1024, 0, s>>>(pts.counts, nframes, sch.offsets);
    return hipGetLastError();
}

}  // namespace surfhip
