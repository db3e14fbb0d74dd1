// surfhip_hess_p0.inc -- octave-0 Hessian with the strip-local integral built
// once per workgroup and the five scales split over consumer waves
// (k_hess_p0, the default for octave 0).
//
// Reference: calcHessianMultiConst (surfd.cu:445-481), getHessian
// (surfd.cu:353-366), getSum (surfd.cu:334-343), launched for octave 0 by
// cuCalcHessianMulti (surfd.cu:2829-2894).
//
// Same arithmetic as k_hess_q0 (surfhip_hess_q0.inc: row-pair F / E / G
// differences in packed fp32 on exact integers, 18-step epochs with the
// accumulator corrections at each rebase), different division of work.
// k_hess_q0 gives one wave a 64-sample strip and all five scales: its
// accumulator rings take ~140 registers (242 in all), so 2 waves fit a SIMD
// and each wave issues in only 61 % of its cycles.  Here a workgroup owns
// the same strip:
//   * wave 0 (producer) loads the u8 rows, scans each row pair once and
//     writes the step's local-integral rows (float2 per column) into LDS
//     slot K % 2B of a ring, and at each epoch start the old integral at the
//     new base row (Delta);
//   * G consumer waves each own a group of scales ({0,1} {2,3} {4} for the
//     default G = 3): they read the step's column entries their scales use
//     (once per wave), fold them into their rings of sample-row accumulators
//     and finalise / store the completed rows.
// Consumers lag the producer by one barrier interval of B steps (one
// s_barrier per interval; a slot is rewritten 2B steps later).
// Measured (batch 256 x 1080p, Hessian stage with k_hess_w): G = 3 1.26 ms,
// G = 2 1.28, G = 5 1.36 (each wave reads its own column entries: 50 instead
// of 34 LDS reads per step), G = 1 1.36, k_hess_q0 1.28; the producer alone
// runs in 0.29 ms and the consumers alone in 0.66 ms of the 0.78.
// Planes are bit-identical to k_hess_q0's (the same float ops on the same
// exact integers), hence to the reference's int32 arithmetic.

namespace p0 {
constexpr int PD = 6;                     // producer: steps of u8 rows loaded ahead
constexpr int PLANE_NT = 1;               // octave-0 plane stores non-temporal (0: default policy)
constexpr int IIW_AUX = 2;                // integral-image stores' cache policy (IIW): nt
static_assert(q0::P % PD == 0, "prefetch slot static within an epoch");
// (RS) the integral writer's strips whose row sums the producer prepares:
// k_hess_w's, halo column X_k = XST k - XHALO (hw::ST, hw::H; checked where
// both are in scope)
constexpr int XST = 480, XHALO = 144;
static_assert(XST % 4 == 0 && XHALO % 4 == 0, "every X on a lane boundary (4 columns per lane)");
}  // namespace p0

// LDS ordering: every wave's LDS ops done, then the workgroup barrier (no
// vmcnt wait: the producer's prefetch loads stay in flight)
__device__ __forceinline__ void p0_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---------------------------------------------------------------- producer
// IIW (plan.iiw == 2): the producer also writes the integral image.  Its
// local integral restarts every epoch (fp32-exact magnitudes), so a second
// set of uint32 accumulators G holds the image's integral at the lane's four
// columns: each row adds the strip-local prefix plus S(r), the row's sum left
// of the strip's halo column (k_ii_rowseg<128, 16>, zero for strip 0), and G
// is stored (16 B per lane, non-temporal) before the row is added -- integral
// row R = the sum of pixel rows < R.  Lanes store the strip's 128 columns
// (the last strip: up to column W); BND: this strip's lane holding W masks
// its pad columns past W to 0.  Rows of steps before the frame (k < 0) get an
// offset past the store resource, rows past H fall outside it.
// RS (plan.rsum, with k_hess_w writing the integral): the producer also
// leaves k_hess_w's row sums half done, in place of k_ii_rowseg's pass over
// the frames.  The ring holds a whole epoch of local-integral rows (NB = P),
// so once per epoch lane j reads the rows around pixel row j at three columns
// from LDS: the strip's first own column (lane 4's), the column after its
// last (lane 36's) and, in the strip that holds a k_hess_w strip's halo
// column X, that column (lane lx's; lx = 4: no X here, 0).  Differences of
// consecutive rows are the pixel row's sums left of those columns; the
// strip's own 128 columns and its columns left of X go as own | left << 16
// into rsl (64 dwords of LDS, lane = row), which the last consumer wave
// stores after the barrier (36 rows, one dword store per epoch).  Nothing is
// added to the steps.  k_rowsum_p0 adds the strips up.
template <int B, bool IIW, bool BND, bool RS>
__device__ __forceinline__ void p0_producer(const uint8_t* __restrict__ frames, int pitch, long long fstride,
                                            const FrameParams& P, int f, int IX0, int niter, uint32_t* Tb,
                                            uint32_t* Tdb, const uint32_t* sg, int32_t* iib, bool last,
                                            int rs_rows, uint32_t* rsl, int lx)
{
    static_assert(!(IIW && RS), "the row sums are prepared for k_hess_w's integral, not for this kernel's own");
    constexpr int NB = 2 * B;                              // ring slots
    static_assert(q0::P % NB == 0, "slot index static within an epoch; Delta read before rewritten");
    static_assert(2 * q0::P <= 64, "an epoch's row sums in one wave load");
    const int lane = (int)lane_id();
    const int xs = 2 * IX0 - 16;
    const int H = P.H;
    const rsrc_t F8 = make_rsrc(frames + (size_t)f * fstride, (long long)H * pitch);
    const int c0 = xs + 4 * lane;
    uint32_t cmask = 0u;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (lane < 40 && c0 + b >= 0 && c0 + b < P.W) cmask |= 0xffu << (8 * b);
    const uint32_t coff = (uint32_t)c0;
    // (IIW) the image's integral at the lane's columns, the store resource /
    // lane offset, the pad masks and the row sums of this epoch and the next
    uint32_t G0 = 0u, G1 = 0u, G2 = 0u, G3 = 0u;
    rsrc_t IR = make_rsrc(iib, 0), SR = make_rsrc(sg, 0);
    uint32_t vst = 0x40000000u, pm1 = ~0u, pm2 = ~0u, pm3 = ~0u, sv_cur = 0u, sv_next = 0u;
    int ip4 = 0;
    if constexpr (IIW) {
        ip4 = P.ip * 4;
        IR = make_rsrc(iib, (long long)P.iH * ip4);
        const int X0 = 2 * IX0;
        const bool own = c0 >= X0 && (last ? c0 <= P.W : c0 < X0 + 128);
        vst = own ? (uint32_t)c0 * 4u : 0x40000000u;
        if constexpr (BND) {
            pm1 = c0 + 1 <= P.W ? ~0u : 0u;
            pm2 = c0 + 2 <= P.W ? ~0u : 0u;
            pm3 = c0 + 3 <= P.W ? ~0u : 0u;
        }
        SR = make_rsrc(sg, (long long)rs_rows * 4);
        // lane j: S of row 2 (-8) + j, the first epoch's rows (negative: past the resource, 0)
        sv_next = __builtin_amdgcn_raw_buffer_load_b32(SR, (uint32_t)(-16 + lane) * 4u, 0, 0);
    }
    (void)vst; (void)pm1; (void)pm2; (void)pm3; (void)sv_cur; (void)ip4; (void)last;
    static_assert(!RS || NB == q0::P, "an epoch's steps all in the ring when its row sums are taken");
    (void)lx; (void)rsl;
    // no row test (k_hess_w's producer): rows outside the frame fall past the
    // buffer, or, for lanes left of the frame (c0 a multiple of 4), into
    // bytes cmask clears
    (void)H;
    auto ldrow = [&](int r) -> uint32_t {
        return __builtin_amdgcn_raw_buffer_load_b32(F8, coff + (uint32_t)(r * pitch), 0, 0);
    };
    uint32_t Ls0 = 0u, Ls1 = 0u, Ls2 = 0u, Ls3 = 0u;
#define FB(x) __float_as_uint((float)(x))
    // (IIW) so: byte offset of integral row 2 k (uniform); s0 / s1: the row
    // sums of rows 2 k, 2 k + 1
    auto scan_write = [&](uint32_t r0, uint32_t r1, uint32_t* Tw, int so, uint32_t s0, uint32_t s1) {
        const uint32_t px0 = r0 & cmask, px1 = r1 & cmask;
        const uint32_t t0 = __builtin_amdgcn_udot4(px0, 0x01010101u, 0u, false);
        const uint32_t t1 = __builtin_amdgcn_udot4(px1, 0x01010101u, 0u, false);
        const uint32_t tp = t0 | (t1 << 16);
        const uint32_t ex = wave_incl_scan(tp) - tp;
        const uint32_t b0 = ex & 0xffffu, b1 = ex >> 16;
        if constexpr (IIW) {
// (the row offset goes into the VGPR offset.  With it as the scalar offset
// (round 5's form, k < 0 rows at 0x40000000), 240 of a 256-frame
// batch's integrals -- every frame from 16 on -- had wrong values in rows
// 11-90 (tools/ii_batch_check.py), which flipped Laplacian signs in config
// #3's frame 127; with the VGPR offset none does.  Cause (round 6, DESIGN §4
// "Buffer range check and a store-data hazard"): not the range check, which
// covers voffset + soffset, but the 16-B store's data VGPRs -- LLVM gives a
// store with an SGPR soffset no wait state before a VALU may rewrite them,
// gfx950 needs one, and the scheduler put the rewrite right behind 48 of
// these 72 stores.  Any offset past the resource is dropped, as the u8 row
// loads rely on)
#define P0_IIST(off)                                                                                             \
    __builtin_amdgcn_raw_buffer_store_b128(v4u32{G0, G1 & pm1, G2 & pm2, G3 & pm3}, IR, vst + (uint32_t)(off), 0, \
                                           p0::IIW_AUX)
            P0_IIST(so);
            const uint32_t e0 = b0 + s0;
            G0 = G0 + e0;
            G1 = __builtin_amdgcn_udot4(px0, 0x00000001u, G1 + e0, false);
            G2 = __builtin_amdgcn_udot4(px0, 0x00000101u, G2 + e0, false);
            G3 = __builtin_amdgcn_udot4(px0, 0x00010101u, G3 + e0, false);
            P0_IIST(so + ip4);
#undef P0_IIST
            const uint32_t e1 = b1 + s1;
            G0 = G0 + e1;
            G1 = __builtin_amdgcn_udot4(px1, 0x00000001u, G1 + e1, false);
            G2 = __builtin_amdgcn_udot4(px1, 0x00000101u, G2 + e1, false);
            G3 = __builtin_amdgcn_udot4(px1, 0x00010101u, G3 + e1, false);
        }
        uint32_t L0[4], L1[4];
        L0[0] = Ls0; L0[1] = Ls1; L0[2] = Ls2; L0[3] = Ls3;
        L1[0] = Ls0 + b0;
        L1[1] = __builtin_amdgcn_udot4(px0, 0x00000001u, Ls1 + b0, false);
        L1[2] = __builtin_amdgcn_udot4(px0, 0x00000101u, Ls2 + b0, false);
        L1[3] = __builtin_amdgcn_udot4(px0, 0x00010101u, Ls3 + b0, false);
        Ls0 = L1[0] + b1;
        Ls1 = __builtin_amdgcn_udot4(px1, 0x00000001u, L1[1] + b1, false);
        Ls2 = __builtin_amdgcn_udot4(px1, 0x00000101u, L1[2] + b1, false);
        Ls3 = __builtin_amdgcn_udot4(px1, 0x00010101u, L1[3] + b1, false);
        *reinterpret_cast<uint4*>(Tw + 4 * lane) = make_uint4(FB(L0[0]), FB(L1[0]), FB(L0[2]), FB(L1[2]));
        *reinterpret_cast<uint4*>(Tw + 2 * q0::NJ + 4 * lane) = make_uint4(FB(L0[1]), FB(L1[1]), FB(L0[3]), FB(L1[3]));
    };
    uint32_t pf0[p0::PD], pf1[p0::PD];
    static_for<p0::PD>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        pf0[K] = ldrow(2 * (K - 8));
        pf1[K] = ldrow(2 * (K - 8) + 1);
    });
    for (int it = 0; it < niter; it++) {
        const int kb = it * q0::P - 8;
        static_for<q0::P>([&](auto kc) {
            constexpr int K = decltype(kc)::value;
            const int k = kb + K;
            const uint32_t r0 = pf0[K % p0::PD], r1 = pf1[K % p0::PD];
            pf0[K % p0::PD] = ldrow(2 * (k + p0::PD));
            pf1[K % p0::PD] = ldrow(2 * (k + p0::PD) + 1);
            if constexpr (K == 0) {
                // the base moves to this step's first row: Delta = L_old there
                // (0 for the first epoch), L restarts at 0
                *reinterpret_cast<uint2*>(Tdb + 2 * lane) = make_uint2(FB(Ls0), FB(Ls2));
                *reinterpret_cast<uint2*>(Tdb + q0::NJ + 2 * lane) = make_uint2(FB(Ls1), FB(Ls3));
                Ls0 = Ls1 = Ls2 = Ls3 = 0u;
                if constexpr (IIW) {
                    // this epoch's row sums; the next epoch's loaded a whole epoch ahead
                    sv_cur = sv_next;
                    sv_next = __builtin_amdgcn_raw_buffer_load_b32(
                        SR, (uint32_t)(2 * (kb + q0::P) + lane) * 4u, 0, 0);
                }
            }
            int so = 0;
            uint32_t s0 = 0u, s1 = 0u;
            if constexpr (IIW) {
                // rows above the frame: past the resource (non-owned lanes'
                // vst + this stays below 2^31: no wrap into range)
                so = k >= 0 ? 2 * k * ip4 : 0x40000000;
                s0 = (uint32_t)__builtin_amdgcn_readlane((int)sv_cur, 2 * K);
                s1 = (uint32_t)__builtin_amdgcn_readlane((int)sv_cur, 2 * K + 1);
            }
            scan_write(r0, r1, Tb + (K % NB) * (4 * q0::NJ), so, s0, s1);
            if constexpr (RS && K == q0::P - 1) {
                // the epoch's 18 steps are all in the ring (NB = P; the next
                // step rewrites slot 0 only after this step's barrier): lane
                // j < 36 takes pixel row 2 kb + j as L at row j + 1 minus L at
                // row j.  Column entry (lane L, first column) is float2 2 L of
                // plane 0: (L at row 2 k, L at row 2 k + 1) in slot k, L = the
                // epoch's rows above summed over the columns left of it.
                // Exact integers below 2^24.
                // As floats: L at row i of the epoch, column entry e, is
                // float (i / 2) 4 NJ + 2 e + (i & 1); row 36 is Ls0 (blended
                // in with bit masks: a select on a loaded value would become
                // a branch, and the loop's row loads would no longer be
                // scheduled ahead across it).
                typedef const float __attribute__((address_space(3))) lds_f;
                const int r0i = lane < 2 * q0::P ? lane : 2 * q0::P - 1, r1i = r0i + 1;
                const bool fin = r1i == 2 * q0::P;
                const int r1c = fin ? r0i : r1i;
                lds_f* F0 = (lds_f*)Tb + (r0i >> 1) * (4 * q0::NJ) + (r0i & 1);
                lds_f* F1 = (lds_f*)Tb + (r1c >> 1) * (4 * q0::NJ) + (r1c & 1);
                const uint32_t fm = fin ? ~0u : 0u;
                auto blend = [&](float v, uint32_t e) {
                    return __uint_as_float((__float_as_uint(v) & ~fm) | (__float_as_uint((float)e) & fm));
                };
                const float la = F0[2 * 8], lb = F0[2 * 72], lxv = F0[4 * lx];
                const float ha = blend(F1[2 * 8], (uint32_t)__builtin_amdgcn_readlane((int)Ls0, 4));
                const float hb = blend(F1[2 * 72], (uint32_t)__builtin_amdgcn_readlane((int)Ls0, 36));
                const float hx = blend(F1[4 * lx], (uint32_t)__builtin_amdgcn_readlane((int)Ls0, lx));
                const float da = ha - la, db = hb - lb, dx = hx - lxv;
                // (to LDS: a store here would sit among the row loads in
                // flight, which the compiler then waits for one by one)
                typedef uint32_t __attribute__((address_space(3))) lds_u;
                ((lds_u*)rsl)[lane] = (uint32_t)(db - da) | ((uint32_t)(dx - da) << 16);
            }
            if constexpr (K % B == B - 1) p0_barrier();
        });
    }
#undef FB
    p0_barrier();                       // the consumers' last interval
}

// --------------------------------------------------------------- consumers
// Scales [S0, S1) of octave 0 (lobe 2s + 3) on one wave: k_hess_q0's step
// for those scales (one read of each column entry they share).
// RSW: this wave also stores the row sums the producer left in rsl at the end
// of its epoch, one barrier earlier (p0_producer), into rsb: the slab of
// this frame and strip, row 2 (18 it - 8) + lane; rows outside [0, H) fall
// outside the resource (a dword store: no store-data hazard).
template <int B, int S0, int S1, int NT, bool RSW>
__device__ __forceinline__ void p0_consumer(float* __restrict__ resp, const FrameParams& P, const OctaveParams& q,
                                            int f, int IX0, int niter, const uint32_t* Tb, const uint32_t* Tdb,
                                            const uint32_t* rsl, uint32_t* rsb)
{
    constexpr int NB = 2 * B;
    constexpr int NSC = S1 - S0;
    constexpr int MASK = ((1 << S1) - 1) & ~((1 << S0) - 1);
    const int lane = (int)lane_id();
    const int ix = IX0 + lane;
    const int sp4 = q.sp * 4;
    rsrc_t RS[NSC];
    uint32_t colb[NSC];
    int32_t roff[NSC];
#pragma unroll
    for (int i = 0; i < NSC; i++) {
        const int s = S0 + i;
        const int b1 = q.b1[s];
        const int nrows = q.sh - 2 * b1 > 0 ? q.sh - 2 * b1 : 0;
        RS[i] = make_rsrc(resp + (size_t)f * P.resp_stride + q.ooff + (size_t)s * q.osize + (size_t)b1 * q.sp,
                          (long long)nrows * sp4);
        colb[i] = (ix >= b1 && ix < q.sw - b1) ? (uint32_t)ix * 4u : 0x40000000u;
        roff[i] = (-8 - q0::fin(s) - b1) * sp4;
    }
    const float rr = INV255 * INV255;
    typedef const volatile v2f32 __attribute__((address_space(3))) lds_v2f;
    typedef const volatile float __attribute__((address_space(3))) lds_f;
    lds_v2f* Tl = (lds_v2f*)Tb + lane;
    lds_f* Tld = (lds_f*)Tdb + lane;
    using q0::md;
    // Accumulator rings, scale pairs packed: scale S0 + 2p in .x, S0 + 2p + 1
    // in .y of ring p.  Scale s keeps sample row k + o in slot md(k + o +
    // fin(s)) (its ring shifted by the row's completion lag), so at step K
    // every scale finalises slot md(K): the finalisation's packed operands
    // are register pairs as they stand (no moves to pack them).
    constexpr int NP = (NSC + 1) / 2;
    v2f32 pxx[NP][q0::P], pyy[NP][q0::P], pxy[NP][q0::P];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int j = 0; j < q0::P; j++) pxx[i][j] = pyy[i][j] = pxy[i][j] = v2f32{0.f, 0.f};
#define AXX(i, o) pxx[(i) >> 1][md((o) + q0::fin(S0 + (i)))][(i) & 1]
#define AYY(i, o) pyy[(i) >> 1][md((o) + q0::fin(S0 + (i)))][(i) & 1]
#define AXY(i, o) pxy[(i) >> 1][md((o) + q0::fin(S0 + (i)))][(i) & 1]
    const rsrc_t QR = make_rsrc(rsb, RSW ? (long long)P.H * 4 : 0);
    (void)QR; (void)rsl;
    p0_barrier();                       // the producer's first interval
    for (int it = 0; it < niter; it++) {
        static_for<q0::P>([&](auto kc) {
            constexpr int K = decltype(kc)::value;
            if constexpr (K == 0) {
                // epoch boundary: correct the accumulators holding terms of
                // the previous epoch (slot md(o) = sample row k + o)
                float d[34];
                static_for<34>([&](auto dcc) {
                    constexpr int dc = decltype(dcc)::value - 16;
                    if constexpr (q0::used(dc, MASK)) d[dc + 16] = Tld[(dc & 1) * q0::NJ + ((16 + dc) >> 1)];
                });
#define DV(dc) d[(dc) + 16]
                const float dC = DV(0) + DV(1);
                static_for<NSC>([&](auto ic) {
                    constexpr int i = decltype(ic)::value, s = S0 + i;
                    constexpr int a = 3 * s + 5, b = -(3 * s + 4), c = s + 2, e = -(s + 1);
                    constexpr int e1 = 2 * s + 3, e2 = -(2 * s + 2), g1 = -(3 * s + 3), g2 = 3 * s + 4;
                    const float QF = __builtin_fmaf(-3.f, DV(c) - DV(e), DV(a) - DV(b));
                    const float QE = DV(e1) - DV(e2);
                    const float QG = (dC - DV(g1)) - DV(g2);
                    static_for<2 * s + 2>([&](auto oc) {
                        constexpr int o = decltype(oc)::value - (s + 1);
                        AXX(i, o) = opqf(AXX(i, o) - QF);
                    });
                    constexpr int h = (s & 1) ? (3 * s + 5) / 2 : (3 * s + 4) / 2;
                    constexpr int g = (s & 1) ? (s + 1) / 2 : (s + 2) / 2;
                    constexpr int hh = (s & 1) ? (3 * s + 3) / 2 : (3 * s + 4) / 2;
                    static_for<2 * h>([&](auto oc) {
                        constexpr int o = decltype(oc)::value - h;
                        if constexpr (o >= g) AYY(i, o) = AYY(i, o) - QE;
                        else if constexpr (o >= -g) AYY(i, o) = __builtin_fmaf(2.f, QE, AYY(i, o));
                        else AYY(i, o) = AYY(i, o) - QE;
                    });
                    static_for<2 * hh>([&](auto oc) {
                        constexpr int o = decltype(oc)::value - hh;
                        if constexpr (o >= 0) AXY(i, o) = AXY(i, o) - QG;
                        else AXY(i, o) = AXY(i, o) + QG;
                    });
                });
#undef DV
            }
            if constexpr (RSW && K == B) {
                // the producer's epoch `it` ended at the barrier before this step
                typedef const volatile uint32_t __attribute__((address_space(3))) lds_u;
                const uint32_t rv = ((lds_u*)rsl)[lane];
                const int row = 2 * (it * q0::P - 8) + lane;
                const uint32_t ro = (lane < 2 * q0::P && row >= 0) ? (uint32_t)row * 4u : 0x40000000u;
                __builtin_amdgcn_raw_buffer_store_b32(rv, QR, ro, 0, 0);
            }
            // the step's row pair at column x0 + dc: slot K % NB, plane dc & 1
            lds_v2f* Ts = Tl + (K % NB) * (2 * q0::NJ);
            v2f32 v[34];
            static_for<34>([&](auto dcc) {
                constexpr int dc = decltype(dcc)::value - 16;
                if constexpr (q0::used(dc, MASK)) v[dc + 16] = Ts[(dc & 1) * q0::NJ + ((16 + dc) >> 1)];
            });
#define V(dc) v[(dc) + 16]
            const v2f32 C = V(0) + V(1);
            static_for<NSC>([&](auto ic) {
                constexpr int i = decltype(ic)::value, s = S0 + i;
                constexpr int a = 3 * s + 5, b = -(3 * s + 4), c = s + 2, e = -(s + 1);
                constexpr int e1 = 2 * s + 3, e2 = -(2 * s + 2), g1 = -(3 * s + 3), g2 = 3 * s + 4;
                const v2f32 m3 = {-3.f, -3.f};
                const v2f32 F = __builtin_elementwise_fma(m3, V(c) - V(e), V(a) - V(b));
                AXX(i, K + s + 1) = opqf(F.x);
                AXX(i, K - s - 1) = opqf(F.y - AXX(i, K - s - 1));
                const v2f32 E = V(e1) - V(e2);
                const v2f32 G = (C - V(g1)) - V(g2);
                if constexpr ((s & 1) == 0) {
                    constexpr int h = (3 * s + 4) / 2, g = (s + 2) / 2;
                    AYY(i, K + h) = opqf(E.x);
                    AYY(i, K + g) = opqf(__builtin_fmaf(-3.f, E.y, AYY(i, K + g)));
                    AYY(i, K - g) = opqf(__builtin_fmaf(3.f, E.x, AYY(i, K - g)));
                    AYY(i, K - h) = opqf(E.y - AYY(i, K - h));
                    AXY(i, K + h) = opqf(G.y);
                    AXY(i, K) = opqf(AXY(i, K) - (G.x + G.y));
                    AXY(i, K - h) = opqf(AXY(i, K - h) + G.x);
                } else {
                    constexpr int h = (3 * s + 5) / 2, g = (s + 1) / 2, hx = (3 * s + 3) / 2;
                    AYY(i, K + h) = opqf(E.y);
                    AYY(i, K + g) = opqf(__builtin_fmaf(-3.f, E.x, AYY(i, K + g)));
                    AYY(i, K - g) = opqf(__builtin_fmaf(3.f, E.y, AYY(i, K - g)));
                    AYY(i, K - h) = opqf(E.x - AYY(i, K - h));
                    AXY(i, K + hx) = opqf(G.x);
                    AXY(i, K) = opqf(AXY(i, K) - (G.x + G.y));
                    AXY(i, K - hx) = opqf(AXY(i, K - hx) + G.y);
                }
            });
#undef V
            // sample rows k - fin(s) are complete (surfd.cu:360-365, 480),
            // scale pairs packed
            static_for<NP>([&](auto pc) {
                constexpr int p = decltype(pc)::value, i0 = 2 * p, i1 = i0 + 1 < NSC ? i0 + 1 : i0;
                const v2f32 dxx = pxx[p][md(K)];
                const v2f32 dyy = pyy[p][md(K)];
                v2f32 dxy = pxy[p][md(K)];
                const v2f32 c06 = {0.6f, 0.6f}, rr2 = {rr, rr}, nrm = {q.norm[S0 + i0], q.norm[S0 + i1]};
                dxy = c06 * dxy;
                const v2f32 pp = dxx * dyy;
                const v2f32 q2 = dxy * dxy;
                const v2f32 hv = (rr2 * (pp - q2)) * nrm;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv.x), RS[i0], colb[i0], (uint32_t)roff[i0],
                                                      NT ? 2 : 0);
                if constexpr (i1 != i0)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv.y), RS[i1], colb[i1],
                                                          (uint32_t)roff[i1], NT ? 2 : 0);
            });
#pragma unroll
            for (int i = 0; i < NSC; i++) roff[i] += sp4;
            if constexpr (K % B == B - 1) p0_barrier();
        });
    }
#undef AXX
#undef AYY
#undef AXY
}

// consumer wave w (1..) of grouping G: its scale range
__host__ __device__ constexpr int p0_lo(int G, int w)
{
    // G = 5: {0} {1} {2} {3} {4};  G = 4: {0} {1} {2,3} {4};  G = 3: {0,1} {2,3} {4};
    // G = 2: {0,1,2} {3,4};  G = 1: {0..4}
    return G == 5 ? w - 1
           : G == 4 ? (w == 1 ? 0 : w == 2 ? 1 : w == 3 ? 2 : 4)
           : G == 3 ? (w == 1 ? 0 : w == 2 ? 2 : 4)
           : G == 2 ? (w == 1 ? 0 : 3)
                    : 0;
}
__host__ __device__ constexpr int p0_hi(int G, int w) { return w == G ? 5 : p0_lo(G, w + 1); }

// Grid: 8 x ceil(nframes / 8) x nstrips workgroups (XCD x takes frames x,
// x + 8, ..., a frame's strips together).  G: consumer waves (scale groups).
// IIW: the producer also writes the integral image into iiw (rowseg: the
// k_ii_rowseg<128, 16> sums of the same frames, rs_rows per strip slab).
// RS: the producer also writes its strips' row sums into rsum (nframes x
// nstrips slabs of rs_rows dwords: own | left << 16 per pixel row) for the xn
// strips of k_hess_w (k_rowsum_p0 turns them into k_hess_w's row sums).
template <int B, int G, int NT, bool IIW, bool RS = false>
__global__ __launch_bounds__(64 * (1 + G)) __attribute__((amdgpu_waves_per_eu(G == 5 ? 5 : G == 4 ? 4 : G == 1 ? 2 : G == 2 ? 3 : 4))) void
k_hess_p0(const uint8_t* __restrict__ frames, int pitch, long long fstride, float* __restrict__ resp, FrameParams P,
          OctaveParams q, int nstrips, int nframes, const uint32_t* __restrict__ rowseg, int32_t* __restrict__ iiw,
          int rs_rows, uint32_t* __restrict__ rsum, int xn)
{
    constexpr int NB = 2 * B;
    __shared__ __attribute__((aligned(16))) uint32_t T[NB][4 * q0::NJ];   // [slot][plane][NJ] float2
    __shared__ __attribute__((aligned(16))) uint32_t TD[2 * q0::NJ];      // Delta: [plane][NJ] float
    // (RS) an epoch's row sums on their way from the producer to the wave that stores them
    uint32_t* rsl = nullptr;
    if constexpr (RS) {
        __shared__ uint32_t RSL[64];
        rsl = RSL;
    }
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7, kb = blockIdx.x >> 3;
    const int f = (kb / nstrips) * 8 + xcd, strip = kb - (kb / nstrips) * nstrips;
    if (f >= nframes) return;
    const int IX0 = strip * 64;
    const int niter = (q.sh + 16 + q0::P - 1) / q0::P;
    if (w == 0) {
        if constexpr (IIW) {
            const bool last = strip == nstrips - 1;
            const uint32_t* sg = rowseg + ((size_t)f * nstrips + strip) * rs_rows;
            int32_t* iib = iiw + (size_t)f * P.ii_stride;
            // the strip whose lane holding column W has pad columns after it
            if (last && (P.W & 3) != 3)
                p0_producer<B, true, true, false>(frames, pitch, fstride, P, f, IX0, niter, &T[0][0], TD, sg, iib,
                                                  last, rs_rows, nullptr, 4);
            else
                p0_producer<B, true, false, false>(frames, pitch, fstride, P, f, IX0, niter, &T[0][0], TD, sg, iib,
                                                   last, rs_rows, nullptr, 4);
        } else if constexpr (RS) {
            // the k_hess_w strip (1 .. xn - 1) whose halo column X lies in
            // this strip's columns [128 strip, + 128), if any: the lane whose
            // first column is X (lane 4's is column 128 strip)
            const int k = (128 * strip + p0::XHALO + p0::XST - 1) / p0::XST;
            const int xo = p0::XST * k - p0::XHALO - 128 * strip;
            const int lx = (k >= 1 && k < xn && xo < 128) ? 4 + (xo >> 2) : 4;
            p0_producer<B, false, false, true>(frames, pitch, fstride, P, f, IX0, niter, &T[0][0], TD, nullptr,
                                               nullptr, false, 0, rsl, lx);
        } else {
            p0_producer<B, false, false, false>(frames, pitch, fstride, P, f, IX0, niter, &T[0][0], TD, nullptr,
                                                nullptr, false, 0, nullptr, 4);
        }
        return;
    }
    static_for<G>([&](auto gc) {
        constexpr int wc = decltype(gc)::value + 1;
        if (w == wc)
            p0_consumer<B, p0_lo(G, wc), p0_hi(G, wc), NT, RS && wc == G>(
                resp, P, q, f, IX0, niter, &T[0][0], TD, rsl,
                RS ? rsum + ((size_t)f * nstrips + strip) * rs_rows : nullptr);
    });
}
