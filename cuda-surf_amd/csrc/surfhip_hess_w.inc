// surfhip_hess_w.inc -- octaves 1..3 of the Hessian in one launch from the
// u8 frame (k_hess_w): a strip's local integral is built ONCE, in LDS, and
// shared by the consumers of three octaves.
//
// Reference: calcHessianMultiConst (surfd.cu:445-481), getHessian
// (surfd.cu:353-366), getSum (surfd.cu:334-343), launched per octave by
// cuCalcHessianMulti (surfd.cu:2829-2894) on the integral image.
//
// Why.  Octave 1 on its own kernel (k_hess_q1) spent 60 % of its VALU
// building a strip-local integral whose halo (2 x 36 columns) costs as much
// as its 256-column core, and octaves 2-3 (k_hess_far) read the whole
// 2.27-GB integral image to write 0.12 GB of responses.  Here a workgroup
// owns one frame's 480-column strip and walks it top to bottom in blocks of 4
// integral rows:
//   * 3 producer waves (256 local-integral columns each, 4 per lane: the
//     strip and octave 3's 144-column halo on both sides) turn the block's u8
//     rows into local integral rows (udot4 byte prefixes, one DPP wave scan
//     per row pair) and write them to one of 5 LDS block buffers, a column's
//     four rows as one 16-B entry (one pad entry per 16 columns keeps the
//     ds_read_b128 of lanes 4 / 8 / 16 columns apart conflict-free);
//   * 6 octave-1 waves (one scale and 64 sample columns each) and 3 + 3
//     octave-2 / octave-3 waves (one scale, 60 / 30 sample columns) read the
//     column entries of their corners and add every corner row's F / E / G
//     term into register accumulators of the sample row it belongs to;
//   * one s_barrier per interval of BPI = 2 blocks (LDS drained, global
//     loads left in flight).  Producer p works on interval-block t - p in
//     interval t (range p's row-prefix carry comes from producer p - 1's
//     same rows, one interval earlier), the consumers on t - 4.
// The local integral L(R, c) = sum of the frame over rows < R and columns
// [cs, c) (cs = the strip's first halo column) differs from the reference's
// integral by a per-row term only, and every getHessian sum has coefficient
// sum 0 along each axis, so the uint32 box sums are the reference's exact
// int32 sums (no sum can wrap); the float finalisation runs the reference's
// ops in its order (surfd.cu:360-365, 480): planes are bit-identical.
//
// Per scale (lobe m = 2K + 1, K = x2, x3 = 2K, x4 = 3K) and sample (x0, y0):
//   F(R) = L(R, x0+3K+2) - L(R, x0-3K-1) - 3 (L(R, x0+K+1) - L(R, x0-K))
//   E(R) = L(R, x0+2K+1) - L(R, x0-2K)
//   G(R) = L(R, x0+3K+1) + L(R, x0-3K) - L(R, x0) - L(R, x0+1)
//   sxx = F(y0+2K+1) - F(y0-2K)
//   syy = E(y0+3K+2) - E(y0-3K-1) - 3 E(y0+K+1) + 3 E(y0-K)
//   sxy = G(y0) + G(y0+1) - G(y0-3K) - G(y0+3K+1)
// The accumulators hold the negated sums; a sample row's first term of each
// sum is an assignment (its first corner row comes first), so no slot is
// ever zeroed.  Octave 1's rings are indexed statically (an iteration of
// U = 20 blocks = the ring length); octaves 2 / 3 (a sample row every 2 / 4
// blocks) shift their rings by one slot per sample row instead.

namespace hw {
constexpr int OCT1_AUX = 0;        // octave-1 response stores' cache policy (2: nt)
constexpr int FAR_AUX = 2;         // octave-2/3 response stores' cache policy (2: nt)
constexpr int IIW_AUX = 2;         // integral-image stores' cache policy (IIW): nt (0: default)
constexpr int ST = 480;            // image columns per strip (30 octave-3 samples)
constexpr int H = 144;             // halo: octave 3's reach (3 x 47 + 2 = 143)
constexpr int NP = 3;              // producer waves, 256 local-integral columns each
constexpr int NCOL = NP * 256;     // 768 >= ST - 16 + 2 x 143 + 1
constexpr int ENT = NCOL + NCOL / 8;       // 16-B entries per block buffer (one pad entry per 8 columns)
constexpr int BPI = 2;             // blocks per barrier interval
constexpr int NLB = 5;             // interval buffers (producer skew 3, consumer lag 4)
constexpr int BLKB = ENT * 16;     // bytes per block
constexpr int BSTR = NLB * BLKB;   // block b of every interval buffer lies at b x BSTR: [BPI][NLB][ENT]
constexpr int LAG = 4;             // consumers work on interval t - LAG in interval t
constexpr int U = 20;              // blocks per octave-1 iteration (= its ring length)
constexpr int PD = 1;              // producer: intervals of u8 rows loaded ahead
constexpr int WAVES = NP + 6 + 3 + 3;
constexpr int THREADS = 64 * WAVES;
static_assert(U % BPI == 0 && (U / BPI) % NLB == 0, "static buffer index in the octave-1 loop");
static_assert(U % 4 == 0 && 4 % BPI == 0, "octave-2/3 periods are whole intervals");
static_assert((U / BPI) % (PD + 1) == 0, "producer unroll divides the interval count");
static_assert(LAG >= NP, "consumers read an interval after its last producer wrote it");
__host__ __device__ constexpr int fdiv(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }
__host__ __device__ constexpr int fmodp(int a, int b) { return a - b * fdiv(a, b); }
// x2 of scale i (0..2) of octave o (1..3) for init_mask_size 9, sampling 2
// (lobes 15/19/23, 31/39/47, 63/79/95)
__host__ __device__ constexpr int kof(int o, int i) { return (4 + i) * (1 << o) - 1; }
// entry of local column dc.  One pad entry per 8 columns: a ds_read_b128 of
// 64 columns 8 apart (octave 1's interleaved halves, octave 2) touches every
// bank once; octave 3 (16 apart) is 2-way
__host__ __device__ constexpr int col(int dc) { return dc + (dc >> 3); }
// a sample's corner rows / columns relative to (y0, x0), in row order:
// the F / E / G term of row offset RO[n] (TY: 0 = F, 1 = E, 2 = G) goes into
// its sum with coefficient CO[n] (negated-sum convention; 0 = assignment)
__host__ __device__ constexpr int ro(int K, int n)
{
    const int t[10] = {-3 * K - 1, -3 * K, -2 * K, -K, 0, 1, K + 1, 2 * K + 1, 3 * K + 1, 3 * K + 2};
    return t[n];
}
__host__ __device__ constexpr int ty(int n)
{
    const int t[10] = {1, 2, 0, 1, 2, 2, 1, 0, 2, 1};
    return t[n];
}
__host__ __device__ constexpr int co(int n)
{
    const int t[10] = {0, 0, 0, -3, -1, -1, 3, -1, 1, -1};
    return t[n];
}
// corner columns: F {-3K-1, -K, K+1, 3K+2}, E {-2K, 2K+1}, G {-3K, 0, 1, 3K+1}
__host__ __device__ constexpr int cof(int K, int i)
{
    const int t[10] = {-3 * K - 1, -K, K + 1, 3 * K + 2, -2 * K, 2 * K + 1, -3 * K, 0, 1, 3 * K + 1};
    return t[i];
}
}  // namespace hw

// LDS ordering: every wave's LDS writes done, then the workgroup barrier.
// Not __syncthreads(): its release fence would also wait for the producers'
// global prefetch loads (vmcnt(0)) at every block.
__device__ __forceinline__ void hw_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ uint32_t opqu(uint32_t x)
{
    asm("" : "+v"(x));
    return x;
}

// (float) of an int32 sum held negated: the reference converts the int sum
// with __int2float_rn, and (float)0 = +0
__device__ __forceinline__ float hw_f(uint32_t neg) { return (float)(int32_t)(0u - neg); }

// the reference's finalisation (surfd.cu:360-365, 480) of negated sums
__device__ __forceinline__ float hw_final(uint32_t nxx, uint32_t nyy, uint32_t nxy, float norm)
{
    const float rr = INV255 * INV255;
    const float dxx = hw_f(nxx);
    const float dyy = hw_f(nyy);
    const float dxy = 0.6f * hw_f(nxy);
    const float pp = dxx * dyy;
    const float q2 = dxy * dxy;
    return (rr * (pp - q2)) * norm;
}

typedef const volatile v4u32 __attribute__((address_space(3))) lds_v4u;

__device__ __forceinline__ v4u32 hw_ld(uint32_t addr)
{
    return *reinterpret_cast<lds_v4u*>((uintptr_t)addr);
}

struct HwStore {
    rsrc_t R;        // plane from its first valid row (b1), exactly the valid rows
    uint32_t colb;   // byte offset of the lane's column (past every buffer if not stored)
    int sp4;
    int b1;
};

__device__ __forceinline__ HwStore hw_store_setup(float* resp, const FrameParams& P, const OctaveParams& q, int f,
                                                  int s, int ix, bool mine)
{
    HwStore st;
    const int b1 = q.b1[s];
    const int nrows = q.sh - 2 * b1 > 0 ? q.sh - 2 * b1 : 0;
    st.sp4 = q.sp * 4;
    st.b1 = b1;
    st.R = make_rsrc(resp + (size_t)f * P.resp_stride + q.ooff + (size_t)(q.init_scale + s) * q.osize +
                         (size_t)b1 * q.sp,
                     (long long)nrows * st.sp4);
    st.colb = (mine && ix >= b1 && ix < q.sw - b1) ? (uint32_t)ix * 4u : 0x40000000u;
    return st;
}

// a row's functional of type T from the block's column entries Q (10 of
// them, hw::cof order), row j of the block
template <int T, int J>
__device__ __forceinline__ uint32_t hw_term(const v4u32 (&Q)[10])
{
    if constexpr (T == 0)
        return (Q[3][J] - Q[0][J]) - mul3(Q[2][J] - Q[1][J]);
    else if constexpr (T == 1)
        return Q[5][J] - Q[4][J];
    else
        return (Q[9][J] + Q[6][J]) - (Q[7][J] + Q[8][J]);
}

template <int CO>
__device__ __forceinline__ uint32_t hw_acc(uint32_t a, uint32_t v)
{
    if constexpr (CO == 0) return opqu(v);
    else if constexpr (CO == 1) return opqu(a + v);
    else if constexpr (CO == -1) return opqu(a - v);
    else if constexpr (CO == 3) return opqu(a + mul3(v));
    else return opqu(a - mul3(v));
}

// which of the 10 column entries a type needs
__host__ __device__ constexpr bool hw_needs(int T, int i)
{
    return T == 0 ? i < 4 : T == 1 ? (i == 4 || i == 5) : i >= 6;
}

// ---------------------------------------------------------------- producer
// Wave p: local columns 256 p + 4 lane + j (j < 4) of every integral row;
// BPI blocks (4 BPI rows) per interval.
// IIW: the producers also write the integral image (plan.iiw).  Producer 0's
// row carries then start from the strip's row sums left of its halo (sg:
// k_ii_rowseg's slab of this frame and strip, zero for strip 0), so L is the
// image's integral itself (the consumers' sums cancel any per-row term, so
// they are unchanged), and each lane stores its four columns of every row as
// one 16-B store when it owns them: the strip's 480 columns (the last strip:
// up to column W).  BND: this wave holds the lane with column W and up to 3
// pad columns past it; that lane's pad values are masked to 0 (pad columns
// stay 0).  Rows past H fall outside the store resource: the row's byte
// offset is part of the VGPR offset, which the range check covers.  (BND is a template
// argument: a per-row branch split the interval's straight-line code into
// basic blocks the scheduler could not interleave.)
template <int PW, bool IIW, bool BND>
__device__ __forceinline__ void hw_producer(const uint8_t* __restrict__ frames, int pitch, long long fstride,
                                            const FrameParams& P, int f, int X0, int nint, uint32_t lds0,
                                            uint32_t* cbuf, const uint32_t* sg, int32_t* iib, bool last, int rs_rows)
{
    constexpr int NR = 4 * hw::BPI;                          // rows per interval
    const int lane = (int)lane_id();
    const int Hh = P.H;
    const rsrc_t F8 = make_rsrc(frames + (size_t)f * fstride, (long long)Hh * pitch);
    const int c0 = X0 - hw::H + 256 * PW + 4 * lane;       // image column of the lane's first pixel
    uint32_t cmask = 0u;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (c0 + b >= 0 && c0 + b < P.W) cmask |= 0xffu << (8 * b);
    const uint32_t coff = (uint32_t)c0;
    // No row test: a row above the frame gives a negative offset (past the
    // buffer as uint32: 0), a row below it an offset past H x pitch (0) --
    // except for lanes left of the frame, whose columns wrap into the
    // previous row, but c0 is a multiple of 4 so those lanes' four bytes are
    // all masked (cmask = 0).  One VALU add per row instead of a compare /
    // select chain.
    (void)Hh;
    auto ldrow = [&](int r) -> uint32_t {
        return __builtin_amdgcn_raw_buffer_load_b32(F8, coff + (uint32_t)(r * pitch), 0, 0);
    };
    // the lane's four entries of a block: 4 lane + j stays inside one
    // 8-column group, so they are consecutive
    const uint32_t ent0 = lds0 + (uint32_t)hw::col(256 * PW + 4 * lane) * 16u;
    uint32_t Lc[4] = {0u, 0u, 0u, 0u};                     // L at the next row, the lane's 4 columns
    uint32_t pf[hw::PD + 1][NR];
    // (IIW) the integral store: resource over the frame's (H + 1) rows; the
    // lane's byte column if it stores all four columns, or the one past W
    rsrc_t IR = make_rsrc(iib, 0);
    rsrc_t SR = make_rsrc(sg, 0);
    uint32_t vst = 0x40000000u;
    int ip4 = 0;
    uint32_t pm[4] = {~0u, ~0u, ~0u, ~0u};                  // (BND) columns <= W
    uint32_t sgv[hw::PD + 1];
    if constexpr (IIW) {
        ip4 = P.ip * 4;
        IR = make_rsrc(iib, (long long)P.iH * ip4);
        const bool own = c0 >= X0 && (last ? c0 <= P.W : c0 < X0 + hw::ST);
        vst = own ? (uint32_t)c0 * 4u : 0x40000000u;
        if constexpr (BND) {
#pragma unroll
            for (int j = 1; j < 4; j++) pm[j] = c0 + j <= P.W ? ~0u : 0u;
        }
        if constexpr (PW == 0) {
            SR = make_rsrc(sg, (long long)rs_rows * 4);
            static_for<hw::PD>([&](auto kc) {
                constexpr int K = decltype(kc)::value;
                sgv[K] = __builtin_amdgcn_raw_buffer_load_b32(SR, (uint32_t)(NR * K + (lane & (NR - 1))) * 4u, 0, 0);
            });
        }
    }
    (void)vst; (void)pm; (void)sgv;
    static_for<hw::PD>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
#pragma unroll
        for (int j = 0; j < NR; j++) pf[K][j] = ldrow(NR * K + j);
    });
    // interval t = d + PW works on interval-block d; PW idle intervals first
    static_for<PW>([&](auto) { hw_barrier(); });
    uint32_t bufoff = 0u;                                    // (d mod NLB) x BLKB
    for (int d0 = 0; d0 < nint; d0 += hw::PD + 1) {
        static_for<hw::PD + 1>([&](auto kc) {
            constexpr int K = decltype(kc)::value;
            const int d = d0 + K;
            // rows of interval d + PD into the slot of interval d - 1
#pragma unroll
            for (int j = 0; j < NR; j++) pf[(K + hw::PD) % (hw::PD + 1)][j] = ldrow(NR * (d + hw::PD) + j);
            if constexpr (IIW && PW == 0)
                sgv[(K + hw::PD) % (hw::PD + 1)] = __builtin_amdgcn_raw_buffer_load_b32(
                    SR, (uint32_t)(NR * (d + hw::PD) + (lane & (NR - 1))) * 4u, 0, 0);
            uint32_t* cb_in = cbuf + ((d & 1) * hw::NP + PW - 1) * NR;
            uint32_t* cb_out = cbuf + ((d & 1) * hw::NP + PW) * NR;
            // the row-pair scans first (they need no carry): one wave scan of
            // both rows' lane totals (16-bit halves: at most 64 x 1020 < 2^16)
            uint32_t px[NR], sc[NR / 2], ex[NR];
#pragma unroll
            for (int j = 0; j < NR; j++) px[j] = pf[K][j] & cmask;
#pragma unroll
            for (int q = 0; q < NR / 2; q++) {
                const uint32_t ta = __builtin_amdgcn_udot4(px[2 * q], 0x01010101u, 0u, false);
                const uint32_t tb = __builtin_amdgcn_udot4(px[2 * q + 1], 0x01010101u, 0u, false);
                const uint32_t tp = ta | (tb << 16);
                sc[q] = wave_incl_scan(tp);
                const uint32_t x = sc[q] - tp;
                ex[2 * q] = x & 0xffffu;
                ex[2 * q + 1] = x >> 16;
            }
            // range carries of the interval's rows (sum of ranges < PW), from producer PW - 1
            uint32_t ci[NR];
#pragma unroll
            for (int j = 0; j < NR; j++) ci[j] = 0u;
            if constexpr (IIW && PW == 0) {
                // the strip's row sums left of its halo (lane j of the load: row j)
#pragma unroll
                for (int j = 0; j < NR; j++) ci[j] = (uint32_t)__builtin_amdgcn_readlane((int)sgv[K], j);
            }
            if constexpr (PW > 0) {
#pragma unroll
                for (int b = 0; b < hw::BPI; b++) {
                    const v4u32 c = hw_ld((uint32_t)(uintptr_t)(cb_in + 4 * b));
                    ci[4 * b] = c.x;
                    ci[4 * b + 1] = c.y;
                    ci[4 * b + 2] = c.z;
                    ci[4 * b + 3] = c.w;
                }
            }
#pragma unroll
            for (int j = 0; j < NR; j++) ex[j] += ci[j];
#pragma unroll
            for (int b = 0; b < hw::BPI; b++) {
                uint32_t L[4][4];                            // [column j][row]
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t p = px[4 * b + r], e = ex[4 * b + r];
#pragma unroll
                    for (int j = 0; j < 4; j++) L[j][r] = Lc[j];
                    if constexpr (IIW) {
                        // integral row R = NR d + 4 b + r, its byte offset in
                        // the VGPR offset: rows R >= iH give vst + R ip4 >= the
                        // resource's iH ip4 bytes and are dropped by the range
                        // check, which sees the VGPR offset (§4 "Buffer range
                        // check"; non-owned lanes: 2^30 + R ip4 < 2^32)
                        const uint32_t ro = vst + (uint32_t)((NR * d + 4 * b + r) * ip4), so = 0u;
                        if constexpr (BND)
                            __builtin_amdgcn_raw_buffer_store_b128(v4u32{Lc[0], Lc[1] & pm[1], Lc[2] & pm[2],
                                                                         Lc[3] & pm[3]}, IR, ro, so, hw::IIW_AUX);
                        else
                            __builtin_amdgcn_raw_buffer_store_b128(v4u32{Lc[0], Lc[1], Lc[2], Lc[3]}, IR, ro, so,
                                                                   hw::IIW_AUX);
                    }
                    Lc[0] = Lc[0] + e;
                    Lc[1] = __builtin_amdgcn_udot4(p, 0x00000001u, Lc[1] + e, false);
                    Lc[2] = __builtin_amdgcn_udot4(p, 0x00000101u, Lc[2] + e, false);
                    Lc[3] = __builtin_amdgcn_udot4(p, 0x00010101u, Lc[3] + e, false);
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                    *reinterpret_cast<volatile v4u32 __attribute__((address_space(3)))*>(
                        (uintptr_t)(ent0 + bufoff + (uint32_t)(b * hw::BSTR) + 16u * j)) =
                        v4u32{L[j][0], L[j][1], L[j][2], L[j][3]};
            }
            if constexpr (PW < hw::NP - 1) {
                // carries into range PW + 1: this range's row totals on top of its carries
                if (lane == 63) {
#pragma unroll
                    for (int b = 0; b < hw::BPI; b++) {
                        const uint32_t ga = sc[2 * b], gb = sc[2 * b + 1];
                        *reinterpret_cast<volatile v4u32 __attribute__((address_space(3)))*>(
                            (uintptr_t)(cb_out + 4 * b)) =
                            v4u32{ci[4 * b] + (ga & 0xffffu), ci[4 * b + 1] + (ga >> 16), ci[4 * b + 2] + (gb & 0xffffu),
                                  ci[4 * b + 3] + (gb >> 16)};
                    }
                }
            }
            bufoff = bufoff + hw::BLKB == hw::BSTR ? 0u : bufoff + hw::BLKB;
            hw_barrier();
        });
    }
    // trailing intervals: LAG + nint barriers in all
    static_for<hw::LAG - PW>([&](auto) { hw_barrier(); });
}

// an empty volatile asm that takes and "redefines" the column entries of term
// type T: code using them stays below the memory operations issued before it
template <typename TC>
__device__ __forceinline__ void hw_pin(v4u32 (&Q)[10])
{
    constexpr int T = TC::value;
#pragma unroll
    for (int i = 0; i < 10; i++)
        if (hw_needs(T, i)) asm volatile("" : "+v"(Q[i]));
}

// ------------------------------------------------------- octave-1 consumer
// One scale (K), 60 sample columns (the strip's even (h = 0) or odd (h = 1)
// ones of 120: 8 columns apart, bank-conflict free), delta 4:
// every block carries the same corner rows; ring slot of sample row iy =
// iy mod U, static inside an iteration of U blocks.
template <int K>
__device__ __forceinline__ void hw_oct1(float* __restrict__ resp, const FrameParams& P, const OctaveParams& q,
                                        int s, int f, int X0, int h, int nblk, uint32_t lds0)
{
    constexpr int D = 4, U = hw::U;
    const int lane = (int)lane_id();
    const int ixl = 2 * lane + h;                             // sample column within the strip
    constexpr int NS = hw::ST / D;
    const int ix = X0 / D + ixl;
    const int cb = hw::H + D * (ixl < NS ? ixl : NS - 1);
    const HwStore st = hw_store_setup(resp, P, q, f, s, ix, ixl < NS);
    const float norm = q.norm[s];
    // two address sets (block 0 / 1 of an interval): ds_read's 16-bit
    // immediate then reaches all NLB buffers
    uint32_t ad[10], ad2[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        ad[i] = lds0 + (uint32_t)hw::col(cb + hw::cof(K, i)) * 16u;
        ad2[i] = ad[i] + (uint32_t)hw::BSTR;
        // opaque: folded into the reads' offsets, ad + BSTR + BO overflows the
        // immediate and every (buffer, column) pair would take a register
        asm volatile("" : "+v"(ad2[i]));
    }
    uint32_t nx[U], ny[U], nz[U];
#pragma unroll
    for (int i = 0; i < U; i++) nx[i] = ny[i] = nz[i] = 0u;
    static_for<hw::LAG>([&](auto) { hw_barrier(); });
    constexpr int FIN = hw::fdiv(3 * K + 2, D);              // block bc finalises sample row bc - FIN
    int roff = (-FIN - st.b1) * st.sp4;
    // Software pipeline over the term types (F, E, G) of consecutive blocks:
    // a type's column entries are read while the previous type's terms are
    // added, and the next block's F entries while this block's G terms are
    // (at most two types, 32 registers, in flight).  The next block may be
    // the next interval's: its interval-block was completed by the
    // producers two barriers ago and is rewritten three intervals later, so
    // reading it before this interval's barrier is safe.  (One type at a
    // time waited an LDS round trip per type: three per block.)
    auto rd = [&](auto jc, auto tc, v4u32 (&Q)[10]) {
        constexpr int JJ = decltype(jc)::value, T = decltype(tc)::value;
        constexpr uint32_t BO = (uint32_t)(((JJ / hw::BPI) % hw::NLB) * hw::BLKB);
        static_assert(BO < 65536u, "ds_read immediate offset");
#pragma unroll
        for (int i = 0; i < 10; i++)
            if (hw_needs(T, i)) Q[i] = hw_ld((JJ % hw::BPI == 0 ? ad[i] : ad2[i]) + BO);
    };
    auto terms = [&](auto jc, auto tc, const v4u32 (&Q)[10]) {
        constexpr int J = decltype(jc)::value, T = decltype(tc)::value;
        static_for<10>([&](auto nc) {
            constexpr int n = decltype(nc)::value;
            if constexpr (hw::ty(n) == T) {
                constexpr int R = hw::ro(K, n), j = hw::fmodp(R, D), sl = hw::fmodp(J - hw::fdiv(R, D), U);
                constexpr int C = hw::co(n);
                const uint32_t v = hw_term<T, j>(Q);
                if constexpr (T == 0) nx[sl] = hw_acc<C>(nx[sl], v);
                else if constexpr (T == 1) ny[sl] = hw_acc<C>(ny[sl], v);
                else nz[sl] = hw_acc<C>(nz[sl], v);
            }
        });
    };
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;
    using T2 = std::integral_constant<int, 2>;
    v4u32 QF[10], QE[10], QG[10];
#pragma unroll
    for (int i = 0; i < 10; i++) QF[i] = QE[i] = QG[i] = v4u32{0u, 0u, 0u, 0u};
    rd(std::integral_constant<int, 0>{}, T0{}, QF);
    for (int b0 = 0; b0 < nblk; b0 += U) {
        static_for<U>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            // (each read group is followed by an empty asm that "rewrites" the
            // entries the next terms use: the terms cannot move above the
            // reads, so the reads go out before the wait for those entries)
            __builtin_amdgcn_sched_barrier(0);
            rd(jc, T1{}, QE);
            hw_pin<T0>(QF);
            terms(jc, T0{}, QF);
            __builtin_amdgcn_sched_barrier(0);
            rd(jc, T2{}, QG);
            hw_pin<T1>(QE);
            terms(jc, T1{}, QE);
            __builtin_amdgcn_sched_barrier(0);
            rd(std::integral_constant<int, (J + 1) % U>{}, T0{}, QF);        // the next block's F entries
            hw_pin<T2>(QG);
            terms(jc, T2{}, QG);
            constexpr int fs = hw::fmodp(J - FIN, U);
            const float hv = hw_final(nx[fs], ny[fs], nz[fs], norm);
            // default cache policy, not nt: the two waves of a scale store
            // alternate columns of the same row within a block of each
            // other, and L2 merges the halves into whole lines (as nt
            // stores, each half went to HBM on its own: 1.57x the plane
            // bytes written, profiles/r03g_pmc.csv)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), st.R, st.colb, (uint32_t)roff, hw::OCT1_AUX);
            roff += st.sp4;
            if constexpr (J % hw::BPI == hw::BPI - 1) hw_barrier();
        });
    }
}

// ---------------------------------------------------- octave 2 / 3 consumer
// One scale (K), delta D = 8 / 16: a sample row every PER = D / 4 blocks;
// block q of a period carries the corner rows R with (R mod D) / 4 = q.  Ring
// index of sample row iy in period m: iy - m - DFIN.  The period loop is
// unrolled KU = 5 times (nblk is a multiple of hw::U = 20, so nblk / PER is a
// multiple of 5): inside the body period M's slots are offset by M (static
// indices) and the ring shifts by KU once per body -- (NR - 1) moves per
// accumulator every 5 periods instead of every period (the per-period shift
// was 48 of the octave-2 wave's 111 VALU instructions per period).
template <int D, int K>
__device__ __forceinline__ void hw_far(float* __restrict__ resp, const FrameParams& P, const OctaveParams& q, int s,
                                       int f, int X0, int nblk, uint32_t lds0)
{
    constexpr int PER = D / 4;
    constexpr int KU = 5;
    static_assert((hw::U / PER) % KU == 0, "unrolled periods divide nblk / PER (nblk: a multiple of hw::U)");
    constexpr int DFIN = -hw::fdiv(3 * K + 2, D), DMAX = -hw::fdiv(-3 * K - 1, D);
    constexpr int NR = DMAX - DFIN + 1;
    constexpr int NRR = NR + KU - 1;                        // slots touched inside one body
    constexpr int NS = hw::ST / D;
    const int lane = (int)lane_id();
    const int ix = X0 / D + lane;
    const int cb = hw::H + D * (lane < NS ? lane : NS - 1);
    const HwStore st = hw_store_setup(resp, P, q, f, s, ix, lane < NS);
    const float norm = q.norm[s];
    uint32_t ad[10];
#pragma unroll
    for (int i = 0; i < 10; i++) ad[i] = lds0 + (uint32_t)hw::col(cb + hw::cof(K, i)) * 16u;
    uint32_t nx[NRR], ny[NRR], nz[NRR];
#pragma unroll
    for (int i = 0; i < NRR; i++) nx[i] = ny[i] = nz[i] = 0u;
    static_for<hw::LAG>([&](auto) { hw_barrier(); });
    constexpr int QF = hw::fmodp(3 * K + 2, D) / 4;         // block of the period that finalises ring slot 0
    int roff = (DFIN - st.b1) * st.sp4;                       // period m finalises sample row m + DFIN
    uint32_t bufoff = 0u;
    for (int m0 = 0; m0 < nblk / PER; m0 += KU) {
        static_for<KU>([&](auto mc) {
            constexpr int M = decltype(mc)::value;
            static_for<PER>([&](auto qc) {
                constexpr int QB = decltype(qc)::value;
                // which column entries this block's corner rows need
                constexpr bool nF = [] {
                    bool r = false;
                    for (int n = 0; n < 10; n++) r = r || (hw::ty(n) == 0 && hw::fmodp(hw::ro(K, n), D) / 4 == QB);
                    return r;
                }();
                constexpr bool nE = [] {
                    bool r = false;
                    for (int n = 0; n < 10; n++) r = r || (hw::ty(n) == 1 && hw::fmodp(hw::ro(K, n), D) / 4 == QB);
                    return r;
                }();
                constexpr bool nG = [] {
                    bool r = false;
                    for (int n = 0; n < 10; n++) r = r || (hw::ty(n) == 2 && hw::fmodp(hw::ro(K, n), D) / 4 == QB);
                    return r;
                }();
                __builtin_amdgcn_sched_barrier(0);
                v4u32 Q[10];
#pragma unroll
                for (int i = 0; i < 10; i++) {
                    const bool need = (nF && hw_needs(0, i)) || (nE && hw_needs(1, i)) || (nG && hw_needs(2, i));
                    if (need) Q[i] = hw_ld(ad[i] + bufoff + (uint32_t)((QB % hw::BPI) * hw::BSTR));
                    else Q[i] = v4u32{0u, 0u, 0u, 0u};
                }
                static_for<10>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    constexpr int R = hw::ro(K, n), rm = hw::fmodp(R, D);
                    if constexpr (rm / 4 == QB) {
                        constexpr int j = rm % 4, ri = -hw::fdiv(R, D) - DFIN;
                        static_assert(ri >= 0 && ri < NR, "ring index");
                        constexpr int T = hw::ty(n), C = hw::co(n);
                        const uint32_t v = hw_term<T, j>(Q);
                        if constexpr (T == 0) nx[ri + M] = hw_acc<C>(nx[ri + M], v);
                        else if constexpr (T == 1) ny[ri + M] = hw_acc<C>(ny[ri + M], v);
                        else nz[ri + M] = hw_acc<C>(nz[ri + M], v);
                    }
                });
                if constexpr (QB == QF) {
                    const float hv = hw_final(nx[M], ny[M], nz[M], norm);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), st.R, st.colb, (uint32_t)roff, hw::FAR_AUX);
                    roff += st.sp4;
                }
                if constexpr (QB % hw::BPI == hw::BPI - 1) {
                    bufoff = bufoff + hw::BLKB == hw::BSTR ? 0u : bufoff + hw::BLKB;
                    hw_barrier();
                }
            });
        });
        // the rows still in flight move down by KU (slots past them are
        // assigned by their first corner row before they are read)
#pragma unroll
        for (int i = 0; i + 1 < NR; i++) {
            nx[i] = nx[i + KU];
            ny[i] = ny[i + KU];
            nz[i] = nz[i + KU];
        }
    }
}

// NO: octaves handled (2: octaves 1-2, 3: octaves 1-3).  Grid: 8 x
// ceil(nframes / 8) x nstrips workgroups, XCD x taking frames x, x + 8, ...
// (a frame's strips share halo columns in that XCD's L2).  nblk: blocks of 4
// integral rows, a multiple of hw::U covering every row a valid sample reads.
template <int NO, bool IIW>
__global__ __launch_bounds__(hw::THREADS) void k_hess_w(const uint8_t* __restrict__ frames, int pitch,
                                                         long long fstride, float* __restrict__ resp, FrameParams P,
                                                         OctaveParams o1, OctaveParams o2, OctaveParams o3,
                                                         int nstrips, int nframes, int nblk,
                                                         const uint32_t* __restrict__ rowseg,
                                                         int32_t* __restrict__ iiw, int rs_rows)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[hw::BPI * hw::BSTR];
    __shared__ __attribute__((aligned(16))) uint32_t cbuf[2 * hw::NP * 4 * hw::BPI];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7, kb = blockIdx.x >> 3;
    const int f = (kb / nstrips) * 8 + xcd, strip = kb - (kb / nstrips) * nstrips;
    if (f >= nframes) return;
    const int X0 = strip * hw::ST;
    const uint32_t l0 = (uint32_t)(uintptr_t)lds;
    // (IIW) this frame's integral image and strip's row-sum slab
    const uint32_t* sg = IIW ? rowseg + ((size_t)f * nstrips + strip) * rs_rows : nullptr;
    int32_t* iib = IIW ? iiw + (size_t)f * P.ii_stride : nullptr;
    const bool last = strip == nstrips - 1;
    // (IIW) the producer wave holding column W, when pad columns follow it in its lane
    const int pbnd = (IIW && last && (P.W & 3) != 3) ? (P.W - X0 + hw::H) / 256 : -1;
#define HW_PROD(PW)                                                                                              \
    if (IIW && pbnd == PW)                                                                                       \
        hw_producer<PW, IIW, true>(frames, pitch, fstride, P, f, X0, nblk / hw::BPI, l0, cbuf, sg, iib, last, rs_rows); \
    else                                                                                                         \
        hw_producer<PW, IIW, false>(frames, pitch, fstride, P, f, X0, nblk / hw::BPI, l0, cbuf, sg, iib, last, rs_rows);
    switch (w) {
        case 0: HW_PROD(0) break;
        case 1: HW_PROD(1) break;
        case 2: HW_PROD(2) break;
#undef HW_PROD
        case 3: case 4: hw_oct1<hw::kof(1, 0)>(resp, P, o1, 0, f, X0, w - 3, nblk, l0); break;
        case 5: case 6: hw_oct1<hw::kof(1, 1)>(resp, P, o1, 1, f, X0, w - 5, nblk, l0); break;
        case 7: case 8: hw_oct1<hw::kof(1, 2)>(resp, P, o1, 2, f, X0, w - 7, nblk, l0); break;
        case 9: hw_far<8, hw::kof(2, 0)>(resp, P, o2, 0, f, X0, nblk, l0); break;
        case 10: hw_far<8, hw::kof(2, 1)>(resp, P, o2, 1, f, X0, nblk, l0); break;
        case 11: hw_far<8, hw::kof(2, 2)>(resp, P, o2, 2, f, X0, nblk, l0); break;
        default:
            if constexpr (NO >= 3) {
                if (w == 12) hw_far<16, hw::kof(3, 0)>(resp, P, o3, 0, f, X0, nblk, l0);
                else if (w == 13) hw_far<16, hw::kof(3, 1)>(resp, P, o3, 1, f, X0, nblk, l0);
                else hw_far<16, hw::kof(3, 2)>(resp, P, o3, 2, f, X0, nblk, l0);
            } else {
                for (int t = 0; t < hw::LAG + nblk / hw::BPI; t++) hw_barrier();
            }
            break;
    }
}
