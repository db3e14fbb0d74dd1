// surfhip_desc_u2.inc -- upright 4x4-cell descriptor, LDS-DMA row ring
// (k_describe_u2, the default for upright wsz-4 descriptors).
//
// Reference: the upright branch of describe (surfd.cu:1566-1615),
// addUprightSample (surfd.cu:1288-1317), placeInIndex (surfd.cu:1199-1271),
// normalize (surfd.cu:2447-2493); launched by cuDescribe (surfd.cu:3251).
//
// Same geometry, sample set and float operations per sample as k_describe_ur
// (one wave per keypoint, lane = grid column, grid rows walked in order; two
// half-waves take alternate rows when the grid is <= 32 columns wide), with
// what round 3's measurements put the time in restructured:
//  * Rows (step <= 3, ~85 % of keypoints): each wave step's integral-row
//    spans go global -> LDS by buffer_load ... lds (LDS-DMA, no VGPR staging,
//    no ds_write) into a RING-slot ring (4), issued RING - 2 steps
//    before they are read and retired by a counted vmcnt, so a step is one
//    LDS read burst, not a write-wait-read round trip through registers.
//  * Keypoints come from a flattened schedule (k_worklist) through a queue
//    atomic and one 16-B load, both issued a keypoint ahead.
//  * Haar responses factored per integral row: with H(row) = II(row, c+s+1)
//    - II(row, c-s) and V(row) = II(row, c) + II(row, c+1) - II(row, c-s) -
//    II(row, c+s+1), haarY = H(r+1) - H(r-s) - H(r+s+1) + H(r) and haarX =
//    V(r-s) - V(r+s+1) (exact in uint32, the reference's int sums); rows r-s
//    and r+s+1 are rows of grid rows t-2 / t+2 (s = 2 step or 2 step - 1), so
//    each row's H / V is computed once and used by three samples.
//  * Bins accumulate with packed FMAs; after the rows the two half-waves fold
//    by one permlane32 swap and the cross-lane column sums read one row of
//    (accumulators, cfrac) per lane, runs found by ballots (no LDS tables);
//    the normalisation tree runs on permlane swaps and DPP row shifts.
// Wider spans (sparse rows) read their columns straight from memory with the
// +-2-lane columns by DPP wave shifts; "exact half-way" scales (s = 2 step +
// 1) take the 12-corner gathers.  Descriptor values agree with the oracle to
// float rounding of the summation order (<= 1e-6 relative, inside the 1e-4
// tolerance); deterministic (no atomics, fixed orders).

namespace du2 {
constexpr int DMA_AUX = 0;                  // the ring DMAs' cache-policy bits
// LDS-DMA ring slots: a step's DMA is issued RING - 2 steps before its rows
// are read.  Measured (kernel trace, one box): 4 slots 2.52 ms, 6 slots 3.24,
// 8 slots 3.33 -- the LDS of the deeper rings costs workgroups per CU (4 / 3
// / 2) and the extra steps in flight do not buy it back.
constexpr int RING = 4;
static_assert(RING >= 4 && RING <= 8 && RING % 2 == 0, "ring: 4, 6 or 8 slots");
// Widest span (16-B chunks) that takes the ring.  64: spans of 33-64 chunks
// (grid steps >= 4) take it too, with 256-word slot rows, so only one row set
// (single mode) fits a slot and they run single even when side <= 32.
// Measured slower than the sparse path (describe 2.20-2.23 vs 2.08-2.11 ms,
// profiles/r04l_*), hence 32
constexpr int SEGW = 32;
constexpr int SLOT = 128;                   // 16-B chunks per step: <= 2 x 64-lane DMA instructions
constexpr int SLOTW = SLOT * 4;             // words per slot
}  // namespace du2

typedef float du_v4f __attribute__((ext_vector_type(4)));

// one grid row's factored Haar terms: H and V of its integral rows r, r + 1
struct DuHV {
    uint32_t h0, h1, v0, v1;
};

__device__ __forceinline__ DuHV du_hv(uint32_t xl0, uint32_t x20, uint32_t x30, uint32_t xr0, uint32_t xl1,
                                      uint32_t x21, uint32_t x31, uint32_t xr1)
{
    return DuHV{xr0 - xl0, xr1 - xl1, (x20 + x30) - (xl0 + xr0), (x21 + x31) - (xl1 + xr1)};
}

// float a + (value of lane i + k) for the tree steps of normalize (lanes < k
// carry the tree; others get garbage, never read)
template <int K>
__device__ __forceinline__ float du_tree_step(float a)
{
    if constexpr (K == 32 || K == 16) {
        const uint32_t u = __float_as_uint(a);
        auto r = K == 32 ? __builtin_amdgcn_permlane32_swap(u, u, false, false)
                         : __builtin_amdgcn_permlane16_swap(u, u, false, false);
        // one output holds the lower half / even rows, the other the upper /
        // odd: their sum is a[i] + a[i + K] in the low lanes (float add commutes)
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else {
        return a + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x100 + K, 0xf, 0xf, false));
    }
}

// Accumulator pairs: sample value S[i] of haar_bins' order (4 bins: dx,
// dx-, dy, dy-; 8 bins: dx, dx|dy<0, |dx|, |dx||dy<0, dy, dy|dx<0, |dy|,
// |dy||dx<0) is component du_comp(i) of pair du_pair(i) -- the pairs the
// sample forms naturally ({dx, dy}, ...), so no register moves pack them.
template <int NS>
__device__ __forceinline__ float du_pick(const v2f32 (&a)[NS / 2], int i)
{
    if constexpr (NS == 4) {
        // pairs {S0, S2}, {S1, S3}
        const v2f32 p = a[i & 1];
        return (i >> 1) ? p.y : p.x;
    } else {
        // pairs {S0, S4}, {S2, S6}, {S1, S5}, {S3, S7}
        const int k = (i & 1) ? 2 + ((i >> 1) & 1) : ((i >> 1) & 1);
        const v2f32 p = a[k];
        return (i >> 2) ? p.y : p.x;
    }
}

template <bool EXT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(EXT ? 3 : 4))) void k_describe_u2(const int32_t* __restrict__ ii, FrameParams P,
                                                     const float4* __restrict__ work, int max_pts,
                                                     const int* __restrict__ offsets, int nframes,
                                                     float* __restrict__ desc, int* __restrict__ queue,
                                                     surfhip_point* __restrict__ pts, int trace)
{
    constexpr int WSZ = 4;
    constexpr int NB = EXT ? 8 : 4;                       // bins per cell
    constexpr int NF = WSZ * WSZ * NB;
    constexpr int NS = NB;                                // per-sample values (haar_bins)
    constexpr int CFI = WSZ * NB;                         // reduction row: bins of 4 cell rows, then cfrac
    constexpr int RW = (CFI + 1 + 3) & ~3;                // (16-B rows: a cell row's bins are one ds_read_b128)
    // The ring's four slots are four separate arrays: the compiler's LDS-DMA
    // tracking then sees that a step's reads (one slot) and its DMAs in
    // flight (other slots) do not alias, and leaves the counted vmcnt waits
    // alone (one array with a run-time offset made it wait for every DMA
    // before every read).  After the rows they hold the reduction rows, 16
    // lanes per slot.
    constexpr int SW = du2::SLOTW > 16 * RW ? du2::SLOTW : 16 * RW;
    constexpr int RING = EXT ? 4 : du2::RING;             // (128-D: wider reduction rows, 4 slots keep 3 workgroups a CU)
    __shared__ __attribute__((aligned(16))) uint32_t s_sl0[4][SW];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl1[4][SW];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl2[4][SW];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl3[4][SW];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl4[RING > 4 ? 4 : 1][RING > 4 ? SW : 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl5[RING > 4 ? 4 : 1][RING > 4 ? SW : 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl6[RING > 6 ? 4 : 1][RING > 6 ? SW : 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_sl7[RING > 6 ? 4 : 1][RING > 6 ? SW : 4];
    __shared__ float4 s_wr[4][64];                        // per grid row: weights of cell rows 0..3
    __shared__ float s_rp[4][64];                         // per grid row: rpos^2
    // Gaussian weights premultiplied by 1/255 (k_describe_ur, same rounding)
    __shared__ float s_lut[40];
    if (threadIdx.x < 40) s_lut[threadIdx.x] = c_tab.lut2[threadIdx.x] * INV255;
    __syncthreads();
    const int lane = (int)lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total = offsets[nframes];
    const float fw = (float)WSZ;
    const float wofs = (float)WSZ * 0.5f - 0.5f;
    KpQueue kq(total, queue, w);
    const int gend = kq.gend;
    typedef const uint32_t __attribute__((address_space(3))) lu32;
    typedef void __attribute__((address_space(3))) lv;
    uint32_t* const slots[8] = {s_sl0[w], s_sl1[w], s_sl2[w], s_sl3[w],
                                RING > 4 ? s_sl4[w] : nullptr, RING > 4 ? s_sl5[w] : nullptr,
                                RING > 6 ? s_sl6[w] : nullptr, RING > 6 ? s_sl7[w] : nullptr};
    const uint32_t lds_sl[4] = {(uint32_t)(size_t)(lu32*)s_sl0[w], (uint32_t)(size_t)(lu32*)s_sl1[w],
                                (uint32_t)(size_t)(lu32*)s_sl2[w], (uint32_t)(size_t)(lu32*)s_sl3[w]};
    // ---- the keypoint pipeline: a keypoint is its queue atomic and one
    // 16-B load of the flattened schedule (k_worklist).  Both run ahead --
    // while keypoint k is described, the atomic for k + 2 and the entry of
    // k + 1 are in flight -- so no keypoint starts on an exposed memory
    // latency.  The entry is a vector load (lanes 0..3): a scalar load
    // would be waited for by the first LDS wait.
    constexpr int EB = kWorkF4 * 16;                      // bytes per entry
    const rsrc_t wrs = make_rsrc(work, (long long)total * EB);
    auto ld_w = [&](int g) -> float {
        // (lanes past the entry's words read the next entry, or 0 past the last)
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, g * EB + (lane & 15) * 4, 0, 0));
    };
    // entry k + 1 is read into scalars at the end of keypoint k, before its
    // descriptor stores: a read at the top of the loop would wait for them
    int gc = kq.grab(lane);
    float pv = 0.f;
    if (gc < gend) pv = ld_w(gc);
    int g1 = kq.grab(lane);
    // the entry's window geometry (k_worklist): {dx0, dy0, spacing, f}, {ix,
    // iy, step | hs << 10 | iradius << 22, f * max_pts + kp}, {getTrace's
    // x0 | y0 << 16, temp (trace), 1 / spacing}
    auto entry = [&](int k) { return __builtin_amdgcn_readlane(__float_as_int(pv), k); };
    float ndx = __int_as_float(entry(0)), ndy = __int_as_float(entry(1)), nsp = __int_as_float(entry(2));
    int nf = entry(3), nix = entry(4), niy = entry(5), npk = entry(6), nidx = entry(7);
    // (the trace words stay in a VGPR, read at their use: SGPRs are full)
    float ptr = pv;
    float nrs = __int_as_float(entry(10));
    while (gc < gend) {
        // the lane index again, opaque (volatile asm): every lane-derived
        // value is recomputed per keypoint instead of hoisted out of the
        // loop, where it held a register across the whole body (spills)
        int lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        const int idx = nidx;                           // f * max_pts + kp
        const int f = nf;
        const float pte = ptr;
        const float dx0 = ndx, dy0 = ndy, spacing = nsp, rsp = nrs;
        const int ix = nix, iy = niy;
        const int step = npk & 1023, hs = (npk >> 10) & 4095, iradius = npk >> 22;
        if (g1 < gend) pv = ld_w(g1);
        const int a2 = kq.issue(lane);
        const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
        const __amdgpu_buffer_rsrc_t rsrc = frame_rsrc(I, P.ii_stride * 4);
        const int rlim = P.iH - 1 - hs, clim = P.W - hs;
        const int side = 2 * iradius + 1;
        // ---- grid row t = lane: exact row geometry (surfd.cu:1290-1292)
        const int sit = lane - iradius;
        // (div_by: the IEEE quotient from the entry's 1 / spacing, as
        // k_describe's upright grid: the same bits, 3 instructions instead of
        // the division's ~10 -- describe -0.4 %, DESIGN 6)
        const float rpos_t = div_by((float)(step * sit) - dy0, spacing, rsp);
        const float rx_t = rpos_t + wofs;
        const int r_t = iy + sit * step;
        const bool rvalid = lane < side && rx_t > -1.f && rx_t < fw && r_t >= 1 + hs && r_t < rlim;
        {
            const int ri_t = f2i_rz(rx_t >= 0.f ? rx_t : rx_t - 1.f);
            const float rf_t = rx_t - (float)ri_t, w0_t = 1.f - rf_t;
            s_rp[w][lane] = rpos_t * rpos_t;
            // placeInIndex's row weights (surfd.cu:1199-1271): 1 - rfrac for
            // cell row ri, rfrac for ri + 1
            s_wr[w][lane] = make_float4(ri_t == 0 ? w0_t : (ri_t == -1 ? rf_t : 0.f),
                                        ri_t == 1 ? w0_t : (ri_t == 0 ? rf_t : 0.f),
                                        ri_t == 2 ? w0_t : (ri_t == 1 ? rf_t : 0.f),
                                        ri_t == 3 ? w0_t : (ri_t == 2 ? rf_t : 0.f));
        }
        // ---- grid column of this lane (dual: two half-waves of 32 lanes walk
        // alternate grid rows)
        const int hmode = hs - 2 * step;          // 0 or -1: rows and columns share integral pairs
        const bool share = hmode == 0 || hmode == -1;
        // the span of integral columns a grid row's samples read, as 16-B
        // chunks from column cs
        const int cs = (ix + (-2 - iradius) * step) & ~3;
        const int W4 = (ix + (side + 1 - iradius) * step + 2 - cs + 3) >> 2;
        const bool wide64 = W4 > 32;
        const bool dual = side <= 32 && !(wide64 && W4 <= du2::SEGW);
        const int j = dual ? (lane & 31) : lane;
        const int h = dual ? (lane >> 5) : 0;
        const int sj = j - iradius;
        const float cpos = div_by((float)(step * sj) - dx0, spacing, rsp);
        const float cx = cpos + wofs;
        const int c = ix + sj * step;
        const bool col_on = j < side && cx > -1.f && cx < fw && c >= 1 + hs && c < clim;
        const int ci = f2i_rz(cx >= 0.f ? cx : cx - 1.f);
        const float cfrac = cx - (float)ci;
        const float cp2 = cpos * cpos;
        const int ip4 = P.ip * 4;
        wave_sync();
        v2f32 acc[WSZ][NS / 2];
#pragma unroll
        for (int R = 0; R < WSZ; R++)
#pragma unroll
            for (int s = 0; s < NS / 2; s++) acc[R][s] = v2f32{0.f, 0.f};
        // the valid grid rows form one contiguous run [t0, t0 + nv); half h
        // takes rows t0 + h, t0 + h + 2, ...
        const unsigned long long vm = __ballot(rvalid);
        const int t0 = vm ? __builtin_ctzll(vm) : 0, nv = __builtin_popcountll(vm);
        // one sample of grid row t from its two Haar responses; `ok` false
        // (column off, or a row past this half's run): contributes 0 (the
        // row's table entries are read unconditionally, ahead of the Haar
        // terms, so a step waits on LDS twice, not four times)
        // the sample's Gaussian weight: the LUT read is unconditional (index
        // 0 for an off sample), then selected -- a load under the condition
        // would become a branch; a zero weight for an off sample (its Haar
        // inputs may be garbage, never inf / NaN)
        auto lut_w = [&](float rp, bool ok) -> float {
            const int li = ok ? f2i_rz(rp + cp2) : 0;      // valid samples index < 40
            const float lw = s_lut[li];
            return ok ? lw : 0.f;
        };
        auto add_sample_w = [&](int32_t wav1, int32_t wav2, float wgt, float4 wr) {
            // {dx, dy} = weight * {haarX, haarY} (one packed multiply)
            const v2f32 d = v2f32{(float)wav2, (float)wav1} * wgt;
            // the sample's values as natural register pairs (du_pair order)
            v2f32 Pv[NS / 2];
            if constexpr (NS == 4) {
                Pv[0] = d;                                              // {dx, dy}
                Pv[1] = v2f32{fminf(d.x, 0.f), fminf(d.y, 0.f)};        // negative parts
            } else {
                const v2f32 a = v2f32{fabsf(d.x), fabsf(d.y)};
                Pv[0] = d;                                              // {dx, dy}
                Pv[1] = a;                                              // {|dx|, |dy|}
                Pv[2] = v2f32{d.y < 0.f ? d.x : 0.f, d.x < 0.f ? d.y : 0.f};
                Pv[3] = v2f32{d.y < 0.f ? a.x : 0.f, d.x < 0.f ? a.y : 0.f};
            }
            const float wrr[WSZ] = {wr.x, wr.y, wr.z, wr.w};
#pragma unroll
            for (int R = 0; R < WSZ; R++) {
                const v2f32 wv = {wrr[R], wrr[R]};
#pragma unroll
                for (int k = 0; k < NS / 2; k++) acc[R][k] = __builtin_elementwise_fma(Pv[k], wv, acc[R][k]);
            }
        };
        auto add_sample = [&](int32_t wav1, int32_t wav2, float rp, float4 wr, bool ok) {
            add_sample_w(wav1, wav2, lut_w(rp, ok), wr);
        };
        // sample of the middle row set Y from the row sets X (t - 2), Y (t),
        // Z (t + 2): rows r - s / r + s + 1 are rows r / r + 1 of X / Z (A:
        // s = 2 step) or r + 1 / r (B: s = 2 step - 1)
        auto wavs = [&](auto AC, const DuHV& X, const DuHV& Y, const DuHV& Z, int32_t& wav1, int32_t& wav2) {
            constexpr bool A = decltype(AC)::value;
            const uint32_t ht = A ? X.h0 : X.h1, hb = A ? Z.h1 : Z.h0;
            const uint32_t vt = A ? X.v0 : X.v1, vb = A ? Z.v1 : Z.v0;
            wav1 = (int32_t)((Y.h1 - ht) - (hb - Y.h0));
            wav2 = (int32_t)(vt - vb);
        };
        auto sample_hv = [&](auto AC, const DuHV& X, const DuHV& Y, const DuHV& Z, float rp, float4 wr, bool ok) {
            int32_t wav1, wav2;
            wavs(AC, X, Y, Z, wav1, wav2);
            add_sample(wav1, wav2, rp, wr, ok);
        };
        // a slot holds 2 G integral rows at a fixed stride of RSW words (64
        // or 128: W4 <= 16 or 32), so every read offset but the lane's own
        // column is a compile-time constant
        // (W4 <= 32: any step <= 3; W4 33..64: single mode, see above)
        const bool seg = share && W4 <= du2::SEGW && (wide64 || step <= 3);
        if (seg) {
            // ---- LDS-DMA ring.  Step s (grid rows t0 + pb + 2 s (+ 1 for
            // the second half)) lands in slot (s + 1) & 3 (four separate
            // arrays, see above): lane k of DMA instruction i loads chunk kk =
            // k + 64 i = integral row rr = kk / (RSW / 4) (2 g + e: half g,
            // row r + e), chunk q of the span starting at column cs, to byte
            // 16 kk of the slot (LDS-DMA destinations are lane-linear); rows
            // past the span's chunks and lanes past 2 G rows load nothing (OOB).
            // The step loop is unrolled by the ring's 4 slots: no branches, 1-2
            // DMAs, 4 paired LDS reads and the rows' 2 table reads a step.
            const int xo = (j < side) ? c - cs : 2 * hs;      // the lane's column in the span
            // (G, the row sets a step holds, is a template argument here: with
            // a run-time DMA count per step the compiler split every step into
            // blocks and moved the steps' arithmetic out of them)
            auto rows_dma = [&](auto AC, auto RSC, auto GC) {
                constexpr int RSW = decltype(RSC)::value;       // words per slot row
                constexpr int GG = decltype(GC)::value;         // 2: dual (two half-waves), 1: single
                constexpr bool DU = GG == 2;
                constexpr int cpr = RSW / 4;                    // chunks per slot row
                constexpr int nd = (2 * GG * cpr + 63) / 64;    // DMA instructions per step (1 or 2)
                int ck[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int kk = lane + 64 * i;
                    const int rr = kk / cpr, q = kk - rr * cpr;
                    // kOOB + any step offset stays past the buffer
                    ck[i] = (rr < 2 * GG && q < W4)
                                ? ((iy + (t0 + (rr >> 1) - iradius) * step + (rr & 1)) * P.ip + cs + 4 * q) * 4
                                : (int)kOOB;
                }
                // the lane's words in a slot: half h's rows r (+0) and r + 1
                // (+RSW) at columns c - s, c, c + 1, c + s + 1
                const int b2 = h * 2 * RSW + xo;
                const int bl = b2 - hs, br = b2 + hs + 1;
                for (int ph = 0; ph < (DU ? 1 : 2); ph++) {
                    const int hh = DU ? h : ph;
                    const int pb = DU ? 0 : ph;
                    const int nstep = max(nv - hh + 1, 0) >> 1;
                    const int nmax = DU ? max(nv + 1, 0) >> 1 : max(nv - ph + 1, 0) >> 1;
                    if (nmax == 0) continue;
                    const int dstep = 2 * step * ip4;           // bytes per step (two grid rows down)
                    const int o0 = ck[0] + (pb - 2) * step * ip4, o1 = ck[1] + (pb - 2) * step * ip4;
                    const bool a0 = ck[0] != (int)kOOB, a1 = ck[1] != (int)kOOB;
                    // step s's DMAs into slot (s + 1) & 3 (static SL)
                    auto dma = [&](auto SLC, int s) {
                        uint32_t* const slot = slots[decltype(SLC)::value];
                        const int d = (s + 1) * dstep;
                        // lanes past the span's chunks are masked off, not sent
                        // out of bounds (lane 0 / 64 always load: no DMA is skipped,
                        // so the counted vmcnt waits hold)
                        if (a0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lv*)slot, 16, o0 + d, 0, 0, du2::DMA_AUX);
                        if constexpr (nd == 2)
                            if (a1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lv*)(slot + 256), 16, o1 + d, 0, 0, du2::DMA_AUX);
                    };
                    auto hv = [&](auto SLC) -> DuHV {
                        lu32* const b = (lu32*)slots[decltype(SLC)::value];
                        return du_hv(b[bl], b[b2], b[b2 + 1], b[br], b[bl + RSW], b[b2 + RSW], b[b2 + RSW + 1],
                                     b[br + RSW]);
                    };
                    auto wait_dma = [&]() {
                        // step n + 1's DMAs: the RING - 2 steps issued after them may be in flight
                        constexpr int IF = RING - 2;
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(nd * IF) : "memory");
                    };
                    // the previous keypoint's reduction rows (and the previous
                    // phase's slots) are read before the ring is refilled
                    // (draining only the LDS reads at phase 0 -- the previous
                    // keypoint's DMAs landed before its reduction -- measured
                    // neutral, DESIGN 6)
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    static_for<RING>([&](auto IC) { dma(IntC<decltype(IC)::value>{}, decltype(IC)::value - 1); });
                    wait_dma();
                    DuHV A = hv(IntC<0>{}), B = hv(IntC<1>{});
                    const int tb = t0 + hh;
                    // step n = n4 + U: DMA of step n + RING - 1 (slot U), table
                    // row tb + 2 n, row set of step n + 1 (slot (U + 2) % RING),
                    // sample n from the sets of steps n - 1 (X), n (Y), n + 1
                    // (Z).  X's terms are taken before Z is read into X's
                    // registers: two row sets rotate, period 2.
                    // rp of the step's row comes from the previous step, so its
                    // LUT read goes out with the row's other table read, before
                    // the DMA wait, and overlaps the slot reads (one LDS round
                    // trip a step, not two)
                    float rpn = s_rp[w][tb];
                    auto stp = [&](auto UC, int n4, DuHV& XZ, const DuHV& Y) {
                        constexpr int U = decltype(UC)::value;
                        // steps do not interleave (the scheduler would hoist the
                        // next steps' reads and cost a wave per SIMD in VGPRs)
                        __builtin_amdgcn_sched_barrier(0);
                        // WAR: this DMA refills the slot whose row set was read
                        // two steps ago; those reads must have retired first.
                        // Nothing else orders them (the compiler may leave a
                        // read's wait until its value's first use, steps later,
                        // while the DMA lands in LDS on its own path): the
                        // missing wait showed as rare wrong descriptors that
                        // changed from run to run (tools/desc_determinism.py).
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        dma(IntC<U>{}, n4 + U + RING - 1);
                        const int t = tb + 2 * (n4 + U);
                        const bool ok = col_on && n4 + U < nstep;
                        // (array-indexed, not a pointer induction: the compiler
                        // must see these are not the DMA's target)
                        const float wgt = lut_w(rpn, ok);
                        const float4 wr = s_wr[w][t];
                        rpn = s_rp[w][t + 2];
                        constexpr bool AM = decltype(AC)::value;
                        const uint32_t ht = AM ? XZ.h0 : XZ.h1, vt = AM ? XZ.v0 : XZ.v1;
                        const uint32_t pre = Y.h1 - ht;
                        wait_dma();
                        XZ = hv(IntC<(U + 2) % RING>{});
                        const uint32_t hb = AM ? XZ.h1 : XZ.h0, vb = AM ? XZ.v1 : XZ.v0;
                        add_sample_w((int32_t)(pre - (hb - Y.h0)), (int32_t)(vt - vb), wgt, wr);
                    };
                    // (the last round stops at nmax: steps past it hold no
                    // sample, and their DMAs feed no later read)
                    for (int n4 = 0; n4 < nmax; n4 += RING) {
                        static_for<RING>([&](auto IC) {
                            constexpr int I = decltype(IC)::value;
                            if (I == 0 || n4 + I < nmax) {
                                if constexpr (I % 2 == 0) stp(IntC<I>{}, n4, A, B);
                                else stp(IntC<I>{}, n4, B, A);
                            }
                        });
                    }
                }
            };
            const bool narrow = W4 <= 16;
            auto rows_g = [&](auto AC, auto RSC) {
                if constexpr (decltype(RSC)::value == 256) rows_dma(AC, RSC, IntC<1>{});
                else if (dual) rows_dma(AC, RSC, IntC<2>{});
                else rows_dma(AC, RSC, IntC<1>{});
            };
            auto rows_w = [&](auto AC) {
                if (narrow) rows_g(AC, IntC<64>{});
                else if (!wide64) rows_g(AC, IntC<128>{});
                else rows_g(AC, IntC<256>{});
            };
            if (hmode == 0) rows_w(std::integral_constant<bool, true>());
            else rows_w(std::integral_constant<bool, false>());
            // the ring's last DMAs have landed before it holds the reduction
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (share) {
            // ---- sparse rows (step > 3 or a wide span): per integral row a
            // lane loads its (c, c + 1) pair; columns c - s and c + s + 1 come
            // from lanes j -+ 2 (DPP wave shifts), the two edge lanes on each
            // side load them themselves
            const bool ld_on = j < side;
            const bool eL = j < 2, eR = j + 2 >= side;
            const int oA = (c - hs) * 4, oB = (c + hs + 1) * 4, oC = c * 4;
            const int oE = eL ? oA : oB;
            const int nph = dual ? 1 : 2;
            struct Raw { v2u32 lo, hi; uint32_t elo, ehi; };
            auto ldraw = [&](int t) {
                const int rb = (iy + (t - iradius) * step) * ip4;
                const int o = ld_on ? rb + oC : (int)kOOB;
                const int oe = (ld_on && (eL || eR)) ? rb + oE : (int)kOOB;
                Raw q;
                // loads only on the lanes that use them (the edge loads: <= 4
                // lanes): masked-off lanes cost no address cycles, unlike
                // out-of-bounds ones; their values are never read
                q.lo = v2u32{0u, 0u};
                q.hi = v2u32{0u, 0u};
                q.elo = 0u;
                q.ehi = 0u;
                if (ld_on) {
                    q.lo = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o, 0, 0);
                    q.hi = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o + ip4, 0, 0);
                }
                if (ld_on && (eL || eR)) {
                    q.elo = bld(rsrc, oe);
                    q.ehi = bld(rsrc, oe + ip4);
                }
                return q;
            };
            auto rows = [&](auto AC) {
                constexpr bool A = decltype(AC)::value;
                // columns c - s / c + s + 1 are column c / c + 1 of lanes j -+ 2 (A)
                // or c + 1 / c (B)
                auto proc = [&](const Raw& q) -> DuHV {
                    const uint32_t l0 = wave_from_lo2(A ? q.lo.x : q.lo.y);
                    const uint32_t r0 = wave_from_hi2(A ? q.lo.y : q.lo.x);
                    const uint32_t l1 = wave_from_lo2(A ? q.hi.x : q.hi.y);
                    const uint32_t r1 = wave_from_hi2(A ? q.hi.y : q.hi.x);
                    return du_hv(eL ? q.elo : l0, q.lo.x, q.lo.y, eR ? q.elo : r0, eL ? q.ehi : l1, q.hi.x, q.hi.y,
                                 eR ? q.ehi : r1);
                };
                for (int ph = 0; ph < nph; ph++) {
                    const int hh = dual ? h : ph;
                    const int nstep = max(nv - hh + 1, 0) >> 1;
                    const int nmax = dual ? max(nv + 1, 0) >> 1 : nstep;
                    if (nmax == 0) continue;
                    const int tb = t0 + hh;
                    auto smp = [&](int n, const DuHV& A0, const DuHV& A1, const DuHV& A2) {
                        const int t = tb + 2 * n;
                        sample_hv(std::integral_constant<bool, A>(), A0, A1, A2, s_rp[w][t], s_wr[w][t],
                                  col_on && n < nstep);
                    };
                    const Raw q0 = ldraw(tb - 2), q1 = ldraw(tb);
                    Raw s0 = ldraw(tb + 2), s1 = ldraw(tb + 4), s2 = ldraw(tb + 6);
                    DuHV X = proc(q0), Y = proc(q1), Z;
                    for (int n = 0; n < nmax; n += 3) {
                        const int t = tb + 2 * n;
                        Z = proc(s0);
                        s0 = ldraw(t + 8);
                        smp(n, X, Y, Z);
                        X = proc(s1);
                        s1 = ldraw(t + 10);
                        smp(n + 1, Y, Z, X);
                        Y = proc(s2);
                        s2 = ldraw(t + 12);
                        smp(n + 2, Z, X, Y);
                    }
                }
            };
            if (hmode == 0) rows(std::integral_constant<bool, true>());
            else rows(std::integral_constant<bool, false>());
        } else {
            // ---- generic (s = 2 step + 1 at exact half-way scales): 12
            // gathers per sample
            const int oA = (c - hs) * 4, oB = (c + hs + 1) * 4, oC = c * 4;
            const int dR0 = -hs * ip4, dR3 = (hs + 1) * ip4;
            const int rstep = dual ? 2 : 1;
            for (int k = h; k < nv; k += rstep) {
                if (col_on) {
                    const int rb = (iy + (t0 + k - iradius) * step) * ip4;
                    const int q0 = rb + dR0, q2 = rb + ip4, q3 = rb + dR3;
                    const uint32_t a00 = bld(rsrc, q0 + oA), a01 = bld(rsrc, q0 + oB), a02 = bld(rsrc, q0 + oC),
                                   a03 = bld(rsrc, q0 + oC + 4), a10 = bld(rsrc, rb + oA), a11 = bld(rsrc, rb + oB),
                                   a20 = bld(rsrc, q2 + oA), a21 = bld(rsrc, q2 + oB), a30 = bld(rsrc, q3 + oA),
                                   a31 = bld(rsrc, q3 + oB), a32 = bld(rsrc, q3 + oC), a33 = bld(rsrc, q3 + oC + 4);
                    const int32_t wav1 = (int32_t)((a21 + a00 - a01 - a20) - (a31 + a10 - a11 - a30));
                    const int32_t wav2 = (int32_t)((a31 + a02 - a01 - a32) - (a33 + a00 - a03 - a30));
                    add_sample(wav1, wav2, s_rp[w][t0 + k], s_wr[w][t0 + k], true);
                }
            }
        }
        // ---- getTrace (surfd.cu:369-377, makePoint's laplace) when the fit
        // left it here (its inputs in the entry, nms_fit_point): lane l < 16
        // loads corner l & 3 of box l >> 2 -- the rows the window's DMAs just
        // brought into L2 -- issued before the reduction, summed after it
        uint32_t tv = 0u;
        if (trace) {
            const int tcen = __builtin_amdgcn_readlane(__float_as_int(pte), 8);
            const int ttemp = __builtin_amdgcn_readlane(__float_as_int(pte), 9);
            const int x0 = (int)(int16_t)(tcen & 0xffff), y0 = tcen >> 16;
            const int t2 = ttemp / 2, t3 = t2 + t2;
            const int b = (lane >> 2) & 3, k = lane & 3;
            // boxes (x1, y1, x2, y2) of trace_sign: lxx = B0 - 3 B1, lyy = B2 - 3 B3
            const int x1 = b == 0 ? x0 + ttemp + t2 : b == 1 ? x0 + t2 : x0 + t3;
            const int x2 = b == 0 ? x0 - ttemp - t2 : b == 1 ? x0 - t2 : x0 - t3;
            const int y1 = b < 2 ? y0 + t3 : b == 2 ? y0 + ttemp + t2 : y0 + t2;
            const int y2 = b < 2 ? y0 - t3 : b == 2 ? y0 - ttemp - t2 : y0 - t2;
            // box_flat's corners: +(y1 + 1, x1 + 1) +(y2, x2) -(y2, x1 + 1) -(y1 + 1, x2)
            const int cy = (k == 0 || k == 3) ? y1 + 1 : y2;
            const int cx = (k == 0 || k == 2) ? x1 + 1 : x2;
            const int fi = cy * P.ip + cx;
            // (flat_at's bounds [0, iH ip) are the frame resource's: a corner
            // outside reads 0, like lanes >= 16, with no branch; against a
            // bounds-checked global load: describe -0.014 ms, DESIGN NMS)
            tv = bld(rsrc, lane < 16 ? fi * 4 : (int)kOOB);
        }
        // ---- the column reduction.  Dual: the half-waves (same grid column,
        // alternate rows) fold inside the row writes below.
        // lane j's row: per cell row R its bins in output order (haar_bins
        // keeps {total, negative part} pairs: bin 2q = negative, 2q + 1 =
        // positive), then cfrac
        // lane jj's row: slot jj / 16, row jj % 16
        // (the slot's LDS address by integer masks: a select, of pointers or
        // of addresses, became a branch per row read)
        typedef float __attribute__((address_space(3))) lf32;
        auto red_row = [&](int jj) -> lf32* {
            const uint32_t k = (uint32_t)jj >> 4;                 // 0..3
            const uint32_t b = lds_sl[0] + ((0u - min(k, 1u)) & (lds_sl[1] - lds_sl[0])) +
                               ((0u - (k >> 1)) & (lds_sl[2] - lds_sl[1])) +
                               ((0u - (k & (k >> 1))) & (lds_sl[3] - lds_sl[2]));
            return (lf32*)(size_t)(b + (uint32_t)((jj & 15) * RW * 4));
        };
        if (dual) {
            // One permlane32 swap per accumulator pair folds both of its
            // components: swap(x, y) leaves x' = {x.lo, y.lo}, y' = {x.hi,
            // y.hi}, so x' + y' is column j's x total in lane j < 32 and its y
            // total in lane j + 32 (the same two addends, in the same order, as
            // folding each register with itself).  The x components are bins
            // 0 .. NB/2 - 1 of a cell row (du_pick), the y components the
            // rest: lane j writes the first half of row j, lane j + 32 the
            // second.  Pair g of a half is {t, n} = {F[g], F[g + NS/4]}.
            // (Against swapping each register with a copy of itself and
            // writing from lanes j < 32: 20 fewer instructions per keypoint,
            // the same descriptors, describe time within noise -- DESIGN 6.)
            lf32* const rw = red_row(lane & 31);
            lf32* const rwh = rw + (lane >> 5) * (NB / 2);
#pragma unroll
            for (int R = 0; R < WSZ; R++) {
                float F[NS / 2];
#pragma unroll
                for (int s = 0; s < NS / 2; s++) {
                    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[R][s].x), __float_as_uint(acc[R][s].y),
                                                              false, false);
                    F[s] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
                }
#pragma unroll
                for (int g = 0; g < NS / 4; g++) {
                    const float t = F[g], n = F[g + NS / 4];
                    *reinterpret_cast<v2f32 __attribute__((address_space(3)))*>(rwh + R * NB + 2 * g) = v2f32{n, t - n};
                }
            }
            rw[CFI] = cfrac;                    // (lanes j and j + 32: the same column, the same value)
        } else if (!dual || lane < 32) {
            lf32* const rw = red_row(lane);
            // bin 2q = the negative / sign-selected part, 2q + 1 = total - it
            // (haar_bins' pairs {S[2q], S[2q + 1]} in du_pair's registers)
#pragma unroll
            for (int R = 0; R < WSZ; R++)
#pragma unroll
                for (int q4 = 0; q4 < NB / 4; q4++) {
                    const float t0 = du_pick<NS>(acc[R], 4 * q4), n0 = du_pick<NS>(acc[R], 4 * q4 + 1);
                    const float t1 = du_pick<NS>(acc[R], 4 * q4 + 2), n1 = du_pick<NS>(acc[R], 4 * q4 + 3);
                    *reinterpret_cast<du_v4f __attribute__((address_space(3)))*>(rw + R * NB + 4 * q4) =
                        du_v4f{n0, t0 - n0, n1, t1 - n1};
                }
            rw[CFI] = cfrac;
        }
        // cell column C's lanes are one contiguous run (cx and the bounds are
        // monotonic in j): [lo_C, hi_C), wave-uniform
        int rlo[WSZ + 1], rhi[WSZ + 1];
#pragma unroll
        for (int C = -1; C < WSZ; C++) {
            unsigned long long mc = __ballot(col_on && ci == C);
            if (dual) mc &= 0xffffffffull;
            rlo[C + 1] = mc ? __builtin_ctzll(mc) : 0;
            rhi[C + 1] = mc ? 64 - __builtin_clzll(mc) : 0;
        }
        wave_sync();
        // Output cell (R, C): lane rc = 4 R + C of each quarter qq = lane / 16
        // sums a cell row's NB bins (ds_read_b128s) over one part of the two
        // runs that feed it -- qq 0 / 1: column C's own run (weight 1 -
        // cfrac), its even / odd rows; qq 2 / 3: column C - 1's run (cfrac)
        // -- and the quarters add in a fixed order (permlane swaps).
        const int qq = lane >> 4, rc = lane & 15, oR = rc >> 2, oC = rc & 3;
        const bool own = qq < 2;
        int lo = rlo[0], hi = rhi[0];
#pragma unroll
        for (int k = 1; k <= WSZ; k++)
            if ((own ? oC + 1 : oC) == k) { lo = rlo[k]; hi = rhi[k]; }
        float v[NB];
#pragma unroll
        for (int b = 0; b < NB; b++) v[b] = 0.f;
        for (int jj = lo + (qq & 1); jj < hi; jj += 2) {
            const lf32* const rr = red_row(jj);
            const float cf = rr[CFI];
            const float wt = own ? 1.f - cf : cf;
#pragma unroll
            for (int q4 = 0; q4 < NB / 4; q4++) {
                const du_v4f x = *reinterpret_cast<const du_v4f __attribute__((address_space(3)))*>(rr + oR * NB + 4 * q4);
                v[4 * q4] = __builtin_fmaf(x.x, wt, v[4 * q4]);
                v[4 * q4 + 1] = __builtin_fmaf(x.y, wt, v[4 * q4 + 1]);
                v[4 * q4 + 2] = __builtin_fmaf(x.z, wt, v[4 * q4 + 2]);
                v[4 * q4 + 3] = __builtin_fmaf(x.w, wt, v[4 * q4 + 3]);
            }
        }
        // quarters: (qq 0 + qq 1) + (qq 2 + qq 3) into lanes 0..15
#pragma unroll
        for (int b = 0; b < NB; b++) {
            v[b] = du_tree_step<16>(v[b]);
            v[b] = du_tree_step<32>(v[b]);
        }
        // ---- normalize (surfd.cu:2447-2493): sum of squares over the 16
        // output lanes' NB values each
        float a = 0.f;
#pragma unroll
        for (int b = 0; b < NB; b++) a = __builtin_fmaf(v[b], v[b], a);
        a = du_tree_step<8>(a);
        a = du_tree_step<4>(a);
        a = du_tree_step<2>(a);
        a = du_tree_step<1>(a);
        const float fac = 1.f / sqrtf(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a))));
        // the pipeline: entry k + 1 (loaded since the top) and the index of k + 2
        ndx = __int_as_float(entry(0));
        ndy = __int_as_float(entry(1));
        nsp = __int_as_float(entry(2));
        nf = entry(3);
        nix = entry(4);
        niy = entry(5);
        npk = entry(6);
        nidx = entry(7);
        ptr = pv;
        nrs = __int_as_float(entry(10));
        gc = g1;
        g1 = kq.finish(a2);
        if (trace) {
            // sum of the 16 corners with their signs and the boxes' weights
            // (1, -3, 1, -3): uint32 arithmetic, as trace_sign, so any
            // summation order gives the same bits
            const int b = (lane >> 2) & 3, k = lane & 3;
            uint32_t t = tv * ((b & 1) ? 3u : 1u);
            t = (k < 2) == ((b & 1) == 0) ? t : 0u - t;
            // row 0's inclusive scan by DPP row shifts: lane 15 holds the sum
            // (lanes >= 16 hold 0 and never reach row 0)
            t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xf, 0xf, true);
            t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xf, 0xf, true);
            t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xf, 0xf, true);
            t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xf, 0xf, true);
            const int32_t tr = (int32_t)__builtin_amdgcn_readlane((int)t, 15);
            // laplace (word 5 of the point) and ori = 0 (word 6), lanes 0 / 1
            if (lane < 2) {
                uint32_t* pw = reinterpret_cast<uint32_t*>(pts + idx) + 5 + lane;
                *pw = lane == 0 ? (uint32_t)(tr > 0 ? 1 : -1) : 0u;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float* out = desc + (size_t)idx * NF;
        if (lane < 16) {
#pragma unroll
            // (non-temporal stores here, to keep them out of the L2 the
            // windows are read from: neutral, DESIGN 6)
            for (int q4 = 0; q4 < NB / 4; q4++)
                *reinterpret_cast<float4*>(out + rc * NB + 4 * q4) =
                    make_float4(v[4 * q4] * fac, v[4 * q4 + 1] * fac, v[4 * q4 + 2] * fac, v[4 * q4 + 3] * fac);
        }
    }
}
