// surfhip_desc_ur.inc -- upright 4x4-cell descriptor from registers
// (k_describe_ur, small batches) and the buffer-load helpers it shares with
// k_describe_u2.  Included by surfhip_kernels.hip; launch_describe is there.

// ----------------------------------------------------------------------
// Upright descriptor (U-SURF, 4x4 cells), deterministic and atomic-free.
// The upright sample grid is separable (surfd.cu:1290-1294): a sample's cell
// row (ri, rfrac) depends only on its grid row i, its cell column (ci, cfrac)
// only on its grid column j.  So:
//  * lane = grid column j; when the grid is at most 32 columns wide (iradius
//    <= 15, ~2/3 of keypoints) the two half-waves walk alternate grid rows,
//    so no lane idles on the wide-grid padding;
//  * the rows are walked in cell-row bands (ri = -1..3, contiguous because ri
//    is monotonic in i), each band compile-time, so the placeInIndex row
//    weights (1 - rfrac, rfrac) go into fixed registers: per band a lane keeps
//    P = sum v and Q = sum v * rfrac, then row ri gets P - Q and row ri + 1
//    gets Q (surfd.cu:1199-1271 with the sums regrouped);
//  * bins are kept as (total, negative part) pairs, so the sign-selected
//    bins cost a min/select instead of a branch;
//  * the column weights (1 - cfrac, cfrac) are applied once per lane in a
//    fixed-order reduction over the lanes of each cell column.
// Grid-row geometry (rpos, rx, ri, rfrac) is computed once per row, with the
// reference's exact float operations, so cell membership and the lookup2
// index match the oracle bit for bit; only the summation order differs
// (<= 1e-6 relative, inside the 1e-4 descriptor tolerance).
// Integral-image reads are raw buffer loads (SGPR descriptor + 32-bit
// offsets, no 64-bit address arithmetic).  iradius <= 22 for wsz 4, so the
// grid fits one wave.
// ----------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const uint32_t* I, long long nbytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)I, (short)0, (int)nbytes, 0x00020000);
}
__device__ __forceinline__ uint32_t bld(__amdgpu_buffer_rsrc_t r, int off)
{
    return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
}

template <int NS>
__device__ __forceinline__ void haar_bins(int32_t wav1, int32_t wav2, float weight, bool ok, float (&S)[NS])
{
    // {dx, dy} = weight * {wav2, wav1} in one packed multiply; a lane
    // outside the grid contributes 0 (a select: its inputs may be garbage)
    v2f32 d = v2f32{(float)wav2, (float)wav1} * weight;
    const float dx = ok ? d.x : 0.f, dy = ok ? d.y : 0.f;
    if constexpr (NS == 4) {
        S[0] = dx; S[1] = fminf(dx, 0.f);          // bins 1 | 0 by sign of dx
        S[2] = dy; S[3] = fminf(dy, 0.f);          // bins 3 | 2 by sign of dy
    } else {
        const float adx = fabsf(dx), ady = fabsf(dy);
        S[0] = dx;  S[1] = dy < 0.f ? dx : 0.f;    // bins 1 | 0 by sign of dy
        S[2] = adx; S[3] = dy < 0.f ? adx : 0.f;   // bins 3 | 2
        S[4] = dy;  S[5] = dx < 0.f ? dy : 0.f;    // bins 5 | 4 by sign of dx
        S[6] = ady; S[7] = dx < 0.f ? ady : 0.f;   // bins 7 | 6
    }
}

template <int R> struct IntC { static constexpr int value = R; };

// value of lane - 2 / lane + 2 across the whole wave (DPP wave_shr:1 /
// wave_shl:1 twice; lanes shifted in from outside the wave get 0)
__device__ __forceinline__ uint32_t wave_from_lo2(uint32_t v)
{
    const int a = __builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(0, a, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_from_hi2(uint32_t v)
{
    const int a = __builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(0, a, 0x130, 0xf, 0xf, false);
}

template <bool EXT>
__global__ __launch_bounds__(256) void k_describe_ur(const int32_t* __restrict__ ii, FrameParams P,
                                                     const surfhip_point* __restrict__ pts, int max_pts,
                                                     const int* __restrict__ offsets,
                                                     const int* __restrict__ order, int nframes,
                                                     float* __restrict__ desc, int* __restrict__ queue)
{
    constexpr int WSZ = 4;
    constexpr int NB = EXT ? 8 : 4;                       // bins per cell
    constexpr int NF = WSZ * WSZ * NB;
    constexpr int RS = WSZ * NB + 1;                      // odd stride: conflict-free writes
    __shared__ float red[4][64][RS];
    __shared__ float s_cf[4][64];
    __shared__ float s_rf[4][64], s_rp[4][64];
    __shared__ int s_ri[4][64];
    __shared__ float4 s_wr[4][64];               // per grid row: weights of cell rows 0..3
    __shared__ __attribute__((aligned(16))) uint32_t s_seg[4][448];   // segment path: the wave's integral rows
    __shared__ int4 s_run[4][6];
    // Gaussian weights premultiplied by 1/255 (the reference scales the Haar
    // response by the weight, then by 1/255: one rounding moves, within the
    // descriptor tolerance)
    __shared__ float s_lut[40];
    if (threadIdx.x < 40) s_lut[threadIdx.x] = c_tab.lut2[threadIdx.x] * INV255;
    __syncthreads();
    const int lane = (int)lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform: SGPR descriptors
    const int total = offsets[nframes];
    const float fw = (float)WSZ;
    const float wofs = (float)WSZ * 0.5f - 0.5f;
    KpQueue kq(total, queue, w);
    const int gend = kq.gend;
    auto grab = [&]() { return kq.grab(lane); };
    // the wave's keypoints ascend, so its frame is tracked incrementally
    // (one binary search per wave) and the next keypoint is fetched while
    // the current one is described
    int gn = grab();
    int fn = 0, fnb = 0, fne = 0, kn = 0;
    surfhip_point pn;
    if (gn < gend) {
        int lo = 0, hi = nframes;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= gn) lo = mid; else hi = mid;
        }
        fn = lo;
        fnb = offsets[lo];
        fne = offsets[lo + 1];
        kn = order[(size_t)fn * max_pts + (gn - fnb)];
        pn = pts[(size_t)fn * max_pts + kn];
    }
    while (gn < gend) {
        const int f = fn, kp = kn;
        const surfhip_point p = pn;
        gn = grab();
        if (gn < gend) {
            while (gn >= fne) { fn++; fnb = fne; fne = offsets[fn + 1]; }
            kn = order[(size_t)fn * max_pts + (gn - fnb)];
            pn = pts[(size_t)fn * max_pts + kn];
        }
        const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
        const __amdgpu_buffer_rsrc_t rsrc = frame_rsrc(I, P.ii_stride * 4);
        const DescAt at = desc_at(P.doubled, p);
        const float scale = at.scale;
        const int step = max(f2i_rn(scale * 0.5f), 1);
        const int ix = f2i_rn(at.x), iy = f2i_rn(at.y);
        const float dx0 = at.x - (float)ix, dy0 = at.y - (float)iy;
        const float spacing = scale * (float)P.mag;
        const int hs = f2i_rz(scale);
        const int rlim = P.iH - 1 - hs, clim = P.W - hs;
        const int iradius = f2i_rn(((spacing * (float)(WSZ + 1)) * 0.5f) / (float)step);
        const int side = 2 * iradius + 1;
        // ---- grid row t = lane: exact row geometry (surfd.cu:1290-1292)
        const int sit = lane - iradius;
        const float rpos_t = ((float)(step * sit) - dy0) / spacing;
        const float rx_t = rpos_t + wofs;
        const int r_t = iy + sit * step;
        const bool rvalid = lane < side && rx_t > -1.f && rx_t < fw && r_t >= 1 + hs && r_t < rlim;
        const int ri_t = f2i_rz(rx_t >= 0.f ? rx_t : rx_t - 1.f);
        s_rf[w][lane] = rx_t - (float)ri_t;
        s_rp[w][lane] = rpos_t * rpos_t;
        s_ri[w][lane] = ri_t;
        {
            // placeInIndex's row weights (surfd.cu:1199-1271): 1 - rfrac for
            // cell row ri, rfrac for ri + 1
            const float rf_t = rx_t - (float)ri_t, w0_t = 1.f - rf_t;
            s_wr[w][lane] = make_float4(ri_t == 0 ? w0_t : (ri_t == -1 ? rf_t : 0.f),
                                        ri_t == 1 ? w0_t : (ri_t == 0 ? rf_t : 0.f),
                                        ri_t == 2 ? w0_t : (ri_t == 1 ? rf_t : 0.f),
                                        ri_t == 3 ? w0_t : (ri_t == 2 ? rf_t : 0.f));
        }
        // ---- grid column of this lane (lane = j; dual: two half-waves of 32
        // lanes walk alternate grid rows)
        const int hmode = hs - 2 * step;          // 0 or -1: rows and columns share integral pairs
        const bool share = hmode == 0 || hmode == -1;
        const bool dual = side <= 32;
        const int j = dual ? (lane & 31) : lane;
        const int h = dual ? (lane >> 5) : 0;
        const int rstep = dual ? 2 : 1;
        const int sj = j - iradius;
        const float cpos = ((float)(step * sj) - dx0) / spacing;
        const float cx = cpos + wofs;
        const int c = ix + sj * step;
        const bool col_on = j < side && cx > -1.f && cx < fw && c >= 1 + hs && c < clim;
        const int ci = f2i_rz(cx >= 0.f ? cx : cx - 1.f);
        const float cfrac = cx - (float)ci;
        const float cp2 = cpos * cpos;
        const int ip4 = P.ip * 4;
        const int oA = (c - hs) * 4, oB = (c + hs + 1) * 4, oC = c * 4;
        const int dR0 = -hs * ip4, dR3 = (hs + 1) * ip4;
        wave_sync();
        constexpr int NS = EXT ? 8 : 4;
        float acc[WSZ][NS];
#pragma unroll
        for (int R = 0; R < WSZ; R++)
#pragma unroll
            for (int s = 0; s < NS; s++) acc[R][s] = 0.f;
        // ---- the valid grid rows form one contiguous run [t0, t0 + nv); half h
        // takes rows t0 + h, t0 + h + rstep, ...
        // A row adds S * (1 - rfrac) to cell row ri and S * rfrac to ri + 1
        // (placeInIndex, surfd.cu:1199-1271); the weights of the 4 cell rows
        // are formed by selects, so the accumulators keep fixed registers.
        const unsigned long long vm = __ballot(rvalid);
        const int t0 = vm ? __builtin_ctzll(vm) : 0, nv = __builtin_popcountll(vm);
        // one sample: its 12 integral-image corners -> haar responses -> bins
        auto accum = [&](uint32_t a00, uint32_t a01, uint32_t a02, uint32_t a03, uint32_t a10, uint32_t a11,
                         uint32_t a20, uint32_t a21, uint32_t a30, uint32_t a31, uint32_t a32, uint32_t a33,
                         int tt) {
            const float rf = s_rf[w][tt];
            const float rp = s_rp[w][tt];
            const int ri = s_ri[w][tt];
            // haarX / haarY (surfd.cu:1171-1182 via getSum); rows r-s, r, r+1,
            // r+s+1 (a0*, a1*, a2*, a3*), cols c-s, c+s+1, c, c+1
            const int32_t wav1 = (int32_t)((a21 + a00 - a01 - a20) - (a31 + a10 - a11 - a30));
            const int32_t wav2 = (int32_t)((a31 + a02 - a01 - a32) - (a33 + a00 - a03 - a30));
            float S[NS];
            haar_bins(wav1, wav2, s_lut[f2i_rz(rp + cp2)], true, S);
            const float w0 = 1.f - rf;
            // the cell row is uniform over the wave except where the two
            // halves (dual mode) straddle a cell-row boundary
            const int riu = __builtin_amdgcn_readfirstlane(ri);
            if (__all(ri == riu)) {
#pragma unroll
                for (int R = 0; R < WSZ; R++) {
                    if (R == riu) {
#pragma unroll
                        for (int s = 0; s < NS; s++) acc[R][s] = fmaf(S[s], w0, acc[R][s]);
                    } else if (R == riu + 1) {
#pragma unroll
                        for (int s = 0; s < NS; s++) acc[R][s] = fmaf(S[s], rf, acc[R][s]);
                    }
                }
            } else {
#pragma unroll
                for (int R = 0; R < WSZ; R++) {
                    const float rw = (R == ri) ? w0 : ((R == ri + 1) ? rf : 0.f);
#pragma unroll
                    for (int s = 0; s < NS; s++) acc[R][s] = fmaf(S[s], rw, acc[R][s]);
                }
            }
        };
        if (share) {
            // ---- Row and column sharing.  step = rn(scale / 2) and hs =
            // rz(scale) give hs = 2 step or 2 step - 1, so the outer rows
            // r - hs and r + hs + 1 of grid row i are rows r and r + 1 of grid
            // rows i - 2 and i + 2, and likewise the columns.  Each half walks
            // every other grid row (dual: rows of its parity; single: even
            // rows, then odd rows).  Per integral row a lane loads its (c, c+1)
            // pair (8 bytes, issued three grid rows ahead into a raw slot);
            // when the row is first needed it takes columns c - hs and
            // c + hs + 1 from lanes j -+ 2, except the two edge lanes on each
            // side, which load that column themselves (the same instruction,
            // every other lane past the buffer).  4 loads per sample (was 12).
            const bool ld_on = j < side;
            const bool eL = j < 2, eR = j + 2 >= side;
            const int oE = eL ? oA : oB;          // edge lanes: c - hs (left) / c + hs + 1 (right)
            const int nph = dual ? 1 : 2;
            struct Raw { v2u32 lo, hi; uint32_t elo, ehi; };
            auto ldraw = [&](int t) {
                const int rb = (iy + (t - iradius) * step) * ip4;
                const int o = ld_on ? rb + oC : (int)kOOB;
                const int oe = (ld_on && (eL || eR)) ? rb + oE : (int)kOOB;
                Raw q;
                q.lo = __builtin_amdgcn_raw_buffer_load_b64(rsrc, o, 0, 0);
                q.hi = __builtin_amdgcn_raw_buffer_load_b64(rsrc, ld_on ? o + ip4 : (int)kOOB, 0, 0);
                q.elo = bld(rsrc, oe);
                q.ehi = bld(rsrc, (ld_on && (eL || eR)) ? oe + ip4 : (int)kOOB);
                return q;
            };
            // The row loop, specialised on hmode (A: hs = 2 step).  A row adds
            // S (1 - rfrac) to cell row ri and S rfrac to ri + 1: the four
            // row weights come precomputed per grid row (s_wr).
            auto rows = [&](auto AC) {
                constexpr bool A = decltype(AC)::value;
                // T = rows r, r+1 x cols c-s, c, c+1, c+s+1
                // columns c -+ hs from lanes j -+ 2: two DPP wave shifts each
                // (VALU) instead of an LDS permute
                auto proc = [&](const Raw& q, uint32_t (&T)[8]) {
                    T[1] = q.lo.x; T[2] = q.lo.y; T[5] = q.hi.x; T[6] = q.hi.y;
                    const uint32_t l0 = wave_from_lo2(A ? q.lo.x : q.lo.y);
                    const uint32_t r0 = wave_from_hi2(A ? q.lo.y : q.lo.x);
                    const uint32_t l1 = wave_from_lo2(A ? q.hi.x : q.hi.y);
                    const uint32_t r1 = wave_from_hi2(A ? q.hi.y : q.hi.x);
                    T[0] = eL ? q.elo : l0;
                    T[3] = eR ? q.elo : r0;
                    T[4] = eL ? q.ehi : l1;
                    T[7] = eR ? q.ehi : r1;
                };
                for (int ph = 0; ph < nph; ph++) {
                    const int hh = dual ? h : ph;
                    // rows t0 + hh, t0 + hh + 2, ...: nstep of them (the halves
                    // of a dual wave may differ by one; the loop runs the larger)
                    const int nstep = max(nv - hh + 1, 0) >> 1;
                    const int nmax = dual ? max(nv + 1, 0) >> 1 : nstep;
                    if (nmax == 0) continue;
                    // one sample of grid row t from the sets of rows t - 2, t, t + 2
                    auto sample = [&](int n, const uint32_t (&Pv)[8], const uint32_t (&Cv)[8],
                                      const uint32_t (&Nv)[8]) {
                        const int t = t0 + hh + 2 * n;
                        if (!(col_on && n < nstep)) return;
                        constexpr bool ok = true;
                        const float rp = s_rp[w][t];
                        const float4 wr = s_wr[w][t];
                        // top row r - hs, bottom row r + hs + 1; rows r-s, r, r+1,
                        // r+s+1 (a0*, a1*, a2*, a3*), cols c-s, c+s+1, c, c+1
                        const uint32_t a00 = A ? Pv[0] : Pv[4], a02 = A ? Pv[1] : Pv[5];
                        const uint32_t a03 = A ? Pv[2] : Pv[6], a01 = A ? Pv[3] : Pv[7];
                        const uint32_t a30 = A ? Nv[4] : Nv[0], a32 = A ? Nv[5] : Nv[1];
                        const uint32_t a33 = A ? Nv[6] : Nv[2], a31 = A ? Nv[7] : Nv[3];
                        const uint32_t a10 = Cv[0], a11 = Cv[3], a20 = Cv[4], a21 = Cv[7];
                        // haarX / haarY (surfd.cu:1171-1182 via getSum)
                        const int32_t wav1 = (int32_t)((a21 + a00 - a01 - a20) - (a31 + a10 - a11 - a30));
                        const int32_t wav2 = (int32_t)((a31 + a02 - a01 - a32) - (a33 + a00 - a03 - a30));
                        float S[NS];
                        haar_bins(wav1, wav2, s_lut[f2i_rz(rp + cp2)], ok, S);
                        // all four cell rows with the row's weights (two are 0):
                        // branch-free, fixed registers
                        const float wrr[WSZ] = {wr.x, wr.y, wr.z, wr.w};
#pragma unroll
                        for (int R = 0; R < WSZ; R++)
#pragma unroll
                            for (int e = 0; e < NS; e++) acc[R][e] = fmaf(S[e], wrr[R], acc[R][e]);
                    };
                    // 8-value sets X, Y, Z rotate through the roles (top, middle,
                    // bottom) and raw slots s0..s2 hold the rows 2, 4, 6 ahead;
                    // unrolled by 3 so no register moves the sets around.  All
                    // loads are unconditional (past the buffer where not needed),
                    // so hipcc's outstanding-load count stays exact.
                    uint32_t X[8], Y[8], Z[8];
                    const int tb = t0 + hh;
                    const Raw q0 = ldraw(tb - 2), q1 = ldraw(tb);
                    Raw s0 = ldraw(tb + 2), s1 = ldraw(tb + 4), s2 = ldraw(tb + 6);
                    proc(q0, X);
                    proc(q1, Y);
                    for (int n = 0; n < nmax; n += 3) {
                        const int t = tb + 2 * n;
                        proc(s0, Z);
                        s0 = ldraw(t + 8);
                        sample(n, X, Y, Z);
                        proc(s1, X);
                        s1 = ldraw(t + 10);
                        sample(n + 1, Y, Z, X);
                        proc(s2, Y);
                        s2 = ldraw(t + 12);
                        sample(n + 2, Z, X, Y);
                    }
                }
            };
            // ---- segment path (step <= 3, ~80 % of keypoints): the needed
            // columns c_j - hs .. c_j + hs + 1 of all grid columns tile one
            // contiguous span of each integral row, so a wave step loads the
            // span of its 2 (dual: 4) integral rows as 16-byte chunks (1-2
            // instructions instead of 4), stages them in a per-wave LDS row
            // buffer and every lane reads its 8 values from there.
            const int G = dual ? 2 : 1;
            const int cs = (ix + (-2 - iradius) * step) & ~3;
            const int W4 = (ix + (side + 1 - iradius) * step + 2 - cs + 3) >> 2;
            const int WP = 4 * W4;
            const int nitem = 2 * G * W4;
            const bool seg = step <= 3 && nitem <= 128 && 2 * G * WP <= 448;
            auto rows_seg = [&](auto AC) {
                constexpr bool A = decltype(AC)::value;
                uint32_t* buf = s_seg[w];
                // chunk i of a wave step: integral row rr = 2 g + e of the step's
                // grid rows, 16-byte chunk q; fixed per lane
                int ckoff[2], cdst[2];
                bool cok[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int k = lane + 64 * i;
                    const int rr = k / W4, q = k - rr * W4;
                    cok[i] = k < nitem;
                    cdst[i] = rr * WP + 4 * q;
                    // integral row of grid row t0 (+ g): iy + (t0 + g - iradius) step + e
                    ckoff[i] = ((iy + (t0 + (rr >> 1) - iradius) * step + (rr & 1)) * P.ip + cs + 4 * q) * 4;
                }
                const int gstride = 2 * step * ip4;             // two grid rows further down
                struct Seg { uint4 c0, c1; };
                auto ldseg = [&](int tt) {                      // grid rows t0 + tt (+ 1): tt relative
                    Seg q;
                    const int d = tt * step * ip4;
                    q.c0 = buf_ld4(rsrc, cok[0] ? (uint32_t)(ckoff[0] + d) : kOOB);
                    q.c1 = buf_ld4(rsrc, cok[1] ? (uint32_t)(ckoff[1] + d) : kOOB);
                    return q;
                };
                const int xo = ld_on ? c - cs : 2 * hs;         // this lane's column in the buffer
                const int rowg = (dual ? h : 0) * 2 * WP;
                // T = rows r, r+1 x cols c-s, c, c+1, c+s+1
                auto proc = [&](const Seg& q, uint32_t (&T)[8]) {
                    if (cok[0]) *reinterpret_cast<uint4*>(buf + cdst[0]) = q.c0;
                    if (cok[1]) *reinterpret_cast<uint4*>(buf + cdst[1]) = q.c1;
                    lds_order();
                    const uint32_t* r0 = buf + rowg + xo;
                    const uint32_t* r1 = r0 + WP;
                    T[0] = r0[-hs]; T[1] = r0[0]; T[2] = r0[1]; T[3] = r0[hs + 1];
                    T[4] = r1[-hs]; T[5] = r1[0]; T[6] = r1[1]; T[7] = r1[hs + 1];
                    lds_order();
                };
                (void)gstride;
                for (int ph = 0; ph < (dual ? 1 : 2); ph++) {
                    const int hh = dual ? h : ph;
                    const int nstep = max(nv - hh + 1, 0) >> 1;
                    const int nmax = dual ? max(nv + 1, 0) >> 1 : nstep;
                    if (nmax == 0) continue;
                    // grid-row offset of this phase's first row relative to t0
                    // (dual: the chunks carry both halves' rows)
                    const int pb = dual ? 0 : ph;
                    auto sample = [&](int n, const uint32_t (&Pv)[8], const uint32_t (&Cv)[8],
                                      const uint32_t (&Nv)[8]) {
                        const int t = t0 + hh + 2 * n;
                        if (!(col_on && n < nstep)) return;
                        constexpr bool ok = true;
                        const float rp = s_rp[w][t];
                        const float4 wr = s_wr[w][t];
                        const uint32_t a00 = A ? Pv[0] : Pv[4], a02 = A ? Pv[1] : Pv[5];
                        const uint32_t a03 = A ? Pv[2] : Pv[6], a01 = A ? Pv[3] : Pv[7];
                        const uint32_t a30 = A ? Nv[4] : Nv[0], a32 = A ? Nv[5] : Nv[1];
                        const uint32_t a33 = A ? Nv[6] : Nv[2], a31 = A ? Nv[7] : Nv[3];
                        const uint32_t a10 = Cv[0], a11 = Cv[3], a20 = Cv[4], a21 = Cv[7];
                        const int32_t wav1 = (int32_t)((a21 + a00 - a01 - a20) - (a31 + a10 - a11 - a30));
                        const int32_t wav2 = (int32_t)((a31 + a02 - a01 - a32) - (a33 + a00 - a03 - a30));
                        float S[NS];
                        haar_bins(wav1, wav2, s_lut[f2i_rz(rp + cp2)], ok, S);
                        const float wrr[WSZ] = {wr.x, wr.y, wr.z, wr.w};
#pragma unroll
                        for (int R = 0; R < WSZ; R++)
#pragma unroll
                            for (int e = 0; e < NS; e++) acc[R][e] = fmaf(S[e], wrr[R], acc[R][e]);
                    };
                    uint32_t X[8], Y[8], Z[8];
                    // all five row loads in flight before the first LDS
                    // staging (proc's fences would otherwise hold each load
                    // back until the previous rows are staged: three memory
                    // round trips per keypoint before the loop)
                    const Seg q0 = ldseg(pb - 2), q1 = ldseg(pb);
                    Seg s0 = ldseg(pb + 2), s1 = ldseg(pb + 4), s2 = ldseg(pb + 6);
                    proc(q0, X);
                    proc(q1, Y);
                    for (int n = 0; n < nmax; n += 3) {
                        const int tt = pb + 2 * n;
                        proc(s0, Z);
                        s0 = ldseg(tt + 8);
                        sample(n, X, Y, Z);
                        proc(s1, X);
                        s1 = ldseg(tt + 10);
                        sample(n + 1, Y, Z, X);
                        proc(s2, Y);
                        s2 = ldseg(tt + 12);
                        sample(n + 2, Z, X, Y);
                    }
                }
            };
            if (seg) {
                if (hmode == 0) rows_seg(std::integral_constant<bool, true>());
                else rows_seg(std::integral_constant<bool, false>());
            } else {
                if (hmode == 0) rows(std::integral_constant<bool, true>());
                else rows(std::integral_constant<bool, false>());
            }
        } else {
            // ---- generic (hs = 2 step + 1 at exact half-way scales): 12
            // gathers per sample
            for (int k = h; k < nv; k += rstep) {
                if (col_on) {
                    const int rb = (iy + (t0 + k - iradius) * step) * ip4;
                    const int q0 = rb + dR0, q2 = rb + ip4, q3 = rb + dR3;
                    accum(bld(rsrc, q0 + oA), bld(rsrc, q0 + oB), bld(rsrc, q0 + oC), bld(rsrc, q0 + oC + 4),
                          bld(rsrc, rb + oA), bld(rsrc, rb + oB), bld(rsrc, q2 + oA), bld(rsrc, q2 + oB),
                          bld(rsrc, q3 + oA), bld(rsrc, q3 + oB), bld(rsrc, q3 + oC), bld(rsrc, q3 + oC + 4),
                          t0 + k);
                }
            }
        }
        // ---- per-lane bins, then the fixed-order column reduction
#pragma unroll
        for (int R = 0; R < WSZ; R++)
#pragma unroll
            for (int q = 0; q < NB / 2; q++) {
                red[w][lane][R * NB + 2 * q] = acc[R][2 * q + 1];                    // negative part
                red[w][lane][R * NB + 2 * q + 1] = acc[R][2 * q] - acc[R][2 * q + 1];
            }
        s_cf[w][lane] = cfrac;
        // The lanes of one cell column (ci == C) are one contiguous run per
        // half (cx and the image-bounds test are monotonic in j); the run's
        // [lo, hi) per half goes to s_run[C + 1] = {lo0, hi0, lo1, hi1}.
#pragma unroll
        for (int C = -1; C < WSZ; C++) {
            const unsigned long long mc = __ballot(col_on && ci == C);
            const uint32_t mlo = (uint32_t)mc, mhi = (uint32_t)(mc >> 32);
            if (lane == 0)
                s_run[w][C + 1] = make_int4(mlo ? __builtin_ctz(mlo) : 0, mlo ? 32 - __builtin_clz(mlo) : 0,
                                            mhi ? 32 + __builtin_ctz(mhi) : 32, mhi ? 64 - __builtin_clz(mhi) : 32);
        }
        wave_sync();
        float v[NF / 64];
#pragma unroll
        for (int hh = 0; hh < NF / 64; hh++) {
            const int o = lane + 64 * hh;                 // (R * WSZ + C) * NB + b
            const int b = o % NB, C = (o / NB) % WSZ, R = o / (NB * WSZ);
            const int col = R * NB + b;
            float s = 0.f;
            // cell column C: its own lanes at weight 1 - cfrac, then the lanes
            // of column C - 1 at cfrac; ascending lanes, 4 reads in flight
            auto run = [&](int lo, int hi, bool own) {
                int k = lo;
                for (; k + 4 <= hi; k += 4) {
                    float r[4], c[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { r[u] = red[w][k + u][col]; c[u] = s_cf[w][k + u]; }
#pragma unroll
                    for (int u = 0; u < 4; u++) s += r[u] * (own ? 1.f - c[u] : c[u]);
                }
                for (; k < hi; k++) {
                    const float c = s_cf[w][k];
                    s += red[w][k][col] * (own ? 1.f - c : c);
                }
            };
            const int4 q0 = s_run[w][C + 1], q1 = s_run[w][C];
            run(q0.x, q0.y, true);
            run(q0.z, q0.w, true);
            run(q1.x, q1.y, false);
            run(q1.z, q1.w, false);
            v[hh] = s;
        }
        wave_sync();
        // ---- normalize (surfd.cu:2447-2493): sequential-addressing tree
        float a = v[0] * v[0];
        if constexpr (NF > 64) a = a + v[NF / 64 - 1] * v[NF / 64 - 1];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) a = a + __shfl_down(a, k, 64);
        const float fac = 1.f / sqrtf(__shfl(a, 0, 64));
        float* out = desc + ((size_t)f * max_pts + kp) * NF;
        out[lane] = v[0] * fac;
        if constexpr (NF > 64) out[lane + 64] = v[NF / 64 - 1] * fac;
    }
}
