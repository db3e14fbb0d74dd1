// surfhip_integral.inc -- the integral image in three passes over row bands
// (k_ii_bandsum, k_ii_bandscan, k_ii_fill / k_ii_fill_w; launch_bandscan,
// launch_integral).  Included by surfhip_kernels.hip.

// ======================================================================
// Integral image.  Three passes over row bands of kBandRows rows:
//  (A) k_ii_bandsum : per band, per column, the sum of the band's pixels
//  (B) k_ii_bandscan: exclusive prefix over bands -> column sums above band
//  (C) k_ii_fill    : the band's first integral row is the exclusive row
//      scan of (B); each further row adds the exclusive row scan of the
//      pixels.  u8 is read twice, the int32 image written once.
// Semantics of integralRow/integralCol (surfd.cu:129-165): ii[y+1][x+1] is
// the sum over rows <= y, cols <= x; row 0 / col 0 are 0 (written here).
// uint32 arithmetic wraps exactly like the reference's int adds.
// ======================================================================

template <int CPT>
__device__ __forceinline__ void load_px(const uint8_t* row, int x0, int W, uint32_t (&px)[CPT])
{
    if constexpr (CPT == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(row + x0);
        const uint32_t w[2] = {v.x, v.y};
#pragma unroll
        for (int k = 0; k < 8; k++) px[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    } else if constexpr (CPT == 32) {
        const uint4 a = *reinterpret_cast<const uint4*>(row + x0);
        // the second half only where it holds frame columns: the caller's
        // pitch is a multiple of 16, not of 32, so x0 + 16 >= W may lie past
        // the row (and past the buffer on the last row)
        const uint4 b = (x0 + 16 < W) ? *reinterpret_cast<const uint4*>(row + x0 + 16) : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 32; k++) px[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    }
#pragma unroll
    for (int k = 0; k < CPT; k++)
        if (x0 + k >= W) px[k] = 0u;
}

template <int CPT>
__global__ __launch_bounds__(256) void k_ii_bandsum(const uint8_t* __restrict__ frames, int pitch,
                                                    long long fstride, int W, int H, int nbands,
                                                    uint32_t* __restrict__ colsum, int CW, int br)
{
    const int band = blockIdx.x, f = blockIdx.y;
    const int x0 = threadIdx.x * CPT;
    if (x0 >= W) return;
    const int y0 = band * br;
    const int rows = min(br, H - y0);
    const uint8_t* src = frames + (size_t)f * fstride + (size_t)y0 * pitch;
    uint32_t acc[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) acc[k] = 0u;
    // 8 rows' loads in flight per iteration (rows past the band re-read the
    // band's last row and are not added)
    for (int r0 = 0; r0 < rows; r0 += 8) {
        uint32_t px[8][CPT];
#pragma unroll
        for (int d = 0; d < 8; d++) load_px<CPT>(src + (size_t)min(r0 + d, rows - 1) * pitch, x0, W, px[d]);
#pragma unroll
        for (int d = 0; d < 8; d++)
            if (r0 + d < rows) {
#pragma unroll
                for (int k = 0; k < CPT; k++) acc[k] += px[d][k];
            }
    }
    uint32_t* dst = colsum + ((size_t)f * nbands + band) * CW + x0;
#pragma unroll
    for (int k = 0; k < CPT; k += 4)
        *reinterpret_cast<uint4*>(dst + k) = make_uint4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
}

template <int CH>
__global__ __launch_bounds__(256) void k_ii_bandscan(uint32_t* __restrict__ colsum, int nbands, int CW, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (x >= W) return;
    uint32_t* c = colsum + (size_t)f * nbands * CW + x;
    uint32_t run = 0u;
    // CH bands' loads in flight per chunk (one memory latency per chunk, not
    // per band): 48 for the 32-row bands of a batch, 136 for the 8-row bands
    // of a single 1080p frame (135 bands: 9 round trips at 16, 12 us,
    // profiles/r05ac2_kernel_stats.csv)
    for (int b0 = 0; b0 < nbands; b0 += CH) {
        uint32_t v[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) v[k] = (b0 + k < nbands) ? c[(size_t)(b0 + k) * CW] : 0u;
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (b0 + k < nbands) {
                c[(size_t)(b0 + k) * CW] = run;
                run += v[k];
            }
    }
}

// Exclusive scan across the 256-thread block of CPT consecutive values per
// thread (wave64 shuffle scan + LDS exchange of the 4 wave totals).
template <int CPT>
__device__ __forceinline__ void block_excl_scan(uint32_t (&v)[CPT], uint32_t* lds4)
{
    uint32_t run = 0u;
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const uint32_t t = v[k];
        v[k] = run;
        run += t;
    }
    const unsigned lane = lane_id();
    const int wave = threadIdx.x >> 6;
    uint32_t inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (unsigned)d) inc += n;
    }
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    uint32_t base = inc - run;
    for (int w = 0; w < wave; w++) base += lds4[w];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; k++) v[k] += base;
}

template <int CPT>
__global__ __launch_bounds__(256) void k_ii_fill(const uint8_t* __restrict__ frames, int pitch,
                                                 long long fstride, int W, int H, int nbands,
                                                 const uint32_t* __restrict__ colpre, int CW,
                                                 int32_t* __restrict__ ii, int ip, long long istride, int br)
{
    __shared__ uint32_t lds4[4];
    const int band = blockIdx.x, f = blockIdx.y;
    const int x0 = threadIdx.x * CPT;
    const bool active = x0 <= W;               // thread owns integral columns x0..x0+CPT-1
    const int y0 = band * br;
    const int rows = min(br, H - y0);
    uint32_t acc[CPT];
    {
        const uint32_t* c = colpre + ((size_t)f * nbands + band) * CW;
#pragma unroll
        for (int k = 0; k < CPT; k++) acc[k] = (x0 + k < W) ? c[x0 + k] : 0u;
    }
    block_excl_scan<CPT>(acc, lds4);           // acc = ii[y0][x0 + k]
    uint32_t* out = reinterpret_cast<uint32_t*>(ii) + (size_t)f * istride;
    if (band == 0 && active) {
#pragma unroll
        for (int k = 0; k < CPT; k += 4)
            *reinterpret_cast<uint4*>(out + x0 + k) = make_uint4(0u, 0u, 0u, 0u);
    }
    const uint8_t* src = frames + (size_t)f * fstride + (size_t)y0 * pitch;
    for (int r = 0; r < rows; r++) {
        uint32_t px[CPT];
        if (x0 < W) load_px<CPT>(src + (size_t)r * pitch, x0, W, px);
        else {
#pragma unroll
            for (int k = 0; k < CPT; k++) px[k] = 0u;
        }
        block_excl_scan<CPT>(px, lds4);
#pragma unroll
        for (int k = 0; k < CPT; k++) acc[k] += px[k];
        if (active) {
            // pad columns (> W) stay zero: the flat reads of getTrace can
            // land on them (see trace_sign)
            uint32_t o[CPT];
#pragma unroll
            for (int k = 0; k < CPT; k++) o[k] = (x0 + k <= W) ? acc[k] : 0u;
            uint32_t* dst = out + (size_t)(y0 + r + 1) * ip + x0;
#pragma unroll
            for (int k = 0; k < CPT; k += 4)
                *reinterpret_cast<uint4*>(dst + k) = make_uint4(o[k], o[k + 1], o[k + 2], o[k + 3]);
        }
    }
}

// Pass (C) with one wave per band and no barriers: lane l owns columns
// 4 l + 256 t + j (t < NT, j < 4), so every load is 256 contiguous bytes and
// every store 1 KiB; the row scan is NT wave scans with a running carry.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v)
{
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xf, false);
}
// inclusive scan over the wave's 64 lanes (gfx9 DPP: row shifts, then the
// row_bcast:15 / row_bcast:31 carries) -- six VALU ops, no LDS round trip
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total)
{
    const uint32_t inc = wave_incl_scan(v);
    total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    return inc - v;
}

template <int NT>
__global__ __launch_bounds__(256) void k_ii_fill_w(const uint8_t* __restrict__ frames, int pitch,
                                                   long long fstride, int W, int H, int nbands,
                                                   const uint32_t* __restrict__ colpre, int CW,
                                                   int32_t* __restrict__ ii, int ip, long long istride, int nframes,
                                                   int br)
{
    const int gw = blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = gw / nbands, band = gw - f * nbands;
    if (f >= nframes) return;
    const int lane = (int)lane_id();
    const int y0 = band * br;
    const int rows = min(br, H - y0);
    // acc = ii[y0][x]: exclusive row scan of the column sums above the band
    uint32_t acc[NT][4];
    {
        const uint32_t* c = colpre + ((size_t)f * nbands + band) * CW;
        uint32_t carry = 0u;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int x = 4 * lane + 256 * t;
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (x + j < W) ? c[x + j] : 0u;
            const uint32_t e1 = v[0], e2 = e1 + v[1], e3 = e2 + v[2], tot = e3 + v[3];
            uint32_t wt;
            const uint32_t base = carry + wave_excl_scan(tot, wt);
            carry += wt;
            acc[t][0] = base; acc[t][1] = base + e1; acc[t][2] = base + e2; acc[t][3] = base + e3;
        }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(ii) + (size_t)f * istride;
    if (band == 0) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int x = 4 * lane + 256 * t;
            if (x < ip) *reinterpret_cast<uint4*>(out + x) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const uint8_t* src = frames + (size_t)f * fstride + (size_t)y0 * pitch;
    // the band's pixel rows stream through a ring of kFillAhead rows loaded
    // ahead (the row scan no longer waits a memory latency per row: a single
    // frame's 34 band waves were latency-bound)
    constexpr int kFillAhead = 4;
    uint32_t wq[kFillAhead][NT];
    auto ldrow = [&](int r, uint32_t (&wv)[NT]) {
        const uint8_t* row = src + (size_t)min(r, rows - 1) * pitch;     // past the band: a repeat, unused
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int x = 4 * lane + 256 * t;
            wv[t] = (x + 4 <= pitch) ? *reinterpret_cast<const uint32_t*>(row + x) : 0u;
        }
    };
    static_for<kFillAhead>([&](auto dc) { ldrow(decltype(dc)::value, wq[decltype(dc)::value]); });
    for (int r0 = 0; r0 < rows; r0 += kFillAhead) {
        static_for<kFillAhead>([&](auto dc) {
            constexpr int D = decltype(dc)::value;
            const int r = r0 + D;
            if (r >= rows) return;
            uint32_t wv[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) wv[t] = wq[D][t];
            ldrow(r + kFillAhead, wq[D]);
            uint32_t* dst = out + (size_t)(y0 + r + 1) * ip;
            uint32_t carry = 0u;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int x = 4 * lane + 256 * t;
                uint32_t p[4];
#pragma unroll
                for (int j = 0; j < 4; j++) p[j] = (x + j < W) ? (wv[t] >> (8 * j)) & 0xffu : 0u;
                const uint32_t e1 = p[0], e2 = e1 + p[1], e3 = e2 + p[2], tot = e3 + p[3];
                uint32_t wt;
                const uint32_t base = carry + wave_excl_scan(tot, wt);
                carry += wt;
                acc[t][0] += base; acc[t][1] += base + e1; acc[t][2] += base + e2; acc[t][3] += base + e3;
                // pad columns (> W) stay zero (set once at detector creation and
                // never written: 6 % of the 1080p row): the flat reads of
                // getTrace can land on them
                if (x <= W) {
                    const uint4 o4 = make_uint4(x <= W ? acc[t][0] : 0u, x + 1 <= W ? acc[t][1] : 0u,
                                                x + 2 <= W ? acc[t][2] : 0u, x + 3 <= W ? acc[t][3] : 0u);
                    // nontemporal: the 2.3-GB batch integral streams past the
                    // caches (whole step 5.21 -> 5.19 ms, 3 A/B pairs)
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(u32x4{o4.x, o4.y, o4.z, o4.w}, reinterpret_cast<u32x4*>(dst + x));
                }
            }
        });
    }
}

static void launch_bandscan(uint32_t* colsum, int nbands, int CW, int W, int nframes, hipStream_t s)
{
    if (nbands <= 48) k_ii_bandscan<48><<<dim3((W + 255) / 256, nframes), 256, 0, s>>>(colsum, nbands, CW, W);
    else if (nbands <= 136) k_ii_bandscan<136><<<dim3((W + 255) / 256, nframes), 256, 0, s>>>(colsum, nbands, CW, W);
    else k_ii_bandscan<272><<<dim3((W + 255) / 256, nframes), 256, 0, s>>>(colsum, nbands, CW, W);
}

hipError_t launch_integral(const FrameBatch& b, const FrameParams& P, const Switches& sw, uint32_t* colsum,
                           int32_t* ii, hipStream_t s)
{
    // small batches: 8-row bands (4x the band waves of the fill pass, which
    // is one wave per band) -- colsum is sized for both (integral_bands())
    const int br = b.n <= kSmallBatch ? sw.ii_band_small : sw.ii_band;
    const int nbands = (P.H + br - 1) / br;
    const int W = P.W;
    dim3 grid(nbands, b.n);
    if (W + 1 <= 2048) {
        const int CW = 2048;
        k_ii_bandsum<8><<<grid, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum, CW, br);
        launch_bandscan(colsum, nbands, CW, W, b.n, s);
        k_ii_fill_w<8><<<(nbands * b.n + 3) / 4, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum, CW,
                                                                    ii, P.ip, P.ii_stride, b.n, br);
    } else if (W + 1 <= 4096) {
        const int CW = 4096;
        k_ii_bandsum<16><<<grid, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum, CW, br);
        launch_bandscan(colsum, nbands, CW, W, b.n, s);
        k_ii_fill_w<16><<<(nbands * b.n + 3) / 4, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum,
                                                                     CW, ii, P.ip, P.ii_stride, b.n, br);
    } else if (W + 1 <= 8192) {
        // wide frames (up to 8,191 columns): 32 columns per thread, the
        // workgroup-scan fill (one 256-thread block per band, two barriers a row)
        const int CW = 8192;
        k_ii_bandsum<32><<<grid, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum, CW, br);
        launch_bandscan(colsum, nbands, CW, W, b.n, s);
        k_ii_fill<32><<<grid, 256, 0, s>>>(b.frames, b.pitch, b.stride, W, P.H, nbands, colsum, CW, ii, P.ip,
                                           P.ii_stride, br);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
