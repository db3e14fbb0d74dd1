// surfhip_desc.inc -- the describe stage's shared helpers (Haar wavelets,
// orientation_wave, KpQueue), the generic k_describe and the rotated
// k_describe_rot.  Included by surfhip_kernels.hip; launch_describe is there.

// ======================================================================
// Orientation + descriptor + normalize, one wave (64 lanes) per keypoint,
// 4 keypoints per 256-thread workgroup, grid-strided over all keypoints of
// the batch.  Haar responses are gathered from the integral image (L1/L2);
// descriptor bins accumulate with LDS float atomics (order-free, like the
// reference's global atomics, surfd.cu:1222-1266); the orientation
// histogram is reduced in fixed sample order so `ori` is reproducible.
// ======================================================================

__device__ __forceinline__ int32_t wavelet1(const uint32_t* __restrict__ I, int ip, int x, int y, int size)
{
    return (int32_t)(box(I, ip, x + size, y, x - size, y - size) - box(I, ip, x + size, y + size, x - size, y));
}
__device__ __forceinline__ int32_t wavelet2(const uint32_t* __restrict__ I, int ip, int x, int y, int size)
{
    return (int32_t)(box(I, ip, x + size, y + size, x, y - size) - box(I, ip, x, y + size, x - size, y - size));
}

// dFastAtan2 (surfd.cu:114-126)
__device__ __forceinline__ float fast_atan2(float y, float x)
{
    const float absx = fabsf(x), absy = fabsf(y);
    const float a = fminf(absx, absy) / fmaxf(absx, absy);
    const float s = a * a;
    float r = fmaf(fmaf(fmaf(-0.0464964749f, s, 0.15931422f), s, -0.327622764f), s * a, a);
    r = (absy > absx ? H_PI_F - r : r);
    r = (x < 0 ? (float)(M_PI_D - (double)r) : r);
    r = (y < 0 ? -r : r);
    return r;
}

// Deterministic sin/cos standing in for __sinf/__cosf (surfd.cu:2423-2424);
// identical operation sequence to the oracle's or_sinf/or_cosf.
__device__ __forceinline__ float sincos_poly(float x, int want_cos)
{
    const float q = x * 0.636619772f;
    const float kf = __builtin_rintf(q);
    int k = (int)kf;
    const float r = ((x - kf * 1.5703125f) - kf * 4.837512969970703125e-4f) - kf * 7.54978995489188216e-8f;
    const float z = r * r;
    float ps = -1.9515295891e-4f * z;
    ps = ps + 8.3321608736e-3f;
    ps = ps * z;
    ps = ps - 1.6666654611e-1f;
    ps = ps * z;
    ps = ps * r;
    const float sn = ps + r;
    float pc = 2.443315711809948e-5f * z;
    pc = pc - 1.388731625493765e-3f;
    pc = pc * z;
    pc = pc + 4.166664568298827e-2f;
    pc = pc * z;
    pc = pc * z;
    const float cs = (pc - 0.5f * z) + 1.0f;
    k += want_cos;
    switch (k & 3) {
        case 0: return sn;
        case 1: return cs;
        case 2: return -sn;
        default: return -cs;
    }
}

// x / y as the IEEE quotient, from r = 1 / y (IEEE, once per keypoint): q0 =
// x r, q = q0 + (x - q0 y) r with the remainder exact (fma).  This is the
// correctly rounded x / y whenever the quotient is a normal number (Markstein;
// 0 mismatches in 8.5e8 trials incl. all-ones significands of y); for |x / y|
// below 2^-100 it may differ in the last bits of a value that only ever enters
// rpos + wofs and rpos^2 + cpos^2, where it vanishes.  3 full-rate
// instructions instead of the ~10 of the IEEE division sequence.
__device__ __forceinline__ float div_by(float x, float y, float r)
{
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, y, x), r, q0);
}

// placeInIndex (surfd.cu:1199-1271) into an LDS descriptor.
__device__ __forceinline__ void place(float* d, int wsz, int osz, float mag1, int ori1, float mag2, int ori2,
                                      float rx, float cx)
{
    const int ri = f2i_rz(rx >= 0.f ? rx : rx - 1.f);
    const int ci = f2i_rz(cx >= 0.f ? cx : cx - 1.f);
    const float rfrac = rx - (float)ri;
    const float cfrac = cx - (float)ci;
    const float cfrac1 = 1 - cfrac;
    if (ri >= 0) {
        const float rw1 = mag1 * (1.f - rfrac), rw2 = mag2 * (1.f - rfrac);
        if (ci >= 0) {
            const int o0 = ri * wsz * osz + ci * osz;
            atomicAdd(&d[o0 + ori1], rw1 * cfrac1);
            atomicAdd(&d[o0 + ori2], rw2 * cfrac1);
        }
        if (ci + 1 < wsz) {
            const int o0 = ri * wsz * osz + (ci + 1) * osz;
            atomicAdd(&d[o0 + ori1], rw1 * cfrac);
            atomicAdd(&d[o0 + ori2], rw2 * cfrac);
        }
    }
    if (ri + 1 < wsz) {
        const float rw1 = mag1 * rfrac, rw2 = mag2 * rfrac;
        if (ci >= 0) {
            const int o0 = (ri + 1) * wsz * osz + ci * osz;
            atomicAdd(&d[o0 + ori1], rw1 * cfrac1);
            atomicAdd(&d[o0 + ori2], rw2 * cfrac1);
        }
        if (ci + 1 < wsz) {
            const int o0 = (ri + 1) * wsz * osz + (ci + 1) * osz;
            atomicAdd(&d[o0 + ori1], rw1 * cfrac);
            atomicAdd(&d[o0 + ori2], rw2 * cfrac);
        }
    }
}


struct OriScratch {
    uint64_t bmask[6][72];          // per 64-sample chunk and bin: member samples (bit = t % 64)
    float2 ap[361];                 // (angle, weighted magnitude) per sample: one ds_read_b64
    int   hist[72];
    float avg[72];
    float part[72];
    float pas[84];
    float ws[72];
    float was[72];
};

// assignOrientationApprox (surfd.cu:1711-1960) for one keypoint on one wave.
// lut1: the orientation weights (lookup1, c_tab.lut1 or an LDS copy of it)
__device__ float orientation_wave(const uint32_t* __restrict__ I, const FrameParams& P, const surfhip_point& p,
                                  OriScratch& S, unsigned lane, const float* lut1 = c_tab.lut1)
{
    const int ip = P.ip;
    const DescAt at = ori_at(P.doubled, p);
    const float scale = at.scale;
    const int pixsi = f2i_rz(2.f * scale + 1.6f);
    const int pixsi2 = f2i_rz(scale + 0.8f);
    const int ixo = f2i_rn(at.x), iyo = f2i_rn(at.y);
    for (int t = lane; t < 6 * 72; t += 64) (&S.bmask[0][0])[t] = 0ull;
    wave_sync();
    for (int t = lane; t < 361; t += 64) {
        const int y1 = t / 19 - 9, x1 = t % 19 - 9;
        const int xx = ixo + x1 * pixsi2, yy = iyo + y1 * pixsi2;
        int hid = -1;
        float angle = 0.f, psum = 0.f;
        if (yy + pixsi + 2 < P.iH && yy - pixsi > -1 && xx + pixsi + 2 < P.W + 1 && xx - pixsi > -1) {
            const int distsq = y1 * y1 + x1 * x1;
            if ((float)distsq < 81.5f) {
                const float dx = (float)wavelet2(I, ip, xx, yy, pixsi) * INV255;
                const float dy = (float)wavelet1(I, ip, xx, yy, pixsi) * INV255;
                const float mag = sqrtf(dx * dx + dy * dy);
                if (mag > 0.f) {
                    angle = fast_atan2(dy, dx);
                    hid = f2i_rz((float)(((double)angle + M_PI_D) / (double)SEP_ANGLE_F)) % 72;
                    psum = lut1[distsq] * mag;
                }
            }
        }
        S.ap[t] = make_float2(angle, psum);
        if (hid >= 0) __hip_atomic_fetch_or(&S.bmask[t >> 6][hid], 1ull << (t & 63), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    wave_sync();
    // per-bin sums in row-major sample order (surfd.cu:1820-1840): a bin's
    // lane walks only its member samples, chunk by chunk, bits ascending
    for (int b = lane; b < 72; b += 64) {
        int cnt = 0;
        float sa = 0.f, sp = 0.f, spa = 0.f, swrap = 0.f;
        for (int c = 0; c < 6; c++) {
            uint64_t m = S.bmask[c][b];
            while (m) {
                const int t = 64 * c + (int)__builtin_ctzll(m);
                m &= m - 1;
                const float2 apt = S.ap[t];
                const float a = apt.x, w = apt.y;
                cnt += 1;
                sa = sa + a;
                sp = sp + w;
                spa = spa + a * w;
                if (b < 6) swrap = swrap + (float)(((double)a + 2 * M_PI_D) * (double)w);
                else if (b >= 66) swrap = swrap + (float)(((double)a - 2 * M_PI_D) * (double)w);
            }
        }
        S.hist[b] = cnt;
        S.avg[b] = cnt > 0 ? sa / (float)cnt : c_tab.bins[b];
        S.part[b] = sp;
        S.pas[b + 6] = spa;
        if (b < 6) S.pas[b + 78] = swrap;
        else if (b >= 66) S.pas[b - 66] = swrap;
    }
    wave_sync();
    for (int i = lane; i < 72; i += 64) {
        float ws = 0.f, was = 0.f;
        for (int j = -6; j <= 6; j++) {
            int k = i + j;
            if (j == -6) {
                float residual;
                if (k < 0) {
                    k += 72;
                    const int k1 = (k + 1) % 72;
                    const float t = (c_tab.bins[k1] + (WINDOW_F / 2)) - S.avg[i];
                    residual = (float)((double)t - (c_tab.bins[k1] < 0 ? 0.0 : 2 * M_PI_D));
                } else {
                    residual = (c_tab.bins[k + 1] + (WINDOW_F / 2)) - S.avg[i];
                }
                const float er = residual / SEP_ANGLE_F;
                ws = ws + er * S.part[k];
                was = was + er * S.pas[i];
            } else if (j == 6) {
                float residual;
                if (k >= 72) {
                    k -= 72;
                    const float t = S.avg[i] + (WINDOW_F / 2);
                    residual = (float)(((double)t - 2 * M_PI_D) - (double)c_tab.bins[k]);
                } else {
                    residual = (S.avg[i] + (WINDOW_F / 2)) - c_tab.bins[k];
                }
                const float er = residual / SEP_ANGLE_F;
                ws = ws + er * S.part[k];
                was = was + er * S.pas[i + 12];
            } else {
                was = was + S.pas[k + 6];
                if (k < 0) k += 72;
                else if (k >= 72) k -= 72;
                ws = ws + S.part[k];
            }
        }
        S.ws[i] = ws;
        S.was[i] = was;
    }
    wave_sync();
    // tree argmax in chunks of 64 and 8, strict '<' (surfd.cu:1921-1947):
    // level `stride` updates slots t < stride from t + stride, which that
    // level never writes, so lane-parallel shuffles give the serial result
    float w64 = S.ws[lane], a64 = S.was[lane];
    const int l8 = (int)(lane & 7);
    float w8 = S.ws[64 + l8], a8 = S.was[64 + l8];
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const float wo = __shfl_down(w64, stride, 64), ao = __shfl_down(a64, stride, 64);
        if ((int)lane < stride && w64 < wo) { w64 = wo; a64 = ao; }
    }
#pragma unroll
    for (int stride = 4; stride > 0; stride >>= 1) {
        const float wo = __shfl_down(w8, stride, 64), ao = __shfl_down(a8, stride, 64);
        if ((int)lane < stride && w8 < wo) { w8 = wo; a8 = ao; }
    }
    float w0 = __shfl(w64, 0, 64), a0 = __shfl(a64, 0, 64);
    const float w1 = __shfl(w8, 0, 64), a1 = __shfl(a8, 0, 64);
    if (w0 < w1) { w0 = w1; a0 = a1; }
    wave_sync();
    return a0 / w0;
}

// XCD-aware keypoint queues for the describe kernels: the workgroups of one
// XCD (blockIdx % 8) take one contiguous eighth of the batch's keypoints (a
// few whole frames, each in the band order k_sort writes), one keypoint per
// grab, so the keypoints in flight on an XCD are consecutive -- a band of a
// frame whose integral-image rows stay in that XCD's L2 (measured on
// k_describe_ur: L2 hit rate 16 % -> 91 %).  The eighth is dealt round-robin
// over kDescQ counters (keypoint gbeg + kDescQ g + q), each on its own 256-B
// line: one same-address atomic per keypoint serialises an XCD at ~50
// cycles a grab.
struct KpQueue {
    int gbeg, gend, qi;
    int* ctr;
    __device__ KpQueue(int total, int* queue, int w)
    {
        const int xcd = blockIdx.x & 7;
        const int chunk = (total + 7) >> 3;
        gbeg = xcd * chunk;
        gend = min(total, gbeg + chunk);
        qi = ((blockIdx.x >> 3) * 4 + w) % kDescQ;
        ctr = queue + (xcd * kDescQ + qi) * 64;
    }
    // the next keypoint (batch index, ascending per wave); >= gend: done
    __device__ int grab(int lane)
    {
        int g = 0;
        if (lane == 0) g = atomicAdd(ctr, 1);
        return gbeg + kDescQ * __builtin_amdgcn_readfirstlane(g) + qi;
    }
    // grab() in two halves: issue the atomic, use its result later
    __device__ int issue(int lane)
    {
        int g = 0;
        if (lane == 0) g = atomicAdd(ctr, 1);
        return g;
    }
    __device__ int finish(int g) { return gbeg + kDescQ * __builtin_amdgcn_readfirstlane(g) + qi; }
};

template <bool UPRIGHT, int MAXF>
__global__ __launch_bounds__(256) void k_describe(const int32_t* __restrict__ ii, FrameParams P,
                                                  surfhip_point* __restrict__ pts, int max_pts,
                                                  const int* __restrict__ counts, const int* __restrict__ offsets,
                                                  const int* __restrict__ order, int nframes, float* __restrict__ desc,
                                                  int* __restrict__ queue)
{
    // four copies of the descriptor per wave (copy = lane & 3, MAXF + 4
    // floats apart so that one bin's copies sit in different banks):
    // neighbouring samples, which mostly hit the same cell and bin, no longer
    // serialise on one LDS address; the copies are summed before
    // normalisation.  MAXF: 128, or 512 for windows past 4 x 4 x 8.
    constexpr int DSTR = MAXF + 4;
    constexpr int NV = MAXF / 64;                // outputs per lane
    __shared__ float sdesc[4][4 * DSTR];
    __shared__ OriScratch sori[UPRIGHT ? 1 : 4];
    const unsigned lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int total = offsets[nframes];
    const int nf = P.nfeat, wsz = P.wsz, osz = P.osz;
    const float fw = (float)wsz;
    const float wofs = (float)wsz * 0.5f - 0.5f;
    float* const d0 = sdesc[w];
    float* d = d0 + (lane & 3) * DSTR;
    KpQueue kq(total, queue, w);
    for (int g = kq.grab((int)lane); g < kq.gend; g = kq.grab((int)lane)) {
        int lo = 0, hi = nframes;            // offsets[lo] <= g < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const int f = lo, i = order[(size_t)lo * max_pts + (g - offsets[lo])];
        surfhip_point* pp = pts + (size_t)f * max_pts + i;
        const surfhip_point p = *pp;
        const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
        const int ip = P.ip;
        float ori = 0.f;
        if constexpr (!UPRIGHT) {
            ori = orientation_wave(I, P, p, sori[w], lane);
            if (lane == 0) pp->ori = ori;
        }
        for (int t = lane; t < 4 * DSTR; t += 64) d0[t] = 0.f;
        wave_sync();
        const DescAt at = desc_at(P.doubled, p);
        const float scale = at.scale;
        const int step = max(f2i_rn(scale * 0.5f), 1);
        const int ix = f2i_rn(at.x), iy = f2i_rn(at.y);
        const float spacing = scale * (float)P.mag;
        const float rspacing = 1.f / spacing;
        const int hs = f2i_rz(scale);
        const int rlim = P.iH - 1 - hs, clim = P.W - hs;   // whps[1].y-1-s, whps[1].x-1-s
        if constexpr (UPRIGHT) {
            const float dx0 = at.x - (float)ix, dy0 = at.y - (float)iy;
            const int iradius = f2i_rn(((spacing * (float)(wsz + 1)) * 0.5f) / (float)step);
            const int side = 2 * iradius + 1;
            const int nsamp = side * side;
            for (int t = lane; t < nsamp; t += 64) {
                const int si = t / side - iradius, sj = t % side - iradius;
                const float rpos = div_by((float)(step * si) - dy0, spacing, rspacing);
                const float cpos = div_by((float)(step * sj) - dx0, spacing, rspacing);
                const float rx = rpos + wofs, cx = cpos + wofs;
                if (!(rx > -1.f && rx < fw && cx > -1.f && cx < fw)) continue;
                const int r = iy + si * step, c = ix + sj * step;
                if (!(r >= 1 + hs && r < rlim && c >= 1 + hs && c < clim)) continue;
                const float weight = c_tab.lut2[f2i_rz(rpos * rpos + cpos * cpos)];
                const float dx = (weight * (float)wavelet2(I, ip, c, r, hs)) * INV255;
                const float dy = (weight * (float)wavelet1(I, ip, c, r, hs)) * INV255;
                if (!P.extend) {
                    place(d, wsz, osz, dx, (dx < 0 ? 0 : 1), dy, (dy < 0 ? 2 : 3), rx, cx);
                } else {
                    place(d, wsz, osz, dx, (dy < 0 ? 0 : 1), fabsf(dx), (dy < 0 ? 2 : 3), rx, cx);
                    place(d, wsz, osz, dy, (dx < 0 ? 4 : 5), fabsf(dy), (dx < 0 ? 6 : 7), rx, cx);
                }
            }
        } else {
            const float fracx = at.x - (float)ix, fracy = at.y - (float)iy;
            const float sine = sincos_poly(ori, 0), cose = sincos_poly(ori, 1);
            const float fracc = ((-sine) * fracy) + (cose * fracx);
            const float fracr = (cose * fracy) + (sine * fracx);
            const int iradius = f2i_rn((((1.4f * spacing) * (float)(wsz + 1)) * 0.5f) / (float)step);
            const int side = 2 * iradius + 1;
            const int nsamp = side * side;
            const float fstep = (float)step;
            for (int t = lane; t < nsamp; t += 64) {
                const int si = t / side - iradius, sj = t % side - iradius;
                const float fi = (float)si, fj = (float)sj;
                const float rpos = div_by((fstep * ((cose * fi) + (sine * fj))) - fracr, spacing, rspacing);
                const float cpos = div_by((fstep * (((-sine) * fi) + (cose * fj))) - fracc, spacing, rspacing);
                const float rx = rpos + wofs, cx = cpos + wofs;
                if (!(rx > -1.f && rx < fw && cx > -1.f && cx < fw)) continue;
                const int r = iy + si * step, c = ix + sj * step;
                if (!(r >= 1 + hs && r < rlim && c >= 1 + hs && c < clim)) continue;
                const float weight = c_tab.lut2[f2i_rz(rpos * rpos + cpos * cpos)];
                const float dxx = (weight * (float)wavelet2(I, ip, c, r, hs)) * INV255;
                const float dyy = (weight * (float)wavelet1(I, ip, c, r, hs)) * INV255;
                const float dx = (cose * dxx) + (sine * dyy);
                const float dy = (sine * dxx) - (cose * dyy);
                if (!P.extend) {
                    place(d, wsz, osz, dx, (dx < 0 ? 0 : 1), dy, (dy < 0 ? 2 : 3), rx, cx);
                } else {
                    place(d, wsz, osz, dx, (dy < 0 ? 0 : 1), fabsf(dx), (dy < 0 ? 2 : 3), rx, cx);
                    place(d, wsz, osz, dy, (dx < 0 ? 4 : 5), fabsf(dy), (dx < 0 ? 6 : 7), rx, cx);
                }
            }
        }
        wave_sync();
        // normalize (surfd.cu:2447-2493): the squares zero-padded to P =
        // max(64, pow2 >= nf) in the sequential-addressing tree: strides P/2
        // .. 64 fold lane + 64 m (m < P / 64) pairwise, then 32 .. 1 across
        // the lanes (for nf = 64 / 128 exactly the reference's order)
        auto sum4 = [&](int b) { return ((d0[b] + d0[DSTR + b]) + d0[2 * DSTR + b]) + d0[3 * DSTR + b]; };
        float v[NV], a2[NV];
#pragma unroll
        for (int m = 0; m < NV; m++) {
            v[m] = (int)lane + 64 * m < nf ? sum4((int)lane + 64 * m) : 0.f;
            a2[m] = v[m] * v[m];
        }
        int np = 1;                                  // P / 64
        while (64 * np < nf) np <<= 1;
#pragma unroll
        for (int half = NV / 2; half >= 1; half >>= 1)
            if (half < np)
#pragma unroll
                for (int m = 0; m < half; m++) a2[m] = a2[m] + a2[m + half];
        float a = a2[0];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) a = a + __shfl_down(a, k, 64);
        const float tot = __shfl(a, 0, 64);
        const float fac = 1.f / sqrtf(tot);
        float* out = desc + ((size_t)f * max_pts + i) * nf;
#pragma unroll
        for (int m = 0; m < NV; m++)
            if ((int)lane + 64 * m < nf) out[lane + 64 * m] = v[m] * fac;
        wave_sync();
    }
}

// ----------------------------------------------------------------------
// Rotated descriptor without atomics (wsz = 4; 64-D or 128-D extended).
// The rotated window's sample grid (surfd.cu:2391-2444) is not separable,
// but each sample adds only into the 2 x 2 cells at its floor cell (ri, ci)
// (placeInIndex, surfd.cu:1199-1271).  So a lane pair owns one floor cell
// of the 5 x 5 set {-1..3}^2: it walks the grid samples inside a
// conservative bounding box of that cell's rotated square (the inverse
// rotation of its corners, one sample of slack), keeps exactly the samples
// whose floor cell -- computed with the reference's float ops -- is its own
// (so every sample is counted once), and accumulates the 4 cells x NB bins
// it can touch in registers.  A fixed-order sum over the (at most 8)
// contributing lanes of each output bin replaces the LDS float atomics,
// so the descriptor is deterministic.  Orientation as k_describe.
// ----------------------------------------------------------------------
struct RotScratch {
    union {
        OriScratch ori;
        float red[64][4 * 8 + 1];   // per lane: 4 relative cells x NB bins (+1 pad)
    };
};

constexpr int kRotWpe = 3;          // 3 waves per SIMD: <= 168 VGPRs (the 128-D form took 185: 2 waves)
template <int NB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kRotWpe))) void k_describe_rot(const int32_t* __restrict__ ii, FrameParams P,
                                                      surfhip_point* __restrict__ pts, int max_pts,
                                                      const int* __restrict__ offsets, const int* __restrict__ order,
                                                      int nframes, float* __restrict__ desc, int* __restrict__ queue)
{
    constexpr int WSZ = 4, NC = WSZ + 1, NF = WSZ * WSZ * NB;
    __shared__ RotScratch sr[4];
    // the Gaussian weight tables in LDS: each sample's weight is one
    // lane-indexed read, from LDS instead of a global load on the walk's
    // dependency chain (same values)
    __shared__ float s_lut1[83], s_lut2[40];
    for (int t = threadIdx.x; t < 83; t += blockDim.x) s_lut1[t] = c_tab.lut1[t];
    for (int t = threadIdx.x; t < 40; t += blockDim.x) s_lut2[t] = c_tab.lut2[t];
    __syncthreads();
    const float* const lut1 = s_lut1;
    const float* const lut2 = s_lut2;
    const unsigned lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int total = offsets[nframes];
    const float fw = (float)WSZ;
    const float wofs = (float)WSZ * 0.5f - 0.5f;
    // this lane's floor cell (lanes 50..63 own none)
    const int cidx = (int)lane >> 1, half = (int)lane & 1;
    const bool owner = cidx < NC * NC;
    const int cri = owner ? cidx / NC - 1 : -100, cci = owner ? cidx % NC - 1 : -100;
    RotScratch& S = sr[w];
    KpQueue kq(total, queue, w);
    for (int g = kq.grab((int)lane); g < kq.gend; g = kq.grab((int)lane)) {
        int lo = 0, hi = nframes;            // offsets[lo] <= g < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const int f = lo, i = order[(size_t)lo * max_pts + (g - offsets[lo])];
        surfhip_point* pp = pts + (size_t)f * max_pts + i;
        const surfhip_point p = *pp;
        const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
        const int ip = P.ip;
        const float ori = orientation_wave(I, P, p, S.ori, lane, lut1);
        if (lane == 0) pp->ori = ori;

        const DescAt at = desc_at(P.doubled, p);
        const float scale = at.scale;
        const int step = max(f2i_rn(scale * 0.5f), 1);
        const int ix = f2i_rn(at.x), iy = f2i_rn(at.y);
        const float spacing = scale * (float)P.mag;
        const int hs = f2i_rz(scale);
        const int rlim = P.iH - 1 - hs, clim = P.W - hs;
        const float fracx = at.x - (float)ix, fracy = at.y - (float)iy;
        const float sine = sincos_poly(ori, 0), cose = sincos_poly(ori, 1);
        const float fracc = ((-sine) * fracy) + (cose * fracx);
        const float fracr = (cose * fracy) + (sine * fracx);
        const int iradius = f2i_rn((((1.4f * spacing) * (float)(WSZ + 1)) * 0.5f) / (float)step);
        const float fstep = (float)step;
        const float rspacing = 1.f / spacing;
        // grid box of this lane's cell: inverse rotation of its corners
        int i0 = 1, i1 = 0, j0 = 0, j1 = 0;
        if (owner) {
            float mni = 1e30f, mxi = -1e30f, mnj = 1e30f, mxj = -1e30f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float A = ((float)(cri + (k >> 1)) - wofs) * spacing + fracr;
                const float B = ((float)(cci + (k & 1)) - wofs) * spacing + fracc;
                const float fi = (cose * A - sine * B) / fstep, fj = (sine * A + cose * B) / fstep;
                mni = fminf(mni, fi); mxi = fmaxf(mxi, fi);
                mnj = fminf(mnj, fj); mxj = fmaxf(mxj, fj);
            }
            // the integer rows / columns inside the box, widened by kSlackBox
            // (the corners' float error is far below it; membership is the
            // exact test below).  Rounding outwards and a sample more on each
            // side walked 2 empty rows per lane (tools/rot_walk_count.py)
            constexpr float kSlackBox = 0.05f;
            i0 = max(-iradius, (int)ceilf(mni - kSlackBox));
            i1 = min(iradius, (int)floorf(mxi + kSlackBox));
            j0 = max(-iradius, (int)ceilf(mnj - kSlackBox));
            j1 = min(iradius, (int)floorf(mxj + kSlackBox));
            i0 += half;                      // the pair splits the box rows by parity
        }
        // per box row, the sj interval where the cell's two slabs (rx in
        // [cri, cri + 1], cx in [cci, cci + 1]) cross the row, widened by
        // kSlack samples (the inverse's float error is < 1e-2 samples for
        // slopes >= 1e-3; membership itself is the exact test below); a
        // near-zero slope keeps the whole box row
        constexpr float kSlack = 0.05f;
        const float Alo = (((float)cri - wofs) * spacing + fracr) / fstep;
        const float Ahi = (((float)(cri + 1) - wofs) * spacing + fracr) / fstep;
        const float Blo = (((float)cci - wofs) * spacing + fracc) / fstep;
        const float Bhi = (((float)(cci + 1) - wofs) * spacing + fracc) / fstep;
        const bool use_s = fabsf(sine) > 1e-3f, use_c = fabsf(cose) > 1e-3f;
        const float inv_s = use_s ? 1.f / sine : 0.f, inv_c = use_c ? 1.f / cose : 0.f;
        int rlo = 0, rhi = -1;
        auto row_range = [&](int row) {
            const float fi = (float)row;
            float lo = (float)j0, hi = (float)j1;
            if (use_s) {                     // sine * fj in [Alo - cose fi, Ahi - cose fi]
                const float a = (Alo - cose * fi) * inv_s, b = (Ahi - cose * fi) * inv_s;
                lo = fmaxf(lo, fminf(a, b) - kSlack);
                hi = fminf(hi, fmaxf(a, b) + kSlack);
            }
            if (use_c) {                     // cose * fj in [Blo + sine fi, Bhi + sine fi]
                const float a = (Blo + sine * fi) * inv_c, b = (Bhi + sine * fi) * inv_c;
                lo = fmaxf(lo, fminf(a, b) - kSlack);
                hi = fminf(hi, fmaxf(a, b) + kSlack);
            }
            // the integers inside [lo, hi] (already widened by kSlack):
            // rounded outwards, a third of the samples walked were rejected
            // by the membership test (tools/rot_walk_count.py: 1,349 walked
            // for 900 members per keypoint, 925 rounded inwards)
            rlo = (int)ceilf(lo);
            rhi = (int)floorf(hi);
            rlo = max(rlo, j0);
            rhi = min(rhi, j1);
        };
        // relative cells q = 0..3 ({(0,0), (0,1), (1,0), (1,1)} from the floor
        // cell) in pairs: accp[h][b] = {cell 2h, cell 2h + 1} of bin b
        v2f32 accp[2][NB];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int b = 0; b < NB; b++) accp[h][b] = v2f32{0.f, 0.f};
        int si = i0, sj = 0;
        if (si <= i1) { row_range(si); sj = rlo; }
        while (si <= i1) {
            if (sj > rhi) {
                si += 2;
                if (si <= i1) { row_range(si); sj = rlo; }
                continue;
            }
            const int cj = sj++;
            const float fi = (float)si, fj = (float)cj;
            // the IEEE quotient as the reference: rpos^2 + cpos^2 indexes the
            // Gaussian LUT, so one ulp can move a sample to the next weight
            // (x * (1 / spacing) alone broke config #5 parity at 1.3e-3 L2);
            // div_by is exact where it matters
            const float rpos = div_by((fstep * ((cose * fi) + (sine * fj))) - fracr, spacing, rspacing);
            const float cpos = div_by((fstep * (((-sine) * fi) + (cose * fj))) - fracc, spacing, rspacing);
            const float rx = rpos + wofs, cx = cpos + wofs;
            if (!(rx > -1.f && rx < fw && cx > -1.f && cx < fw)) continue;
            const int ri = f2i_rz(rx >= 0.f ? rx : rx - 1.f);
            const int ci = f2i_rz(cx >= 0.f ? cx : cx - 1.f);
            if (ri != cri || ci != cci) continue;
            const int r = iy + si * step, c = ix + cj * step;
            if (!(r >= 1 + hs && r < rlim && c >= 1 + hs && c < clim)) continue;
            const float weight = lut2[f2i_rz(rpos * rpos + cpos * cpos)];
            const float dxx = (weight * (float)wavelet2(I, ip, c, r, hs)) * INV255;
            const float dyy = (weight * (float)wavelet1(I, ip, c, r, hs)) * INV255;
            const float dx = (cose * dxx) + (sine * dyy);
            const float dy = (sine * dxx) - (cose * dyy);
            const float rfrac = rx - (float)ri, cfrac = cx - (float)ci;
            const float cfrac1 = 1 - cfrac;
            const float rfrac1 = 1.f - rfrac;
            const v2f32 cw = {cfrac1, cfrac};
            // placeInIndex products (surfd.cu:1222-1266): cell weight by row,
            // then column -- {r0, r0} * {cfrac1, cfrac} is the reference's two
            // products of row ri in one packed multiply.  One placeInIndex
            // value goes to bin BN when `neg`, else BP (both static): a packed
            // FMA by 1 or 0 adds it exactly (v * 1 + acc rounds once, as acc +
            // v; v * 0 + acc = acc), 4 packed FMAs for the 4 cells x 2 bins
            // instead of 8 selects and 8 adds (the kernel's time did not move:
            // it waits on its gathers, DESIGN.md 6)
            auto put = [&](auto bn, auto bp, float mag, bool neg) {
                constexpr int BN = decltype(bn)::value, BP = decltype(bp)::value;
                const float r0 = mag * rfrac1, r1 = mag * rfrac;
                const v2f32 v01 = v2f32{r0, r0} * cw, v23 = v2f32{r1, r1} * cw;
                const float mn = neg ? 1.f : 0.f, mp = neg ? 0.f : 1.f;
                const v2f32 n2 = {mn, mn}, p2 = {mp, mp};
                accp[0][BN] = __builtin_elementwise_fma(v01, n2, accp[0][BN]);
                accp[1][BN] = __builtin_elementwise_fma(v23, n2, accp[1][BN]);
                accp[0][BP] = __builtin_elementwise_fma(v01, p2, accp[0][BP]);
                accp[1][BP] = __builtin_elementwise_fma(v23, p2, accp[1][BP]);
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            using I3 = std::integral_constant<int, 3>;
            if constexpr (NB == 4) {
                put(I0{}, I1{}, dx, dx < 0);
                put(I2{}, I3{}, dy, dy < 0);
            } else {
                using I4 = std::integral_constant<int, 4>;
                using I5 = std::integral_constant<int, 5>;
                using I6 = std::integral_constant<int, 6>;
                using I7 = std::integral_constant<int, 7>;
                put(I0{}, I1{}, dx, dy < 0);
                put(I2{}, I3{}, fabsf(dx), dy < 0);
                put(I4{}, I5{}, dy, dx < 0);
                put(I6{}, I7{}, fabsf(dy), dx < 0);
            }
        }
        wave_sync();                          // orientation scratch is dead: reuse it
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < NB; b++) S.red[lane][q * NB + b] = (q & 1) ? accp[q >> 1][b].y : accp[q >> 1][b].x;
        wave_sync();
        // output bin (R, C, b): floor cells (R, C), (R, C-1), (R-1, C), (R-1, C-1)
        // via relative cells 0..3, each by its two lanes, in that fixed order
        float vout[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int o = (int)lane + 64 * h;
            float a = 0.f;
            if (o < NF) {
                const int cell = o / NB, b = o % NB, R = cell / WSZ, C = cell % WSZ;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int fr = R - (q >> 1), fc = C - (q & 1);      // floor cell of the contributors
                    const int fl = ((fr + 1) * NC + (fc + 1)) * 2;
                    a = a + S.red[fl][q * NB + b];
                    a = a + S.red[fl + 1][q * NB + b];
                }
            }
            vout[h] = a;
        }
        // normalize (surfd.cu:2447-2493)
        float a2 = vout[0] * vout[0];
        if (NF > 64) a2 = a2 + vout[1] * vout[1];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) a2 = a2 + __shfl_down(a2, k, 64);
        const float tot = __shfl(a2, 0, 64);
        const float fac = 1.f / sqrtf(tot);
        float* out = desc + ((size_t)f * max_pts + i) * NF;
        out[lane] = vout[0] * fac;
        if (NF > 64) out[lane + 64] = vout[1] * fac;
        wave_sync();
    }
}
