// surfhip_nms.inc -- scale-space NMS, interpolation and makePoint: OctView,
// k_nms_scan, the exclusive scan (k_scan_local / k_scan_top / k_scan_add),
// k_nms_fit; launch_nms.  Included by surfhip_kernels.hip.

// ======================================================================
// Scale-space NMS + interpolation + makePoint (findMaximumWithInterp,
// surfd.cu:676-832; fitQuadrat 942-988; solveLinearSystem 835-887;
// makePoint 1001-1022).  One thread per 2x2 block of one NMS level.
// Survivors are compacted per wave (ballot + one atomic per wave) into the
// frame's candidate buffer with a canonical key (octave, level, row, col);
// k_sort restores that order, so the output is deterministic.
// ======================================================================

__device__ void solve3(float* sol, float (&sq)[3][3])
{
    int row, col, c, pivot = 0, i;
    float maxc, coef, temp, mult, val;
    for (col = 0; col < 2; col++) {
        maxc = -1.f;
        for (row = col; row < 3; row++) {
            coef = sq[row][col];
            coef = (coef < 0.f ? -coef : coef);
            if (coef > maxc) { maxc = coef; pivot = row; }
        }
        if (pivot != col) {
            for (i = 0; i < 3; i++) { temp = sq[pivot][i]; sq[pivot][i] = sq[col][i]; sq[col][i] = temp; }
            temp = sol[pivot]; sol[pivot] = sol[col]; sol[col] = temp;
        }
        for (row = col + 1; row < 3; row++) {
            mult = sq[row][col] / sq[col][col];
            for (c = col; c < 3; c++) sq[row][c] = sq[row][c] - mult * sq[col][c];
            sol[row] = sol[row] - mult * sol[col];
        }
    }
    for (row = 2; row >= 0; row--) {
        val = sol[row];
        for (col = 2; col > row; col--) val = val - sol[col] * sq[row][col];
        sol[row] = val / sq[row][row];
    }
}

// Response planes of one octave as the reference lays them out after its
// halfImage copies: planes 0/1 of octave o > 0 are read in place from octave
// o-1's planes 2/4 at (2r, 2c), which is exactly what halfImage copied.
struct OctView {
    const float* F;                 // the frame's response block
    int cur;                        // float offset of this octave's plane 0
    int sp, osize;
    int half;                       // octave > 0: planes 0 / 1 are the halfImage views
    // plane 0's view and plane 1's differences from it (a select against a
    // constant: selecting between two fields became a select of their
    // addresses and put the view in scratch)
    int hb, hr, hc, dhb, dhr, dhc;
    // branch-free (selects): a branch around a load makes hipcc wait for the
    // loads issued before it at the join, which serialised the NMS scan's 32
    // block loads into 16 memory round trips
    __device__ __forceinline__ int off(int s, int r, int c) const
    {
        const bool h = half && s < 2;
        const bool p1 = s != 0;
        const int base = h ? hb + (p1 ? dhb : 0) : cur + s * osize;
        return base + r * (h ? hr + (p1 ? dhr : 0) : sp) + c * (h ? hc + (p1 ? dhc : 0) : 1);
    }
    __device__ __forceinline__ float operator()(int s, int r, int c) const { return F[off(s, r, c)]; }
    // (s, r, c) and (s, r, c + 1) of a plane that is not a halfImage view:
    // one 8-byte load (4-byte aligned)
    __device__ __forceinline__ void pair_full(int s, int r, int c, float& a, float& b) const
    {
        typedef float f2a4 __attribute__((ext_vector_type(2), aligned(4)));
        const f2a4 v = *reinterpret_cast<const f2a4*>(F + cur + s * osize + r * sp + c);
        a = v.x;
        b = v.y;
    }
    // (s, r, c) and (s, r, c + 1)
    __device__ __forceinline__ void pair(int s, int r, int c, float& a, float& b) const
    {
        const bool h = half && s < 2;
        const int o = off(s, r, c);
        a = F[o];
        b = F[o + (h ? hc + (s != 0 ? dhc : 0) : 1)];
    }
};

// fitQuadrat (surfd.cu:942-988) on the 19 responses it reads around (s, r,
// c): v = {c, s+1, s-1, r+1, r-1, c+1, c-1, (s+1, r+1), (s+1, r-1),
// (s-1, r+1), (s-1, r-1), (s+1, c+1), (s+1, c-1), (s-1, c+1), (s-1, c-1),
// (r+1, c+1), (r+1, c-1), (r-1, c+1), (r-1, c-1)} (the NMS scan writes this
// record for its survivors, k_nms_scan)
__device__ float fit_quad_v(const float* v, float (&off)[3])
{
    const float c0 = v[0];
    const float nx0 = v[1], pv0 = v[2];
    const float cnr = v[3], cpr = v[4], cnc = v[5], cpc = v[6];
    float g[3], H[3][3];
    g[0] = (nx0 - pv0) * 0.5f;
    g[1] = (cnr - cpr) * 0.5f;
    g[2] = (cnc - cpc) * 0.5f;
    const float temp = c0 + c0;
    H[0][0] = (pv0 + nx0) - temp;
    H[1][1] = (cnr + cpr) - temp;
    H[2][2] = (cnc + cpc) - temp;
    H[0][1] = ((v[7] - v[8]) - (v[9] - v[10])) * 0.25f;
    H[0][2] = ((v[11] - v[12]) - (v[13] - v[14])) * 0.25f;
    H[1][2] = ((v[15] - v[16]) - (v[17] - v[18])) * 0.25f;
    H[1][0] = H[0][1];
    H[2][0] = H[0][2];
    H[2][1] = H[1][2];
    off[0] = -g[0];
    off[1] = -g[1];
    off[2] = -g[2];
    solve3(off, H);
    const float dot = (off[0] * g[0] + off[1] * g[1]) + off[2] * g[2];
    return c0 + 0.5f * dot;
}

__device__ float fit_quad(const OctView& V, float (&off)[3], int s, int r, int c)
{
    const float v[19] = {V(s, r, c),
                         V(s + 1, r, c),         V(s - 1, r, c),
                         V(s, r + 1, c),         V(s, r - 1, c),
                         V(s, r, c + 1),         V(s, r, c - 1),
                         V(s + 1, r + 1, c),     V(s + 1, r - 1, c),     V(s - 1, r + 1, c),     V(s - 1, r - 1, c),
                         V(s + 1, r, c + 1),     V(s + 1, r, c - 1),     V(s - 1, r, c + 1),     V(s - 1, r, c - 1),
                         V(s, r + 1, c + 1),     V(s, r + 1, c - 1),     V(s, r - 1, c + 1),     V(s, r - 1, c - 1)};
    return fit_quad_v(v, off);
}

// getTrace (surfd.cu:369-377).  makePoint builds this box from the
// interpolated scale without a bounds check (surfd.cu:1010-1020), so near a
// border a corner can leave [0, W] x [0, H]; the reference then reads the
// flat pitched buffer at that index (column -1 = the previous row's zero
// pad).  Same flat read here; indices outside the frame's buffer read 0.
__device__ __forceinline__ uint32_t flat_at(const uint32_t* __restrict__ I, int idx, int len)
{
    return (idx >= 0 && idx < len) ? I[idx] : 0u;
}
__device__ __forceinline__ uint32_t box_flat(const uint32_t* __restrict__ I, int ip, int len, int x1, int y1,
                                             int x2, int y2)
{
    const int yp1 = (y1 + 1) * ip;
    const int yp2 = y2 * ip;
    return flat_at(I, yp1 + x1 + 1, len) + flat_at(I, yp2 + x2, len) - flat_at(I, yp2 + x1 + 1, len) -
           flat_at(I, yp1 + x2, len);
}
__device__ __forceinline__ int32_t trace_sign(const uint32_t* __restrict__ I, int ip, int len, const int* v)
{
    const int32_t lxx = (int32_t)(box_flat(I, ip, len, v[5] + v[2], v[1] + v[3], v[6] - v[2], v[1] - v[3])
                                  - 3u * box_flat(I, ip, len, v[0] + v[2], v[1] + v[3], v[0] - v[2], v[1] - v[3]));
    const int32_t lyy = (int32_t)(box_flat(I, ip, len, v[0] + v[3], v[7] + v[2], v[0] - v[3], v[8] - v[2])
                                  - 3u * box_flat(I, ip, len, v[0] + v[3], v[1] + v[2], v[0] - v[3], v[1] - v[2]));
    return ((int32_t)((uint32_t)lxx + (uint32_t)lyy) > 0) ? 1 : -1;
}

// Sub-pixel interpolation + acceptance + makePoint (surfd.cu:794-831,
// 942-1022) for one NMS survivor.
// cube: the scan's record of the 19 responses around (s, r, c) (nullptr:
// read them from the planes)
// stash: leave getTrace to k_describe_u2 (choose_describe): laplace holds
// its box centre x0 | y0 << 16 (int16 each: choose_describe keeps frames of
// 32768 integral rows or more off this path) and ori the lobe `temp`, which
// the describe kernel replaces by the sign and 0
__device__ bool nms_fit_point(const uint32_t* __restrict__ I, const OctView& V, const FrameParams& P,
                              const OctaveParams& q, int o, int s, int r, int c, const float4* cube,
                              surfhip_point& pt, bool stash)
{
    const int sw = q.sw, sh = q.sh;
    float off[3] = {0.f, 0.f, 0.f};
    float strength = 0.f;
    int newr = r, newc = c;
    for (int mv = 0; mv < 5; mv++) {
        r = newr; c = newc;
        if (mv == 0 && cube) {
            float v[20];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const float4 t = cube[k];
                v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
            }
            strength = fit_quad_v(v, off);
        } else {
            strength = fit_quad(V, off, s, r, c);
        }
        const int bs = q.borders[s];
        if (off[1] > 0.6f && r < sh - bs) newr++;
        if (off[1] < -0.6f && r > bs) newr--;
        if (off[2] > 0.6f && c < sw - bs) newc++;
        if (off[2] < -0.6f && c > bs) newc--;
        if (newr == r && newc == c) break;
    }
    if (__builtin_isnan(off[0]) || __builtin_isnan(off[1]) || __builtin_isnan(off[2]) ||
        fabsf(off[0]) > 1.5f || fabsf(off[1]) > 1.5f || fabsf(off[2]) > 1.5f || strength < P.thresh)
        return false;

    const int octave = q.octave;
    const float t2 = (((float)s + off[0]) * 2.f) * (float)octave;
    const float ns = ((float)(P.init_lobe + (octave - 1) * P.max_scale) + t2) / 3.f;
    const float ny = (float)octave * ((float)r + off[1]);
    const float nx = (float)octave * ((float)c + off[2]);
    const float temp_delta = (float)P.sampling * P.divisor;
    pt.x = nx * temp_delta;
    pt.y = ny * temp_delta;
    pt.scale = (1.2f * ns) * P.divisor;
    pt.o = o;
    pt.strength = strength;
    pt.ori = 0.f;
    pt.score = 0.f;
    pt.match = -1;
    pt.match_x = 0.f;
    pt.match_y = 0.f;
    pt.ambiguity = 0.f;
    int v[9];
    const int temp = f2i_rz(fmaf(3.f, ns, 0.5f));
    v[0] = f2i_rz(fmaf(nx, (float)P.sampling, 0.5f));
    v[1] = f2i_rz(fmaf(ny, (float)P.sampling, 0.5f));
    v[2] = temp / 2;
    v[3] = v[2] + v[2];
    v[4] = v[2] + v[3];
    v[5] = v[0] + temp;
    v[6] = v[0] - temp;
    v[7] = v[1] + temp;
    v[8] = v[1] - temp;
    if (stash) {
        pt.laplace = (int)(((uint32_t)v[0] & 0xffffu) | ((uint32_t)v[1] << 16));
        pt.ori = __int_as_float(temp);
    } else {
        pt.laplace = trace_sign(I, P.ip, P.iH * P.ip, v);
    }
    return true;
}

__device__ __forceinline__ OctView make_view(const float* F, const OctaveParams& q, int o)
{
    OctView V;
    V.F = F;
    V.cur = (int)q.ooff;
    V.sp = q.sp;
    V.osize = q.osize;
    V.half = o > 0 ? 1 : 0;
    V.hb = (int)q.hbase[0];
    V.dhb = (int)(q.hbase[1] - q.hbase[0]);
    V.hr = q.hrow[0];
    V.dhr = q.hrow[1] - q.hrow[0];
    V.hc = q.hcol[0];
    V.dhc = q.hcol[1] - q.hcol[0];
    return V;
}

// Wave-aggregated append: one atomic per wave for all its `ok` lanes.
__device__ __forceinline__ int wave_append(bool ok, int* counter)
{
    const unsigned long long m = __ballot(ok);
    if (m == 0ull) return -1;
    const int leader = __builtin_ctzll(m);
    int base = 0;
    if ((int)lane_id() == leader) base = atomicAdd(counter, (int)__popcll(m));
    base = __shfl(base, leader, 64);
    return ok ? base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))
              : -1;
}

// Pass 1: the 3x3x3 test for every 2x2x2 block of every octave and both NMS
// levels.  Streams the response planes once; survivors (~1 % of blocks) are
// appended to the frame's scan list with their canonical key (octave, level,
// block row, block col) and argmax (s, r, c).
// One workgroup = 4 waves x (64 block columns x kScanRows/4 block rows) of
// one (frame, octave, level), a wave's rows in passes of 4 whose loads are
// issued one pass ahead; XCD x takes frames x, x + 8, ...
// HK: plane k of this item is a halfImage view (octave > 0, level 1): its
// column pairs are two loads; every other pair is one 8-byte load
template <bool CUBE, bool HK>
__device__ __forceinline__ void nms_scan_item(const float* __restrict__ resp, const FrameParams& P,
                                              const OctaveParams* __restrict__ oct, const LaunchPlan& plan,
                                              uint32_t* __restrict__ scan_key, uint32_t* __restrict__ scan_src,
                                              float* __restrict__ scan_cube,
                                              int* __restrict__ item_count, int nitems_frame, int f, int gb, int wv,
                                              float* sbest, uint32_t* sinfo, float* sblk)
{
    constexpr int NU = 4;                    // block rows per lane per pass
    constexpr int NIT = kScanRows / 4 / NU;  // passes: the next pass's loads are issued first
    const int o = octave_of(plan.nms_start, P.noct, gb);
    const OctaveParams& q = oct[o];
    const int nbx = plan.nms_nbx[o], nby = plan.nms_nby[o];
    int lb = gb - plan.nms_start[o];
    const int z = lb / (nbx * nby);
    lb -= z * nbx * nby;
    const int x = (lb % nbx) * 64 + (int)lane_id();
    const int ybase = (lb / nbx) * kScanRows + wv;     // this wave: rows ybase + 4 u, u < 4 NIT
    const OctView V = make_view(resp + (size_t)f * P.resp_stride, q, o);
    const rsrc_t RF = make_rsrc(resp + (size_t)f * P.resp_stride, (long long)P.resp_stride * 4);
    const int k = 2 * z + 1, mb = q.mb[z];
    const int j = mb + x * 2;
    const int bx0 = (lb % nbx) * 64;
    // survivors go to this wave item's own region (no atomics): kItemCap
    // entries at item * kItemCap, the count in item_count[item]
    const size_t item = ((size_t)f * nitems_frame + gb) * 4 + wv;
    uint32_t* rkey = scan_key + item * kItemCap;
    uint32_t* rsrc_ = scan_src + item * kItemCap;
    float* rcube = scan_cube + item * kCubeCap * kCubeF;
    int nsurv = 0;
    // ---- a pass's 2x2x2 block loads, all issued before any use
    float v[2][NU][8];
    bool in[2][NU];
    auto load = [&](int it, float (&vv)[NU][8], bool (&inn)[NU]) {
#pragma unroll
        for (int u = 0; u < NU; u++) {
            const int y = ybase + 4 * (it * NU + u), i = mb + y * 2;
            inn[u] = x < q.nms_gx && y < q.nms_gy && i < q.sh - mb && j < q.sw - mb;
            const int ii = inn[u] ? i : mb, jj = inn[u] ? j : mb;
            if constexpr (HK) {
                V.pair(k, ii, jj, vv[u][0], vv[u][1]);
                V.pair(k, ii + 1, jj, vv[u][2], vv[u][3]);
            } else {
                V.pair_full(k, ii, jj, vv[u][0], vv[u][1]);
                V.pair_full(k, ii + 1, jj, vv[u][2], vv[u][3]);
            }
            V.pair_full(k + 1, ii, jj, vv[u][4], vv[u][5]);
            V.pair_full(k + 1, ii + 1, jj, vv[u][6], vv[u][7]);
        }
    };
    load(0, v[0], in[0]);
    static_for<NIT>([&](auto itc) {
        constexpr int it = decltype(itc)::value;
        if constexpr (it + 1 < NIT) load(it + 1, v[(it + 1) & 1], in[(it + 1) & 1]);
        const float (&vc)[NU][8] = v[it & 1];
        const bool (&ic)[NU] = in[it & 1];
        const int y0 = ybase + 4 * it * NU;
        // ---- argmax over the 2x2x2 block in the reference's order (k: w,x,y,z;
        // k+1: w,x,y,z), strict '>', threshold and top-scale rejection
        // (surfd.cu:678-756)
        bool cnd[NU];
        float bst[NU];
        int cs[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) {
            int cas = 0;
            float best = vc[u][0];
#pragma unroll
            for (int t = 1; t < 8; t++)
                if (vc[u][t] > best) { best = vc[u][t]; cas = t; }
            cnd[u] = ic[u] && !(best < P.thresh * 0.8f || (k + 1 == P.max_scale - 1 && cas > 3));
            // 4 of the 19 neighbours, (s / si, r / rp, cn), are the adjacent
            // block column of lane -+ 1 (the same block row): a candidate below
            // any of them cannot survive, so it is dropped before the gathers
            // (same result; a lane whose neighbour block lies outside the grid
            // or the wave keeps its candidate for the full test)
            const float ninf = -__builtin_inff();
            const float lmax = ic[u] ? fmaxf(fmaxf(vc[u][0], vc[u][2]), fmaxf(vc[u][4], vc[u][6])) : ninf;
            const float rmax = ic[u] ? fmaxf(fmaxf(vc[u][1], vc[u][3]), fmaxf(vc[u][5], vc[u][7])) : ninf;
            // lane - 1's right column (wave_shr:1) / lane + 1's left column (wave_shl:1)
            const float fromL = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ninf), __float_as_int(rmax),
                                                                           0x138, 0xf, 0xf, false));
            const float fromR = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ninf), __float_as_int(lmax),
                                                                           0x130, 0xf, 0xf, false));
            cnd[u] = cnd[u] && !(best < ((cas & 1) ? fromR : fromL));
            bst[u] = best;
            cs[u] = cas;
        }
        // ---- compact the candidates of the pass's NU rows into dense lanes
        // (LDS), so the 19-neighbour test costs 19 loads per 64 candidates
        unsigned long long m[NU];
        int ncand = 0;
#pragma unroll
        for (int u = 0; u < NU; u++) {
            m[u] = __ballot(cnd[u]);
            if (cnd[u]) {
                const int slot = ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m[u] >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)m[u], 0u));
                sbest[slot] = bst[u];
                sinfo[slot] = ((uint32_t)u << 9) | ((uint32_t)cs[u] << 6) | lane_id();
                // the block's 8 values for the fit record (first 64 candidates)
                if (CUBE && slot < 64) {
                    float4* bd = reinterpret_cast<float4*>(sblk + 8 * slot);
                    bd[0] = make_float4(vc[u][0], vc[u][1], vc[u][2], vc[u][3]);
                    bd[1] = make_float4(vc[u][4], vc[u][5], vc[u][6], vc[u][7]);
                }
            }
            ncand += (int)__popcll(m[u]);
        }
        if (ncand == 0) return;
        wave_sync();
        for (int c0 = 0; c0 < ncand; c0 += 64) {
            const int ci = c0 + (int)lane_id();
            bool ok = false;
            int s = 0, r = 0, c = 0, xx = 0, y = 0, ds = 1, dr = 1, dc = 1;
            int u = 0, cas = 0;
            float best = 0.f, nb[19];
            if (ci < ncand) {
                best = sbest[ci];
                const uint32_t info = sinfo[ci];
                u = (int)(info >> 9); cas = (int)((info >> 6) & 7u);
                xx = bx0 + (int)(info & 63u);
                y = y0 + 4 * u;
                const int i = mb + y * 2, jx = mb + xx * 2;
                s = k + (cas >> 2); r = i + ((cas >> 1) & 1); c = jx + (cas & 1);
                ds = (cas >> 2) ? 1 : -1; dr = ((cas >> 1) & 1) ? 1 : -1; dc = (cas & 1) ? 1 : -1;
                const int so = s + ds, si = s - ds;
                const int rn = r + dr, rp = r - dr, cn = c + dc;
                // the 19 neighbours outside the block, ties survive (surfd.cu:757-792),
                // in six rounds, each only for the candidates the previous
                // ones left: plane s's row rn, its column cn, plane si, then
                // plane so's rows r, rp, rn.  Gathers for every candidate cost
                // half the scan (0.87 ms with all 19 up front, 0.42 without
                // any); in rounds with 12-byte row loads it takes 0.69.
                ok = true;
                // one round of the test: its loads, then its compares (nb keeps
                // the values for the fit record)
                auto test = [&](int at, float v) {
                    nb[at] = v;
                    ok = ok & !(best < v);          // '&': no branch between the loads and a compare
                };
                // (pl, rr, c - 1 .. c + 1): one 12-byte load where plane pl is
                // not a halfImage view
                auto row3 = [&](int at, int pl, int rr) {
                    float a0, a1, a2;
                    if (HK && pl < 2) {
                        a0 = V(pl, rr, c - 1); a1 = V(pl, rr, c); a2 = V(pl, rr, c + 1);
                    } else {
                        typedef uint32_t v3u32 __attribute__((ext_vector_type(3)));
                        const v3u32 t3 = __builtin_amdgcn_raw_buffer_load_b96(
                            RF, (V.cur + pl * V.osize + rr * V.sp + c - 1) * 4, 0, 0);
                        a0 = __uint_as_float(t3.x); a1 = __uint_as_float(t3.y); a2 = __uint_as_float(t3.z);
                    }
                    test(at, a0); test(at + 1, a1); test(at + 2, a2);
                };
                row3(9, s, rn);
                if (ok) { test(12, V(s, r, cn)); test(13, V(s, rp, cn)); }
                if (ok) { row3(14, si, rn); test(17, V(si, rp, cn)); test(18, V(si, r, cn)); }
                if (ok) row3(3, so, r);
                if (ok) row3(0, so, rp);
                if (ok) row3(6, so, rn);
            }
            const unsigned long long mo = __ballot(ok);
            if (ok) {
                const int slot = nsurv + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mo >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)mo, 0u));
                // (octave 3 bits, level 2, block row 13, block column 14): the canonical order
                rkey[slot] = ((uint32_t)o << 29) | ((uint32_t)z << 27) | ((uint32_t)y << 14) | (uint32_t)xx;
                rsrc_[slot] = ((uint32_t)s << 28) | ((uint32_t)r << 14) | (uint32_t)c;
                if (CUBE && slot < kCubeCap) {
                    // the 19 values fitQuadrat's first pass reads (fit_quad),
                    // from the test's registers: k_nms_fit then gathers
                    // nothing for a survivor that does not move; plus the six
                    // block values it needs (the block's opposite corner is
                    // not read), block index cas ^ {col, row, scale} bits, from
                    // the block the candidate's lane staged in LDS at
                    // compaction (a memory reload cost the scan a round trip,
                    // cross-lane reads kept the block registers live: 76 VGPRs)
                    // (a candidate past the first 64 of its pass reloads them:
                    // the fit reads a record for every survivor slot < kCubeCap)
                    float b_r_cm, b_rp_c, b_rp_cm, i_r_c, i_r_cm, i_rp_c;
                    if (ci < 64) {
                        const float* bs = sblk + 8 * ci;
                        b_r_cm = bs[cas ^ 1]; b_rp_c = bs[cas ^ 2]; b_rp_cm = bs[cas ^ 3];
                        i_r_c = bs[cas ^ 4]; i_r_cm = bs[cas ^ 5]; i_rp_c = bs[cas ^ 6];
                    } else {
                        const int si = s - ds, rp = r - dr;
                        b_r_cm = V(s, r, c - dc); b_rp_c = V(s, rp, c); b_rp_cm = V(s, rp, c - dc);
                        i_r_c = V(si, r, c); i_r_cm = V(si, r, c - dc); i_rp_c = V(si, rp, c);
                    }
                    // V(s + a, r + b, c + e) for the positions fit_quad reads
                    // (selects, not indexing: nb stays in registers)
                    auto pick = [](int e, float m, float z, float p) -> float { return e < 0 ? m : (e == 0 ? z : p); };
                    auto so_at = [&](int b, int e) -> float {
                        return b == 0 ? pick(e, nb[3], nb[4], nb[5])
                                      : (b == dr ? pick(e, nb[6], nb[7], nb[8]) : pick(e, nb[0], nb[1], nb[2]));
                    };
                    auto s_at = [&](int b, int e) -> float {
                        if (b == 0) return e == 0 ? best : (e == dc ? nb[12] : b_r_cm);
                        if (b == dr) return pick(e, nb[9], nb[10], nb[11]);
                        return e == 0 ? b_rp_c : (e == dc ? nb[13] : b_rp_cm);
                    };
                    auto si_at = [&](int b, int e) -> float {       // no corner is read
                        if (b == 0) return e == 0 ? i_r_c : (e == dc ? nb[18] : i_r_cm);
                        if (b == dr) return pick(e, nb[14], nb[15], nb[16]);
                        return i_rp_c;
                    };
                    auto at = [&](int a, int b, int e) -> float {
                        return a == 0 ? s_at(b, e) : (a == ds ? so_at(b, e) : si_at(b, e));
                    };
                    float4* dst = reinterpret_cast<float4*>(rcube + (size_t)slot * kCubeF);
                    dst[0] = make_float4(best, at(1, 0, 0), at(-1, 0, 0), at(0, 1, 0));
                    dst[1] = make_float4(at(0, -1, 0), at(0, 0, 1), at(0, 0, -1), at(1, 1, 0));
                    dst[2] = make_float4(at(1, -1, 0), at(-1, 1, 0), at(-1, -1, 0), at(1, 0, 1));
                    dst[3] = make_float4(at(1, 0, -1), at(-1, 0, 1), at(-1, 0, -1), at(0, 1, 1));
                    dst[4] = make_float4(at(0, 1, -1), at(0, -1, 1), at(0, -1, -1), 0.f);
                }
            }
            nsurv += (int)__popcll(mo);
        }
        wave_sync();                          // sbest / sinfo are rewritten by the next pass
    });
    // every item writes its count, zero included (no per-batch memset)
    if (lane_id() == 0u) item_count[item] = nsurv;
}

// CUBE: write the survivors' fit records (k_nms_fit's first pass then reads
// no planes); without it the scan keeps 38 instead of 76 VGPRs, which single
// frames (config #2: a few hundred survivors) prefer
template <bool CUBE>
__global__ __launch_bounds__(256) void k_nms_scan(const float* __restrict__ resp, FrameParams P,
                                                  const OctaveParams* __restrict__ oct, LaunchPlan plan,
                                                  uint32_t* __restrict__ scan_key, uint32_t* __restrict__ scan_src,
                                                  float* __restrict__ scan_cube, int* __restrict__ item_count,
                                                  int nframes, int* __restrict__ cand_count, int* __restrict__ status)
{
    __shared__ float sbest[4][64 * 4];                // one pass's candidates per wave
    __shared__ __attribute__((aligned(16))) float sblk[4][64 * 8];   // blocks of its first 64 (CUBE)
    __shared__ uint32_t sinfo[4][64 * 4];
    int f, gb;
    if (!xcd_frame_block(plan.nms_start[kMaxOct], nframes, f, gb)) return;
    // the batch's counters the fit and sort use after this kernel: the
    // frame's accepted-candidate count and the truncation flag (no memsets)
    if (gb == 0 && threadIdx.x == 0) {
        cand_count[f] = 0;
        if (f == 0) *status = 0;
    }
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // plane k (= 2 z + 1) is a halfImage view for octaves > 0 at level z = 0
    const int o = octave_of(plan.nms_start, P.noct, gb);
    const int z = (gb - plan.nms_start[o]) / (plan.nms_nbx[o] * plan.nms_nby[o]);
    if (o > 0 && z == 0)
        nms_scan_item<CUBE, true>(resp, P, oct, plan, scan_key, scan_src, scan_cube, item_count,
                                  plan.nms_start[kMaxOct], f, gb, wv, sbest[wv], sinfo[wv], sblk[wv]);
    else
        nms_scan_item<CUBE, false>(resp, P, oct, plan, scan_key, scan_src, scan_cube, item_count,
                                   plan.nms_start[kMaxOct], f, gb, wv, sbest[wv], sinfo[wv], sblk[wv]);
}

// Exclusive prefix of n ints (n up to ~2M): each workgroup scans 2048
// elements (block_excl_scan) and records its total, one workgroup scans the
// totals, then the block offsets are added.  out[n] = total.
constexpr int kScanChunk = 2048;

__global__ __launch_bounds__(256) void k_scan_local(const int* __restrict__ in, int n, int* __restrict__ out,
                                                    int* __restrict__ bsum)
{
    __shared__ uint32_t lds4[4];
    const int b0 = blockIdx.x * kScanChunk + threadIdx.x * 8;
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = (b0 + k < n) ? (uint32_t)in[b0 + k] : 0u;
    const uint32_t last = v[7];
    block_excl_scan<8>(v, lds4);
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (b0 + k < n) out[b0 + k] = (int)v[k];
    if (threadIdx.x == 255) {
        // one chunk (n <= kScanChunk: a frame or two's NMS items): the total
        // goes straight to out[n] and the other two kernels are not launched
        if (gridDim.x == 1) out[n] = (int)(v[7] + last);
        else bsum[blockIdx.x] = (int)(v[7] + last);
    }
}

__global__ __launch_bounds__(1024) void k_scan_top(int* __restrict__ bsum, int nb, int* __restrict__ out, int n)
{
    __shared__ int part[16];
    const int per = (nb + 1023) / 1024;
    const int b = threadIdx.x * per;
    int sum = 0;
    for (int i = 0; i < per; i++) if (b + i < nb) sum += bsum[b + i];
    // exclusive scan of the 1,024 partial sums: DPP wave scans and the 16
    // wave totals (was one thread walking all 1,024)
    const uint32_t inc = wave_incl_scan((uint32_t)sum);
    const int wv = (int)(threadIdx.x >> 6);
    if (lane_id() == 63) part[wv] = (int)inc;
    __syncthreads();
    uint32_t wbase = 0u, total = 0u;
    for (int t = 0; t < 16; t++) {
        const uint32_t v = (uint32_t)part[t];
        wbase += t < wv ? v : 0u;
        total += v;
    }
    if (threadIdx.x == 0) out[n] = (int)total;
    int run = (int)(wbase + inc) - sum;
    for (int i = 0; i < per; i++)
        if (b + i < nb) { const int v = bsum[b + i]; bsum[b + i] = run; run += v; }
}

__global__ __launch_bounds__(256) void k_scan_add(int* __restrict__ out, int n, const int* __restrict__ bsum)
{
    const int add = bsum[blockIdx.x];
    const int b0 = blockIdx.x * kScanChunk;
    for (int i = threadIdx.x; i < kScanChunk && b0 + i < n; i += 256) out[b0 + i] += add;
}

static void launch_excl_scan(const int* in, int n, int* out, int* bsum, hipStream_t s)
{
    const int nb = (n + kScanChunk - 1) / kScanChunk;
    k_scan_local<<<nb, 256, 0, s>>>(in, n, out, bsum);
    if (nb == 1) return;
    k_scan_top<<<1, 1024, 0, s>>>(bsum, nb, out, n);
    k_scan_add<<<nb, 256, 0, s>>>(out, n, bsum);
}

// Pass 2: interpolation + makePoint, one lane per survivor of the whole batch
// (grid-stride over the prefix of the scan items' survivor counts), so no
// lane idles on the ~99 % of blocks that fail the 3x3x3 test and no
// workgroup is launched for empty space.
__global__ __launch_bounds__(256) void k_nms_fit(const int32_t* __restrict__ ii, const float* __restrict__ resp,
                                                 FrameParams P, const OctaveParams* __restrict__ oct,
                                                 const uint32_t* __restrict__ scan_key,
                                                 const uint32_t* __restrict__ scan_src,
                                                 const float* __restrict__ scan_cube,
                                                 const int* __restrict__ soff, int nitems, int items_per_frame,
                                                 surfhip_point* __restrict__ cand, uint32_t* __restrict__ keys,
                                                 int* __restrict__ cand_count, int cap, int stash)
{
    const int total = soff[nitems];
    const int stride = (int)gridDim.x * 256;
    for (int base = blockIdx.x * 256 + (threadIdx.x & ~63); base < total; base += stride) {
        const int t = base + (int)lane_id();
        const bool act = t < total;
        int f = 0;
        surfhip_point pt;
        bool ok = false;
        uint32_t key = 0;
        // the scan item holding each lane's survivor t = base + lane: the
        // wave finds base's item by a 64-way search (one coalesced load of
        // 64 probes per level: ~3-4 levels instead of a lane's ~19 dependent
        // loads), then lane t counts the item starts after it that are <= t
        // among the next 64 (ascending: a 6-step search over the lanes'
        // values); a lane past those 64 items searches on its own
        int wlo = 0;
        {
            int hi = nitems;                                 // soff[wlo] <= base < soff[hi]
            while (hi - wlo > 1) {
                const int sw = (hi - wlo + 63) >> 6;
                const int pr = wlo + ((int)lane_id() + 1) * sw;
                const bool le = pr < hi && soff[pr] <= base;
                const unsigned long long m = __ballot(le);
                const int k = m ? 64 - __builtin_clzll(m) : 0;
                wlo += k * sw;
                hi = min(wlo + sw, hi);
            }
        }
        const int wi = wlo + 1 + (int)lane_id();
        const int wst = wi <= nitems ? soff[wi] : 0x7fffffff; // item starts after wlo, ascending
        int cnt = 0;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) {
            const int v = __shfl(wst, cnt + sft - 1, 64);
            if (v <= t) cnt += sft;
        }
        if (cnt == 63 && __shfl(wst, 63, 64) <= t) cnt = 64;      // (all 64 starts <= t)
        if (act) {
            int lo = wlo + cnt;                          // scan item holding survivor t
            if (cnt == 64) {
                int hi = nitems;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (soff[mid] <= t) lo = mid; else hi = mid;
                }
            }
            f = lo / items_per_frame;
            const int idx = t - soff[lo];                // survivor index within its scan item
            const size_t src_i = (size_t)lo * kItemCap + idx;
            key = scan_key[src_i];
            const uint32_t src = scan_src[src_i];
            const int o = (int)(key >> 29);
            const OctaveParams& q = oct[o];
            const OctView V = make_view(resp + (size_t)f * P.resp_stride, q, o);
            const uint32_t* I = reinterpret_cast<const uint32_t*>(ii) + (size_t)f * P.ii_stride;
            const float4* cube = idx < kCubeCap && scan_cube
                ? reinterpret_cast<const float4*>(scan_cube + ((size_t)lo * kCubeCap + idx) * kCubeF) : nullptr;
            ok = nms_fit_point(I, V, P, q, o, (int)(src >> 28), (int)((src >> 14) & 0x3fffu), (int)(src & 0x3fffu),
                               cube, pt, stash != 0);
        }
        // Survivor t of frame f goes to slot t - (f's first survivor): the
        // slots are the survivors' scan order, so which candidates a frame
        // with more than `cap` survivors keeps is deterministic (the first
        // cap survivors; k_sort then orders them canonically).  A rejected
        // survivor leaves an invalid key, sorted last.
        if (act) {
            const int slot = t - soff[f * items_per_frame];
            if (slot < cap) {
                if (ok) cand[(size_t)f * cap + slot] = pt;
                keys[(size_t)f * cap + slot] = ok ? key : kNoKey;
            }
        }
        // accepted candidates per frame (a wave spans at most a few frames);
        // k_sort compares it with the ones inside the cap to flag truncation
        bool pending = ok;
        while (__ballot(pending)) {
            const int leader = __builtin_ctzll(__ballot(pending));
            const int ff = __shfl(f, leader, 64);
            const bool mine = pending && f == ff;
            const unsigned long long m = __ballot(mine);
            if ((int)lane_id() == leader) atomicAdd(&cand_count[ff], __popcll(m));
            if (mine) pending = false;
        }
    }
}

hipError_t launch_nms(const HessianArgs& a, const Candidates& c, hipStream_t s, const Switches& sw, bool stash_trace)
{
    const LaunchPlan& plan = *a.plan;
    const int nframes = a.b.n, per = plan.nms_start[kMaxOct];
    if (per == 0) {
        // (no NMS level: nothing to scan; the counters the sort reads are 0)
        hipError_t e = hipMemsetAsync(c.cand_count, 0, sizeof(int) * (size_t)nframes, s);
        if (e == hipSuccess) e = hipMemsetAsync(c.status, 0, sizeof(int), s);
        return e;
    }
    // the scan's fit records for every batch size (round 5: one 1080p frame's
    // NMS 0.038 -> 0.034 ms with them; round 2's cross-lane variant had made
    // single frames slower); SURFHIP_FIT_CUBE=0: the fit reads the planes (A/B)
    const bool cube = sw.fit_cube;
    float* scan_cube = cube ? c.scan_cube : nullptr;
    auto* scan = cube ? &k_nms_scan<true> : &k_nms_scan<false>;
    scan<<<dim3(frame_grid(nframes) * per), 256, 0, s>>>(a.resp, *a.P, a.d_oct, plan, c.scan_key, c.scan_src, scan_cube,
                                                                c.item_count, nframes, c.cand_count, c.status);
    const int items = scan_items(plan), nitems = nframes * items;
    launch_excl_scan(c.item_count, nitems, c.item_off, c.item_off + nitems + 1, s);
    // 5 waves per SIMD fit (90 VGPRs) = 1,280 workgroups of 4 waves; SURFHIP_FIT_GRID overrides (A/B)
    k_nms_fit<<<sw.fit_grid, 256, 0, s>>>(a.ii, a.resp, *a.P, a.d_oct, c.scan_key, c.scan_src, scan_cube, c.item_off,
                                          nitems, items, c.cand, c.keys, c.cand_count, c.cap, stash_trace ? 1 : 0);
    return hipGetLastError();
}
