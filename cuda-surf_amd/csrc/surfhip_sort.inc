// surfhip_sort.inc -- canonical keypoint order, the per-frame cap and the describe
// schedule (k_sort, k_sort_rank, k_offsets; launch_sort).  Included by
// surfhip_kernels.hip after surfhip_keep.inc.

// ======================================================================
// Canonical order + max_pts cap.  The reference emits in atomicInc order
// and can write past max_pts (surfd.cu:827-830, no pi<max guard); here each
// frame's candidates are sorted by key (bitonic, in LDS up to kSortCap, in
// a global scratch beyond) and the first max_pts are kept.
// ======================================================================

template <typename PtrT>
__device__ void bitonic_sort(PtrT s, int n)
{
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = s[i], b = s[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { s[i] = b; s[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// The same network on an LDS array with 1024 threads: pair p of pass (k, j)
// is elements (i, i + j), i = 2p - (p mod j), so every thread works every
// pass, and a wave's 64 pairs (p = 64 w .. 64 w + 63 + 1024 m) cover the
// 128-element blocks [128 (w + 16 m), +128) whenever j <= 64: those passes
// need only a wave-level sync; a block barrier is kept around every pass
// with j >= 128 (63 of the 78 passes of a 4,096-key sort skip it).
__device__ void bitonic_sort_lds(uint64_t* s, int n)
{
    const int npairs = n >> 1;
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < npairs; p += 1024) {
                const int i = 2 * p - (p & (j - 1));
                const uint64_t a = s[i], b = s[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { s[i] = b; s[i + j] = a; }
            }
            const int nj = j > 1 ? j >> 1 : k;          // the next pass's distance
            if (j >= 128 || (nj >= 128 && k < n)) __syncthreads();
            else wave_sync();
        }
    }
    __syncthreads();
}

// The value of lane (lane ^ J) (J = 1 .. 32) of a 64-bit element, by DPP /
// permlane swaps (no LDS round trip).
template <int J>
__device__ __forceinline__ uint32_t xor_lane32(uint32_t v, int lane)
{
    if constexpr (J == 1) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    } else if constexpr (J == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    } else if constexpr (J == 4 || J == 8) {
        const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + J, 0xf, 0xf, false);   // lane + J
        const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + J, 0xf, 0xf, false);   // lane - J
        return (lane & J) ? dn : up;
    } else {
        auto r = J == 16 ? __builtin_amdgcn_permlane16_swap(v, v, false, false)
                         : __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & J) ? r[0] : r[1];
    }
}
template <int J>
__device__ __forceinline__ uint64_t xor_lane64(uint64_t v, int lane)
{
    return ((uint64_t)xor_lane32<J>((uint32_t)(v >> 32), lane) << 32) | xor_lane32<J>((uint32_t)v, lane);
}
// One compare-exchange pass (k, J <= 32) of a 128-element block held two per
// lane (positions lane and lane + 64 of the block starting at `base`).
template <int J>
__device__ __forceinline__ void bitonic_reg_pass(uint64_t& e0, uint64_t& e1, int base, int k, int lane)
{
    const uint64_t p0 = xor_lane64<J>(e0, lane), p1 = xor_lane64<J>(e1, lane);
    const bool lower = (lane & J) == 0;
    const bool up0 = ((base + lane) & k) == 0, up1 = ((base + lane + 64) & k) == 0;
    e0 = (lower == up0) ? (e0 < p0 ? e0 : p0) : (e0 < p0 ? p0 : e0);
    e1 = (lower == up1) ? (e1 < p1 ? e1 : p1) : (e1 < p1 ? p1 : e1);
}
__device__ __forceinline__ void bitonic_reg_tail(uint64_t& e0, uint64_t& e1, int base, int k, int jmax, int lane)
{
    // passes J = jmax .. 1 (jmax <= 32)
    if (jmax >= 32) bitonic_reg_pass<32>(e0, e1, base, k, lane);
    if (jmax >= 16) bitonic_reg_pass<16>(e0, e1, base, k, lane);
    if (jmax >= 8) bitonic_reg_pass<8>(e0, e1, base, k, lane);
    if (jmax >= 4) bitonic_reg_pass<4>(e0, e1, base, k, lane);
    if (jmax >= 2) bitonic_reg_pass<2>(e0, e1, base, k, lane);
    bitonic_reg_pass<1>(e0, e1, base, k, lane);
}

// The same network with every pass of distance <= 64 in registers: a wave
// holds a 128-element block two per lane and runs those passes with DPP /
// permlane swaps; only the passes of distance >= 128 go through LDS (with a
// workgroup barrier each).  n >= 128, blockDim.x == 1024.
__device__ void bitonic_sort_lds_reg(uint64_t* s, int n)
{
    const int lane = (int)lane_id(), wv = (int)(threadIdx.x >> 6);
    const int nblk = n >> 7;
    // k = 2 .. 64: within blocks only
    for (int b = wv; b < nblk; b += 16) {
        const int base = b << 7;
        uint64_t e0 = s[base + lane], e1 = s[base + lane + 64];
        for (int k = 2; k <= 64; k <<= 1) bitonic_reg_tail(e0, e1, base, k, k >> 1, lane);
        s[base + lane] = e0;
        s[base + lane + 64] = e1;
    }
    __syncthreads();
    const int npairs = n >> 1;
    for (int k = 128; k <= n; k <<= 1) {
        for (int j = k >> 1; j >= 128; j >>= 1) {
            for (int p = threadIdx.x; p < npairs; p += 1024) {
                const int i = 2 * p - (p & (j - 1));
                const uint64_t a = s[i], b = s[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { s[i] = b; s[i + j] = a; }
            }
            __syncthreads();
        }
        for (int b = wv; b < nblk; b += 16) {
            const int base = b << 7;
            uint64_t e0 = s[base + lane], e1 = s[base + lane + 64];
            // distance 64: the lane's own two elements
            const bool up = (base & k) == 0;
            if ((e0 > e1) == up) { const uint64_t t = e0; e0 = e1; e1 = t; }
            bitonic_reg_tail(e0, e1, base, k, 32, lane);
            s[base + lane] = e0;
            s[base + lane + 64] = e1;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void k_sort(const surfhip_point* __restrict__ cand,
                                               const uint32_t* __restrict__ keys,
                                               uint64_t* __restrict__ gscratch, const int* __restrict__ cand_count,
                                               const int* __restrict__ soff, int items_per_frame, int cap,
                                               surfhip_point* __restrict__ out, int max_pts,
                                               int* __restrict__ out_count, int* __restrict__ order, int* status,
                                               int keep_n, const int* __restrict__ pre_valid)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];
    __shared__ int nvalid;
    const int f = blockIdx.x;
    // slots written by k_nms_fit: the frame's survivors, at most cap
    const int cnt = min(soff[(f + 1) * items_per_frame] - soff[f * items_per_frame], cap);
    int n = 1;
    while (n < cnt) n <<= 1;                  // <= cap (a power of 2)
    const bool in_lds = n <= kSortCap;
    uint64_t* s = in_lds ? sk : gscratch + (size_t)f * cap;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t k = (i < cnt) ? keys[(size_t)f * cap + i] : kNoKey;
        mine += k != kNoKey;
        s[i] = ((uint64_t)k << 32) | (uint32_t)i;
    }
    if (mine) atomicAdd(&nvalid, mine);
    __syncthreads();
    if (in_lds && blockDim.x == 1024 && n >= 128) bitonic_sort_lds_reg(s, n);
    else if (in_lds && blockDim.x == 1024) bitonic_sort_lds(s, n);
    else bitonic_sort(s, n);
    const int valid = nvalid;
    // accepted candidates beyond the cap were dropped: report it (pre_valid:
    // k_keep_strongest ran, the frame's valid count from before its selection)
    if (threadIdx.x == 0 && cand_count[f] > (pre_valid ? pre_valid[f] : valid)) atomicOr(status, 1);
    const int keep = min(valid, keep_n);        // the per-frame budget (<= max_pts, the slot stride)
    for (int t = threadIdx.x; t < keep; t += blockDim.x)
        out[(size_t)f * max_pts + t] = cand[(size_t)f * cap + (uint32_t)(s[t] & 0xffffffffu)];
    if (threadIdx.x == 0) out_count[f] = keep;
    // Describe schedule (processing order only; descriptors land at their
    // canonical index): keypoints in 16-row bands of the frame, canonical
    // order within a band.  The canonical order sweeps the frame 2 x noctaves
    // times (octave, layer, y); the band order sweeps it once, so the few
    // hundred keypoints an XCD describes at a time share their integral-image
    // rows in that XCD's L2.
    constexpr int BAND_SHIFT = 4;             // log2 of the band height
    // A counting sort by band: the order within a band is free (describe
    // writes each descriptor at its canonical index; the order only groups
    // the keypoints an XCD describes at a time), so two passes of LDS atomics
    // replace round 2's second bitonic sort (78 barrier passes for 4,096 keys).
    int* ord = order + (size_t)f * max_pts;
    __threadfence_block();
    __syncthreads();                          // s[] is dead, out[] is written
    constexpr int NBAND = 4096;               // 16-row bands of frames up to 65,536 rows
    uint32_t* bc = reinterpret_cast<uint32_t*>(sk);
    __shared__ uint32_t wsum[32];
    for (int b = threadIdx.x; b < NBAND; b += blockDim.x) bc[b] = 0u;
    __syncthreads();
    auto band_of = [&](int t) -> uint32_t {
        const float y = out[(size_t)f * max_pts + t].y;
        return min((uint32_t)max(y, 0.f) >> BAND_SHIFT, (uint32_t)NBAND - 1u);
    };
    for (int t = threadIdx.x; t < keep; t += blockDim.x) atomicAdd(&bc[band_of(t)], 1u);
    __syncthreads();
    {
        constexpr int PER = NBAND / 1024;     // blockDim.x == 1024
        uint32_t v[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) v[k] = bc[PER * threadIdx.x + k];
        block_excl_scan<PER>(v, wsum);
#pragma unroll
        for (int k = 0; k < PER; k++) bc[PER * threadIdx.x + k] = v[k];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < keep; t += blockDim.x) ord[atomicAdd(&bc[band_of(t)], 1u)] = t;
}

// Small batches (nframes <= kRankBatch): the canonical order by ranks,
// spread over many workgroups per frame instead of one bitonic workgroup
// (config #2: one frame's sort ran on one CU of 256).  Valid keys are unique
// (one survivor per 2x2x2 block), so a valid candidate's rank is the number
// of keys below its own -- exactly its position in the bitonic result;
// rejected slots (kNoKey) sort last and are dropped.  Workgroup r of a frame
// ranks candidates [256 r, 256 r + 256) against all of the frame's keys
// (staged in LDS when they fit).  Processing order for describe = canonical.
constexpr int kRankBatch = 8;
constexpr int kRankLds = 16384;
// Rank sort of a frame's candidates (small batches): a valid key's rank
// among the frame's keys is its canonical position (keys are unique).  16
// lanes share a candidate, each counting the smaller keys in every 16th slot
// (lane-interleaved LDS reads), then a 16-lane DPP sum: 16 candidates per
// workgroup.  (One lane per candidate walked all ~3,000 keys of a 1080p
// frame on one wave per SIMD of a dozen CUs: 27-29 us per frame.)
constexpr int kRankT = 16;                      // lanes per candidate
constexpr int kRankMaxWgs = 256;                // workgroups per frame at most
__global__ __launch_bounds__(256) void k_sort_rank(const surfhip_point* __restrict__ cand,
                                                   const uint32_t* __restrict__ keys,
                                                   const int* __restrict__ cand_count,
                                                   const int* __restrict__ soff, int items_per_frame, int cap,
                                                   int wgs_per_frame, surfhip_point* __restrict__ out, int max_pts,
                                                   int* __restrict__ out_count, int* __restrict__ order,
                                                   int* __restrict__ status, int keep_n,
                                                   const int* __restrict__ pre_valid)
{
    __shared__ __attribute__((aligned(16))) uint32_t sk[kRankLds];
    __shared__ int nvalid;
    constexpr int CPW = 256 / kRankT;           // candidates per workgroup
    const int f = blockIdx.x / wgs_per_frame, r = blockIdx.x - f * wgs_per_frame;
    const int cnt = min(soff[(f + 1) * items_per_frame] - soff[f * items_per_frame], cap);
    const uint32_t* fk = keys + (size_t)f * cap;
    if (r > 0 && r * CPW >= cnt) return;        // nothing to rank here (workgroup 0 writes the count)
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    const bool lds = cnt <= kRankLds;
    int mine = 0;
    // 8 loads in flight per thread (a loop of single loads waited a memory
    // latency per 256 keys)
    for (int i0 = threadIdx.x; i0 < cnt; i0 += 256 * 8) {
        uint32_t k[8];
#pragma unroll
        for (int u = 0; u < 8; u++) k[u] = (i0 + 256 * u < cnt) ? fk[i0 + 256 * u] : kNoKey;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (i0 + 256 * u < cnt) {
                if (lds) sk[i0 + 256 * u] = k[u];
                mine += k[u] != kNoKey;
            }
    }
    if (mine) atomicAdd(&nvalid, mine);
    __syncthreads();
    const int valid = nvalid;
    const int keep = min(valid, keep_n);        // the per-frame budget (<= max_pts, the slot stride)
    if (r == 0 && threadIdx.x == 0) {
        out_count[f] = keep;
        if (cand_count[f] > (pre_valid ? pre_valid[f] : valid)) atomicOr(status, 1);
    }
    const int part = (int)(threadIdx.x & (kRankT - 1));
    // candidate groups r, r + wgs, ...: a dense frame (cnt up to the cap)
    // reuses the keys staged in LDS for several groups instead of restaging
    // them in cnt / 16 workgroups (ADVICE r05: 16x the key loads)
    for (int g = r; g * CPW < cnt; g += wgs_per_frame) {
        const int i = g * CPW + (int)(threadIdx.x / kRankT);
        const uint32_t ki = (i < cnt) ? (lds ? sk[i] : fk[i]) : kNoKey;
        int rank = 0;
        if (ki != kNoKey) {
            if (lds) {
                int j = part;
                for (; j + 7 * kRankT < cnt; j += 8 * kRankT) {
                    uint32_t q[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) q[u] = sk[j + u * kRankT];
#pragma unroll
                    for (int u = 0; u < 8; u++) rank += q[u] < ki;
                }
                for (; j < cnt; j += kRankT) rank += sk[j] < ki;
            } else {
                for (int j = part; j < cnt; j += kRankT) rank += fk[j] < ki;
            }
        }
        // the 16 partial counts of a candidate: DPP row shifts (16-lane rows)
        rank += __builtin_amdgcn_update_dpp(0, rank, 0x111, 0xf, 0xf, false);      // row_shr:1
        rank += __builtin_amdgcn_update_dpp(0, rank, 0x112, 0xf, 0xf, false);      // row_shr:2
        rank += __builtin_amdgcn_update_dpp(0, rank, 0x114, 0xf, 0xf, false);      // row_shr:4
        rank += __builtin_amdgcn_update_dpp(0, rank, 0x118, 0xf, 0xf, false);      // row_shr:8
        // lane 15 of each row holds the row's sum
        if (part == kRankT - 1 && ki != kNoKey && rank < keep) {
            out[(size_t)f * max_pts + rank] = cand[(size_t)f * cap + i];
            order[(size_t)f * max_pts + rank] = rank;
        }
    }
}

__global__ __launch_bounds__(1024) void k_offsets(const int* __restrict__ counts, int nframes, int* __restrict__ offsets)
{
    __shared__ int part[16];
    const int per = (nframes + 1023) / 1024;
    const int b = threadIdx.x * per;
    int sum = 0;
    for (int i = 0; i < per; i++) if (b + i < nframes) sum += counts[b + i];
    // exclusive scan of the 1,024 partial sums: DPP wave scans and the 16
    // wave totals (was one thread walking all 1,024: ~10 us, on config #2's
    // single-frame path too)
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
    if (threadIdx.x == 0) offsets[nframes] = (int)total;
    int run = (int)(wbase + inc) - sum;
    for (int i = 0; i < per; i++)
        if (b + i < nframes) { offsets[b + i] = run; run += counts[b + i]; }
}

hipError_t launch_sort(const Candidates& c, const LaunchPlan& plan, int nframes, const PointSlots& out,
                       const DescribeSchedule& sch, hipStream_t s, const Switches& sw, const KeepRule& keep)
{
    const int items = scan_items(plan), cap = c.cap;
    // SURFHIP_KEEP_STRONGEST: the losers' keys become kNoKey ahead of the sort
    // (SURFHIP_KEEP_FIRST is the sort kernels' own cut at keep.n)
    const int* pre_valid = nullptr;
    if (keep.mode == SURFHIP_KEEP_STRONGEST) {
        const int slots = std::min(cap, kSortCap);
        hipError_t e = set_max_lds(reinterpret_cast<const void*>(&k_keep_strongest), (int)(kSortCap * sizeof(uint64_t)));
        if (e != hipSuccess) return e;
        k_keep_strongest<<<nframes, 1024, slots * sizeof(uint64_t), s>>>(c.cand, c.keys, c.item_off, items, cap, slots,
                                                                         keep.n, keep.valid);
        pre_valid = keep.valid;
    }
    if (nframes <= kRankBatch && !sw.sort_bitonic) {
        // workgroups per frame: one per 16 candidates up to 256 (~3,000
        // candidates of a 1080p frame: 188), beyond that each takes several
        // groups of 16 with the keys it staged once
        const int per = std::min((cap + 256 / kRankT - 1) / (256 / kRankT), kRankMaxWgs);
        k_sort_rank<<<nframes * per, 256, 0, s>>>(c.cand, c.keys, c.cand_count, c.item_off, items, cap, per, out.pts,
                                                  out.max_pts, out.counts, sch.order, c.status, keep.n, pre_valid);
    } else {
        hipError_t e = set_max_lds(reinterpret_cast<const void*>(&k_sort), (int)(kSortCap * sizeof(uint64_t)));
        if (e != hipSuccess) return e;
        k_sort<<<nframes, 1024, kSortCap * sizeof(uint64_t), s>>>(c.cand, c.keys, c.gscratch, c.cand_count, c.item_off,
                                                                  items, cap, out.pts, out.max_pts, out.counts,
                                                                  sch.order, c.status, keep.n, pre_valid);
    }
    k_offsets<<<1, 1024, 0, s>>>(out.counts, nframes, sch.offsets);
    return hipGetLastError();
}
