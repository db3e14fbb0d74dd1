// surfhip_keep.inc -- the per-frame keypoint budget of SURFHIP_KEEP_STRONGEST
// (k_keep_strongest; launched by launch_sort ahead of the sort kernel).
// Included by surfhip_kernels.hip.

// ======================================================================
// The n strongest candidates of a frame.  Candidate a beats b when
// m(a.strength) > m(b.strength), m the order-preserving map of the IEEE bits
// (-0.0 below +0.0, a NaN has its place), or on equal strengths when a is the
// earlier in canonical order (the smaller key): one 64-bit composite
// (m(strength) << 32) | ~key per candidate, unique within a frame since valid
// keys are.  One workgroup per frame finds the composite of rank n from the
// top by an MSB-first radix select (8-bit digits, a 256-bin LDS histogram per
// pass, at most 8 passes; it stops once the bin holding the cut is taken
// whole) and writes kNoKey over the key of every candidate below it: the sort
// kernels then drop the losers as they drop rejected survivors, and the kept
// n come out in canonical order.  pre_valid[f]: the frame's valid count before
// the selection (the sort kernels' truncation test).
// ======================================================================

__device__ __forceinline__ uint32_t strength_order(uint32_t u)
{
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// One histogram count per `on` lane, pre-aggregated in the wave as
// wave_append is: the lanes sharing the first `on` lane's digit are counted
// by one atomic, twice over; what is left adds singly.  (Strengths of one
// frame share their sign and most of their exponent: the first pass puts
// nearly every lane of a wave into one or two bins, a 64-way serialised LDS
// atomic otherwise.)  Called by whole waves.
__device__ __forceinline__ void keep_hist_add(uint32_t* hist, bool on, uint32_t digit)
{
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const unsigned long long m = __ballot(on);
        if (m == 0ull) return;
        const int leader = __builtin_ctzll(m);
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
        const bool same = on && digit == d0;
        const unsigned long long ms = __ballot(same);
        if ((int)lane_id() == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(ms));
        on = on && !same;
    }
    if (on) atomicAdd(&hist[digit], 1u);
}

__global__ __launch_bounds__(1024) void k_keep_strongest(const surfhip_point* __restrict__ cand, uint32_t* keys,
                                                         const int* __restrict__ soff, int items_per_frame, int cap,
                                                         int lds_slots, int keep_n, int* __restrict__ pre_valid)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sc[];     // the frame's composites (lds_slots)
    __shared__ uint32_t hist[256];
    __shared__ int nvalid;
    __shared__ uint32_t sel_bin, sel_k, sel_whole;
    const int f = blockIdx.x;
    const int cnt = min(soff[(f + 1) * items_per_frame] - soff[f * items_per_frame], cap);
    uint32_t* fk = keys + (size_t)f * cap;
    const surfhip_point* fc = cand + (size_t)f * cap;
    const bool in_lds = cnt <= lds_slots;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < cnt; i += 1024) {
        const uint32_t k = fk[i];
        mine += k != kNoKey;
        if (in_lds) sc[i] = (uint32_t)~k;       // 0: a rejected survivor (a valid key's complement is not)
    }
    if (mine) atomicAdd(&nvalid, mine);
    __syncthreads();
    const int valid = nvalid;
    if (threadIdx.x == 0) pre_valid[f] = valid;
    if (valid <= keep_n) return;                // the frame fits its budget: every key stays
    // (each thread completes the slots it wrote above)
    if (in_lds)
        for (int i = threadIdx.x; i < cnt; i += 1024) {
            const uint32_t lo = (uint32_t)sc[i];
            if (lo) sc[i] = ((uint64_t)strength_order(__float_as_uint(fc[i].strength)) << 32) | lo;
        }
    // more slots than LDS holds: the passes re-read keys and strengths
    auto comp = [&](int i) -> uint64_t {
        if (in_lds) return sc[i];
        const uint32_t k = fk[i];
        return k == kNoKey ? 0ull : ((uint64_t)strength_order(__float_as_uint(fc[i].strength)) << 32) | (uint32_t)~k;
    };
    uint64_t cut = 0ull;                        // the digits of the rank-n composite found so far
    uint32_t want = (uint32_t)keep_n;           // its rank from the top among the composites sharing them
    for (int shift = 56;; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
        __syncthreads();
        for (int i0 = 0; i0 < cnt; i0 += 1024) {
            const int i = i0 + (int)threadIdx.x;
            const uint64_t c = i < cnt ? comp(i) : 0ull;
            const bool on = c != 0ull && (shift == 56 || (c >> (shift + 8)) == (cut >> (shift + 8)));
            keep_hist_add(hist, on, (uint32_t)(c >> shift) & 255u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // bins from the top, 4 per lane: the bin where the running count reaches `want`
            const int b0 = 255 - 4 * (int)threadIdx.x;
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = hist[b0 - j];
            const uint32_t sum = v[0] + v[1] + v[2] + v[3];
            uint32_t above = wave_incl_scan(sum) - sum;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (above < want && want <= above + v[j]) {
                    sel_bin = (uint32_t)(b0 - j);
                    sel_k = want - above;
                    sel_whole = v[j] == want - above;
                }
                above += v[j];
            }
        }
        __syncthreads();
        cut |= (uint64_t)sel_bin << shift;
        want = sel_k;
        if (sel_whole || shift == 0) break;     // everything in the bin is kept: `cut` with zeros below is the cut
    }
    for (int i = threadIdx.x; i < cnt; i += 1024) {
        const uint64_t c = comp(i);
        if (c != 0ull && c < cut) fk[i] = kNoKey;
    }
}
