// surfhip_internal.h -- parameter blocks and launch helpers shared by the
// kernel TU (surfhip_kernels.hip) and the C-ABI TU (surfhip_api.hip).
//
// The reference keeps these values in process-global __constant__ symbols
// that every frame re-uploads (surfd.cu:13-24, 27-102; 22 cudaMemcpyToSymbol
// per frame at 4 octaves).  Here they are computed once per detector and
// passed by value as kernel arguments, so detectors are independent and a
// frame costs no host->device parameter traffic.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>

#include "surfhip.h"

namespace surfhip {

constexpr int kMaxOct = 8;
constexpr int kMaxScale = 8;
constexpr int kSortCap = 16384;     // candidates per frame sorted in LDS
constexpr uint32_t kNoKey = 0xffffffffu;   // candidate slot of a rejected NMS survivor
constexpr int kDescQ = 16;          // describe work queues per XCD (<= 16: the queue memset covers 16)
constexpr int kDescQueueBytes = 8 * kDescQ * 64 * 4;
constexpr int kBandRows = 32;       // integral-image band height
constexpr int kBandRowsSmall = 16;  // ... for batches of <= kSmallBatch frames (one 1080p frame: 16 -> 0.1281-0.1287 ms vs 8 -> 0.1298-0.1305, 4 -> 0.131)
constexpr int kSmallBatch = 8;
// The run-time switches (the SURFHIP_* environment variables of INTEGRATION.md's
// table).  A detector reads them once, when it is created (read_switches, the
// library's only reader of the environment), and its plan, its scratch sizes
// and every launch take them from there: a variable changed later does not
// reach it.  Values are normalised by read_switches; -1: unset, where the
// default depends on the detector or the batch.
struct Switches {
    unsigned set = 0;               // bit i: variable i, in the order below, was in the environment (switches_text)
    // make_plan
    int hess_gather = -1;           // HESS_GATHER 0 / 1; unset: max_batch <= kGatherBatch
    bool hess_w = true;             // HESS_W
    bool q01 = true;                // Q01
    int p0 = 93;                    // P0: 0 (k_hess_q0), 95, 93, 92, 91, 32
    bool hess_t0 = true;            // HESS_T0
    int ii_fuse = 1;                // II_FUSE: 0, 1, 2
    bool rowsum_rowseg = false;     // ROWSUM=rowseg
    // choose_describe, launch_sort
    int desc_ur = -1;               // DESC_UR 0 / 1; unset: batches <= kGatherBatch
    bool trace_desc = true;         // TRACE_DESC
    bool rot_atomic = false;        // ROT_ATOMIC: set to anything
    bool sort_bitonic = false;      // SORT_BITONIC: set to anything
    // prefetch_place, launch_describe, launch_nms, launch_integral
    int prefetch = -1;              // PREFETCH 0 nms / 1 describe; unset: by the plan
    int desc_beside = 3;            // DESC_BESIDE
    int u2_ldspad = 0;              // U2_LDSPAD
    int fit_grid = 1280;            // FIT_GRID: >= 64
    bool fit_cube = true;           // FIT_CUBE
    int ii_band = kBandRows;        // II_BAND 8..64: band height for batches > kSmallBatch
    int ii_band_small = kBandRowsSmall;   // II_BAND_SMALL 4..32: ... for batches <= kSmallBatch
};
Switches read_switches();                       // from the environment (surfhip_api.hip)
std::string switches_text(const Switches& sw);  // "NAME=value" of the variables that were set, or ""
// colsum entries (per column) the integral of a batch of up to max_batch frames needs
inline long long integral_bands(int H, int max_batch, const Switches& sw)
{
    const int bb = sw.ii_band, sb = sw.ii_band_small;
    const long long big = (long long)max_batch * ((H + bb - 1) / bb);
    const long long small = (long long)(max_batch < kSmallBatch ? max_batch : kSmallBatch) * ((H + sb - 1) / sb);
    return big > small ? big : small;
}
constexpr int kScanRows = 16;       // NMS block rows per scan workgroup (4 per wave)
constexpr int kItemCap = 64 * (kScanRows / 4);   // 2x2x2 blocks (= survivor slots) per scan item
constexpr int kCubeCap = 8;         // survivors per scan item whose fit inputs the scan records
constexpr int kCubeF = 20;          // floats per record (fit_quad's 19 responses + pad)

// Per-octave geometry and Hessian/NMS parameters, exactly as the reference
// host code derives them (surf.cpp:240-292, surfd.cu:2844-2865, 3062-3076).
struct OctaveParams {
    int sw, sh, sp, osize;          // response grid (swhp) and plane size
    long long ooff;                 // float offset of plane 0 in a frame block
    int octave, delta, init_scale, nscale;
    int mask[kMaxScale], b1[kMaxScale], x2[kMaxScale], x3[kMaxScale], x4[kMaxScale];
    float norm[kMaxScale];
    int borders[kMaxScale];         // host borders[] (d_borders), index s
    int mb[(kMaxScale - 2) / 2];    // NMS start offsets (maximum_borders, one per level)
    int nms_gx, nms_gy;             // NMS launch extent in threads
    // planes 0 and 1 of an octave > 0 are the reference's halfImage copies of
    // the previous octave's planes max_scale - 3 / max_scale - 1
    // (surf.cpp:252-258), never materialised: read in place at (r, c) ->
    // hbase[t] + r * hrow[t] + c * hcol[t] (floats).  With 4 scales plane
    // max_scale - 3 = 1 is itself a copy, so the chain is followed back to a
    // computed plane (stride 4, 8, ..).
    long long hbase[2];
    int hrow[2], hcol[2];
};

// Frame-level parameters (SurfParam + integral geometry).
struct FrameParams {
    int W, H, ip, iH;               // integral: (W+1) x (H+1), pitch ip ints
    long long ii_stride;            // ints per frame
    long long resp_stride;          // floats per frame
    int max_scale, init_lobe, sampling, noct;
    float thresh, divisor;
    int upright, extend, wsz, mag, osz, nfeat;
    int doubled;                    // the integral is of the 2x frame: describe at (2x, 2y)
};

struct Tables {
    float lut1[83];
    float lut2[40];
    float bins[72];
};

// ---- launch helpers (defined in surfhip_kernels.hip) -------------------
hipError_t set_tables(const Tables& t);

// A batch of u8 frames: n frames `stride` bytes apart, their rows `pitch` apart
struct FrameBatch {
    const uint8_t* frames = nullptr;
    int n = 0, pitch = 0;
    long long stride = 0;           // one integer type inside the library (the C-ABI's is size_t)
};
inline bool operator==(const FrameBatch& a, const FrameBatch& b)
{
    return a.frames == b.frames && a.n == b.n && a.pitch == b.pitch && a.stride == b.stride;
}
// (colsum: integral_bands() of the same switches)
hipError_t launch_integral(const FrameBatch& b, const FrameParams& P, const Switches& sw, uint32_t* colsum,
                           int32_t* ii, hipStream_t s);
// Block ranges of the fused all-octave launches and the Hessian kernel of
// each octave (computed once per detector; make_plan).
struct LaunchPlan {
    int hess_start[kMaxOct + 1];    // k_hessian blocks of octave o: [start[o], start[o+1])
    int hess_nbx[kMaxOct];          // blocks per row of samples
    int nms_start[kMaxOct + 1];     // NMS blocks of octave o (every level)
    int nms_nbx[kMaxOct], nms_nby[kMaxOct];
    int q0, q0_strips;              // octave 0 on k_hess_q0 (u8 vertical streaming), 64-sample strips
    int p0;                         // ... on k_hess_p0 instead (producer + per-scale waves): its interval B; 0: q0
    int q1, q1_strips;              // octave 1 on k_hess_q1 (when k_hess_w is off)
    int q01;                        // q0 and q1 in one launch (k_hess_q01)
    int hw_n;                       // octaves 1 .. hw_n on k_hess_w (u8, shared strip integral); 0: off
    int hw_nstrips, hw_nblk;        // its strips per frame and blocks of 4 integral rows
    int t0, t0_nbx, t0_nby;         // octave 0 of the gather plan on k_hessian_t0 (LDS tiles): its blocks
    // A u8 Hessian kernel also writes the integral image (its producers'
    // strip integral plus the row sums left of the strip, k_ii_rowseg): no
    // separate integral pass.  Set when octaves 0-3 are on the u8 kernels
    // (p0 + k_hess_w); k_hessian octaves (past 3) run after them on the same
    // stream.  1: k_hess_w writes it (480-column strips), 2: k_hess_p0
    // (128-column strips).
    int iiw;
    int rs_rows;                    // rows per rowseg slab (4 x hw_nblk, zero past H)
    int rs_nstrips;                 // rowseg slabs per frame: the writer's strips
    // iiw 1: k_hess_w's row sums come from k_hess_p0's producers (per
    // 128-column strip, added up by k_rowsum_p0 between the two launches)
    // instead of k_ii_rowseg's pass over the frames
    int rsum;
};
// the plan has kernels that read the u8 frames (not only the integral image)
inline bool plan_reads_frames(const LaunchPlan& p) { return p.q0 || p.q1 || p.hw_n > 0; }
// max_batch <= kGatherBatch (or Switches::hess_gather 1; 0 disables) puts every
// octave on the one-thread-per-response gather kernel: the streaming kernels
// walk whole strips, one wave each, too few waves to fill the chip for a few
// frames (measured crossover, 1080p: gather 9,956 vs streaming 7,981 frames/s
// at 8 frames, 12,474 vs 14,085 at 16).
constexpr int kGatherBatch = 8;
// float4s per k_worklist entry (k_describe_u2's flattened schedule)
constexpr int kWorkF4 = 3;
void make_plan(const FrameParams& P, const OctaveParams* oct, const Switches& sw, LaunchPlan& plan, int max_batch);
// the Hessian stage's kernels of a plan, as text (surfhip_hessian_plan)
std::string hessian_plan_text(const LaunchPlan& plan, const FrameParams& P);

// The Hessian stage's launches of one batch, in the order one stream runs them.  The first two read the u8
// frames (b.frames must be given where the plan has such kernels), the third reads ii: two streams may run them.
struct HessianArgs {
    FrameBatch b;
    const int32_t* ii;
    float* resp;
    const FrameParams* P;
    const OctaveParams *d_oct, *h_oct;
    const LaunchPlan* plan;
    // plan.iiw: k_hess_w (iiw 1) or k_hess_p0 (iiw 2) writes the frames' integral image into ii_out, adding
    // the row sums in rowseg (nframes x rs_nstrips x rs_rows uint32; slab 0 and rows >= H stay zero); nullptr:
    // neither does.  psum (plan.rsum): nframes x q0_strips x rs_rows uint32 of scratch; the octave-0 launch
    // then fills rowseg itself (k_hess_p0's strip sums, k_rowsum_p0).
    uint32_t* rowseg;
    int32_t* ii_out;
    uint32_t* psum;
};
// k_hess_q01, or k_hess_p0 (+ k_rowsum_p0: plan.rsum), or k_hess_q0; then k_hess_q1 where the plan has it
hipError_t launch_hess_oct0(const HessianArgs& a, hipStream_t s);
hipError_t launch_hess_w(const HessianArgs& a, hipStream_t s);      // octaves 1 .. plan.hw_n on k_hess_w
hipError_t launch_hess_ii(const HessianArgs& a, hipStream_t s);     // k_hessian_t0, k_hessian
// plan.iiw without plan.rsum: rowseg of the batch by k_ii_rowseg's pass over its frames; else no launch
hipError_t launch_rowseg(const FrameBatch& b, const FrameParams& P, const LaunchPlan& plan, uint32_t* rowseg,
                         hipStream_t s);
// NMS scan items: one wave's 64 block columns x kScanRows / 4 block rows;
// each item owns kItemCap survivor slots (no atomics in the scan).
inline int scan_items(const LaunchPlan& plan) { return plan.nms_start[kMaxOct] * 4; }   // per frame
// What the NMS stage produces and the sort consumes, per frame of n = scan_items(plan)
struct Candidates {
    uint32_t *scan_key, *scan_src;  // NMS survivors awaiting interpolation: n x kItemCap
    float* scan_cube;               // the survivors' fit inputs: n x kCubeCap x kCubeF
    int* item_count;                // survivors per scan item
    int* item_off;                  // their exclusive prefix (+ total), then the scan's per-chunk totals
    surfhip_point* cand;            // cap per frame, in scan order
    uint32_t* keys;                 // their canonical keys; kNoKey: rejected by the fit
    uint64_t* gscratch;             // cap > kSortCap: k_sort's sort space
    int* cand_count;                // accepted candidates per frame
    int cap;
    int* status;                    // [0] bit 0: a frame was cut at cap; from [64]: DescribeSchedule::queue
};
// The describe schedule: written by launch_sort or launch_plant, read by launch_describe and launch_pack
struct DescribeSchedule {
    int* offsets;                   // exclusive prefix of the frames' counts (+ total)
    int* order;                     // per frame: keypoint slots in describe order
    float4* work;                   // the schedule flattened: max_pts x kWorkF4 float4 per frame (k_worklist)
    int* queue;                     // kDescQueueBytes: the describe kernels' per-XCD work counters, 256 B apart
};
// The caller's output: frame f's points from pts[f * max_pts], counts[f] of them
struct PointSlots {
    surfhip_point* pts;
    int max_pts;
    int* counts;
};
// Scan, prefix and fit of a.b.n frames' planes a.resp into c (a.ii: the laplace sign's integral)
// (also zeroes c.cand_count[0, a.b.n) and *c.status, the per-batch counters)
hipError_t launch_nms(const HessianArgs& a, const Candidates& c, hipStream_t s, const Switches& sw,
                      bool stash_trace);
// The per-frame keypoint budget (surfhip_detector_set_keep): at most n (1 .. max_pts) points per frame, the
// first n in canonical order or the n strongest.  valid: max_batch ints of device scratch, each frame's valid
// candidates before k_keep_strongest's selection (SURFHIP_KEEP_STRONGEST only).
struct KeepRule {
    int mode = SURFHIP_KEEP_FIRST;
    int n = 0;
    int* valid = nullptr;
};
// c's candidates of nframes (launch_nms's, of the same plan) in canonical order into out, their schedule into sch
// (SURFHIP_KEEP_STRONGEST writes kNoKey over the keys of the candidates it drops)
hipError_t launch_sort(const Candidates& c, const LaunchPlan& plan, int nframes, const PointSlots& out,
                       const DescribeSchedule& sch, hipStream_t s, const Switches& sw, const KeepRule& keep);
hipError_t set_max_lds(const void* fn, int bytes);
// The describe kernel of a batch of nframes and where its laplace sign is
// taken, chosen once per call (surfhip_detect_batch_next).  kDescU2: upright
// 4 x 4 windows, the packed worklist fields large enough, and
// SURFHIP_DESC_UR=0 or, unset, batches > kGatherBatch.  trace: the sign
// (getTrace, surfd.cu:369-377) is taken in k_describe_u2, from the integral
// rows the keypoint's window brings into L2, instead of in k_nms_fit: only on
// kDescU2 with both integral extents below 32768; SURFHIP_TRACE_DESC=0 keeps
// it in the fit (A/B).
enum DescKernel { kDescU2, kDescUr, kDescWide, kDescUpright, kDescRot, kDescRotAtomic };
struct DescribeChoice {
    DescKernel kernel;
    bool trace;
};
DescribeChoice choose_describe(const Switches& sw, const FrameParams& P, int nframes);
// sch: pts' schedule (sch.queue is zeroed by the launch; sch.work is k_describe_u2's)
// beside: another stream's kernels (the next batch's integral, not a mere
// row-sum pass) run beside it, so the persistent grid leaves each CU a workgroup slot
// cus: compute units of the detector's device (sizes the persistent grid)
// how: the batch's choose_describe(); its trace was the same call's stash_trace of launch_nms
hipError_t launch_describe(const int32_t* ii, const FrameParams& P, const PointSlots& pts,
                           const DescribeSchedule& sch, int nframes, float* desc, hipStream_t s, bool beside,
                           int cus, const Switches& sw, DescribeChoice how);
// The describe schedule of caller-given points (surfhip_run_describe), in
// place of launch_sort's: pts.counts[f] = counts[f] cut to [0, max_pts] (the
// caller's counts stay as they are), their prefix in sch.offsets (k_offsets)
// and the identity order of each frame's first pts.counts[f] slots.
hipError_t launch_plant(const int* counts, int nframes, const PointSlots& pts, const DescribeSchedule& sch,
                        hipStream_t s);
// Doubled-image input (surfhip_double.hip): frames (W x H) -> D ((2W-2) x
// (2H-2) u8, row pitch dpitch, a multiple of 4).
// HBM stream-rate kernels (surfhip_stream.hip): mode 0 copy, 1 read, 2 write
hipError_t launch_stream(int mode, const void* src, void* dst, size_t bytes, int ncu, hipStream_t s);
hipError_t launch_double(const uint8_t* frames, int pitch, long long fstride, int nframes, int W, int H,
                         uint8_t* dst, int dpitch, long long dstride, hipStream_t s);
// Descriptor matching (surfhip_match.hip): scratch = match_scratch_bytes().
size_t match_scratch_bytes(int n1, int n2, int flags);
hipError_t launch_match(surfhip_point* pts1, const surfhip_point* pts2, const float* f1, const float* f2, int n1,
                        int n2, int nf, int flags, void* scratch, hipStream_t s);
// Batched matching on the f32 MFMA: pair i = frame i of set 1 ([npairs][slots1]
// points / descriptors, counts on the device) against frame i of set 2.  The
// point arrays may overlap (set 2 = set 1 advanced one frame).
// What is offered to a set-1 point: every set-2 point, those in a window
// around it, those in a window around its predicted position, or those in a
// window around it that also lie in a band along its epipolar line.
enum { MATCH_PLAIN = 0, MATCH_WINDOW = 1, MATCH_GUIDED = 2, MATCH_EPIPOLAR = 3 };
// The arguments of a batched match, the kernels' too (by value).  The caller
// fills the sets, npairs, nf, flags and, by mode, win (not MATCH_PLAIN), hm,
// h_stride (MATCH_GUIDED, MATCH_EPIPOLAR: pair i's 3 x 3 matrix is the nine
// row-major floats at hm + i * h_stride in device memory, read in stream
// order) and band (MATCH_EPIPOLAR: the half width of the band, pixels);
// launch_match_batch places back, boxes and tiles in its scratch.
struct MatchBatch {
    surfhip_point* pts1;
    const float* f1;
    const int* counts1;
    int slots1;
    const surfhip_point* pts2;
    const float* f2;
    const int* counts2;
    int slots2;
    int npairs, nf, flags;
    unsigned long long* back;       // SURFHIP_MATCH_MUTUAL: [npairs][slots2] keys of the back direction
    float4* boxes;                  // not MATCH_PLAIN: [npairs][tiles] boxes of set 2's 32-point tiles
    int tiles;
    surfhip_match_window win;
    const float* hm;
    int h_stride;
    float band;
    // the pairs from p0 on
    MatchBatch from(int p0) const
    {
        MatchBatch b = *this;
        b.pts1 += (size_t)p0 * slots1;
        b.f1 += (size_t)p0 * slots1 * nf;
        b.counts1 += p0;
        b.pts2 += (size_t)p0 * slots2;
        b.f2 += (size_t)p0 * slots2 * nf;
        b.counts2 += p0;
        b.npairs -= p0;
        if (back) b.back += (size_t)p0 * slots2;
        if (boxes) b.boxes += (size_t)p0 * tiles;
        if (hm) b.hm += (size_t)p0 * h_stride;
        return b;
    }
};
// flags may carry SURFHIP_MATCH_MUTUAL in every mode: then a match (p1 -> p2)
// stays only when p1 is the best set-1 point of p2.  scratch:
// match_batch_scratch_bytes() of device memory in any state, 16-B aligned:
// first the tile boxes (not MATCH_PLAIN: 16 B per 32 set-2 slots), then the
// keys (SURFHIP_MATCH_MUTUAL: one 64-bit word per set-2 slot, cleared on s).
size_t match_batch_scratch_bytes(int mode, int npairs, int slots2, int flags);
hipError_t launch_match_batch(const MatchBatch& b, int mode, void* scratch, hipStream_t s);
// Batched RANSAC homographies and fundamental matrices (surfhip_ransac.inc,
// with the model of surfhip_homography.hip or surfhip_fundamental.hip): one
// workgroup per pair on the match fields of its set-1 points; kRansacCap
// candidates per pair stay in LDS, more are re-read from the point array.
constexpr int kRansacCap = 3072;
hipError_t launch_homography_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                   float thresh, int nhyp, uint32_t seed, surfhip_homography* out, uint8_t* inlier,
                                   hipStream_t s);
hipError_t launch_fundamental_batch(const surfhip_point* pts, const int* counts, int slots, int npairs, float max_amb,
                                    float thresh, int nhyp, uint32_t seed, surfhip_fundamental* out, uint8_t* inlier,
                                    hipStream_t s);
// bytes ahead of a result slab's points: int32 header[4], then the frames' counts padded to 16 B
inline size_t slab_head_bytes(int nframes) { return 16 + (((size_t)nframes * 4 + 15) & ~(size_t)15); }
// (sch.offsets: the prefix of counts, as the batch's launch_sort left it)
hipError_t launch_pack(const surfhip_point* pts, const float* desc, const int* counts, const DescribeSchedule& sch,
                       int nframes, int max_pts, int nfeat, const int* status, size_t cap_bytes, uint8_t* slab,
                       hipStream_t s);

}  // namespace surfhip
