/*
 * surfhip.h -- the C-ABI boundary of the MI355X SURF engine (libsurfhip.so).
 *
 * Plain C: plain pointers, sizes and int status codes; no HIP, torch or C++
 * types.  Device pointers are `void*`/typed pointers into HBM allocated with
 * surfhip_malloc (or by any HIP user in the same process, e.g. PyTorch).
 *
 * Every entry point names the reference interface it replaces (file:line in
 * the CUDA-SURF reference).  The C++ drop-in layer (include/surf.h,
 * include/cuda_utils.h, cuda-surf_amd/csrc/surf.cpp) is built only on these.
 */
#ifndef SURFHIP_H
#define SURFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (replaces cudaError_t in CHECK(), cuda_utils.h:18-25) */
#define SURFHIP_OK               0
#define SURFHIP_ERR_INVALID     -1   /* bad argument / shape              */
#define SURFHIP_ERR_HIP         -2   /* HIP runtime error (see last error) */
#define SURFHIP_ERR_CAPACITY    -3   /* candidate buffer overflowed        */
#define SURFHIP_ERR_UNSUPPORTED -4   /* option outside the built path      */
#define SURFHIP_ERR_NOMEM       -5

/* copy kinds (cudaMemcpyKind) */
#define SURFHIP_H2H 0
#define SURFHIP_H2D 1
#define SURFHIP_D2H 2
#define SURFHIP_D2D 3

#ifdef __cplusplus
#define SURFHIP_BOOL bool
#else
#define SURFHIP_BOOL _Bool
#endif

/* Byte-identical to surf::SurfParam (surf_structures.h:45-72, 48 B). */
typedef struct surfhip_param {
    float thresh;
    int   init_lobe;
    SURFHIP_BOOL doubled;
    int   max_scale;
    int   noctaves;
    int   sampling;
    float divisor;
    SURFHIP_BOOL upright;
    SURFHIP_BOOL extend;
    int   desc_wsz;
    int   mag_factor;
    int   orient_size;
    int   nfeatures;
} surfhip_param;

/* Byte-identical to surf::SurfPoint (surf_structures.h:10-30, 48 B). */
typedef struct surfhip_point {
    float x, y, scale;
    int   o;
    float strength;
    int   laplace;
    float ori, score;
    int   match;
    float match_x, match_y, ambiguity;
} surfhip_point;

/* ------------------------------------------------------------ runtime --
 * Replaces cuda_utils.h:41-108 (initDevice, GpuTimer) and the cudart calls
 * main.cpp makes through it (main.cpp:16, 97, 100, 155, 219-226, 273-281). */
const char* surfhip_error_string(int status);     /* cudaGetErrorString      */
int  surfhip_last_hip_error(void);                /* raw hipError_t of the last failure */
int  surfhip_get_device_count(int* count);        /* cudaGetDeviceCount      */
int  surfhip_set_device(int dev);                 /* cudaSetDevice           */
int  surfhip_get_device(int* dev);
int  surfhip_device_name(int dev, char* buf, int len, int* cu_count);
int  surfhip_versions(int* driver, int* runtime); /* cudaDriver/RuntimeGetVersion */
int  surfhip_malloc(void** ptr, size_t bytes);    /* cudaMalloc              */
int  surfhip_malloc_pitch(void** ptr, size_t* pitch, size_t width_bytes, size_t height); /* cudaMallocPitch */
int  surfhip_free(void* ptr);                     /* cudaFree                */
int  surfhip_memset(void* ptr, int value, size_t bytes);             /* cudaMemset */
int  surfhip_memset_async(void* ptr, int value, size_t bytes, void* stream);
int  surfhip_memcpy(void* dst, const void* src, size_t bytes, int kind);  /* cudaMemcpy */
int  surfhip_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream);
int  surfhip_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width_bytes, size_t height, int kind);     /* cudaMemcpy2D */
int  surfhip_device_synchronize(void);            /* cudaDeviceSynchronize   */
int  surfhip_device_reset(void);                  /* cudaDeviceReset         */
int  surfhip_stream_create(void** stream);
int  surfhip_stream_destroy(void* stream);
int  surfhip_stream_synchronize(void* stream);
int  surfhip_event_create(void** ev);             /* cudaEventCreate (GpuTimer) */
int  surfhip_event_destroy(void* ev);
int  surfhip_event_record(void* ev, void* stream);
int  surfhip_event_synchronize(void* ev);
int  surfhip_stream_wait_event(void* stream, void* ev);  /* cudaStreamWaitEvent */
int  surfhip_event_elapsed(float* ms, void* start, void* stop);

/* ----------------------------------------------------------- detector --
 * One detector = one geometry (W x H) + SurfParam + scratch for up to
 * max_batch frames, bound to one HIP stream.  Replaces the process-global
 * __constant__/__device__ state of surfd.cu:13-24 and the scratch members of
 * Surfor (surf.h:43-53), so several detectors (one per GPU / host thread)
 * can coexist. */
typedef struct surfhip_detector surfhip_detector;

/* Surfor::init + allocMemory (surf.cpp:60-91, 374-415).  `param` must come
 * from surfhip_make_param.  Frames up to 8,191 columns (after doubling) and
 * octave-0 sample grids below 16,384 x 16,384 (NMS record fields);
 * SURFHIP_ERR_UNSUPPORTED otherwise.  cand_cap = per-frame candidate capacity before
 * the canonical sort, rounded up to a power of 2 (0 = max(max_pts, 16384)).
 * stream = hipStream_t or NULL. */
int surfhip_detector_create(surfhip_detector** det, const surfhip_param* param,
                            int width, int height, int max_batch, int max_pts,
                            int cand_cap, void* stream);
int surfhip_detector_destroy(surfhip_detector* det);
int surfhip_detector_set_stream(surfhip_detector* det, void* stream);

/* Surfor::init parameter derivation (surf.cpp:63-79); returns
 * SURFHIP_ERR_UNSUPPORTED for max_scale != 5 or more than 128 features;
 * doubled = true doubles the sampling step and halves the divisor. */
int surfhip_make_param(surfhip_param* out, int noctaves, float thresh, int doubled,
                       int init_mask_size, int sampling_step, int upright,
                       int extend, int desc_wsz);

/* Batched detect+describe, asynchronous on the detector's stream.
 * Replaces the per-frame sequence cuIntegral (surfd.cu:2683) ->
 * cuHalfImage/cuCalcHessianMulti/cuFindMaximumWithInterp per octave
 * (surf.cpp:248-294, surfd.cu:2775, 2829, 3058) -> cuDescribe (surfd.cu:3251).
 *   d_frames : nframes u8 frames, row pitch `pitch` bytes (>= W, multiple of
 *              16), frame f at d_frames + f*frame_stride (16-B aligned;
 *              frame_stride >= pitch*H and a multiple of 16 when nframes >
 *              1).  Pad bytes past column W and bytes between frames are
 *              never used, whatever they hold.  Any size the detector was
 *              created with is supported: widths to 8,191 columns (after
 *              doubling) and any height whose octave-0 sample grid stays
 *              below 16,384 rows (about 65,000 rows at sampling_step 4),
 *              frames of 32,767 rows and more included -- for those the
 *              laplace sign is taken in the fit, not in the describe kernel
 *              (its stash holds 16-bit coordinates); SURFHIP_ERR_INVALID for
 *              a layout outside this contract
 *   d_points : [nframes][max_pts] SurfPoint slots (device)
 *   d_desc   : [nframes][max_pts][nfeatures] f32 (device) or NULL (desc=false)
 *   d_counts : [nframes] int (device): keypoints kept per frame
 * Keypoints of a frame are in canonical order (octave, nms level, row, col);
 * descriptors are L2-normalised (surfd.cu:2447-2493). */
int surfhip_detect_batch(surfhip_detector* det, const uint8_t* d_frames, int nframes,
                         int pitch, size_t frame_stride, surfhip_point* d_points,
                         float* d_desc, int* d_counts);

/* detect_batch with the next batch's integral image computed on the
 * detector's side stream beside this batch's describe stage (software
 * pipelining across batches).  The next call that passes the same
 * next_frames (pointer, count, pitch, stride) as its `d_frames` uses the
 * prefetched integral instead of computing it.  next_frames must hold their
 * data when this call is made (in the detector stream's order) and stay
 * unchanged until that next call, or until surfhip_detector_drain; NULL =
 * detect_batch.  Doubled detectors compute every integral in line. */
int surfhip_detect_batch_next(surfhip_detector* det, const uint8_t* d_frames, int nframes,
                              int pitch, size_t frame_stride, surfhip_point* d_points,
                              float* d_desc, int* d_counts, const uint8_t* d_next_frames,
                              int next_nframes, int next_pitch, size_t next_frame_stride);

/* Orders the detector's side-stream work (a pending prefetch of the next
 * batch's integral, which reads next_frames) before anything later on the
 * detector's stream: after drain, synchronising that stream means
 * next_frames are no longer read.  The prefetch stays valid. */
int surfhip_detector_drain(surfhip_detector* det);

/* Record `event` (a surfhip_event_create / hipEvent_t) on the detector's
 * stream right before the describe stage of every following detect_batch /
 * detect_batch_next call (NULL: no longer).  A multi-GPU caller makes its
 * comm stream wait on it so the previous batch's all-gather lands beside the
 * latency-bound describe instead of the HBM-bound Hessian and NMS (SURVEY
 * 8e; no reference counterpart). */
int surfhip_detector_set_describe_event(surfhip_detector* det, void* event);

/* Surfor::detectAndCompute (surf.cpp:205-355) for one frame, synchronous.
 * Writes min(found, max_pts) SurfPoints to d_points, returns the count in
 * *num_pts; when desc != 0 allocates *d_desc_out = num_pts*nfeatures floats
 * (caller frees with surfhip_free, as main.cpp:275-282 does with cudaFree).
 * A frame with more NMS survivors than the candidate capacity returns
 * SURFHIP_OK with the first cand_cap survivors in scan order (as the
 * reference returns some max_pts points without a signal, surfd.cu:822-831):
 * callers that must know query surfhip_detector_status (the C++ Surfor
 * prints a warning). */
int surfhip_detect(surfhip_detector* det, const uint8_t* d_image, int pitch,
                   surfhip_point* d_points, int max_pts, int* num_pts,
                   float** d_desc_out, int desc);

/* Raw candidate count per frame of the last call (before the max_pts clamp,
 * surf.cpp:302-303); host array of nframes ints.  Returns
 * SURFHIP_ERR_CAPACITY (counts still written) when the last batch truncated
 * a frame at the candidate capacity. */
int surfhip_detector_candidates(surfhip_detector* det, int* h_counts, int nframes);

/* Did the last detect_batch / detect drop accepted candidates because a
 * frame had more NMS survivors than the candidate capacity (cand_cap of
 * surfhip_detector_create, rounded up to a power of 2)?  Such a frame keeps
 * its first cand_cap survivors in scan order -- deterministic -- sorted
 * canonically, then the first max_pts (the reference keeps an arbitrary
 * subset, surfd.cu:822-831).  The flag is reset by every batch. */
int surfhip_detector_status(surfhip_detector* det, int* truncated);
int surfhip_detector_capacity(surfhip_detector* det, int* cand_cap);

/* The per-frame keypoint budget: which points of a frame are kept when it
 * holds more than n.  The candidates considered are the frame's valid ones
 * among its first cand_cap NMS survivors in scan order; the kept points are
 * always written in canonical order and the count is min(valid, n).
 *   SURFHIP_KEEP_FIRST      the first n in canonical order (octave 0 first).
 *   SURFHIP_KEEP_STRONGEST  the n strongest, selected on the device between
 *       the fit and the sort, before anything is described.  Strengths are
 *       ordered by m(u) = u ^ ((u >> 31) ? 0xffffffff : 0x80000000) of their
 *       IEEE bits (a total order: -0.0 below +0.0, a NaN has its place);
 *       candidate a beats b when m(a.strength) > m(b.strength), or when they
 *       are equal and a is the earlier in canonical order.  The result is the
 *       same bits from run to run and at every position of a batch.
 * n: 0 = max_pts, else 1 .. max_pts.  SURFHIP_ERR_INVALID for any other n, an
 * unknown mode or a NULL detector (the setting stays as it was).  Host state
 * only (no GPU call, no synchronisation): it applies to every later
 * detect_batch, detect_batch_next, detect, run_nms and ingest submit of the
 * detector and may be changed between calls.  A new detector is
 * (SURFHIP_KEEP_FIRST, max_pts); get_keep reports the resolved n, never 0.
 * Slot strides (d_points, d_desc, slabs) stay max_pts whatever n is; laplace,
 * ori, descriptors, offsets, surfhip_batch_total and the pack functions
 * follow the kept set.  Dropping points by n never sets `truncated`
 * (surfhip_detector_status), and surfhip_detector_candidates keeps returning
 * the raw counts: candidates[f] - counts[f] points of frame f were dropped. */
#define SURFHIP_KEEP_FIRST     0
#define SURFHIP_KEEP_STRONGEST 1
int surfhip_detector_set_keep(surfhip_detector* det, int mode, int n);
int surfhip_detector_get_keep(surfhip_detector* det, int* mode, int* n);

/* Stage timing (HIP events on the detector's stream) for the last
 * detect_batch: ms[0..5] = integral, hessian, nms, sort, describe, total. */
#define SURFHIP_NSTAGE 6
int surfhip_detector_set_profiling(surfhip_detector* det, int on);
int surfhip_detector_stage_times(surfhip_detector* det, float* ms);

/* In-step Hessian timing: with `on`, every following detect_batch records a
 * HIP event pair on the detector's stream around its Hessian launches, in
 * their normal (pipelined) arrangement -- the integral runs beside them on
 * the side stream -- for up to SURFHIP_MAX_HESS_EV batches.
 * surfhip_detector_hessian_times waits for them, writes the per-batch
 * milliseconds to ms[0..*n) and starts a new record. */
#define SURFHIP_MAX_HESS_EV 64
int surfhip_detector_time_hessian(surfhip_detector* det, int on);
int surfhip_detector_hessian_times(surfhip_detector* det, float* ms, int max, int* n);

/* Workspace access for parity tests: device pointers to frame 0's integral
 * image ((H+1) x ipitch int32, frame stride ii_stride ints) and response
 * planes (resp_stride floats per frame; octave o plane s at
 * ooff[o] + s*osize[o], row pitch swhp[o].z). */
int surfhip_detector_workspace(surfhip_detector* det, int32_t** d_ii, size_t* ii_stride,
                               float** d_resp, size_t* resp_stride);
int surfhip_detector_geometry(surfhip_detector* det, int* iwhp /*3*/, int* swhp /*3*8*/,
                              long long* ooff /*8*/, int* osize /*8*/);
/* The row sums the integral-writing Hessian kernel adds to its strips'
 * local integrals, as the last batch left them (parity tests): device
 * pointer to [max_batch][nstrips][rows] uint32, slab k row r = the sum of
 * pixel row r over the columns left of writer strip k's first halo column
 * (slab 0 and rows >= H zero).  *source: 0 = the plan has none (pointer NULL,
 * counts 0), 1 = k_ii_rowseg's pass over the frames, 2 = k_hess_p0's
 * producers (+ k_rowsum_p0). */
int surfhip_detector_rowsums(surfhip_detector* det, uint32_t** d_rowseg, int* nstrips, int* rows,
                             int* source);

/* Stage-level entry points on frames already resident (parity tests and the
 * Hessian roofline run): integral only, Hessian only.  run_hessian needs a
 * prior run_integral (or detect_batch) on frames that are still live: the
 * u8 Hessian kernels re-read those frames (SURFHIP_ERR_INVALID if there were
 * none). */
int surfhip_run_integral(surfhip_detector* det, const uint8_t* d_frames, int nframes,
                         int pitch, size_t frame_stride);
int surfhip_run_hessian(surfhip_detector* det, int nframes);

/* The describe stage alone, on caller-given points and the integral images
 * the last run_integral or detect_batch left resident (SURFHIP_ERR_INVALID if
 * there was none): d_points[nframes][max_pts], frame f's first
 * clamp(d_counts[f], 0, max_pts) slots in slot order, described into
 * d_desc[nframes][max_pts][nfeatures] with the kernel, grid and schedule a
 * detect_batch of nframes frames would use (the order array is the
 * identity).  A rotated detector also writes `ori` of exactly those points;
 * no other point field, no slot at or past the count and no count is written
 * (the laplace sign stays the caller's).  Asynchronous on the detector's
 * stream.  The detector's batch schedule (surfhip_batch_total, the offsets
 * surfhip_pack_slab uses) is then that of these counts. */
int surfhip_run_describe(surfhip_detector* det, surfhip_point* d_points, const int* d_counts, int nframes,
                         float* d_desc);

/* The NMS stage alone (scan, prefix, fit, sort: findMaximumWithInterp,
 * surfd.cu:676-832) on what is resident: the response planes in the
 * detector's workspace (surfhip_detector_workspace's d_resp, frame f at
 * d_resp + f * resp_stride; the caller may have overwritten them) and the
 * integral images the last run_integral or detect_batch left
 * (SURFHIP_ERR_INVALID if there was none), with the launches a detect_batch
 * of nframes frames without descriptors makes: the laplace sign is taken in
 * the fit.  Planes 0 / 1 of octaves > 0 are read as views of the previous
 * octave's planes 2 / 4 at (2r, 2c), never from their own storage, and no
 * pad column [sw, sp) is read.  d_points[nframes][max_pts] and
 * d_counts[nframes] are written as detect_batch writes them (canonical
 * order, min(found, max_pts) per frame).  Asynchronous on the detector's
 * stream.  surfhip_detector_candidates, surfhip_detector_status and
 * surfhip_batch_total then answer for this run. */
int surfhip_run_nms(surfhip_detector* det, int nframes, surfhip_point* d_points, int* d_counts);

/* Algorithmic (compulsory) HBM bytes per frame of the Hessian stage:
 * integral image read once + valid responses written. */
long long surfhip_hessian_bytes_per_frame(surfhip_detector* det);

/* The Hessian stage's kernels for this detector's launch plan, as text
 * (e.g. "k_hess_q0 (octave 0) + k_hess_v1 (octave 1) + k_hess_far (octaves
 * 2-3)"), NUL-terminated in buf[len]; returns the full length. */
int surfhip_hessian_plan(surfhip_detector* det, char* buf, int len);

/* The run-time switches (the SURFHIP_* environment variables of
 * INTEGRATION.md) as text: "NAME=value" of each variable that is set, its
 * value normalised as the library takes it, separated by single spaces; ""
 * when none is.  A detector reads them once, when it is created:
 * surfhip_detector_switches gives what that detector holds,
 * surfhip_switches_from_env what one created now would (no GPU needed).
 * Like surfhip_hessian_plan, both return the full length and NUL-terminate
 * what fits in buf[len]. */
int surfhip_switches_from_env(char* buf, int len);
int surfhip_detector_switches(surfhip_detector* det, char* buf, int len);

/* Result slab for the multi-GPU all-gather, compacted to the
 * keypoints actually found by the last detect_batch:
 *   int32 {nframes, total, nfeatures (0 without descriptors), flags}
 *     (flags bit 0: a frame was truncated at the candidate capacity;
 *      bit 1: the slab exceeded surfhip_pack_slab_cap's capacity)
 *   int32 counts[nframes] padded to 16 B
 *   SurfPoint points[total]          (frame-major, canonical order)
 *   float desc[total][nfeatures]
 * surfhip_batch_total synchronises the stream and returns the batch's total
 * keypoint count (needed to size the collective). */
size_t surfhip_slab_bytes(int nframes, int total, int nfeatures);
int surfhip_batch_total(surfhip_detector* det, int nframes, int* total);
int surfhip_pack_slab(surfhip_detector* det, const surfhip_point* d_points, const float* d_desc,
                      const int* d_counts, int nframes, void* d_slab);
/* Both pack functions read the detector's per-batch offsets and status
 * word: enqueue them on the detector's stream BEFORE the next detect_batch
 * (which resets both), as bench.py and the ingest ring do.
 * The same into a buffer of cap_bytes, with no host synchronisation: the
 * multi-GPU path sizes every rank's slab once (a per-frame keypoint budget,
 * SURVEY.md 8e) and all-gathers that many bytes per batch.  A batch that
 * does not fit writes its header and counts with flags bit 1 set and no
 * payload; the receiver must check the flags. */
int surfhip_pack_slab_cap(surfhip_detector* det, const surfhip_point* d_points, const float* d_desc,
                          const int* d_counts, int nframes, void* d_slab, size_t cap_bytes);

/* ------------------------------------------------------------ matching --
 * Surfor::match (surf.cpp:418-428) -> cuFindMaxCorr (surfd.cu:3554-3566) ->
 * findMaxCorr (surfd.cu:2530-2656), asynchronous on `stream` (NULL = the
 * null stream).  For each of the n1 points of set 1 writes score (best dot
 * product), match (index into set 2, -1 when no score is positive),
 * match_x/match_y (that point's x, y; 0 for -1) and ambiguity
 * (second / (best + 1e-6)) -- the reference's per-thread-row top-2 and row
 * merge, bit-exact.  Descriptors: n x nfeatures f32 rows (nfeatures a
 * multiple of 4, 4 .. 1024; 16-B aligned).  flags:
 * SURFHIP_MATCH_FULL_TAIL also scores the last partial 32-point tile of set 2, which the reference drops
 * (surfd.cu:2569); 0 follows the reference.  Scratch (surfhip_match_scratch
 * bytes, device) is caller-provided (the call is then asynchronous), or
 * NULL: the library allocates it and the call returns after the stream has
 * finished the match. */
#define SURFHIP_MATCH_FULL_TAIL 1
size_t surfhip_match_scratch(int n1, int n2, int flags);
int surfhip_match(surfhip_point* d_pts1, const surfhip_point* d_pts2, const float* d_feat1,
                  const float* d_feat2, int n1, int n2, int nfeatures, int flags,
                  void* d_scratch, void* stream);

/* Batched matching (no reference counterpart: Surfor::match handles one
 * pair): pair i = frame i of set 1 against frame i of set 2, i in
 * [0, npairs), directly on the surfhip_detect_batch output layout with
 * slots = its max_pts:
 *   d_pts1    : [npairs][slots1] SurfPoint slots
 *   d_desc1   : [npairs][slots1][nfeatures] f32 (16-B aligned)
 *   d_counts1 : [npairs] int, read on the device; pair i uses
 *               n1 = clamp(d_counts1[i], 0, slots1)
 *   set 2     : the same shapes with slots2
 * For each pair the result is exactly what surfhip_match writes for that
 * pair: score, match (index within the set-2 frame, -1 when no score is
 * positive), match_x, match_y and ambiguity of the first n1 points of the
 * set-1 frame, bit-exact (the scores are the same k-ordered fp32 FMA chains,
 * computed by the f32 matrix instruction).  Nothing else is written: the
 * other fields of the points, slots at or past n1 and both descriptor
 * arrays stay untouched.  One launch, no scratch, no host synchronisation;
 * asynchronous on `stream`.
 * Consecutive frames of one batch: pass set 2 as the same three buffers
 * advanced by one frame (d_pts + slots, d_desc + slots * nfeatures,
 * d_counts + 1) and npairs = nframes - 1.  The buffers then overlap; this is
 * supported: only the five match fields of set-1 points are written and
 * only x, y and laplace of set-2 points are read.
 * flags: SURFHIP_MATCH_FULL_TAIL as above; SURFHIP_MATCH_SAME_LAPLACE (the
 * batched calls only) offers a set-2 point to a set-1 point's top-2 scan only when
 * their `laplace` fields are equal (the classic SURF sign-of-Laplacian
 * pruning); a skipped point keeps its position in its 32-point tile.
 * nfeatures: a multiple of 4, 4 .. 1024.  SURFHIP_ERR_INVALID for
 * npairs < 0, slots <= 0, a bad nfeatures, unknown flag bits, or a NULL
 * pointer with npairs > 0; npairs == 0 returns SURFHIP_OK without touching
 * the GPU.  For one or a few pairs surfhip_match, which splits set 2 over
 * the chip, is the faster call. */
#define SURFHIP_MATCH_SAME_LAPLACE 2
int surfhip_match_batch(surfhip_point* d_pts1, const float* d_desc1, const int* d_counts1, int slots1,
                        const surfhip_point* d_pts2, const float* d_desc2, const int* d_counts2, int slots2,
                        int npairs, int nfeatures, int flags, void* stream);

/* Batched matching with the mutual-best test (OpenCV's crossCheck): the
 * layouts, count clamping, flags, nfeatures rule and argument checks of
 * surfhip_match_batch, plus a scratch buffer.  For pair i with clamped
 * counts n1, n2, the scanned set-2 points [0, nscan) (nscan = n2 with
 * SURFHIP_MATCH_FULL_TAIL, else 32 * (n2 / 32)) and S(p1, p2) the score:
 *   forward  F(p1): the five fields surfhip_match_batch writes with the same
 *            flags, bit for bit.
 *   back     B(p2), p2 < nscan: the p1 in [0, n1) with the largest
 *            S(p1, p2) > 0 among the points p2 is offered to (all of them, or
 *            with SURFHIP_MATCH_SAME_LAPLACE those of equal `laplace`); the
 *            lowest p1 on a tie, -1 when there is none.  A NaN score never
 *            wins.  Every set-1 point below n1 takes part.
 *   output   point p1 gets F(p1), except that a match I >= 0 with B(I) != p1
 *            is cleared: match = -1, match_x = match_y = 0; its score and
 *            ambiguity stay the forward values.  The kept matches of a pair
 *            are injective (no two points share a partner), and
 *            surfhip_homography_batch skips the cleared ones.
 * Nothing else is written: not the other point fields, slots at or past n1,
 * the descriptors or set 2 (of which only x, y, laplace are read), so the
 * consecutive-frames layout (set 2 = set 1 advanced one frame) is supported
 * as in surfhip_match_batch.  Every score is computed once: the forward
 * kernel's score tiles also feed the back direction.  Results are the same
 * bits from run to run and at every position of a batch.
 * d_scratch: surfhip_match_batch_cross_scratch(npairs, slots1, slots2) bytes
 * of device memory, 16-B aligned (8 * npairs * slots2: one word per set-2
 * slot; 0 for non-positive arguments).  It may hold anything on entry; the
 * call clears it on `stream`.  Asynchronous on `stream`, no host
 * synchronisation.  SURFHIP_ERR_INVALID as surfhip_match_batch, and for a
 * NULL or misaligned d_scratch with npairs > 0; npairs == 0 returns
 * SURFHIP_OK without touching the GPU. */
size_t surfhip_match_batch_cross_scratch(int npairs, int slots1, int slots2);
int surfhip_match_batch_cross(surfhip_point* d_pts1, const float* d_desc1, const int* d_counts1, int slots1,
                              const surfhip_point* d_pts2, const float* d_desc2, const int* d_counts2, int slots2,
                              int npairs, int nfeatures, int flags, void* d_scratch, void* stream);

/* Batched matching inside a search window (OpenCV users know it as windowed
 * or guided matching): the layouts, count clamping, nfeatures rule and
 * overlap rule of surfhip_match_batch, for callers that know where a partner
 * can lie -- a tracker the largest motion between frames, a stereo caller the
 * disparity range on (nearly) one row.  Set-2 point p2 is offered to set-1
 * point p1 when
 *   p2 < nscan (as for surfhip_match_batch_cross),
 *   with SURFHIP_MATCH_SAME_LAPLACE their `laplace` fields are equal, and
 *   dx_min <= x2 - x1 <= dx_max and dy_min <= y2 - y1 <= dy_max: each
 *   difference one fp32 subtraction, all four comparisons inclusive.  A NaN
 *   difference (a NaN coordinate, inf - inf) is not offered.
 * A point that is not offered keeps its position in its 32-point tile.
 *   forward  surfhip_match_batch's per-thread-row top-2 scan and row merge
 *            over the offered points only, on the same k-ordered fp32 FMA
 *            chains.  A point with nothing offered gets match = -1 and
 *            score = match_x = match_y = ambiguity = 0.
 *   with SURFHIP_MATCH_MUTUAL  the back direction B(p2) and the clearing
 *            rule of surfhip_match_batch_cross, with this "offered".
 * The window {-inf, +inf, -inf, +inf} gives, for finite coordinates, the
 * bits of surfhip_match_batch, with SURFHIP_MATCH_MUTUAL those of
 * surfhip_match_batch_cross.  Only the five match fields of set-1 points
 * below n1 are written; x, y of set 1 and x, y, laplace of set 2 are read.
 * surfhip_detect_batch writes keypoints in the order octave, level, row,
 * column, so 32 consecutive points cover a narrow band of rows: the call
 * skips the 32 x 32 score tiles in which no pair can be offered (that changes
 * no bit of the result; with points in another order it skips less and is
 * as right).
 * window: host memory, read during the call.  d_scratch:
 * surfhip_match_batch_window_scratch(npairs, slots1, slots2, flags) bytes of
 * device memory, 16-B aligned, in any state on entry:
 *   16 * npairs * ceil(slots2 / 32)   the set-2 tiles' bounding boxes
 *   + 8 * npairs * slots2             with SURFHIP_MATCH_MUTUAL, the keys
 * and 0 for non-positive npairs or slots.  Asynchronous on `stream`, no host
 * synchronisation, no allocation.  SURFHIP_ERR_INVALID for everything
 * surfhip_match_batch rejects (flag bits other than 1 | 2 | 4 here), a NULL
 * window, a NaN bound or min > max on an axis (infinite bounds are allowed)
 * -- these for npairs == 0 too -- and a NULL or misaligned d_scratch with
 * npairs > 0; otherwise npairs == 0 returns SURFHIP_OK without touching the
 * GPU. */
typedef struct surfhip_match_window { float dx_min, dx_max, dy_min, dy_max; } surfhip_match_window;
#define SURFHIP_MATCH_MUTUAL 4   /* surfhip_match_batch_window, _guided, _epipolar */
size_t surfhip_match_batch_window_scratch(int npairs, int slots1, int slots2, int flags);
int surfhip_match_batch_window(surfhip_point* d_pts1, const float* d_desc1, const int* d_counts1, int slots1,
                               const surfhip_point* d_pts2, const float* d_desc2, const int* d_counts2, int slots2,
                               int npairs, int nfeatures, int flags, const surfhip_match_window* window,
                               void* d_scratch, void* stream);

/* Guided matching: surfhip_match_batch_window with the window measured from
 * each set-1 point's predicted position under a per-pair 3 x 3 homography
 * instead of from the point itself -- the second pass of a tracker whose
 * camera pans, rolls or zooms: detect -> window match ->
 * surfhip_homography_batch -> guided match inside a tight window, with the
 * matrices never leaving the device.  Layouts, count clamping, flags
 * (SURFHIP_MATCH_FULL_TAIL | SURFHIP_MATCH_SAME_LAPLACE | SURFHIP_MATCH_MUTUAL),
 * the nfeatures rule, the overlap rule for consecutive frames and the scratch
 * (layout and size: surfhip_match_batch_guided_scratch returns the numbers of
 * surfhip_match_batch_window_scratch) are those of surfhip_match_batch_window.
 * d_h: device memory, 4-byte aligned, read on the device in stream order, so
 * the output of a surfhip_homography_batch enqueued earlier on the same
 * stream can be passed directly.  Pair i uses the nine row-major floats at
 * d_h + i * h_stride, h_stride in floats: 16 for an array of
 * surfhip_homography (h is its first member; nothing else of the record is
 * read, not even status: a TOO_FEW / DEGENERATE record holds the identity and
 * so degrades to the plain window), 9 for packed matrices, any value >= 9, or
 * 0 for one matrix shared by all pairs.
 * Predicted position of (x1, y1), every written operation one fp32 rounding
 * (the order of surfhip_homography_batch's transfer error) and the quotients
 * IEEE:
 *   X = (h0*x1 + h1*y1) + h2;  Y = (h3*x1 + h4*y1) + h5;  W = (h6*x1 + h7*y1) + h8;
 *   u = X / W;  v = Y / W;
 * Set-2 point p2 is offered to set-1 point p1 when W > 0, p2 < nscan, with
 * SURFHIP_MATCH_SAME_LAPLACE their `laplace` fields are equal, and
 * dx_min <= x2 - u <= dx_max and dy_min <= y2 - v <= dy_max: one fp32
 * subtraction each, all comparisons inclusive, a NaN difference not offered.
 * W > 0 is false for W <= 0 and for a NaN W: such a point is offered nothing
 * whatever the window, the infinite one included, and gets match = -1 and
 * zeros (surfhip_homography_batch likewise counts w <= 0 as an outlier).  So
 * a matrix that holds a NaN, or is all zero, makes its pair match nothing,
 * deterministically.  Forward, back direction and SURFHIP_MATCH_MUTUAL
 * clearing are those of surfhip_match_batch_window over this "offered"; only
 * the five match fields of set-1 points below n1 are written.
 *   With the identity matrix and finite coordinates the result is, bit for
 *   bit, that of surfhip_match_batch_window with the same window and flags.
 *   With the infinite window as well it is that of surfhip_match_batch /
 *   surfhip_match_batch_cross, for points with W > 0.
 * The tile skipping works on the boxes of the predicted positions and, as in
 * the window call, changes no bit of the result.  Asynchronous on `stream`,
 * no host synchronisation, no allocation.  SURFHIP_ERR_INVALID for everything
 * surfhip_match_batch_window rejects and for an h_stride that is neither 0
 * nor >= 9 -- these for npairs == 0 too -- and for a NULL or misaligned d_h
 * or d_scratch with npairs > 0; otherwise npairs == 0 returns SURFHIP_OK
 * without touching the GPU. */
size_t surfhip_match_batch_guided_scratch(int npairs, int slots1, int slots2, int flags);
int surfhip_match_batch_guided(surfhip_point* d_pts1, const float* d_desc1, const int* d_counts1, int slots1,
                               const surfhip_point* d_pts2, const float* d_desc2, const int* d_counts2, int slots2,
                               int npairs, int nfeatures, int flags,
                               const float* d_h, int h_stride,
                               const surfhip_match_window* window, void* d_scratch, void* stream);

/* ---------------------------------------------------------- homography --
 * Batched RANSAC homographies (no reference counterpart: main.cpp:250-262
 * only draws the matches): one 3 x 3 matrix per frame pair from the match
 * fields surfhip_match_batch left in the set-1 points, asynchronous on
 * `stream`, one launch sequence, no scratch, no host synchronisation.
 *   d_pts1    : [npairs][slots1] SurfPoint slots, as surfhip_match_batch
 *               wrote them; only x, y, match, match_x, match_y and ambiguity
 *               are read, nothing is written
 *   d_counts1 : [npairs] int, read on the device, clamped to [0, slots1]
 *   d_out     : [npairs] results
 *   d_inlier  : [npairs][slots1] bytes or NULL: 1 for a final inlier, 0 for
 *               every other slot (slots at or past the count included)
 * A point below the count is a candidate when match >= 0 and ambiguity <=
 * max_ambiguity; candidates keep the order of their indices.  nhyp (1 ..
 * 4096) four-point hypotheses are drawn by a counter hash of (seed,
 * hypothesis index, ncand) alone, so a pair gives the same bits
 * wherever it sits in a batch and from run to run.  An inlier has a squared
 * transfer error in image 2 below inlier_thresh^2 (strict, fp32; a point
 * that projects to w <= 0 is an outlier).  The hypothesis with the most
 * inliers (the lowest index on a tie) is refined by exactly two rounds of a
 * Hartley-normalised least-squares DLT over the current inliers (fp64) and
 * a recount; h, ninliers, rms and the mask belong to the last round.
 * Fewer than 4 candidates: SURFHIP_HOMOG_TOO_FEW; no usable hypothesis or
 * refit (collinear or coincident points, |h33| vanishing against ||H||):
 * SURFHIP_HOMOG_DEGENERATE; both with h = identity, ninliers = 0, rms = 0
 * and a zero mask row.  The output never holds a NaN or an infinity.
 * SURFHIP_ERR_INVALID for npairs < 0, slots1 <= 0, nhyp outside 1 .. 4096,
 * an inlier_thresh or max_ambiguity that is not finite and positive, or a
 * NULL d_pts1 / d_counts1 / d_out with npairs > 0; npairs == 0 returns
 * SURFHIP_OK without touching the GPU. */
#define SURFHIP_HOMOG_OK          0
#define SURFHIP_HOMOG_TOO_FEW     1   /* fewer than 4 candidates */
#define SURFHIP_HOMOG_DEGENERATE  2   /* no usable hypothesis / refit */
typedef struct surfhip_homography {   /* 64 B */
    float h[9];        /* row-major, maps (x, y) -> (match_x, match_y); h[8] == 1.0f when status == OK */
    int   status;
    int   ncand;       /* points that passed the filter */
    int   ninliers;    /* of the final model */
    float rms;         /* rms transfer error of the final inliers, px */
    int   reserved[3]; /* written as 0 */
} surfhip_homography;
int surfhip_homography_batch(const surfhip_point* d_pts1, const int* d_counts1, int slots1,
                             int npairs, float max_ambiguity, float inlier_thresh,
                             int nhyp, uint32_t seed, surfhip_homography* d_out,
                             uint8_t* d_inlier, void* stream);
/* Candidates per pair the kernel keeps in LDS; pairs with more are still
 * exact, the rest is re-read from the point array. */
int surfhip_homography_lds_capacity(void);

/* --------------------------------------------------------- fundamental --
 * Batched RANSAC fundamental matrices (no reference counterpart): one 3 x 3
 * matrix F with (match_x, match_y, 1) F (x, y, 1)^T = 0 per frame pair, the
 * model of a stereo rig or of a camera that translates through a scene with
 * depth, from the match fields surfhip_match_batch left in the set-1
 * points, asynchronous on `stream`, one launch sequence, no scratch, no host
 * synchronisation.
 *   d_pts1    : [npairs][slots1] SurfPoint slots, as surfhip_match_batch
 *               wrote them; only x, y, match, match_x, match_y and ambiguity
 *               are read, nothing is written
 *   d_counts1 : [npairs] int, read on the device, clamped to [0, slots1]
 *   d_out     : [npairs] results
 *   d_inlier  : [npairs][slots1] bytes or NULL: 1 for a final inlier, 0 for
 *               every other slot (slots at or past the count included)
 * A point below the count is a candidate when match >= 0 and ambiguity <=
 * max_ambiguity; candidates keep the order of their indices.
 *
 * Distance: the squared Sampson distance of (x, y) -> (u, v) = (match_x,
 * match_y) under f, in fp32, every written operation rounded once:
 *   a  = (f0*x + f1*y) + f2;   b  = (f3*x + f4*y) + f5;   c = (f6*x + f7*y) + f8;
 *   a' = (f0*u + f3*v) + f6;   b' = (f1*u + f4*v) + f7;
 *   r  = (u*a + v*b) + c;      d  = (a*a + b*b) + (a'*a' + b'*b');
 *   e2 = (r*r) / d;            inlier  <=>  e2 < inlier_thresh^2
 * (strict; d == 0 or any NaN: outlier).
 *
 * Search: nhyp (1 .. 4096) eight-point hypotheses, their samples drawn by a
 * counter hash of (seed, hypothesis index, ncand) alone, so a
 * pair gives the same bits wherever it sits in a batch and from run to run.
 * A hypothesis is the null vector of the 8 x 9 epipolar system of its
 * Hartley-normalised sample (fp64), de-normalised, scaled to Frobenius norm
 * 1, stored as fp32; it is not rank-2 projected.  A sample with coincident
 * points or whose system has no one-dimensional null space (last pivot <=
 * 1e-7 of the first under full pivoting) scores nothing.  The hypothesis
 * with the most inliers wins, the lowest index on a tie.
 *
 * Refinement: exactly two rounds, the first over the winner's inliers: the
 * Hartley-normalised 8-point least squares over the current inliers (fp64:
 * the eigenvector of the smallest eigenvalue of the 9 x 9 normal matrix),
 * the smallest singular value of that matrix set to 0, de-normalised, scaled
 * to Frobenius norm 1, the entry of largest magnitude (the lowest index on a
 * tie) positive, stored as fp32; then a recount over all candidates.  f,
 * ninliers, rms and the mask belong to the second round's recount under the
 * f that is returned.
 *
 * Fewer than 8 candidates: SURFHIP_FUND_TOO_FEW.  No hypothesis with 8
 * inliers, a round with fewer than 8 inliers, coincident inliers, a normal
 * matrix whose second smallest eigenvalue is <= 1e-12 of its largest (the
 * inliers do not determine F: all on one line, say), a non-finite result or
 * a vanishing norm: SURFHIP_FUND_DEGENERATE.  Both with f all zero (under
 * which nothing is an inlier), ninliers = 0, rms = 0 and a zero mask row.
 * The output never holds a NaN or an infinity.
 * SURFHIP_ERR_INVALID for npairs < 0, slots1 <= 0, nhyp outside 1 .. 4096,
 * an inlier_thresh or max_ambiguity that is not finite and positive, or a
 * NULL d_pts1 / d_counts1 / d_out with npairs > 0; npairs == 0 returns
 * SURFHIP_OK without touching the GPU. */
#define SURFHIP_FUND_OK          0
#define SURFHIP_FUND_TOO_FEW     1   /* fewer than 8 candidates */
#define SURFHIP_FUND_DEGENERATE  2   /* no usable hypothesis / refit */
typedef struct surfhip_fundamental {  /* 64 B, same offsets as surfhip_homography */
    float f[9];        /* row-major; (match_x, match_y, 1) F (x, y, 1)^T = 0; ||f|| = 1, rank 2 when status == OK */
    int   status;
    int   ncand;       /* points that passed the filter */
    int   ninliers;    /* of the final model */
    float rms;         /* root mean squared Sampson distance of the final inliers, px */
    int   reserved[3]; /* written as 0 */
} surfhip_fundamental;
int surfhip_fundamental_batch(const surfhip_point* d_pts1, const int* d_counts1, int slots1,
                              int npairs, float max_ambiguity, float inlier_thresh,
                              int nhyp, uint32_t seed, surfhip_fundamental* d_out,
                              uint8_t* d_inlier, void* stream);
/* Candidates per pair the kernel keeps in LDS; pairs with more are still
 * exact, the rest is re-read from the point array. */
int surfhip_fundamental_lds_capacity(void);

/* Epipolar matching: surfhip_match_batch_window with, beside the window, a
 * band along each set-1 point's epipolar line under a per-pair fundamental
 * matrix -- the second pass of a stereo rig or of a camera that translates:
 * match -> surfhip_fundamental_batch -> epipolar match, with the matrices
 * never leaving the device.  The best partner on the line may be the third
 * best overall, so this cannot be had by filtering the matches of a plain
 * call.  Layouts, count clamping, flags (SURFHIP_MATCH_FULL_TAIL |
 * SURFHIP_MATCH_SAME_LAPLACE | SURFHIP_MATCH_MUTUAL), the nfeatures rule, the
 * overlap rule for consecutive frames and the scratch (layout and size:
 * surfhip_match_batch_epipolar_scratch returns the numbers of
 * surfhip_match_batch_window_scratch) are those of surfhip_match_batch_window.
 * d_f: device memory, 4-byte aligned, read on the device in stream order, so
 * the output of a surfhip_fundamental_batch enqueued earlier on the same
 * stream can be passed directly.  Pair i uses the nine row-major floats at
 * d_f + i * f_stride, f_stride in floats: 16 for an array of
 * surfhip_fundamental (f is its first member; nothing else of the record is
 * read, not even status), 9 for packed matrices, any value >= 9, or 0 for one
 * matrix shared by all pairs.  F has the convention of
 * surfhip_fundamental_batch: (x2, y2, 1) F (x1, y1, 1)^T = 0.
 * Set-2 point p2 is offered to set-1 point p1 when
 *   p2 < nscan,
 *   with SURFHIP_MATCH_SAME_LAPLACE their `laplace` fields are equal,
 *   dx_min <= x2 - x1 <= dx_max and dy_min <= y2 - y1 <= dy_max around the raw
 *   (x1, y1), as in surfhip_match_batch_window (the infinite window switches
 *   this off; a stereo caller puts the disparity range here), and
 *   (x2, y2) lies within `band` pixels of p1's epipolar line, tested squared
 *   and cross-multiplied, every written operation one fp32 rounding:
 *     a = (f0*x1 + f1*y1) + f2;  b = (f3*x1 + f4*y1) + f5;  c = (f6*x1 + f7*y1) + f8;
 *     lim = (band * band) * (a*a + b*b);
 *     r = (x2*a + y2*b) + c;     offered  <=>  r*r <= lim
 *   (inclusive; any NaN: not offered).  a, b, c are the Sampson a, b, c above.
 * Forward, back direction and SURFHIP_MATCH_MUTUAL clearing are those of
 * surfhip_match_batch_window over this "offered"; only the five match fields
 * of set-1 points below n1 are written.  There is no special case for a
 * degenerate line; the arithmetic as written decides:
 *   An all-zero matrix (what a TOO_FEW / DEGENERATE surfhip_fundamental holds)
 *   gives, for finite coordinates, a = b = c = r = lim = 0 and 0 <= 0: the
 *   result is, bit for bit, that of surfhip_match_batch_window with the same
 *   window and flags -- a failed F degrades to the plain window, as a failed
 *   homography does in the guided call.
 *   The rectified matrix (0,0,0, 0,0,-1, 0,1,0) gives a = 0, b = -1, c = y1 and
 *   r = -(y2 - y1) exactly: with the window (dx_min, dx_max, -inf, +inf) and
 *   band B the result is, bit for bit, that of surfhip_match_batch_window
 *   with (dx_min, dx_max, -B, B), for finite coordinates and a B with
 *   |d| <= B <=> d*d <= B*B in fp32 (1.5, say).
 *   A matrix that holds a NaN offers nothing: its pair's points get
 *   match = -1 and zeros.
 * band = 0 is valid: only r*r == 0 is offered.
 * The tile skipping of the window call applies as it is, and a 32 x 32 score
 * tile is also skipped when none of its set-1 points' lines can come within
 * the band of the tile's bounding box (r at the box's four corners bounds r
 * over the box; a NaN keeps the tile).  That changes no bit of the result.
 * The boxes of surfhip_detect_batch's point order are bands of rows, so the
 * line test prunes for lines that run along the rows (stereo); for steep
 * lines only the window prunes.  Asynchronous on `stream`, no host
 * synchronisation, no allocation.  SURFHIP_ERR_INVALID for everything
 * surfhip_match_batch_window rejects, for an f_stride that is neither 0 nor
 * >= 9 and for a band that is NaN, infinite or negative -- these for
 * npairs == 0 too -- and for a NULL or misaligned d_f or d_scratch with
 * npairs > 0; otherwise npairs == 0 returns SURFHIP_OK without touching the
 * GPU. */
size_t surfhip_match_batch_epipolar_scratch(int npairs, int slots1, int slots2, int flags);
int surfhip_match_batch_epipolar(surfhip_point* d_pts1, const float* d_desc1, const int* d_counts1, int slots1,
                                 const surfhip_point* d_pts2, const float* d_desc2, const int* d_counts2, int slots2,
                                 int npairs, int nfeatures, int flags,
                                 const float* d_f, int f_stride, float band,
                                 const surfhip_match_window* window, void* d_scratch, void* stream);

/* ------------------------------------------------------------- ingest --
 * Pipelined host-frame ingest.  Replaces the
 * per-frame blocking cudaMemcpy2D of a pageable frame (main.cpp:212-226) and
 * the blocking per-frame point copy-back (surf.cpp:335-342) with a ring of
 * `depth` pinned host frame slots / HBM frame slots / result slabs:
 *   acquire  -> pinned u8 slot [max_batch][H][pitch], pitch = align128(W)
 *               (SURFHIP_ERR_CAPACITY when `depth` batches await collect)
 *   submit   -> H2D on a copy stream, detect+describe on the detector's
 *               stream after that copy only, pack into the slot's slab
 *   collect  -> oldest batch's compacted result slab (format above) in
 *               pinned host memory, valid until that slot is collected again
 * Results are bit-identical to surfhip_detect_batch + surfhip_pack_slab. */
#define SURFHIP_INGEST_MAX_DEPTH 8
typedef struct surfhip_ingest surfhip_ingest;
int surfhip_ingest_create(surfhip_ingest** ing, surfhip_detector* det, int depth);
int surfhip_ingest_destroy(surfhip_ingest* ing);
int surfhip_ingest_acquire(surfhip_ingest* ing, uint8_t** h_frames, int* pitch, size_t* frame_stride);
int surfhip_ingest_submit(surfhip_ingest* ing, int nframes);
int surfhip_ingest_collect(surfhip_ingest* ing, const void** h_slab, size_t* bytes);
int surfhip_ingest_pending(surfhip_ingest* ing, int* n);

/* --------------------------------------------------------------- dump --
 * On-disk keypoint + descriptor file (no reference counterpart: main.cpp
 * only draws the points, main.cpp:21-71).  A file is a sequence of records;
 * a record is this 64-B little-endian header followed by slab_bytes of one
 * result slab exactly as surfhip_pack_slab / surfhip_ingest_collect return
 * it.  surfhip_dump_append appends one record (creating the file). */
#define SURFHIP_DUMP_MAGIC "SURFKPD1"
#define SURFHIP_DUMP_VERSION 1
typedef struct surfhip_dump_header {
    char     magic[8];              /* "SURFKPD1"                         */
    uint32_t header_bytes;          /* 64                                 */
    uint32_t version;               /* 1                                  */
    uint32_t width, height;         /* frame size                         */
    uint32_t nframes, nfeatures;    /* nfeatures 0: no descriptors        */
    uint64_t total;                 /* keypoints in the slab              */
    uint64_t slab_bytes;            /* bytes following this header       */
    uint64_t first_frame;           /* caller's index of the first frame  */
    float    thresh;
    uint8_t  noctaves, upright, extend, doubled;
} surfhip_dump_header;
int surfhip_dump_append(const char* path, const void* h_slab, size_t bytes, int width, int height,
                        const surfhip_param* param, long long first_frame);

/* Measured HBM stream rates (SURVEY 8d "also report measured peak from an
 * in-repo stream-copy kernel"; no reference counterpart).  One launch of a
 * 16-B-per-lane streaming kernel over `bytes` (a multiple of 16, src and dst
 * 16-B aligned) on `stream`, all 256 CUs, grid-stride:
 *   mode 0 copy  src -> dst  (moves 2 x bytes: read + write)
 *   mode 1 read  src only    (dst written only if a running XOR hits a
 *                             64-bit magic: never, for practical data)
 *   mode 2 write dst only    (writes bytes)
 * The caller times launches with events; surfhip_stream_bytes gives the HBM
 * bytes one launch of a mode moves. */
int surfhip_stream_run(int mode, const void* src, void* dst, size_t bytes, void* stream);
size_t surfhip_stream_bytes(int mode, size_t bytes);

/* Library build identification (for the loaded-.so audit). */
const char* surfhip_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SURFHIP_H */
