// surfhip_api.hip -- the C-ABI of libsurfhip.so (declared in include/surfhip.h).
//
// Host orchestration of the detect+describe path.  The reference does this
// per frame in Surfor::detectAndCompute (surf.cpp:205-355) with 22 symbol
// uploads, 4 blocking syncs, a cudaMalloc and two scratch memsets per frame;
// here a detector derives every parameter once at creation, owns HBM scratch
// for a whole batch of frames, and enqueues ~14 launches per batch on its own
// stream with no host synchronisation.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "surfhip.h"
#include "surfhip_internal.h"

using namespace surfhip;

static_assert(sizeof(surfhip_point) == 48, "SurfPoint layout (surf_structures.h:10-30)");
static_assert(sizeof(surfhip_param) == 48, "SurfParam layout (surf_structures.h:45-72)");
static_assert(offsetof(surfhip_param, doubled) == 8 && offsetof(surfhip_param, upright) == 28 &&
              offsetof(surfhip_param, extend) == 29 && offsetof(surfhip_param, nfeatures) == 44,
              "SurfParam field offsets");
static_assert(offsetof(surfhip_point, o) == 12 && offsetof(surfhip_point, laplace) == 20 &&
              offsetof(surfhip_point, ori) == 24 && offsetof(surfhip_point, ambiguity) == 44,
              "SurfPoint field offsets");

static_assert(sizeof(surfhip_dump_header) == 64, "dump record header");

static thread_local hipError_t g_last_hip = hipSuccess;

#define HIPCHK(x)                                    \
    do {                                             \
        hipError_t e_ = (x);                         \
        if (e_ != hipSuccess) {                      \
            g_last_hip = e_;                         \
            return SURFHIP_ERR_HIP;                  \
        }                                            \
    } while (0)

static inline int align_up(int a, int b) { return (a % b != 0) ? (a - a % b + b) : a; }  // cuda_utils.h:160-163

// How a plan orders its Hessian stage (hessian_stage), and where a call
// enqueues the next batch's prefetch (prefetch_place)
enum HessSched { kFused, kIntegralFirst, kSideStream };
enum Prefetch { kPrefNone, kPrefNms, kPrefDescribe };

// The detector's device memory: a buffer is named once, where it is allocated, and is freed with the detector
struct DeviceBuffers {
    std::vector<void*> owned;
    template <class T> hipError_t alloc(T*& ptr, size_t bytes)
    {
        const hipError_t e = hipMalloc((void**)&ptr, bytes);
        if (e == hipSuccess) owned.push_back(ptr);
        return e;
    }
    ~DeviceBuffers() { for (void* p : owned) (void)hipFree(p); }
};

struct surfhip_detector {
    DeviceBuffers mem;
    int dev = 0;
    int cus = 256;                      // compute units of dev (the describe kernels' persistent grid)
    hipStream_t stream = nullptr;
    surfhip_param param{};
    Switches sw;                        // the SURFHIP_* switches as they were when the detector was created
    FrameParams P{};
    OctaveParams oct[kMaxOct]{};
    OctaveParams* d_oct = nullptr;      // device copy read by the fused launches
    LaunchPlan plan{};
    HessSched sched = kFused;
    int W = 0, H = 0, max_batch = 0, max_pts = 0;   // W x H: the frames the integral is taken of
    int srcW = 0, srcH = 0;             // the caller's frames (= W x H unless doubled)
    uint8_t* dbl = nullptr;             // doubled: the (2 srcW - 2) x (2 srcH - 2) frames D
    int dpitch = 0;
    long long dstride = 0;
    int CW = 0;
    size_t tot_osize = 0;
    int32_t* ii = nullptr;              // integral of the last processed batch (one of iib)
    int32_t* iib[2] = {nullptr, nullptr};   // integral buffers: the batch's, and the next batch's prefetch
    int icur = 0;                       // iib index of ii
    // prefetched integral (surfhip_detect_batch_next): which frames, in iib[ipref]
    bool pref_valid = false;
    int ipref = 0;
    FrameBatch pref;
    hipEvent_t fork2 = nullptr;
    float* resp = nullptr;
    uint32_t* colsum = nullptr;
    // plan.iiw: k_ii_rowseg's row sums of the batch (or of the next batch,
    // prefetched) that k_hess_w adds to its strip integrals
    uint32_t* rowseg = nullptr;
    // plan.rsum: k_hess_p0's per-strip row sums of the batch, which
    // k_rowsum_p0 adds up into rowseg (no k_ii_rowseg pass, no prefetch)
    uint32_t* psum = nullptr;
    Candidates cands{};                 // launch_nms -> launch_sort
    KeepRule keep;                      // surfhip_detector_set_keep: (SURFHIP_KEEP_FIRST, max_pts) until set
    DescribeSchedule schedule{};        // launch_sort / launch_plant -> launch_describe, launch_pack
    int* pcount = nullptr;              // surfhip_run_describe: the caller's counts cut to [0, max_pts]
    // single-frame API slots
    surfhip_point* pts1 = nullptr;
    float* desc1 = nullptr;
    int* count1 = nullptr;
    bool profiling = false;
    hipEvent_t ev[SURFHIP_NSTAGE]{};
    hipStream_t side = nullptr;         // integral + integral-image Hessian kernels, beside the u8 ones
    hipEvent_t fork = nullptr, join = nullptr;
    bool time_hess = false;             // in-step Hessian event pairs (surfhip_detector_time_hessian)
    // per timed batch: [0] on the detector stream before the Hessian's fork,
    // [1] on it after the u8 kernels, [2] on the side stream after the
    // integral-image kernels (only when the plan has some: hev_side)
    hipEvent_t hev[SURFHIP_MAX_HESS_EV][3]{};
    hipEvent_t desc_ev = nullptr;       // caller's event, recorded before each describe stage
    bool hev_side[SURFHIP_MAX_HESS_EV]{};
    int hev_n = 0;
    FrameBatch last;                    // u8 source of the last integral (surfhip_run_hessian)
    long long hess_bytes = 0;

    ~surfhip_detector()                 // (then mem's buffers)
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& batch : hev)
            for (hipEvent_t e : batch)
                if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {fork, fork2, join})
            if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
};

// t into buf[len], cut to fit and NUL-terminated; returns the full length
static int text_out(const std::string& t, char* buf, int len)
{
    if (buf && len > 0) {
        const size_t n = std::min((size_t)len - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

// The switches in the order of Switches' fields (bit i of Switches::set), and their names
enum {
    kSwHessGather, kSwHessW, kSwQ01, kSwP0, kSwHessT0, kSwIIFuse, kSwRowsum, kSwDescUr, kSwTraceDesc, kSwRotAtomic,
    kSwSortBitonic, kSwPrefetch, kSwDescBeside, kSwU2LdsPad, kSwFitGrid, kSwFitCube, kSwIIBand, kSwIIBandSmall,
    kSwitches
};
static const char* const kSwitchNames[kSwitches] = {
    "SURFHIP_HESS_GATHER", "SURFHIP_HESS_W",      "SURFHIP_Q01",        "SURFHIP_P0",         "SURFHIP_HESS_T0",
    "SURFHIP_II_FUSE",     "SURFHIP_ROWSUM",      "SURFHIP_DESC_UR",    "SURFHIP_TRACE_DESC", "SURFHIP_ROT_ATOMIC",
    "SURFHIP_SORT_BITONIC", "SURFHIP_PREFETCH",   "SURFHIP_DESC_BESIDE", "SURFHIP_U2_LDSPAD", "SURFHIP_FIT_GRID",
    "SURFHIP_FIT_CUBE",    "SURFHIP_II_BAND",     "SURFHIP_II_BAND_SMALL"};

namespace surfhip {

Switches read_switches()
{
    Switches w;
    const char* v[kSwitches];
    for (int i = 0; i < kSwitches; i++)
        if ((v[i] = getenv(kSwitchNames[i])) != nullptr) w.set |= 1u << i;
    auto num = [&](int i, int dflt) { return v[i] ? atoi(v[i]) : dflt; };
    auto is = [&](int i, const char* text) { return v[i] && !strcmp(v[i], text); };
    if (v[kSwHessGather]) w.hess_gather = atoi(v[kSwHessGather]) != 0;
    w.hess_w = num(kSwHessW, w.hess_w) != 0;
    w.q01 = num(kSwQ01, w.q01) != 0;
    w.p0 = num(kSwP0, w.p0);
    if (w.p0 != 0 && w.p0 != 95 && w.p0 != 93 && w.p0 != 92 && w.p0 != 91 && w.p0 != 32) w.p0 = 93;
    w.hess_t0 = num(kSwHessT0, w.hess_t0) != 0;
    const int fuse = num(kSwIIFuse, w.ii_fuse);
    w.ii_fuse = fuse == 0 || fuse == 2 ? fuse : 1;
    w.rowsum_rowseg = is(kSwRowsum, "rowseg");
    if (v[kSwDescUr]) w.desc_ur = atoi(v[kSwDescUr]) != 0;
    w.trace_desc = num(kSwTraceDesc, w.trace_desc) != 0;
    w.rot_atomic = v[kSwRotAtomic] != nullptr;
    w.sort_bitonic = v[kSwSortBitonic] != nullptr;
    if (v[kSwPrefetch]) w.prefetch = is(kSwPrefetch, "describe");
    w.desc_beside = num(kSwDescBeside, w.desc_beside);
    w.u2_ldspad = num(kSwU2LdsPad, w.u2_ldspad);
    if (v[kSwFitGrid]) w.fit_grid = std::max(64, atoi(v[kSwFitGrid]));
    w.fit_cube = num(kSwFitCube, w.fit_cube) != 0;
    // a band height out of range counts as unset
    auto band = [&](int i, int lo, int hi, int& rows) {
        const int b = num(i, rows);
        if (b >= lo && b <= hi) rows = b;
        else w.set &= ~(1u << i);
    };
    band(kSwIIBand, 8, 64, w.ii_band);
    band(kSwIIBandSmall, 4, 32, w.ii_band_small);
    return w;
}

std::string switches_text(const Switches& w)
{
    const std::string val[kSwitches] = {
        std::to_string(w.hess_gather), std::to_string(w.hess_w),      std::to_string(w.q01),
        std::to_string(w.p0),          std::to_string(w.hess_t0),     std::to_string(w.ii_fuse),
        w.rowsum_rowseg ? "rowseg" : "p0", std::to_string(w.desc_ur), std::to_string(w.trace_desc),
        std::to_string(w.rot_atomic),  std::to_string(w.sort_bitonic), w.prefetch == 1 ? "describe" : "nms",
        std::to_string(w.desc_beside), std::to_string(w.u2_ldspad),   std::to_string(w.fit_grid),
        std::to_string(w.fit_cube),    std::to_string(w.ii_band),     std::to_string(w.ii_band_small)};
    std::string t;
    for (int i = 0; i < kSwitches; i++)
        if (w.set >> i & 1) t += (t.empty() ? "" : " ") + std::string(kSwitchNames[i]) + "=" + val[i];
    return t;
}

}  // namespace surfhip

extern "C" {

// ---------------------------------------------------------------- runtime

const char* surfhip_error_string(int status)
{
    switch (status) {
        case SURFHIP_OK: return "no error";
        case SURFHIP_ERR_INVALID: return "invalid argument";
        case SURFHIP_ERR_HIP: return hipGetErrorString(g_last_hip);
        case SURFHIP_ERR_CAPACITY: return "candidate capacity exceeded";
        case SURFHIP_ERR_UNSUPPORTED: return "unsupported option";
        case SURFHIP_ERR_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}

int surfhip_last_hip_error(void) { return (int)g_last_hip; }

int surfhip_get_device_count(int* count)
{
    HIPCHK(hipGetDeviceCount(count));
    return SURFHIP_OK;
}
int surfhip_set_device(int dev)
{
    HIPCHK(hipSetDevice(dev));
    return SURFHIP_OK;
}
int surfhip_get_device(int* dev)
{
    HIPCHK(hipGetDevice(dev));
    return SURFHIP_OK;
}
int surfhip_device_name(int dev, char* buf, int len, int* cu_count)
{
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    if (buf && len > 0) {
        snprintf(buf, (size_t)len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    return SURFHIP_OK;
}
int surfhip_versions(int* driver, int* runtime)
{
    HIPCHK(hipDriverGetVersion(driver));
    HIPCHK(hipRuntimeGetVersion(runtime));
    return SURFHIP_OK;
}
int surfhip_malloc(void** ptr, size_t bytes)
{
    HIPCHK(hipMalloc(ptr, bytes));
    return SURFHIP_OK;
}
int surfhip_malloc_pitch(void** ptr, size_t* pitch, size_t width_bytes, size_t height)
{
    HIPCHK(hipMallocPitch(ptr, pitch, width_bytes, height));
    return SURFHIP_OK;
}
int surfhip_free(void* ptr)
{
    HIPCHK(hipFree(ptr));
    return SURFHIP_OK;
}
int surfhip_memset(void* ptr, int value, size_t bytes)
{
    HIPCHK(hipMemset(ptr, value, bytes));
    return SURFHIP_OK;
}
int surfhip_memset_async(void* ptr, int value, size_t bytes, void* stream)
{
    HIPCHK(hipMemsetAsync(ptr, value, bytes, (hipStream_t)stream));
    return SURFHIP_OK;
}
static hipMemcpyKind kind_of(int k)
{
    switch (k) {
        case SURFHIP_H2H: return hipMemcpyHostToHost;
        case SURFHIP_H2D: return hipMemcpyHostToDevice;
        case SURFHIP_D2H: return hipMemcpyDeviceToHost;
        case SURFHIP_D2D: return hipMemcpyDeviceToDevice;
        default: return hipMemcpyDefault;
    }
}
int surfhip_memcpy(void* dst, const void* src, size_t bytes, int kind)
{
    HIPCHK(hipMemcpy(dst, src, bytes, kind_of(kind)));
    return SURFHIP_OK;
}
int surfhip_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream)
{
    HIPCHK(hipMemcpyAsync(dst, src, bytes, kind_of(kind), (hipStream_t)stream));
    return SURFHIP_OK;
}
int surfhip_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                     size_t height, int kind)
{
    HIPCHK(hipMemcpy2D(dst, dpitch, src, spitch, width_bytes, height, kind_of(kind)));
    return SURFHIP_OK;
}
int surfhip_device_synchronize(void)
{
    HIPCHK(hipDeviceSynchronize());
    return SURFHIP_OK;
}
int surfhip_device_reset(void)
{
    HIPCHK(hipDeviceReset());
    return SURFHIP_OK;
}
int surfhip_stream_create(void** stream)
{
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return SURFHIP_OK;
}
int surfhip_stream_destroy(void* stream)
{
    HIPCHK(hipStreamDestroy((hipStream_t)stream));
    return SURFHIP_OK;
}
int surfhip_stream_synchronize(void* stream)
{
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return SURFHIP_OK;
}
int surfhip_event_create(void** ev)
{
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    *ev = (void*)e;
    return SURFHIP_OK;
}
int surfhip_event_destroy(void* ev)
{
    HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return SURFHIP_OK;
}
int surfhip_event_record(void* ev, void* stream)
{
    HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return SURFHIP_OK;
}
int surfhip_stream_wait_event(void* stream, void* ev)
{
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return SURFHIP_OK;
}
int surfhip_event_synchronize(void* ev)
{
    HIPCHK(hipEventSynchronize((hipEvent_t)ev));
    return SURFHIP_OK;
}
int surfhip_event_elapsed(float* ms, void* start, void* stop)
{
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return SURFHIP_OK;
}

// --------------------------------------------------------------- detector

// Surfor::init (surf.cpp:63-79).
int surfhip_make_param(surfhip_param* out, int noctaves, float thresh, int doubled, int init_mask_size,
                       int sampling_step, int upright, int extend, int desc_wsz)
{
    if (!out) return SURFHIP_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    if (noctaves < 1 || noctaves > kMaxOct || desc_wsz < 1 || sampling_step < 1)
        return SURFHIP_ERR_INVALID;
    out->doubled = doubled != 0;
    out->noctaves = noctaves;
    out->divisor = doubled ? 0.5f : 1.f;
    out->init_lobe = init_mask_size / 3;
    out->max_scale = out->init_lobe + 2;
    out->sampling = sampling_step + (doubled ? sampling_step : 0);
    out->thresh = thresh;
    out->upright = upright != 0;
    out->extend = extend != 0;
    out->desc_wsz = desc_wsz;
    out->mag_factor = 12 / desc_wsz;
    out->orient_size = 4 + (extend ? 4 : 0);
    out->nfeatures = desc_wsz * desc_wsz * out->orient_size;
    // scales per octave: MAX_SCALE (surfd.h:9) bounds them; below 4 the
    // octaves > 0 compute fewer than 2 scales and the lobes degenerate
    if (out->max_scale < 4 || out->max_scale > kMaxScale) return SURFHIP_ERR_UNSUPPORTED;
    // a sample's Gaussian weight is lookup2[(int)(rpos^2 + cpos^2)]
    // (surfd.cu:1303, 1335, 1999) with |rpos|, |cpos| < (desc_wsz + 1) / 2,
    // and lookup2 has 40 entries (surfd.cu:23): from desc_wsz 8 on the
    // reference reads past it.  desc_wsz <= 7: at most 7 x 7 x 8 = 392 features.
    if (desc_wsz > 7) return SURFHIP_ERR_UNSUPPORTED;
    return SURFHIP_OK;
}

// Geometry (surf.cpp:374-392) and the host parameter recurrences
// (surf.cpp:240-292, surfd.cu:2844-2865, 3062-3076).
static int derive(surfhip_detector* d)
{
    const surfhip_param& p = d->param;
    FrameParams& P = d->P;
    P.W = d->W;
    P.H = d->H;
    const int iw = d->W + 1, ih = d->H + 1;
    P.ip = align_up(iw, 128);
    P.iH = ih;
    P.ii_stride = (long long)ih * P.ip;
    P.max_scale = p.max_scale;
    P.init_lobe = p.init_lobe;
    P.sampling = p.sampling;
    P.noct = p.noctaves;
    P.thresh = p.thresh;
    P.divisor = p.divisor;
    P.upright = p.upright;
    P.extend = p.extend;
    P.wsz = p.desc_wsz;
    P.mag = p.mag_factor;
    P.osz = p.orient_size;
    P.nfeat = p.nfeatures;
    P.doubled = p.doubled ? 1 : 0;

    int sw[kMaxOct], sh[kMaxOct], sp[kMaxOct];
    long long off = 0;
    for (int o = 0; o < p.noctaves; o++) {
        sw[o] = o == 0 ? (iw - 1) / p.sampling : sw[o - 1] >> 1;
        sh[o] = o == 0 ? (ih - 1) / p.sampling : sh[o - 1] >> 1;
        sp[o] = align_up(std::max(sw[o], 1), 128);
        OctaveParams& q = d->oct[o];
        q.sw = sw[o];
        q.sh = sh[o];
        q.sp = sp[o];
        q.osize = sh[o] * sp[o];
        q.ooff = off;
        off += (long long)q.osize * p.max_scale;
    }
    P.resp_stride = off;
    d->tot_osize = (size_t)off;

    int mask_size = p.init_lobe - 2;
    int octave = 1;
    int borders[kMaxScale] = {0};
    long long hbytes = 0;
    for (int o = 0; o < p.noctaves; o++) {
        OctaveParams& q = d->oct[o];
        int s, border1;
        if (o > 0) {
            border1 = ((3 * (mask_size + 4 * octave)) / 2) / (p.sampling * octave) + 1;
            borders[0] = border1;
            borders[1] = border1;
            s = 2;
            for (int t = 0; t < 2; t++) {
                int pl = t == 0 ? p.max_scale - 3 : p.max_scale - 1, oo = o - 1, st = 2;
                while (pl < 2 && oo > 0) {      // a copy of a copy (4 scales per octave)
                    pl = pl == 0 ? p.max_scale - 3 : p.max_scale - 1;
                    oo--;
                    st *= 2;
                }
                q.hbase[t] = d->oct[oo].ooff + (long long)pl * d->oct[oo].osize;
                q.hrow[t] = d->oct[oo].sp * st;
                q.hcol[t] = st;
            }
        } else {
            border1 = ((3 * (mask_size + 6 * octave)) / 2) / (p.sampling * octave) + 1;
            s = 0;
        }
        q.octave = octave;
        q.init_scale = s;
        q.nscale = p.max_scale - s;
        q.delta = p.sampling * octave;
        for (int i = 0, ss = s; ss < p.max_scale; i++, ss++) {
            borders[ss] = border1;
            const int m = mask_size + 2 * octave * (i + 1);
            if (ss > 2) border1 = 3 * m / 2 / q.delta + 1;
            q.mask[i] = m;
            q.b1[i] = border1;
            float nrm = 9.f / (float)(m * m);
            nrm *= nrm;
            q.norm[i] = nrm;
            q.x2[i] = m / 2;
            q.x3[i] = q.x2[i] + q.x2[i];
            q.x4[i] = q.x2[i] + q.x3[i];
            // every box corner inside the integral image (the reference never checks)
            const int reach = std::max(m + q.x2[i], q.x4[i]);
            const int vx = q.sw - 2 * border1, vy = q.sh - 2 * border1;
            if (vx > 0 && vy > 0) {
                if (q.delta * border1 - reach < 0 || q.delta * (q.sw - border1 - 1) + reach + 1 >= iw ||
                    q.delta * (q.sh - border1 - 1) + reach + 1 >= ih)
                    return SURFHIP_ERR_INVALID;
                hbytes += (long long)vx * vy * 4;
            }
        }
        mask_size = q.mask[q.nscale - 1];
        for (int k = 0; k < kMaxScale; k++) q.borders[k] = borders[k];
        int n = 0, maxw = 0, maxh = 0;
        for (int k = 1; k < p.max_scale - 1; k += 2) {
            q.mb[n] = borders[k + 1] + 1;
            const int b = q.mb[n] + q.mb[n];
            maxw = std::max(maxw, q.sw - b);
            maxh = std::max(maxh, q.sh - b);
            n++;
        }
        q.nms_gx = ((maxw / 2 + 16 - 1) / 16) * 16;   // DX = 16, surfd.cu:3060, 3076
        q.nms_gy = ((maxh / 2 + 16 - 1) / 16) * 16;
        octave += octave;
    }
    // compulsory Hessian bytes: the integral image read once + valid responses
    d->hess_bytes = (long long)iw * ih * 4 + hbytes;
    return SURFHIP_OK;
}

// A derived detector's plan and what it owns on the device (a failure's leftovers go with the detector)
static hipError_t create_device_state(surfhip_detector* d)
{
    const size_t B = (size_t)d->max_batch, max_pts = (size_t)d->max_pts;
    Candidates& c = d->cands;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto*& ptr, size_t bytes) {        // (nothing more after a failure)
        if (e == hipSuccess) e = d->mem.alloc(ptr, bytes);
    };
    d->CW = (d->W + 1 <= 2048) ? 2048 : (d->W + 1 <= 4096 ? 4096 : 8192);
    make_plan(d->P, d->oct, d->sw, d->plan, d->max_batch);
    // the u8 kernels write the integral image: one stream; no kernel reads the u8 frames: integral first, one
    // stream; else: u8 kernels on the detector stream, the integral and the integral-image kernels beside them
    d->sched = d->plan.iiw ? kFused : !plan_reads_frames(d->plan) ? kIntegralFirst : kSideStream;
    const size_t rowseg_bytes = B * d->plan.rs_nstrips * d->plan.rs_rows * sizeof(uint32_t);
    if (d->plan.iiw) {
        // the stage also writes the integral image (read: the u8 frame)
        d->hess_bytes += (long long)d->W * d->H;
        alloc(d->rowseg, rowseg_bytes);
        if (d->plan.rsum) alloc(d->psum, B * d->plan.q0_strips * d->plan.rs_rows * sizeof(uint32_t));
    }
    alloc(d->d_oct, sizeof(OctaveParams) * kMaxOct);
    alloc(d->iib[0], B * d->P.ii_stride * sizeof(int32_t));
    d->ii = d->iib[0];
    alloc(d->resp, B * d->tot_osize * sizeof(float));
    alloc(d->colsum, (size_t)integral_bands(d->H, d->max_batch, d->sw) * d->CW * sizeof(uint32_t));
    alloc(c.cand, B * c.cap * sizeof(surfhip_point));
    alloc(c.keys, B * c.cap * sizeof(uint32_t));
    alloc(c.cand_count, B * sizeof(int));
    d->keep.n = d->max_pts;
    alloc(d->keep.valid, B * sizeof(int));
    const size_t items = B * (size_t)scan_items(d->plan);
    alloc(c.scan_key, items * kItemCap * sizeof(uint32_t));
    alloc(c.scan_src, items * kItemCap * sizeof(uint32_t));
    alloc(c.scan_cube, items * kCubeCap * kCubeF * sizeof(float));
    alloc(c.item_count, items * sizeof(int));
    alloc(c.item_off, (2 * items + 64) * sizeof(int));
    alloc(d->schedule.offsets, (B + 1) * sizeof(int));
    alloc(d->schedule.order, B * max_pts * sizeof(int));
    alloc(d->pcount, B * sizeof(int));
    alloc(d->schedule.work, B * max_pts * kWorkF4 * sizeof(float4));
    alloc(c.status, 256 + kDescQueueBytes);
    d->schedule.queue = c.status + 64;
    alloc(d->pts1, max_pts * sizeof(surfhip_point));
    alloc(d->desc1, max_pts * d->param.nfeatures * sizeof(float));
    alloc(d->count1, 16);
    if (c.cap > kSortCap) alloc(c.gscratch, B * c.cap * sizeof(uint64_t));
    if (d->param.doubled) {
        d->dpitch = align_up(d->W, 128);
        d->dstride = (long long)d->H * d->dpitch;
        alloc(d->dbl, B * (size_t)d->dstride);
    }
    // zero once: integral pad columns and response pad columns are never
    // written by the kernels and never read by them either
    if (e == hipSuccess) e = hipMemcpy(d->d_oct, d->oct, sizeof(OctaveParams) * kMaxOct, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d->iib[0], 0, B * d->P.ii_stride * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(d->resp, 0, B * d->tot_osize * sizeof(float));
    if (e == hipSuccess) e = hipMemset(c.status, 0, 16);
    // strip 0's slab and the rows past H stay zero (k_ii_rowseg never writes them)
    if (e == hipSuccess && d->rowseg) e = hipMemset(d->rowseg, 0, rowseg_bytes);
    if (e != hipSuccess) return e;
    // LUTs (surf.cpp:358-371) and orientation bins (surf.cpp:83-89); the
    // values are geometry-independent, so one constant table serves all
    Tables t;
    for (int n = 0; n < 83; n++) t.lut1[n] = expf(-(n + 0.5f) / 12.5f);
    for (int n = 0; n < 40; n++) t.lut2[n] = expf(-(n + 0.5f) / 8.f);
    t.bins[0] = (float)(-3.14159265358979323846);
    for (int i = 1; i < 72; i++) t.bins[i] = t.bins[i - 1] + 0.08726646259971647f;
    e = set_tables(t);
    for (int i = 0; i < SURFHIP_NSTAGE && e == hipSuccess; i++) e = hipEventCreate(&d->ev[i]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->fork2, hipEventDisableTiming);
    return e;
}

int surfhip_detector_create(surfhip_detector** out, const surfhip_param* param, int width, int height,
                            int max_batch, int max_pts, int cand_cap, void* stream)
{
    if (!out || !param || width < 16 || height < 16 || max_batch < 1 || max_pts < 1) return SURFHIP_ERR_INVALID;
    if (width + 1 > 8192) return SURFHIP_ERR_UNSUPPORTED;     // integral kernels: <= 32 columns per thread
    surfhip_param chk;
    int rc = surfhip_make_param(&chk, param->noctaves, param->thresh, param->doubled, param->init_lobe * 3,
                                param->doubled ? param->sampling / 2 : param->sampling, param->upright,
                                param->extend, param->desc_wsz);
    if (rc != SURFHIP_OK) return rc;
    // doubled (surf.cpp:234-235, 377-378): the integral is taken of the
    // (2W-2) x (2H-2) upsampled frames D, giving the (2W-1) x (2H-1) grid
    const int W = chk.doubled ? 2 * width - 2 : width;
    if (W + 1 > 8192) return SURFHIP_ERR_UNSUPPORTED;
    surfhip_detector* d = new surfhip_detector();
    d->sw = read_switches();
    d->param = chk;
    d->srcW = width;
    d->srcH = height;
    d->W = W;
    d->H = chk.doubled ? 2 * height - 2 : height;
    d->max_batch = max_batch;
    d->max_pts = max_pts;
    const int cap = cand_cap > 0 ? cand_cap : std::max(max_pts, kSortCap);
    d->cands.cap = 1;
    while (d->cands.cap < cap) d->cands.cap <<= 1;
    d->stream = (hipStream_t)stream;
    hipError_t e = hipGetDevice(&d->dev);
    if (e == hipSuccess) {
        hipDeviceProp_t pr;
        e = hipGetDeviceProperties(&pr, d->dev);
        if (e == hipSuccess) d->cus = pr.multiProcessorCount;
    }
    rc = (e == hipSuccess) ? derive(d) : SURFHIP_ERR_HIP;
    // the NMS survivor records pack the sample row / column into 14 bits and
    // the block row of the canonical key into 13 (k_nms_scan): octave 0 is
    // the largest octave, so its extent bounds them all
    if (rc == SURFHIP_OK && (d->oct[0].sh >= 16384 || d->oct[0].sw >= 16384 || d->oct[0].nms_gy >= 8192))
        rc = SURFHIP_ERR_UNSUPPORTED;
    if (rc == SURFHIP_OK && (e = create_device_state(d)) != hipSuccess)
        rc = e == hipErrorOutOfMemory ? SURFHIP_ERR_NOMEM : SURFHIP_ERR_HIP;
    if (rc != SURFHIP_OK) {
        if (e != hipSuccess) g_last_hip = e;
        delete d;
        return rc;
    }
    *out = d;
    return SURFHIP_OK;
}

int surfhip_detector_destroy(surfhip_detector* d)
{
    if (!d) return SURFHIP_ERR_INVALID;
    (void)hipStreamSynchronize(d->stream);
    if (d->side) (void)hipStreamSynchronize(d->side);    // a next-batch integral may still run there
    delete d;
    return SURFHIP_OK;
}

int surfhip_detector_set_stream(surfhip_detector* d, void* stream)
{
    if (!d) return SURFHIP_ERR_INVALID;
    d->stream = (hipStream_t)stream;
    return SURFHIP_OK;
}

static int check_frames(surfhip_detector* d, const FrameBatch& b)
{
    if (!d || !b.frames || b.n < 1 || b.n > d->max_batch) return SURFHIP_ERR_INVALID;
    if (b.pitch < d->srcW || (b.pitch & 15) != 0) return SURFHIP_ERR_INVALID;
    if (((uintptr_t)b.frames & 15) != 0) return SURFHIP_ERR_INVALID;
    if (b.n > 1 && (b.stride < (long long)b.pitch * d->srcH || (b.stride & 15) != 0)) return SURFHIP_ERR_INVALID;
    return SURFHIP_OK;
}

// doubled: upsample the caller's frames into d->dbl and continue from there
static hipError_t source_frames(surfhip_detector* d, FrameBatch& b, hipStream_t s)
{
    if (!d->param.doubled) return hipSuccess;
    hipError_t e = launch_double(b.frames, b.pitch, b.stride, b.n, d->srcW, d->srcH, d->dbl, d->dpitch, d->dstride, s);
    b = FrameBatch{d->dbl, b.n, d->dpitch, d->dstride};
    return e;
}

// Everything queued on the side stream so far is ordered before s's later work
static hipError_t side_before(surfhip_detector* d, hipStream_t s)
{
    hipError_t e = hipEventRecord(d->join, d->side);
    return e == hipSuccess ? hipStreamWaitEvent(s, d->join, 0) : e;
}

// (plan.iiw: the stage writes the integral image it is given, d->ii)
static HessianArgs hessian_args(surfhip_detector* d, const FrameBatch& b)
{
    return {b, d->ii, d->resp, &d->P, d->d_oct, d->oct, &d->plan, d->rowseg, d->plan.iiw ? d->ii : nullptr, d->psum};
}

int surfhip_run_integral(surfhip_detector* d, const uint8_t* frames, int nframes, int pitch, size_t stride)
{
    FrameBatch b{frames, nframes, pitch, (long long)stride};
    int rc = check_frames(d, b);
    if (rc) return rc;
    // a prefetch on the side stream may still be using the colsum scratch
    HIPCHK(side_before(d, d->stream));
    HIPCHK(source_frames(d, b, d->stream));
    HIPCHK(launch_integral(b, d->P, d->sw, d->colsum, d->ii, d->stream));
    // (plan.iiw) the row sums a following run_hessian's k_hess_w adds: it
    // rewrites the same integral image
    HIPCHK(launch_rowseg(b, d->P, d->plan, d->rowseg, d->stream));
    d->pref_valid = false;
    d->last = b;
    return SURFHIP_OK;
}

int surfhip_run_hessian(surfhip_detector* d, int nframes)
{
    if (!d || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    // the u8 Hessian kernels read the frames of the last run_integral
    if (!d->last.frames && plan_reads_frames(d->plan)) return SURFHIP_ERR_INVALID;
    FrameBatch b = d->last;
    b.n = nframes;
    const HessianArgs a = hessian_args(d, b);
    HIPCHK(launch_hess_oct0(a, d->stream));
    HIPCHK(launch_hess_w(a, d->stream));
    HIPCHK(launch_hess_ii(a, d->stream));
    return SURFHIP_OK;
}

// The describe stage of detect_batch on caller-given points: launch_plant's schedule (the identity order) in
// place of launch_sort's, then the same choose_describe and launch_describe on the resident integral.  The
// laplace sign stays where the caller put it (the fit's stash is what k_describe_u2 would take it from).
int surfhip_run_describe(surfhip_detector* d, surfhip_point* points, const int* counts, int nframes, float* desc)
{
    if (!d || !points || !counts || !desc || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    if (!d->last.frames) return SURFHIP_ERR_INVALID;    // no run_integral / detect_batch yet: no integral
    DescribeChoice how = choose_describe(d->sw, d->P, nframes);
    how.trace = false;
    const PointSlots slots{points, d->max_pts, d->pcount};
    HIPCHK(launch_plant(counts, nframes, slots, d->schedule, d->stream));
    HIPCHK(launch_describe(d->ii, d->P, slots, d->schedule, nframes, desc, d->stream, false, d->cus, d->sw, how));
    return SURFHIP_OK;
}

// The NMS stage of detect_batch on what is resident: the response planes in d->resp (the caller may have
// written them through surfhip_detector_workspace) and the integral of the last run_integral / detect_batch.
// launch_nms and launch_sort on the detector's blocks, as in surfhip_detect_batch_next; laplace sign in the fit.
int surfhip_run_nms(surfhip_detector* d, int nframes, surfhip_point* points, int* counts)
{
    if (!d || !points || !counts || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    if (!d->last.frames) return SURFHIP_ERR_INVALID;    // no run_integral / detect_batch yet: no integral
    FrameBatch b = d->last;
    b.n = nframes;
    HIPCHK(launch_nms(hessian_args(d, b), d->cands, d->stream, d->sw, false));
    HIPCHK(launch_sort(d->cands, d->plan, nframes, {points, d->max_pts, counts}, d->schedule, d->stream, d->sw,
                       d->keep));
    return SURFHIP_OK;
}

// This batch's integral buffer: the one the previous call prefetched into (`have`), else the current
// one; a fused plan's Hessian writes the integral itself, into buffer 0.  The second buffer is allocated
// on first use of the pipelined entry point (a plain detect_batch caller never pays for it).
static hipError_t pick_integral(surfhip_detector* d, bool have, bool pipe)
{
    if (pipe && d->sched != kFused && !d->iib[1]) {
        const size_t bytes = (size_t)d->max_batch * d->P.ii_stride * sizeof(int32_t);
        hipError_t e = d->mem.alloc(d->iib[1], bytes);
        if (e == hipSuccess) e = hipMemset(d->iib[1], 0, bytes);     // pad columns stay 0
        if (e != hipSuccess) return e;
    }
    d->icur = d->sched == kFused ? 0 : have ? d->ipref : d->icur;
    d->ii = d->iib[d->icur];
    d->pref_valid = false;
    return hipSuccess;
}

// The Hessian stage of batch a.b: its integral image (fused: its row sums) unless the previous call
// prefetched it (`have`), and its response planes; the detector stream s ends up ordered after all of it.
// Profiled: serial on s, so that the stage events bracket each stage alone (ev[1] between the integral /
// row-sum pass and the Hessian kernels); the caller ordered the side stream before ev[0].
// In-step timing brackets the WHOLE stage: from hev[0] to the end of the kernels on s and of the
// integral-image kernels on the side stream, whichever is later (surfhip_detector_hessian_times).  Without
// a prefetched integral the side stream's part starts after the integral, which the bracket then includes.
static int hessian_stage(surfhip_detector* d, const HessianArgs& a, bool have)
{
    hipStream_t s = d->stream;
    const bool prof = d->profiling;
    const bool timed = !prof && d->time_hess && d->hev_n < SURFHIP_MAX_HESS_EV;
    hipEvent_t* hev = d->hev[timed ? d->hev_n : 0];
    const hipEvent_t begin = timed ? hev[0] : nullptr, mid = prof ? d->ev[1] : nullptr;
    const hipEvent_t end = timed ? hev[1] : prof ? d->ev[2] : nullptr;
    auto mark = [](hipEvent_t ev, hipStream_t st) { return ev ? hipEventRecord(ev, st) : hipSuccess; };
    // (profiled: a side-stream plan runs integral first, everything on s)
    const HessSched sched = prof && d->sched == kSideStream ? kIntegralFirst : d->sched;
    const bool side_hess = sched == kSideStream && d->plan.hess_start[kMaxOct] > 0;
    const bool late = sched == kFused && have && d->plan.iiw != 2;
    switch (sched) {
        case kFused:
            // octaves 0-3 on the u8 kernels, the integral image written by
            // k_hess_w, any later octave's k_hessian after them (it reads
            // that integral): one stream.  The side stream's last work (a
            // prefetch of d->rowseg) is ordered before the row sums' use:
            // before this call's own row-sum pass, or, prefetched, between
            // the octave-0 kernel and k_hess_w, where the wait's latency
            // hides behind the running octave-0 kernel (iiw 2: the octave-0
            // kernel writes the integral, so the wait precedes it).
            if (!prof && !late) HIPCHK(side_before(d, s));
            if (!have) HIPCHK(launch_rowseg(a.b, d->P, d->plan, d->rowseg, s));
            HIPCHK(mark(mid, s));
            HIPCHK(mark(begin, s));
            HIPCHK(launch_hess_oct0(a, s));
            if (late) HIPCHK(side_before(d, s));
            HIPCHK(launch_hess_w(a, s));
            HIPCHK(launch_hess_ii(a, s));
            break;
        case kIntegralFirst:
            // Every Hessian kernel reads the integral image (the gather plan
            // of batches <= kGatherBatch, config #2): nothing would run beside
            // them, so they stay on the detector stream -- the fork / join
            // round trip through the side stream cost a one-frame step ~30 us
            // of idle GPU in a kernel trace (profiles/r05ac2_*).  The side
            // stream's last work (a prefetch into d->ii, or one using the
            // colsum scratch) is ordered first; it finished long ago.
            HIPCHK(mark(begin, s));
            if (!prof) HIPCHK(side_before(d, s));
            if (!have) HIPCHK(launch_integral(a.b, d->P, d->sw, d->colsum, d->ii, s));
            HIPCHK(mark(mid, s));
            if (prof) HIPCHK(launch_hess_oct0(a, s));        // (the plan's own u8 launches are empty)
            if (prof) HIPCHK(launch_hess_w(a, s));
            HIPCHK(launch_hess_ii(a, s));
            break;
        case kSideStream:
            // the u8 Hessian kernels need no integral image: they run on s;
            // the integral (unless prefetched) and the integral-image Hessian
            // kernels run on the side stream beside them; s waits for both
            // before NMS
            HIPCHK(mark(begin, s));
            HIPCHK(hipEventRecord(d->fork, s));
            HIPCHK(hipStreamWaitEvent(d->side, d->fork, 0));
            if (!have) HIPCHK(launch_integral(a.b, d->P, d->sw, d->colsum, d->ii, d->side));
            HIPCHK(launch_hess_ii(a, d->side));
            if (timed && side_hess) HIPCHK(hipEventRecord(hev[2], d->side));
            HIPCHK(launch_hess_oct0(a, s));
            HIPCHK(launch_hess_w(a, s));
            break;
    }
    HIPCHK(mark(end, s));
    if (sched == kSideStream) HIPCHK(side_before(d, s));
    if (timed) d->hev_side[d->hev_n++] = side_hess;
    return SURFHIP_OK;
}

// Where this call enqueues the next batch's prefetch.  Default: after this batch's Hessian, beside its NMS
// scan, fit and sort (the Hessian and describe then run alone); a fused plan's prefetch is only the row-sum
// pass and its default is before describe (its HBM use is low and describe's waves leave room for its
// 16-VGPR waves).  SURFHIP_PREFETCH=describe / any other value (nms), as the detector read it, overrides the
// default.  plan.rsum: k_hess_p0 makes the row sums of its own batch, nothing to prefetch.
static Prefetch prefetch_place(const LaunchPlan& plan, const Switches& sw, bool pipe)
{
    if (!pipe || (plan.iiw && plan.rsum)) return kPrefNone;
    return (sw.prefetch >= 0 ? sw.prefetch == 0 : !plan.iiw) ? kPrefNms : kPrefDescribe;
}

// The next batch's integral (into the other buffer; fused: its row sums) on the side stream, ordered after
// everything on s so far, so that buffer's last readers (the previous batch's fit and describe; fused: this
// batch's k_hess_w of d->rowseg) are done.
static hipError_t prefetch_next(surfhip_detector* d, const FrameBatch& next, hipStream_t s)
{
    const int nx = d->icur ^ 1;
    hipError_t e = hipEventRecord(d->fork2, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(d->side, d->fork2, 0);
    if (e == hipSuccess)
        e = d->sched == kFused ? launch_rowseg(next, d->P, d->plan, d->rowseg, d->side)
                               : launch_integral(next, d->P, d->sw, d->colsum, d->iib[nx], d->side);
    if (e != hipSuccess) return e;
    d->pref_valid = true;
    d->ipref = nx;
    d->pref = next;
    return hipSuccess;
}

int surfhip_detect_batch_next(surfhip_detector* d, const uint8_t* frames, int nframes, int pitch, size_t stride,
                              surfhip_point* points, float* desc, int* counts, const uint8_t* next_frames,
                              int next_nframes, int next_pitch, size_t next_stride)
{
    FrameBatch b{frames, nframes, pitch, (long long)stride};
    const FrameBatch next{next_frames, next_nframes, next_pitch, (long long)next_stride};
    int rc = check_frames(d, b);
    if (rc) return rc;
    if (!points || !counts) return SURFHIP_ERR_INVALID;
    // no prefetch for doubled frames (the upsampled frames share one scratch
    // buffer) or while stage profiling (serial stages)
    const bool prof = d->profiling;
    const bool pipe = next.frames != nullptr && !d->param.doubled && !prof;
    if (next.frames && !d->param.doubled) {
        rc = check_frames(d, next);
        if (rc) return rc;
    }
    const Prefetch pf = prefetch_place(d->plan, d->sw, pipe);
    hipStream_t s = d->stream;
    // this batch's integral (fused: its row sums): prefetched by the previous
    // call (same frames), or computed now
    const bool have = !prof && d->pref_valid && d->pref == b;
    HIPCHK(pick_integral(d, have, pipe));
    // (the per-batch counters -- accepted candidates per frame, the
    // truncation flag, the scan items' survivor counts -- are written by the
    // NMS scan itself: no memsets ahead of the Hessian)
    if (prof) {
        // a prefetch left on the side stream by an earlier pipelined call may
        // still be using the colsum scratch the integral reuses
        HIPCHK(side_before(d, s));
        HIPCHK(hipEventRecord(d->ev[0], s));
    }
    HIPCHK(source_frames(d, b, s));
    const HessianArgs a = hessian_args(d, b);
    rc = hessian_stage(d, a, have);
    if (rc) return rc;
    if (pf == kPrefNms) HIPCHK(prefetch_next(d, next, s));
    // the describe kernel, and getTrace in k_describe_u2 (its integral rows
    // are in L2 there) rather than in the fit (16 scattered integral loads per
    // survivor from HBM); no describe: the fit takes it
    DescribeChoice how = choose_describe(d->sw, d->P, nframes);
    if (!desc) how.trace = false;
    const PointSlots slots{points, d->max_pts, counts};
    HIPCHK(launch_nms(a, d->cands, s, d->sw, how.trace));
    if (prof) HIPCHK(hipEventRecord(d->ev[3], s));
    HIPCHK(launch_sort(d->cands, d->plan, nframes, slots, d->schedule, s, d->sw, d->keep));
    if (prof) HIPCHK(hipEventRecord(d->ev[4], s));
    if (pf == kPrefDescribe) HIPCHK(prefetch_next(d, next, s));
    if (d->desc_ev) HIPCHK(hipEventRecord(d->desc_ev, s));
    if (desc)
        HIPCHK(launch_describe(d->ii, d->P, slots, d->schedule, nframes, desc, s, pf == kPrefDescribe && !d->plan.iiw,
                               d->cus, d->sw, how));
    if (prof) HIPCHK(hipEventRecord(d->ev[5], s));
    d->last = b;
    return SURFHIP_OK;
}

int surfhip_detector_set_describe_event(surfhip_detector* d, void* ev)
{
    if (!d) return SURFHIP_ERR_INVALID;
    d->desc_ev = (hipEvent_t)ev;
    return SURFHIP_OK;
}

int surfhip_detector_drain(surfhip_detector* d)
{
    if (!d) return SURFHIP_ERR_INVALID;
    // (a prefetch of the next batch's integral, which reads next_frames)
    HIPCHK(side_before(d, d->stream));
    return SURFHIP_OK;
}

int surfhip_detect_batch(surfhip_detector* d, const uint8_t* frames, int nframes, int pitch,
                         size_t stride, surfhip_point* points, float* desc, int* counts)
{
    return surfhip_detect_batch_next(d, frames, nframes, pitch, stride, points, desc, counts, nullptr, 0, 0, 0);
}

int surfhip_detect(surfhip_detector* d, const uint8_t* image, int pitch, surfhip_point* points,
                   int max_pts, int* num_pts, float** desc_out, int desc)
{
    if (!d || !points || !num_pts || max_pts < 0) return SURFHIP_ERR_INVALID;
    int rc = surfhip_detect_batch(d, image, 1, pitch, 0, d->pts1, desc ? d->desc1 : nullptr, d->count1);
    if (rc) return rc;
    // A frame with more candidates than the detector's capacity keeps the
    // first `cap` NMS survivors in scan order (deterministic) and returns
    // them like any other frame, as the reference returns max_pts points
    // (surf.cpp:302-303); surfhip_detector_status() tells the caller.
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d->count1, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const int n = std::min(cnt, max_pts);                  // surf.cpp:303
    if (n > 0)
        HIPCHK(hipMemcpyAsync(points, d->pts1, sizeof(surfhip_point) * n, hipMemcpyDeviceToDevice, d->stream));
    if (desc && desc_out) {
        const size_t nb = sizeof(float) * (size_t)std::max(n, 1) * d->param.nfeatures;
        HIPCHK(hipMalloc((void**)desc_out, nb));                // cuDescribe's per-call cudaMalloc, surfd.cu:3264
        if (n > 0)
            HIPCHK(hipMemcpyAsync(*desc_out, d->desc1, sizeof(float) * (size_t)n * d->param.nfeatures,
                                  hipMemcpyDeviceToDevice, d->stream));
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    *num_pts = n;
    return SURFHIP_OK;
}

int surfhip_detector_candidates(surfhip_detector* d, int* h_counts, int nframes)
{
    if (!d || !h_counts || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    HIPCHK(hipMemcpyAsync(h_counts, d->cands.cand_count, sizeof(int) * nframes, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    int st = 0;
    HIPCHK(hipMemcpy(&st, d->cands.status, sizeof(int), hipMemcpyDeviceToHost));
    return st ? SURFHIP_ERR_CAPACITY : SURFHIP_OK;
}

int surfhip_detector_status(surfhip_detector* d, int* truncated)
{
    if (!d || !truncated) return SURFHIP_ERR_INVALID;
    int st = 0;
    HIPCHK(hipMemcpyAsync(&st, d->cands.status, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *truncated = st & 1;
    return SURFHIP_OK;
}

int surfhip_detector_set_keep(surfhip_detector* d, int mode, int n)
{
    if (!d || (mode != SURFHIP_KEEP_FIRST && mode != SURFHIP_KEEP_STRONGEST) || n < 0 || n > d->max_pts)
        return SURFHIP_ERR_INVALID;
    d->keep.mode = mode;
    d->keep.n = n ? n : d->max_pts;
    return SURFHIP_OK;
}

int surfhip_detector_get_keep(surfhip_detector* d, int* mode, int* n)
{
    if (!d || !mode || !n) return SURFHIP_ERR_INVALID;
    *mode = d->keep.mode;
    *n = d->keep.n;
    return SURFHIP_OK;
}

int surfhip_detector_capacity(surfhip_detector* d, int* cand_cap)
{
    if (!d || !cand_cap) return SURFHIP_ERR_INVALID;
    *cand_cap = d->cands.cap;
    return SURFHIP_OK;
}

int surfhip_detector_set_profiling(surfhip_detector* d, int on)
{
    if (!d) return SURFHIP_ERR_INVALID;
    d->profiling = on != 0;
    return SURFHIP_OK;
}

int surfhip_detector_stage_times(surfhip_detector* d, float* ms)
{
    if (!d || !ms || !d->profiling) return SURFHIP_ERR_INVALID;
    HIPCHK(hipEventSynchronize(d->ev[SURFHIP_NSTAGE - 1]));
    for (int i = 0; i < SURFHIP_NSTAGE - 1; i++) HIPCHK(hipEventElapsedTime(&ms[i], d->ev[i], d->ev[i + 1]));
    HIPCHK(hipEventElapsedTime(&ms[SURFHIP_NSTAGE - 1], d->ev[0], d->ev[SURFHIP_NSTAGE - 1]));
    return SURFHIP_OK;
}

int surfhip_detector_time_hessian(surfhip_detector* d, int on)
{
    if (!d) return SURFHIP_ERR_INVALID;
    if (on) {
        for (int i = 0; i < SURFHIP_MAX_HESS_EV; i++)
            for (int j = 0; j < 3; j++)
                if (!d->hev[i][j]) HIPCHK(hipEventCreate(&d->hev[i][j]));
    }
    d->time_hess = on != 0;
    d->hev_n = 0;
    return SURFHIP_OK;
}

int surfhip_detector_hessian_times(surfhip_detector* d, float* ms, int max, int* n)
{
    if (!d || !n || (max > 0 && !ms)) return SURFHIP_ERR_INVALID;
    const int k = std::min(d->hev_n, std::max(max, 0));
    for (int i = 0; i < k; i++) {
        HIPCHK(hipEventSynchronize(d->hev[i][1]));
        HIPCHK(hipEventElapsedTime(&ms[i], d->hev[i][0], d->hev[i][1]));
        if (d->hev_side[i]) {
            float t2 = 0.f;
            HIPCHK(hipEventSynchronize(d->hev[i][2]));
            HIPCHK(hipEventElapsedTime(&t2, d->hev[i][0], d->hev[i][2]));
            ms[i] = std::max(ms[i], t2);
        }
    }
    *n = k;
    d->hev_n = 0;
    return SURFHIP_OK;
}

int surfhip_detector_workspace(surfhip_detector* d, int32_t** ii, size_t* ii_stride, float** resp,
                               size_t* resp_stride)
{
    if (!d) return SURFHIP_ERR_INVALID;
    if (ii) *ii = d->ii;
    if (ii_stride) *ii_stride = (size_t)d->P.ii_stride;
    if (resp) *resp = d->resp;
    if (resp_stride) *resp_stride = (size_t)d->P.resp_stride;
    return SURFHIP_OK;
}

int surfhip_detector_rowsums(surfhip_detector* d, uint32_t** rowseg, int* nstrips, int* rows, int* source)
{
    if (!d) return SURFHIP_ERR_INVALID;
    const bool on = d->plan.iiw && d->plan.rs_nstrips >= 2;
    if (rowseg) *rowseg = on ? d->rowseg : nullptr;
    if (nstrips) *nstrips = on ? d->plan.rs_nstrips : 0;
    if (rows) *rows = on ? d->plan.rs_rows : 0;
    if (source) *source = !on ? 0 : d->plan.rsum ? 2 : 1;
    return SURFHIP_OK;
}

int surfhip_detector_geometry(surfhip_detector* d, int* iwhp, int* swhp, long long* ooff, int* osize)
{
    if (!d) return SURFHIP_ERR_INVALID;
    if (iwhp) { iwhp[0] = d->W + 1; iwhp[1] = d->H + 1; iwhp[2] = d->P.ip; }
    for (int o = 0; o < kMaxOct; o++) {
        const bool v = o < d->param.noctaves;
        if (swhp) { swhp[3 * o] = v ? d->oct[o].sw : 0; swhp[3 * o + 1] = v ? d->oct[o].sh : 0; swhp[3 * o + 2] = v ? d->oct[o].sp : 0; }
        if (ooff) ooff[o] = v ? d->oct[o].ooff : 0;
        if (osize) osize[o] = v ? d->oct[o].osize : 0;
    }
    return SURFHIP_OK;
}

long long surfhip_hessian_bytes_per_frame(surfhip_detector* d) { return d ? d->hess_bytes : -1; }

int surfhip_hessian_plan(surfhip_detector* d, char* buf, int len)
{
    return d ? text_out(hessian_plan_text(d->plan, d->P), buf, len) : SURFHIP_ERR_INVALID;
}

int surfhip_switches_from_env(char* buf, int len) { return text_out(switches_text(read_switches()), buf, len); }

int surfhip_detector_switches(surfhip_detector* d, char* buf, int len)
{
    return d ? text_out(switches_text(d->sw), buf, len) : SURFHIP_ERR_INVALID;
}

size_t surfhip_slab_bytes(int nframes, int total, int nfeatures)
{
    return slab_head_bytes(nframes) + (size_t)total * (sizeof(surfhip_point) + sizeof(float) * (size_t)nfeatures);
}

int surfhip_batch_total(surfhip_detector* d, int nframes, int* total)
{
    if (!d || !total || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    HIPCHK(hipMemcpyAsync(total, d->schedule.offsets + nframes, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return SURFHIP_OK;
}

int surfhip_pack_slab_cap(surfhip_detector* d, const surfhip_point* pts, const float* desc, const int* counts,
                          int nframes, void* slab, size_t cap_bytes)
{
    if (!d || !pts || !counts || !slab || nframes < 1 || nframes > d->max_batch) return SURFHIP_ERR_INVALID;
    if (cap_bytes < surfhip_slab_bytes(nframes, 0, 0)) return SURFHIP_ERR_INVALID;
    HIPCHK(launch_pack(pts, desc, counts, d->schedule, nframes, d->max_pts, d->param.nfeatures, d->cands.status,
                       cap_bytes, (uint8_t*)slab, d->stream));
    return SURFHIP_OK;
}

int surfhip_pack_slab(surfhip_detector* d, const surfhip_point* pts, const float* desc, const int* counts,
                      int nframes, void* slab)
{
    return surfhip_pack_slab_cap(d, pts, desc, counts, nframes, slab, (size_t)-1);
}

size_t surfhip_match_scratch(int n1, int n2, int flags)
{
    if (n1 < 0 || n2 < 0) return 0;
    return match_scratch_bytes(n1, n2, flags);
}

int surfhip_match(surfhip_point* pts1, const surfhip_point* pts2, const float* f1, const float* f2, int n1, int n2,
                  int nf, int flags, void* scratch, void* stream)
{
    if (n1 < 0 || n2 < 0 || nf < 4 || nf > 1024 || (nf & 3) || (flags & ~SURFHIP_MATCH_FULL_TAIL))
        return SURFHIP_ERR_INVALID;
    if (n1 == 0) return SURFHIP_OK;
    if (!pts1 || !f1 || (n2 > 0 && (!pts2 || !f2))) return SURFHIP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = match_scratch_bytes(n1, n2, flags);
    void* own = nullptr;
    if (!scratch && bytes) {            // no caller scratch: allocate, and finish before freeing it
        HIPCHK(hipMalloc(&own, bytes));
        scratch = own;
    }
    hipError_t e = launch_match(pts1, pts2, f1, f2, n1, n2, nf, flags, scratch, s);
    if (own) {
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        hipError_t e2 = hipFree(own);
        if (e == hipSuccess) e = e2;
    }
    HIPCHK(e);
    return SURFHIP_OK;
}

// the checks the five batched match calls share; the scalars first, so that they are checked for npairs == 0 too.
// b: the sets, npairs, nf and flags as the caller gave them (MATCH_GUIDED, MATCH_EPIPOLAR: hm, h_stride too;
// MATCH_EPIPOLAR: band); allowed: the call's flag bits; window: required unless MATCH_PLAIN, and copied into b;
// scratch: checked where the call needs one
static int match_batch_args(MatchBatch& b, int allowed, int mode, const surfhip_match_window* window,
                            bool need_scratch, const void* scratch)
{
    if (b.npairs < 0 || b.slots1 <= 0 || b.slots2 <= 0 || b.nf < 4 || b.nf > 1024 || (b.nf & 3) ||
        (b.flags & ~allowed))
        return SURFHIP_ERR_INVALID;
    if (mode != MATCH_PLAIN) {
        // (a NaN bound fails its comparison)
        if (!window || !(window->dx_min <= window->dx_max) || !(window->dy_min <= window->dy_max))
            return SURFHIP_ERR_INVALID;
        b.win = *window;
    }
    const bool matrix = mode == MATCH_GUIDED || mode == MATCH_EPIPOLAR;
    if (matrix && b.h_stride != 0 && b.h_stride < 9) return SURFHIP_ERR_INVALID;
    if (mode == MATCH_EPIPOLAR && !(std::isfinite(b.band) && b.band >= 0.0f)) return SURFHIP_ERR_INVALID;
    if (b.npairs == 0) return SURFHIP_OK;
    if (!b.pts1 || !b.f1 || !b.counts1 || !b.pts2 || !b.f2 || !b.counts2) return SURFHIP_ERR_INVALID;
    if (need_scratch && (!scratch || ((uintptr_t)scratch & 15))) return SURFHIP_ERR_INVALID;
    if (matrix && (!b.hm || ((uintptr_t)b.hm & 3))) return SURFHIP_ERR_INVALID;
    return SURFHIP_OK;
}

constexpr int kMatchBatchFlags = SURFHIP_MATCH_FULL_TAIL | SURFHIP_MATCH_SAME_LAPLACE;

int surfhip_match_batch(surfhip_point* pts1, const float* f1, const int* counts1, int slots1,
                        const surfhip_point* pts2, const float* f2, const int* counts2, int slots2, int npairs,
                        int nf, int flags, void* stream)
{
    MatchBatch b = {pts1, f1, counts1, slots1, pts2, f2, counts2, slots2, npairs, nf, flags};
    const int bad = match_batch_args(b, kMatchBatchFlags, MATCH_PLAIN, nullptr, false, nullptr);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_match_batch(b, MATCH_PLAIN, nullptr, (hipStream_t)stream));
    return SURFHIP_OK;
}

size_t surfhip_match_batch_cross_scratch(int npairs, int slots1, int slots2)
{
    if (npairs <= 0 || slots1 <= 0 || slots2 <= 0) return 0;
    return match_batch_scratch_bytes(MATCH_PLAIN, npairs, slots2, SURFHIP_MATCH_MUTUAL);
}

// (SURFHIP_MATCH_MUTUAL is not one of this call's flags: it is what the call means)
int surfhip_match_batch_cross(surfhip_point* pts1, const float* f1, const int* counts1, int slots1,
                              const surfhip_point* pts2, const float* f2, const int* counts2, int slots2, int npairs,
                              int nf, int flags, void* scratch, void* stream)
{
    MatchBatch b = {pts1, f1, counts1, slots1, pts2, f2, counts2, slots2, npairs, nf, flags};
    const int bad = match_batch_args(b, kMatchBatchFlags, MATCH_PLAIN, nullptr, true, scratch);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    b.flags |= SURFHIP_MATCH_MUTUAL;
    HIPCHK(launch_match_batch(b, MATCH_PLAIN, scratch, (hipStream_t)stream));
    return SURFHIP_OK;
}

size_t surfhip_match_batch_window_scratch(int npairs, int slots1, int slots2, int flags)
{
    if (npairs <= 0 || slots1 <= 0 || slots2 <= 0) return 0;
    return match_batch_scratch_bytes(MATCH_WINDOW, npairs, slots2, flags);
}

int surfhip_match_batch_window(surfhip_point* pts1, const float* f1, const int* counts1, int slots1,
                               const surfhip_point* pts2, const float* f2, const int* counts2, int slots2,
                               int npairs, int nf, int flags, const surfhip_match_window* window, void* scratch,
                               void* stream)
{
    MatchBatch b = {pts1, f1, counts1, slots1, pts2, f2, counts2, slots2, npairs, nf, flags};
    const int bad = match_batch_args(b, kMatchBatchFlags | SURFHIP_MATCH_MUTUAL, MATCH_WINDOW, window, true, scratch);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_match_batch(b, MATCH_WINDOW, scratch, (hipStream_t)stream));
    return SURFHIP_OK;
}

size_t surfhip_match_batch_guided_scratch(int npairs, int slots1, int slots2, int flags)
{
    return surfhip_match_batch_window_scratch(npairs, slots1, slots2, flags);
}

int surfhip_match_batch_guided(surfhip_point* pts1, const float* f1, const int* counts1, int slots1,
                               const surfhip_point* pts2, const float* f2, const int* counts2, int slots2,
                               int npairs, int nf, int flags, const float* h, int h_stride,
                               const surfhip_match_window* window, void* scratch, void* stream)
{
    MatchBatch b = {pts1, f1, counts1, slots1, pts2, f2, counts2, slots2, npairs, nf, flags};
    b.hm = h;
    b.h_stride = h_stride;
    const int bad = match_batch_args(b, kMatchBatchFlags | SURFHIP_MATCH_MUTUAL, MATCH_GUIDED, window, true, scratch);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_match_batch(b, MATCH_GUIDED, scratch, (hipStream_t)stream));
    return SURFHIP_OK;
}

size_t surfhip_match_batch_epipolar_scratch(int npairs, int slots1, int slots2, int flags)
{
    return surfhip_match_batch_window_scratch(npairs, slots1, slots2, flags);
}

int surfhip_match_batch_epipolar(surfhip_point* pts1, const float* f1, const int* counts1, int slots1,
                                 const surfhip_point* pts2, const float* f2, const int* counts2, int slots2,
                                 int npairs, int nf, int flags, const float* f, int f_stride, float band,
                                 const surfhip_match_window* window, void* scratch, void* stream)
{
    MatchBatch b = {pts1, f1, counts1, slots1, pts2, f2, counts2, slots2, npairs, nf, flags};
    b.hm = f;
    b.h_stride = f_stride;
    b.band = band;
    const int bad = match_batch_args(b, kMatchBatchFlags | SURFHIP_MATCH_MUTUAL, MATCH_EPIPOLAR, window, true, scratch);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_match_batch(b, MATCH_EPIPOLAR, scratch, (hipStream_t)stream));
    return SURFHIP_OK;
}

static_assert(sizeof(surfhip_homography) == 64, "surfhip_homography is 64 bytes");
static_assert(offsetof(surfhip_homography, h) == 0, "surfhip_match_batch_guided reads h at the record's start");

// the arguments surfhip_homography_batch and surfhip_fundamental_batch share; the scalars first, so
// that they are checked for npairs == 0 too
static int ransac_args(const void* pts1, const int* counts1, int slots1, int npairs, float max_ambiguity,
                       float inlier_thresh, int nhyp, const void* out)
{
    if (npairs < 0 || slots1 <= 0 || nhyp < 1 || nhyp > 4096 || !std::isfinite(max_ambiguity) ||
        !(max_ambiguity > 0.0f) || !std::isfinite(inlier_thresh) || !(inlier_thresh > 0.0f))
        return SURFHIP_ERR_INVALID;
    if (npairs > 0 && (!pts1 || !counts1 || !out)) return SURFHIP_ERR_INVALID;
    return SURFHIP_OK;
}

int surfhip_homography_batch(const surfhip_point* pts1, const int* counts1, int slots1, int npairs,
                             float max_ambiguity, float inlier_thresh, int nhyp, uint32_t seed,
                             surfhip_homography* out, uint8_t* inlier, void* stream)
{
    const int bad = ransac_args(pts1, counts1, slots1, npairs, max_ambiguity, inlier_thresh, nhyp, out);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_homography_batch(pts1, counts1, slots1, npairs, max_ambiguity, inlier_thresh, nhyp, seed, out,
                                   inlier, (hipStream_t)stream));
    return SURFHIP_OK;
}

int surfhip_homography_lds_capacity(void) { return kRansacCap; }

static_assert(sizeof(surfhip_fundamental) == 64, "surfhip_fundamental is 64 bytes");
static_assert(offsetof(surfhip_fundamental, f) == 0 && offsetof(surfhip_fundamental, status) == 36,
              "surfhip_fundamental has surfhip_homography's offsets");

int surfhip_fundamental_batch(const surfhip_point* pts1, const int* counts1, int slots1, int npairs,
                              float max_ambiguity, float inlier_thresh, int nhyp, uint32_t seed,
                              surfhip_fundamental* out, uint8_t* inlier, void* stream)
{
    const int bad = ransac_args(pts1, counts1, slots1, npairs, max_ambiguity, inlier_thresh, nhyp, out);
    if (bad != SURFHIP_OK || npairs == 0) return bad;
    HIPCHK(launch_fundamental_batch(pts1, counts1, slots1, npairs, max_ambiguity, inlier_thresh, nhyp, seed, out,
                                    inlier, (hipStream_t)stream));
    return SURFHIP_OK;
}

int surfhip_fundamental_lds_capacity(void) { return kRansacCap; }

/* ------------------------------------------------------------- ingest --
 * Pipelined host -> HBM -> result-slab ring.  The
 * reference feeds one frame per call through a blocking cudaMemcpy2D of a
 * pageable OpenCV buffer (main.cpp:212-226) and copies each frame's points
 * back with a blocking cudaMemcpy (surf.cpp:335-342).  Here `depth` pinned
 * host frame slots feed `depth` HBM frame slots over a copy stream; the
 * detector stream waits only on its own slot's copy event, so batch i+1's
 * PCIe transfer runs under batch i's kernels.  Each batch is packed into its
 * slot's device slab right after describe (before the next batch may reuse
 * the detector's scratch) and its 16-B header + counts come back
 * asynchronously; collect() then copies exactly the slab's bytes to pinned
 * host memory on a third stream while later batches keep computing. */
struct surfhip_ingest {
    surfhip_detector* det = nullptr;
    int depth = 0, pitch = 0, hdr_bytes = 0;
    size_t frame_bytes = 0, dslab_cap = 0;
    hipStream_t copy = nullptr, out = nullptr;
    uint8_t* h_frames[SURFHIP_INGEST_MAX_DEPTH]{};
    uint8_t* d_frames[SURFHIP_INGEST_MAX_DEPTH]{};
    uint8_t* d_slab[SURFHIP_INGEST_MAX_DEPTH]{};
    int32_t* h_hdr[SURFHIP_INGEST_MAX_DEPTH]{};
    uint8_t* h_slab[SURFHIP_INGEST_MAX_DEPTH]{};
    size_t h_slab_cap[SURFHIP_INGEST_MAX_DEPTH]{};
    int nframes[SURFHIP_INGEST_MAX_DEPTH]{};
    hipEvent_t ev_h2d[SURFHIP_INGEST_MAX_DEPTH]{}, ev_done[SURFHIP_INGEST_MAX_DEPTH]{};
    surfhip_point* d_pts = nullptr;
    float* d_desc = nullptr;
    int* d_counts = nullptr;
    long long submitted = 0, collected = 0;
    int acquired = -1;                  // slot handed out by acquire, not yet submitted
};

static void ingest_free(surfhip_ingest* g)
{
    for (int s = 0; s < SURFHIP_INGEST_MAX_DEPTH; ++s) {
        if (g->h_frames[s]) (void)hipHostFree(g->h_frames[s]);
        if (g->h_hdr[s]) (void)hipHostFree(g->h_hdr[s]);
        if (g->h_slab[s]) (void)hipHostFree(g->h_slab[s]);
        if (g->d_frames[s]) (void)hipFree(g->d_frames[s]);
        if (g->d_slab[s]) (void)hipFree(g->d_slab[s]);
        if (g->ev_h2d[s]) (void)hipEventDestroy(g->ev_h2d[s]);
        if (g->ev_done[s]) (void)hipEventDestroy(g->ev_done[s]);
    }
    if (g->d_pts) (void)hipFree(g->d_pts);
    if (g->d_desc) (void)hipFree(g->d_desc);
    if (g->d_counts) (void)hipFree(g->d_counts);
    if (g->copy) (void)hipStreamDestroy(g->copy);
    if (g->out) (void)hipStreamDestroy(g->out);
    delete g;
}

static int ingest_alloc(surfhip_ingest* g)
{
    surfhip_detector* d = g->det;
    const int nf = d->param.nfeatures, B = d->max_batch;
    g->pitch = (d->srcW + 127) & ~127;
    g->frame_bytes = (size_t)g->pitch * d->srcH;
    g->hdr_bytes = (int)slab_head_bytes(B);
    g->dslab_cap = surfhip_slab_bytes(B, B * d->max_pts, nf);
    HIPCHK(hipStreamCreateWithFlags(&g->copy, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&g->out, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&g->d_pts, sizeof(surfhip_point) * (size_t)B * d->max_pts));
    if (nf) HIPCHK(hipMalloc(&g->d_desc, sizeof(float) * (size_t)B * d->max_pts * nf));
    HIPCHK(hipMalloc(&g->d_counts, sizeof(int) * (size_t)B));
    for (int s = 0; s < g->depth; ++s) {
        HIPCHK(hipHostMalloc(&g->h_frames[s], g->frame_bytes * B, hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&g->h_hdr[s], g->hdr_bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc(&g->d_frames[s], g->frame_bytes * B));
        HIPCHK(hipMalloc(&g->d_slab[s], g->dslab_cap));
        HIPCHK(hipEventCreateWithFlags(&g->ev_h2d[s], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->ev_done[s], hipEventDisableTiming));
        memset(g->h_frames[s], 0, g->frame_bytes * B);
    }
    return SURFHIP_OK;
}

int surfhip_ingest_create(surfhip_ingest** out, surfhip_detector* det, int depth)
{
    if (!out || !det || depth < 1 || depth > SURFHIP_INGEST_MAX_DEPTH) return SURFHIP_ERR_INVALID;
    *out = nullptr;
    surfhip_ingest* g = new surfhip_ingest;
    g->det = det;
    g->depth = depth;
    int rc = ingest_alloc(g);
    if (rc != SURFHIP_OK) {
        ingest_free(g);
        return rc;
    }
    *out = g;
    return SURFHIP_OK;
}

int surfhip_ingest_destroy(surfhip_ingest* g)
{
    if (!g) return SURFHIP_ERR_INVALID;
    // wait on the ring's own events only: the detector may already be gone
    hipError_t e = hipStreamSynchronize(g->copy);
    for (long long b = g->collected; b < g->submitted; ++b) {
        hipError_t e1 = hipEventSynchronize(g->ev_done[b % g->depth]);
        if (e == hipSuccess) e = e1;
    }
    hipError_t e2 = hipStreamSynchronize(g->out);
    ingest_free(g);
    HIPCHK(e);
    HIPCHK(e2);
    return SURFHIP_OK;
}

int surfhip_ingest_acquire(surfhip_ingest* g, uint8_t** h_frames, int* pitch, size_t* frame_stride)
{
    if (!g || !h_frames) return SURFHIP_ERR_INVALID;
    if (g->submitted - g->collected >= g->depth) return SURFHIP_ERR_CAPACITY;   // collect first
    const int s = (int)(g->submitted % g->depth);
    // the slot's previous batch was collected, so its copy and kernels are done
    g->acquired = s;
    *h_frames = g->h_frames[s];
    if (pitch) *pitch = g->pitch;
    if (frame_stride) *frame_stride = g->frame_bytes;
    return SURFHIP_OK;
}

int surfhip_ingest_submit(surfhip_ingest* g, int nframes)
{
    if (!g || g->acquired < 0 || nframes < 1 || nframes > g->det->max_batch) return SURFHIP_ERR_INVALID;
    surfhip_detector* d = g->det;
    const int s = g->acquired;
    g->acquired = -1;
    g->nframes[s] = nframes;
    HIPCHK(hipMemcpyAsync(g->d_frames[s], g->h_frames[s], g->frame_bytes * nframes, hipMemcpyHostToDevice,
                          g->copy));
    HIPCHK(hipEventRecord(g->ev_h2d[s], g->copy));
    HIPCHK(hipStreamWaitEvent(d->stream, g->ev_h2d[s], 0));
    int rc = surfhip_detect_batch(d, g->d_frames[s], nframes, g->pitch, g->frame_bytes, g->d_pts, g->d_desc,
                                  g->d_counts);
    if (rc != SURFHIP_OK) return rc;
    rc = surfhip_pack_slab(d, g->d_pts, g->d_desc, g->d_counts, nframes, g->d_slab[s]);
    if (rc != SURFHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(g->h_hdr[s], g->d_slab[s], slab_head_bytes(nframes), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipEventRecord(g->ev_done[s], d->stream));
    ++g->submitted;
    return SURFHIP_OK;
}

int surfhip_ingest_collect(surfhip_ingest* g, const void** h_slab, size_t* bytes)
{
    if (!g || !h_slab || !bytes) return SURFHIP_ERR_INVALID;
    if (g->collected >= g->submitted) return SURFHIP_ERR_INVALID;        // nothing in flight
    const int s = (int)(g->collected % g->depth);
    HIPCHK(hipEventSynchronize(g->ev_done[s]));
    const int32_t* hdr = g->h_hdr[s];
    if (hdr[0] != g->nframes[s] || hdr[1] < 0) return SURFHIP_ERR_HIP;
    const size_t n = surfhip_slab_bytes(hdr[0], hdr[1], hdr[2]);
    if (n > g->h_slab_cap[s]) {
        if (g->h_slab[s]) HIPCHK(hipHostFree(g->h_slab[s]));
        g->h_slab[s] = nullptr;
        g->h_slab_cap[s] = 0;
        const size_t cap = n + n / 4;
        HIPCHK(hipHostMalloc(&g->h_slab[s], cap, hipHostMallocDefault));
        g->h_slab_cap[s] = cap;
    }
    HIPCHK(hipMemcpyAsync(g->h_slab[s], g->d_slab[s], n, hipMemcpyDeviceToHost, g->out));
    HIPCHK(hipStreamSynchronize(g->out));
    ++g->collected;
    *h_slab = g->h_slab[s];
    *bytes = n;
    return SURFHIP_OK;
}

int surfhip_ingest_pending(surfhip_ingest* g, int* n)
{
    if (!g || !n) return SURFHIP_ERR_INVALID;
    *n = (int)(g->submitted - g->collected);
    return SURFHIP_OK;
}

/* --------------------------------------------------------------- dump --
 * Keypoint + descriptor file: a sequence of records, each a 64-B header
 * followed by one result slab (the all-gather format above).  The reference
 * has no on-disk format (it only draws keypoints, main.cpp:21-71). */
int surfhip_dump_append(const char* path, const void* h_slab, size_t bytes, int width, int height,
                        const surfhip_param* p, long long first_frame)
{
    if (!path || !h_slab || bytes < 16 || !p) return SURFHIP_ERR_INVALID;
    const int32_t* sh = (const int32_t*)h_slab;
    if (sh[0] < 0 || sh[1] < 0 || surfhip_slab_bytes(sh[0], sh[1], sh[2]) != bytes) return SURFHIP_ERR_INVALID;
    surfhip_dump_header h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, SURFHIP_DUMP_MAGIC, 8);
    h.header_bytes = sizeof h;
    h.version = SURFHIP_DUMP_VERSION;
    h.width = (uint32_t)width;
    h.height = (uint32_t)height;
    h.nframes = (uint32_t)sh[0];
    h.nfeatures = (uint32_t)sh[2];
    h.total = (uint64_t)sh[1];
    h.slab_bytes = (uint64_t)bytes;
    h.first_frame = (uint64_t)first_frame;
    h.thresh = p->thresh;
    h.noctaves = (uint8_t)p->noctaves;
    h.upright = p->upright ? 1 : 0;
    h.extend = p->extend ? 1 : 0;
    h.doubled = p->doubled ? 1 : 0;
    FILE* f = fopen(path, "ab");
    if (!f) return SURFHIP_ERR_INVALID;
    int ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(h_slab, 1, bytes, f) == bytes;
    ok = (fclose(f) == 0) && ok;
    return ok ? SURFHIP_OK : SURFHIP_ERR_INVALID;
}

int surfhip_stream_run(int mode, const void* src, void* dst, size_t bytes, void* stream)
{
    if (mode < 0 || mode > 2 || bytes % 16 != 0 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15) ||
        (mode != 2 && !src) || (mode != 1 && !dst))
        return SURFHIP_ERR_INVALID;
    if (bytes == 0) return SURFHIP_OK;
    int dev = 0, ncu = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCHK(surfhip::launch_stream(mode, src, dst, bytes, ncu, (hipStream_t)stream));
    return SURFHIP_OK;
}

size_t surfhip_stream_bytes(int mode, size_t bytes) { return mode == 0 ? 2 * bytes : mode == 1 || mode == 2 ? bytes : 0; }

const char* surfhip_build_info(void)
{
    return "libsurfhip gfx950 (" __DATE__ " " __TIME__ ")";
}

}  // extern "C"
