// A bounded delay on a HIP stream, for tests/stream_ref.py: one workgroup of 64 threads that waits for a
// number of wall-clock ticks, or for kSpinCap turns of its loop, whichever comes first.  It occupies one
// wave slot of one CU, so kernels launched on other streams meanwhile find the whole chip free.
//
// The kernel ends on its own in every case: the loop's only exit conditions are `turn < kSpinCap`, where
// `turn` is a local counter that grows by one per turn and nothing else writes, and the clock comparison.
// A clock that never advances (or runs backwards) leaves the first condition, which fails after kSpinCap
// turns.  A turn is one clock read and one s_sleep of 32 * 64 cycles, about 1 us: the cap is reached after
// about one second, far above the longest delay the tests ask for (0.4 s) and far below any watchdog.
#include <hip/hip_runtime.h>

static constexpr int kSpinCap = 1 << 20;
static constexpr float kSpinMaxMs = 400.0f;

__global__ __launch_bounds__(64) void k_spin(long long ticks)
{
    const long long t0 = (long long)wall_clock64();
    for (int turn = 0; turn < kSpinCap; ++turn) {
        if ((long long)wall_clock64() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// Launches the delay of `ms` milliseconds (clamped to [0, kSpinMaxMs]) on `stream`; returns the hipError_t.
extern "C" int spin_launch(float ms, void* stream)
{
    static int khz = 0;                       // hipDeviceAttributeWallClockRate, kHz = ticks per millisecond
    if (khz <= 0) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
        if (e != hipSuccess) return (int)e;
        if (khz <= 0) return (int)hipErrorInvalidValue;
    }
    if (!(ms >= 0.0f)) ms = 0.0f;
    if (ms > kSpinMaxMs) ms = kSpinMaxMs;
    const long long ticks = (long long)((double)ms * (double)khz);
    k_spin<<<1, 64, 0, (hipStream_t)stream>>>(ticks);
    return (int)hipGetLastError();
}
