"""Helpers of the caller-stream tests (test_gpu_streams_*.py): does a call
order its work on the stream it was given?

On the null stream a launch that goes to the wrong stream is the right launch,
so those tests run every call on a non-blocking stream S behind a delay, with
the inputs arriving late ("Caller streams"):

    S:  e0, spin, e1, staging -> live copies, the call(s), output -> snapshot

Everything is enqueued while the spin still runs and the live inputs still
hold a benign poison (zeros: no points, black frames).  Work that is not
ordered behind S's earlier work runs at once, on the poison, and the snapshot
then differs from the null-stream run of the same chain.

No torch here: the process holds one HIP runtime, the library's.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPIN_SRC = os.path.join(HERE, "gpu", "spin.hip")
SPIN_MIN_MS, SPIN_MAX_MS, SPIN_FACTOR, RETRY_FACTOR = 5.0, 100.0, 20.0, 4.0
COLD_MS = SPIN_MAX_MS / SPIN_FACTOR      # a reference run slower than this is run again, warm
POISON_IN, POISON_SCRATCH, POISON_OUT = 0x00, 0xFF, 0xA5

_spin = None


def hipcc():
    return shutil.which("hipcc") or (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))


def spin_lib():
    """tests/gpu/spin.hip as a shared object, built once per session under
    tests/build/ (ignored by git; the temporary directory when the tree is
    read-only) and loaded with ctypes."""
    global _spin
    if _spin is None:
        out_dir = os.path.join(HERE, "build")
        try:
            os.makedirs(out_dir, exist_ok=True)
            if not os.access(out_dir, os.W_OK):
                raise OSError
        except OSError:
            out_dir = tempfile.mkdtemp(prefix="surfhip_spin_")
        out = os.path.join(out_dir, "libspin.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(SPIN_SRC):
            cmd = [hipcc(), "--offload-arch=gfx950", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SPIN_SRC,
                   "-o", out + ".tmp"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.spin_launch.restype = C.c_int
        lib.spin_launch.argtypes = [C.c_float, C.c_void_p]
        _spin = lib
    return _spin


def spin(ms: float, stream) -> None:
    rc = spin_lib().spin_launch(ms, stream)
    assert rc == 0, f"spin_launch: hip error {rc}"


# ------------------------------------------------------------ API wrappers

def stream_create(surf) -> int:
    """A hipStreamNonBlocking stream (surfhip_stream_create)."""
    s = C.c_void_p()
    surf.check(surf.lib.surfhip_stream_create(C.byref(s)), "stream_create")
    assert s.value
    return s.value


def stream_destroy(surf, stream) -> None:
    surf.check(surf.lib.surfhip_stream_destroy(stream), "stream_destroy")


def stream_synchronize(surf, stream) -> None:
    surf.check(surf.lib.surfhip_stream_synchronize(stream), "stream_synchronize")


def copy_async(surf, dst: int, src: int, nbytes: int, stream) -> None:
    """Device to device, asynchronous on `stream`."""
    if nbytes:
        surf.check(surf.lib.surfhip_memcpy_async(dst, src, nbytes, surf.D2D, stream), "memcpy_async")


def memset_async(surf, ptr: int, value: int, nbytes: int, stream) -> None:
    if nbytes:
        surf.check(surf.lib.surfhip_memset_async(ptr, value, nbytes, stream), "memset_async")


def event_create(surf) -> int:
    return surf.event_create()


def event_destroy(surf, ev) -> None:
    surf.event_destroy(ev)


def event_record(surf, ev, stream) -> None:
    surf.check(surf.lib.surfhip_event_record(ev, stream), "event_record")


def event_synchronize(surf, ev) -> None:
    surf.check(surf.lib.surfhip_event_synchronize(ev), "event_synchronize")


def event_elapsed(surf, start, stop) -> float:
    ms = C.c_float()
    surf.check(surf.lib.surfhip_event_elapsed(C.byref(ms), start, stop), "event_elapsed")
    return float(ms.value)


class Streams:
    """`with Streams(surf, n) as (s, t): ...`: n non-blocking streams, destroyed at the end (a process
    has 4 hardware queues: the tests hold at most three user streams at once)."""

    def __init__(self, surf, n=1):
        assert 1 <= n <= 3
        self.surf, self.n, self.streams = surf, n, []

    def __enter__(self):
        self.streams = [stream_create(self.surf) for _ in range(self.n)]
        return self.streams[0] if self.n == 1 else tuple(self.streams)

    def __exit__(self, *exc):
        for s in self.streams:
            try:
                stream_synchronize(self.surf, s)
            finally:
                stream_destroy(self.surf, s)
        return False


# --------------------------------------------------- the late-upload protocol

def fill(surf, buf, value: int) -> None:
    surf.check(surf.lib.surfhip_memset(buf.ptr, value, buf.nbytes), "memset")


class Chain:
    """What one chain reads and writes.

    inputs   [(live DeviceBuffer, true bytes: numpy array or DeviceBuffer)]: the true bytes go to a
             staging buffer once; every run poisons `live` with zeros and copies staging -> live on
             the stream, ahead of the calls.  An input the calls also write (the set-1 points of a
             match) is listed among the outputs as well.
    outputs  [DeviceBuffer]: snapshotted on the stream after the calls; an output that is no input is
             filled with 0xA5 before every run.
    scratch  [DeviceBuffer]: filled with 0xFF before every run and (refill) again on the stream, beside
             the uploads: a call that clears its scratch on another stream clears it too early.
    resident [(DeviceBuffer, numpy array)]: inputs that are NOT late: uploaded before every run.  With
             the counts resident and the points late, a helper kernel that runs too early works on
             real counts and zero points and leaves wrong, not merely missing, results in the scratch
             (refill=False then keeps the late fill from covering them).
    counts   [DeviceBuffer] among the outputs that hold per-frame counts which later stages of the
             same call read back on the device (the detector's d_counts): zero, not 0xA5, before every
             run, so that a stage running too early reads "no points" and not a wild count.
    enqueue  enqueue(stream) makes the asynchronous call(s) under test on `stream` (None: the null
             stream) and nothing else: no host wait, no blocking copy.
    last     last(stream) or None: one entry point that synchronises inside (surfhip_detect,
             batch_total, ...); it runs after enqueue, and the host clock stops before it.
    setup    setup(stream) or None: runs after the buffers are prepared and the device is idle,
             right before the clock starts (a detector constructed with no wait after it).
    """

    def __init__(self, surf, inputs, outputs, enqueue, scratch=(), last=None, setup=None, counts=(), resident=(),
                 refill=True):
        self.surf, self.enqueue, self.last, self.setup = surf, enqueue, last, setup
        self.counts = {b.ptr for b in counts}
        self.resident, self.refill = list(resident), refill
        self.live, self.staging, self.own = [], [], []
        for live, true in inputs:
            if isinstance(true, np.ndarray):
                a = np.ascontiguousarray(true)
                assert a.nbytes <= live.nbytes
                st = surf.DeviceBuffer(max(a.nbytes, 4))
                st.upload(a)
                self.own.append(st)
                n = a.nbytes
            else:
                st, n = true, min(true.nbytes, live.nbytes)
            self.live.append(live)
            self.staging.append((st, n))
        self.outputs = list(outputs)
        self.scratch = list(scratch)
        self.snaps = [surf.DeviceBuffer(o.nbytes) for o in self.outputs]
        self.own += self.snaps
        self.ev = [surf.event_create() for _ in range(3)]

    def close(self):
        for b in self.own:
            b.free()
        for e in self.ev:
            self.surf.event_destroy(e)
        self.own, self.ev = [], []

    def prepare(self):
        """Step 1: poison, synchronously, then the device idle."""
        surf = self.surf
        lives = {b.ptr for b in self.live}
        for b in self.live:
            fill(surf, b, POISON_IN)
        for b in self.scratch:
            fill(surf, b, POISON_SCRATCH)
        for b in self.outputs:
            if b.ptr not in lives:
                fill(surf, b, POISON_IN if b.ptr in self.counts else POISON_OUT)
        for b in self.snaps:
            fill(surf, b, 0x5A)
        for b, a in self.resident:
            b.upload(a)
        surf.synchronize()

    def uploads(self, stream):
        for live, (st, n) in zip(self.live, self.staging):
            copy_async(self.surf, live.ptr, st.ptr, n, stream)
        for b in self.scratch if self.refill else ():
            memset_async(self.surf, b.ptr, POISON_SCRATCH, b.nbytes, stream)

    def snapshots(self, stream):
        for o, s in zip(self.outputs, self.snaps):
            copy_async(self.surf, s.ptr, o.ptr, o.nbytes, stream)

    def download(self):
        return [s.download(np.uint8, s.nbytes).tobytes() for s in self.snaps]

    def run(self, stream, spin_ms=0.0, call_stream="same", early=False):
        """One run of the chain on `stream`, the calls themselves on call_stream ("same": on `stream`).
        early: the calls first, to their end, then the uploads -- what a run looks like whose calls did
        not wait for anything.  Returns (snapshot bytes, value of `last`, t_enq ms, t_gpu ms, t_spin ms):
        host time from before the first enqueue to after the last asynchronous one, and the event times
        of the whole chain and of the spin alone."""
        surf, (e0, e1, e2) = self.surf, self.ev
        cs = stream if call_stream == "same" else call_stream
        self.prepare()
        if self.setup is not None:
            self.setup(stream)
        value = None
        if spin_ms > 0:
            spin_lib()                          # (built and loaded before the clock starts)
        t0 = time.perf_counter()
        event_record(surf, e0, stream)
        if spin_ms > 0:
            spin(spin_ms, stream)
        event_record(surf, e1, stream)
        if early:
            self.enqueue(cs)
            if self.last is not None:
                value = self.last(cs)
            surf.synchronize()
        self.uploads(stream)
        if not early:
            self.enqueue(cs)
        if self.last is not None and not early:
            t1 = time.perf_counter()
            value = self.last(cs)
            self.snapshots(stream)
        else:
            self.snapshots(stream)
            t1 = time.perf_counter()
        event_record(surf, e2, stream)
        if stream is None:
            surf.synchronize()
        else:
            stream_synchronize(surf, stream)
            if cs != stream:
                surf.synchronize()
        return (self.download(), value, 1e3 * (t1 - t0), event_elapsed(surf, e0, e2), event_elapsed(surf, e0, e1))


class LateResult:
    def __init__(self, got, ref, value, ref_value, times, poison=None):
        self.got, self.ref, self.value, self.ref_value, self.times, self.poison = got, ref, value, ref_value, times, poison

    def assert_equal(self, names=None):
        for k, (g, r) in enumerate(zip(self.got, self.ref)):
            if g != r:
                a, b = np.frombuffer(g, np.uint8), np.frombuffer(r, np.uint8)
                bad = np.nonzero(a != b)[0]
                what = names[k] if names else f"output {k}"
                raise AssertionError(f"{what}: {len(bad)} of {len(a)} bytes differ from the null-stream run, the "
                                     f"first at byte {bad[0]}: {a[bad[0]:bad[0] + 8]} vs {b[bad[0]:bad[0] + 8]}")
        assert self.value == self.ref_value, (self.value, self.ref_value)


def late(surf, stream, inputs, outputs, enqueue, scratch=(), last=None, setup=None, call_stream="same",
         poison=False, label="", counts=(), resident=(), refill=True):
    """The late-upload protocol (module docstring; DESIGN.md "Caller streams").

    Reference: the same chain, without the spin, on the null stream: enqueue(None), last(None); it is
    also the warm-up, and its event time is t_ref (a cold run, over 5 ms, is repeated and must give the
    same bytes).  Then the chain on `stream` behind a spin of 20 t_ref, clamped to [5, 100] ms.

    The run counts only when  t_enq + t_ref <= t_spin / 2  (t_enq: host time of all the enqueues,
    t_spin: event time of the spin): the spin cannot have begun before the host clock started, so all
    was enqueued, and anything that did not wait had the time to run to its end, while the live inputs
    were still poison.  Otherwise the run is repeated once with four times the spin, and after that
    the test FAILS as inconclusive -- it never skips.  The three times are printed on every run.

    poison=True also returns the outcome of the calls running early, before the uploads (controls).
    Returns a LateResult; the caller asserts on it."""
    ch = Chain(surf, inputs, outputs, enqueue, scratch, last, None, counts, resident, refill)
    try:
        ref, ref_value, _, t_ref, _ = ch.run(None)
        if t_ref > COLD_MS:
            again, again_value, _, t_ref, _ = ch.run(None)
            assert again == ref and again_value == ref_value, "two null-stream runs of the chain differ"
        early = ch.run(None, early=True)[0] if poison else None
        ch.setup = setup
        ms = min(max(SPIN_FACTOR * t_ref, SPIN_MIN_MS), SPIN_MAX_MS)
        for attempt in range(2):
            got, value, t_enq, _, t_spin = ch.run(stream, spin_ms=ms, call_stream=call_stream)
            valid = t_enq + t_ref <= 0.5 * t_spin
            print(f"late[{label}] attempt {attempt}: t_enq {t_enq:.3f} ms, t_ref {t_ref:.3f} ms, "
                  f"t_spin {t_spin:.3f} ms (asked {ms:.1f}), {'valid' if valid else 'NOT valid'}")
            if valid:
                break
            ms *= RETRY_FACTOR
        assert valid, (f"inconclusive: t_enq {t_enq:.3f} ms + t_ref {t_ref:.3f} ms exceeds half of t_spin "
                       f"{t_spin:.3f} ms twice: the inputs may have arrived before the calls were enqueued")
        return LateResult(got, ref, value, ref_value, (t_enq, t_ref, t_spin), early)
    finally:
        ch.close()


def late_interleaved(surf, parts, enqueue, label=""):
    """The protocol on several streams at once (two detectors, interleaved calls).

    parts: [(stream, inputs, outputs, counts, solo)]: per stream its late inputs and outputs and
    solo(stream_or_None), the calls of this part alone; enqueue(): the calls of all parts,
    interleaved, each on its own stream.  Reference of a part: its solo chain on the null stream.
    Every stream gets its own spin, uploads and snapshots; the run is valid when
    t_enq + the largest t_ref <= half the shortest t_spin.  Returns [LateResult] per part."""
    chains = [Chain(surf, inp, out, solo, counts=cnt) for _, inp, out, cnt, solo in parts]
    streams = [p[0] for p in parts]
    try:
        refs = []
        for ch in chains:
            ref, _, _, t_ref, _ = ch.run(None)
            if t_ref > COLD_MS:
                again, _, _, t_ref, _ = ch.run(None)
                assert again == ref, "two null-stream runs of the chain differ"
            refs.append((ref, t_ref))
        t_ref = max(t for _, t in refs)
        ms = min(max(SPIN_FACTOR * t_ref, SPIN_MIN_MS), SPIN_MAX_MS)
        spin_lib()
        for attempt in range(2):
            for ch in chains:
                ch.prepare()
            t0 = time.perf_counter()
            for ch, st in zip(chains, streams):
                event_record(surf, ch.ev[0], st)
                spin(ms, st)
                event_record(surf, ch.ev[1], st)
                ch.uploads(st)
            enqueue()
            for ch, st in zip(chains, streams):
                ch.snapshots(st)
            t_enq = 1e3 * (time.perf_counter() - t0)
            for st in streams:
                stream_synchronize(surf, st)
            t_spin = min(event_elapsed(surf, ch.ev[0], ch.ev[1]) for ch in chains)
            valid = t_enq + t_ref <= 0.5 * t_spin
            print(f"late[{label}] attempt {attempt}: t_enq {t_enq:.3f} ms, t_ref {t_ref:.3f} ms, "
                  f"t_spin {t_spin:.3f} ms (asked {ms:.1f}), {'valid' if valid else 'NOT valid'}")
            if valid:
                break
            ms *= RETRY_FACTOR
        assert valid, (f"inconclusive: t_enq {t_enq:.3f} ms + t_ref {t_ref:.3f} ms exceeds half of t_spin "
                       f"{t_spin:.3f} ms twice: the inputs may have arrived before the calls were enqueued")
        return [LateResult(ch.download(), ref, None, None, (t_enq, t_ref, t_spin)) for ch, (ref, _) in zip(chains, refs)]
    finally:
        for ch in chains:
            ch.close()
