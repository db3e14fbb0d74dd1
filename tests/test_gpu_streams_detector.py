"""The detector on a caller's non-blocking stream S, through the late-upload
protocol of stream_ref.late ("Caller streams"): the frames reach
the live buffers on S behind a delay, every call is enqueued while they still
hold zeros, and the snapshots taken on S after the calls equal, byte for byte,
what a second detector of the same kind computes on the null stream.

Frames, Out, set_plan, N and SCHEDULES are those of test_gpu_schedule.py:
fused with both row-sum sources, the side stream without and with
integral-image Hessian kernels, and integral first.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from stream_ref import Streams, late, late_interleaved, stream_synchronize
from test_gpu_layouts import set_plan
from test_gpu_schedule import H5, SCHEDULES, W5, H, N, Out, W, frames_on_gpu, plain_results

pytestmark = pytest.mark.gpu

SMALL = (256, 128)                                  # the small frames of test_hessian_times_stop_at_capacity


def trimmed(surf, pb, db, cb, max_pts, nf, n=N):
    """Out.fetch's (counts, points, descriptors) from the snapshot bytes of an Out's three buffers."""
    c = np.frombuffer(cb, np.int32)[:n]
    assert (c >= 0).all() and (c <= max_pts).all(), c
    p = np.frombuffer(pb, surf.POINT_DTYPE).reshape(-1, max_pts)
    d = np.frombuffer(db, np.float32).reshape(-1, max_pts, nf)
    return (c.tobytes(), b"".join(p[f, :c[f]].tobytes() for f in range(n)),
            b"".join(d[f, :c[f]].tobytes() for f in range(n)))


def bufs(outs):
    return [b for o in outs for b in (o.pb, o.db, o.cb)]


def names(k):
    return [f"call {i} {what}" for i in range(k) for what in ("points", "descriptors", "counts")]


class Pair:
    """Two detectors of one kind: `ref` on the null stream, the one under test on S; chains pick
    theirs by the stream they are given.  make(S) (re)creates the one under test."""

    def __init__(self, surf, gp, w, h, max_pts, max_batch=N):
        self.surf, self.kw = surf, dict(param=gp, width=w, height=h, max_batch=max_batch, max_pts=max_pts)
        self.dets = {None: surf.Detector(**self.kw)}

    def make(self, stream):
        if stream in self.dets:
            self.dets[stream].close()
        self.dets[stream] = self.surf.Detector(stream=stream, **self.kw)
        return self.dets[stream]

    def __getitem__(self, stream):
        return self.dets[stream]

    def close(self):
        for d in self.dets.values():
            d.close()


# --------------------------------------------------------------- schedules

@pytest.mark.parametrize("fresh", [False, True], ids=["idle-after-create", "first-use-after-create"])
@pytest.mark.parametrize("env,noct", SCHEDULES, ids=[f"{e or 'default'}-{n}oct" for e, n in SCHEDULES])
def test_schedules_on_a_caller_stream(surf, monkeypatch, env, noct, fresh):
    """detect_batch(A), detect_batch_next(A, next = B), detect_batch_next(B, none) on a detector created
    on S, A and B uploaded late ahead of them.  fresh: the detector is constructed right before the
    chain with no synchronisation of any kind in between -- first use straight after the
    constructor's null-stream memsets and table upload."""
    set_plan(monkeypatch, env)
    w, h = (W5, H5) if noct == 5 else (W, H)
    max_pts = 16384 if noct == 5 else 4096
    gp = surf.make_param(noct, 4.0, upright=True)
    (a, pa), (b, pb) = sets = frames_on_gpu(surf, w, h)
    want = plain_results(surf, gp, w, h, max_pts, sets)
    la, lb = surf.DeviceBuffer(a.nbytes), surf.DeviceBuffer(b.nbytes)
    outs = [Out(surf, max_pts) for _ in range(3)]
    pair = Pair(surf, gp, w, h, max_pts)

    def chain(st):
        det = pair[st]
        det.detect_batch(la.ptr, N, pa, h * pa, *outs[0].args())
        det.detect_batch_next(la.ptr, N, pa, h * pa, *outs[1].args(), lb.ptr, N, pb, h * pb)
        det.detect_batch_next(lb.ptr, N, pb, h * pb, *outs[2].args(), None, 0, 0, 0)

    with Streams(surf) as s:
        if not fresh:
            pair.make(s)
        r = late(surf, s, [(la, a), (lb, b)], bufs(outs), chain, setup=pair.make if fresh else None,
                 counts=[o.cb for o in outs], label=f"schedule {env or 'default'} {noct}oct fresh {fresh}")
        pair.close()
    r.assert_equal(names(3))
    for k, which in enumerate((0, 0, 1)):
        assert trimmed(surf, *r.got[3 * k:3 * k + 3], max_pts, 64) == want[which], f"call {k}"
    for b_ in (la, lb):
        b_.free()


def test_set_stream(surf, monkeypatch):
    """A detector created on the null stream, moved to S (late-upload detect_batch), and, after S is
    synchronised, back to the null stream (a plain run): both give the reference bytes."""
    set_plan(monkeypatch, "")
    max_pts = 4096
    gp = surf.make_param(4, 4.0, upright=True)
    (a, pa), _ = sets = frames_on_gpu(surf, W, H)
    want = plain_results(surf, gp, W, H, max_pts, sets)
    la = surf.DeviceBuffer(a.nbytes)
    out = Out(surf, max_pts)
    pair = Pair(surf, gp, W, H, max_pts)
    with Streams(surf) as s:
        det = pair.dets[s] = surf.Detector(gp, W, H, max_batch=N, max_pts=max_pts)
        det.set_stream(s)
        r = late(surf, s, [(la, a)], bufs([out]),
                 lambda st: pair[st].detect_batch(la.ptr, N, pa, H * pa, *out.args()), counts=[out.cb],
                 label="set_stream")
        r.assert_equal(names(1))
        assert trimmed(surf, *r.got, max_pts, 64) == want[0]
        stream_synchronize(surf, s)                 # the detector does not order the new stream after the old
        det.set_stream(None)
        det.detect_batch(a.ptr, N, pa, H * pa, *out.args())
        surf.synchronize()
        assert out.fetch() == want[0]
        pair.close()
    la.free()


# ------------------------------------------------------ staged entry points

@pytest.mark.parametrize("env", ["SURFHIP_II_FUSE=0", "SURFHIP_ROWSUM=rowseg"])
def test_staged_entry_points(surf, monkeypatch, env):
    """run_integral -> run_hessian -> run_nms -> run_describe -> pack_slab on S in one chain, behind a
    detect_batch_next that leaves a prefetch of the next batch (its integral; fused: its row sums)
    running on the side stream when run_integral arrives (SURFHIP_PREFETCH=describe: the prefetch is
    the call's last launch); drain at the end, batch_total -- it synchronises -- last."""
    set_plan(monkeypatch, env)
    monkeypatch.setenv("SURFHIP_PREFETCH", "describe")
    max_pts = 4096
    gp = surf.make_param(4, 4.0, upright=True)
    (a, pa), (b, pb) = sets = frames_on_gpu(surf, W, H)
    want = plain_results(surf, gp, W, H, max_pts, sets)
    la, lb = surf.DeviceBuffer(a.nbytes), surf.DeviceBuffer(b.nbytes)
    first, out = Out(surf, max_pts), Out(surf, max_pts)
    pair = Pair(surf, gp, W, H, max_pts)
    slab = surf.DeviceBuffer(pair[None].slab_bytes(N, N * max_pts))      # (pack_slab takes no capacity)

    def chain(st):
        det = pair[st]
        det.detect_batch_next(lb.ptr, N, pb, H * pb, first.pb.ptr, None, first.cb.ptr, la.ptr, N, pa, H * pa)
        det.run_integral(la.ptr, N, pa, H * pa)
        det.run_hessian(N)
        det.run_nms(N, out.pb.ptr, out.cb.ptr)
        det.run_describe(out.pb.ptr, out.cb.ptr, N, out.db.ptr)
        det.pack_slab(out.pb.ptr, out.db.ptr, out.cb.ptr, N, slab.ptr)
        det.drain()

    with Streams(surf) as s:
        pair.make(s)
        r = late(surf, s, [(la, a), (lb, b)], [first.pb, first.cb] + bufs([out]) + [slab], chain,
                 last=lambda st: pair[st].batch_total(N), counts=[first.cb, out.cb], label=f"staged {env}")
        pair.close()
    r.assert_equal(["first call points", "first call counts", "points", "descriptors", "counts", "slab"])
    counts = np.frombuffer(want[0][0], np.int32)
    assert r.value == int(counts.sum())
    assert r.got[1][:4 * N] == want[1][0] and r.got[4][:4 * N] == want[0][0]
    c, p, d = surf.parse_slab(np.frombuffer(r.got[5], np.uint8))
    assert c.tobytes() == want[0][0] and len(p) == r.value and d.shape == (r.value, 64)
    for b_ in (la, lb, slab):
        b_.free()


# ------------------------------------------------------ other detector cases

def one_call(surf, gp, w, h, max_pts, label, nframes=N, keep=None, nf=64, min_count=1):
    """One late-upload detect_batch of set A's first nframes on a detector bound to S against the
    same call on a null-stream detector; returns the trimmed (counts, points, descriptors)."""
    (a, pa), _ = frames_on_gpu(surf, w, h)
    la = surf.DeviceBuffer(a.nbytes)
    out = Out(surf, max_pts, nf=nf)
    pair = Pair(surf, gp, w, h, max_pts)
    with Streams(surf) as s:
        pair.make(s)
        for det in pair.dets.values():
            if keep is not None:
                det.set_keep(*keep)
        r = late(surf, s, [(la, a)], bufs([out]),
                 lambda st: pair[st].detect_batch(la.ptr, nframes, pa, h * pa, *out.args()), counts=[out.cb],
                 label=label)
        pair.close()
    la.free()
    r.assert_equal(names(1))
    got = trimmed(surf, *r.got, max_pts, nf, nframes)
    assert (np.frombuffer(got[0], np.int32) >= min_count).all(), np.frombuffer(got[0], np.int32)
    return got


def test_keep_strongest_over_budget(surf, monkeypatch):
    """Every frame holds more than 32 points: k_keep_strongest."""
    set_plan(monkeypatch, "")
    gp = surf.make_param(4, 4.0, upright=True)
    got = one_call(surf, gp, W, H, 4096, "keep strongest", keep=(surf.KEEP_STRONGEST, 32), min_count=32)
    assert (np.frombuffer(got[0], np.int32) == 32).all()


def test_doubled_detector(surf, monkeypatch):
    """k_double ahead of the integral."""
    set_plan(monkeypatch, "")
    gp = surf.make_param(4, 4.0, doubled=True, upright=True)
    one_call(surf, gp, *SMALL, 4096, "doubled")


def test_small_batch_describe_default(surf, monkeypatch):
    """SURFHIP_DESC_UR unset and 8 frames: k_describe_ur."""
    set_plan(monkeypatch, "")
    monkeypatch.delenv("SURFHIP_DESC_UR", raising=False)
    gp = surf.make_param(4, 4.0, upright=True)
    one_call(surf, gp, W, H, 4096, "describe_ur", nframes=8, min_count=50)


def test_single_frame_detect(surf, monkeypatch):
    """The synchronous surfhip_detect on a detector bound to S, the frame uploaded late: the call is
    the chain's last; its descriptors (an allocation of its own) are copied out behind it."""
    set_plan(monkeypatch, "")
    max_pts = 4096
    gp = surf.make_param(4, 4.0, upright=True)
    (a, pa), _ = frames_on_gpu(surf, W, H)
    la = surf.DeviceBuffer(H * pa)
    pts, desc = surf.DeviceBuffer(48 * max_pts), surf.DeviceBuffer(4 * 64 * max_pts)
    pair = Pair(surf, gp, W, H, max_pts, max_batch=1)

    def detect(st):
        n, dptr = pair[st].detect(la.ptr, pa, pts.ptr, max_pts)
        surf.check(surf.lib.surfhip_memcpy(desc.ptr, dptr, 4 * 64 * n, surf.D2D), "memcpy")
        surf.check(surf.lib.surfhip_free(dptr), "free")
        return n

    with Streams(surf) as s:
        pair.make(s)
        r = late(surf, s, [(la, a)], [pts, desc], lambda st: None, last=detect, label="detect")
        pair.close()
    r.assert_equal(["points", "descriptors"])
    assert r.value >= 50
    for b_ in (la, pts, desc):
        b_.free()


# ----------------------------------------------------- profiling and timing

def test_profiled_and_timed_calls(surf, monkeypatch):
    """set_profiling and time_hessian record their events on S: one profiled and one timed call on
    late frames give the reference bytes and finite, non-negative times (the values are not judged)."""
    set_plan(monkeypatch, "SURFHIP_II_FUSE=0")
    max_pts = 4096
    gp = surf.make_param(4, 4.0, upright=True)
    (a, pa), _ = sets = frames_on_gpu(surf, W, H)
    want = plain_results(surf, gp, W, H, max_pts, sets)
    la = surf.DeviceBuffer(a.nbytes)
    out = Out(surf, max_pts)
    pair = Pair(surf, gp, W, H, max_pts)
    stages = {}

    def call(st):
        pair[st].detect_batch(la.ptr, N, pa, H * pa, *out.args())

    def stage_times(st):
        stages[st] = pair[st].stage_times()          # (waits for the call's last event)

    with Streams(surf) as s:
        det = pair.make(s)
        for d in pair.dets.values():
            d.set_profiling(True)
        r = late(surf, s, [(la, a)], bufs([out]), call, last=stage_times, counts=[out.cb], label="profiled")
        r.assert_equal(names(1))
        assert trimmed(surf, *r.got, max_pts, 64) == want[0]
        print("stage_times on S", stages[s])
        assert len(stages[s]) == 6 and all(math.isfinite(v) and v >= 0 for v in stages[s].values()), stages[s]
        for d in pair.dets.values():
            d.set_profiling(False)
            d.time_hessian(True)
        r = late(surf, s, [(la, a)], bufs([out]), call, counts=[out.cb], label="timed")
        r.assert_equal(names(1))
        assert trimmed(surf, *r.got, max_pts, 64) == want[0]
        times = det.hessian_times()
        print("hessian_times on S", times)
        assert 1 <= len(times) <= 2 and all(math.isfinite(t) and t >= 0 for t in times), times
        pair.close()
    la.free()


# ------------------------------------------------------ two detectors at once

def test_two_detectors_interleaved(surf, monkeypatch):
    """An upright 64-feature detector on S1 and a rotated extended 128-feature one on S2, their calls
    interleaved A1, B1, A2, B2 with late uploads on both streams: each detector's bytes are those of
    its calls alone on the null stream.  (Every create rewrites the process-wide constant table.)"""
    set_plan(monkeypatch, "")
    max_pts = 4096
    (a, pa), (b, pb) = frames_on_gpu(surf, W, H)
    gps = [surf.make_param(4, 4.0, upright=True), surf.make_param(4, 4.0, upright=False, extend=True)]
    nfs = [64, 128]
    pairs = [Pair(surf, gp, W, H, max_pts) for gp in gps]
    lives = [[surf.DeviceBuffer(a.nbytes), surf.DeviceBuffer(b.nbytes)] for _ in gps]
    outs = [[Out(surf, max_pts, nf=nf) for _ in range(2)] for nf in nfs]

    def call(k, i, st):
        buf, pitch = (lives[k][i], (pa, pb)[i])
        pairs[k][st].detect_batch(buf.ptr, N, pitch, H * pitch, *outs[k][i].args())

    with Streams(surf, 2) as ss:
        for pair, st in zip(pairs, ss):
            pair.make(st)
        parts = [(ss[k], [(lives[k][0], a), (lives[k][1], b)], bufs(outs[k]), [o.cb for o in outs[k]],
                  (lambda st, k=k: (call(k, 0, st), call(k, 1, st)))) for k in range(2)]
        rs = late_interleaved(surf, parts, lambda: [call(k, i, ss[k]) for i in range(2) for k in range(2)],
                              label="two detectors")
        for pair in pairs:
            pair.close()
    for k, r in enumerate(rs):
        r.assert_equal([f"detector {k} {n}" for n in names(2)])
        for i in range(2):
            c = np.frombuffer(trimmed(surf, *r.got[3 * i:3 * i + 3], max_pts, nfs[k])[0], np.int32)
            assert (c >= 50).all(), c
    assert rs[0].got[2] == rs[1].got[2]               # the same keypoint counts, rotated or not
    for pairbufs in lives:
        for b_ in pairbufs:
            b_.free()


# -------------------------------------------------------------- ingest ring

def test_ingest_ring_on_a_caller_stream(surf, monkeypatch):
    """The ring (its copy and out streams against the detector's) over a detector bound to S, depth 2,
    three batches: the slabs of test_gpu_parity.test_ingest_ring_equals_resident_batches' resident
    path.  The ring is driven by the host: no late upload here."""
    set_plan(monkeypatch, "")
    w, h, B, max_pts = 320, 240, 3, 4096
    param = surf.make_param(4, 4.0, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    sizes = [3, 3, 2]
    frames = surf.synth_frames(sum(sizes), w, h, first=40)
    pitch = frames.shape[2]
    ref = []
    det = surf.Detector(param, w, h, max_batch=B, max_pts=max_pts)
    fb, pb = surf.DeviceBuffer(frames[:B].nbytes), surf.DeviceBuffer(48 * B * max_pts)
    db, cb = surf.DeviceBuffer(4 * B * max_pts * nf), surf.DeviceBuffer(4 * B)
    first = 0
    for n in sizes:
        fb.upload(np.ascontiguousarray(frames[first:first + n]))
        det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
        total = det.batch_total(n)
        sb = surf.DeviceBuffer(det.slab_bytes(n, total))
        det.pack_slab(pb.ptr, db.ptr, cb.ptr, n, sb.ptr)
        surf.synchronize()
        ref.append(sb.download(np.uint8, det.slab_bytes(n, total)))
        sb.free()
        first += n
    det.close()
    with Streams(surf) as s:
        det = surf.Detector(param, w, h, max_batch=B, max_pts=max_pts, stream=s)
        ing = surf.Ingest(det, 2)
        got, first = [], 0
        for n in sizes:
            if ing.pending() == 2:
                got.append(ing.collect())
            slot = ing.acquire()
            slot[:n, :, :w] = frames[first:first + n, :, :w]
            ing.submit(n)
            first += n
        while ing.pending():
            got.append(ing.collect())
        ing.close()
        det.close()
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.tobytes() == r.tobytes(), f"batch {i} slab differs"
        assert surf.parse_slab(g)[0].min() >= 20
    for b_ in (fb, pb, db, cb):
        b_.free()
