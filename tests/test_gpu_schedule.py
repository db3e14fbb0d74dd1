"""The host side of the Hessian stage: which kernels each plan names, and that
every way of calling a detector -- plain, pipelined, with in-step Hessian
timing, stage-profiled -- enqueues work that computes the same bytes.

Results are compared byte for byte with a fresh detector's detect_batch of the
same frames under the same plan; no tolerance anywhere.  The plan texts are
literals taken from the library before the stage's host code was rewritten.
"""
from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_layouts import PLANS, set_plan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_HESS_EV = 64                    # SURFHIP_MAX_HESS_EV (include/surfhip.h)
# 9 frames cross the 8-frame XCD grouping; 640 columns are two k_hess_w strips
# and five k_hess_p0 strips, so both row-sum sources are live
N, W, H = 9, 640, 480
W5, H5 = 1920, 1080                 # the 5-octave shape of test_gpu_configs.py

P0W = "k_hess_p0 (octave 0) + k_hess_w (octaves 1-3)"
PLAN_TEXT = {
    "": P0W + ", writing the integral image, row sums from k_hess_p0 + k_rowsum_p0",
    "SURFHIP_II_FUSE=2": P0W + ", writing the integral image (k_hess_p0), row sums from k_ii_rowseg",
    "SURFHIP_II_FUSE=0": P0W,
    "SURFHIP_HESS_W=0": "k_hess_q01 (octaves 0-1) + k_hessian (octaves 2-3)",
    "SURFHIP_HESS_W=0,SURFHIP_Q01=0": "k_hess_p0 (octave 0) + k_hess_q1 (octave 1) + k_hessian (octaves 2-3)",
    "SURFHIP_P0=0": "k_hess_q0 (octave 0) + k_hess_w (octaves 1-3)",
    "SURFHIP_HESS_GATHER=1": "k_hessian_t0 (octave 0) + k_hessian (octaves 1-3)",
    "doubled": "k_hessian (octaves 0-3)",
    "SURFHIP_ROWSUM=rowseg": P0W + ", writing the integral image, row sums from k_ii_rowseg",
    "SURFHIP_HESS_GATHER=1,SURFHIP_HESS_T0=0": "k_hessian (octaves 0-3)",
    "octaves=2": "k_hess_q01 (octaves 0-1)",
    "octaves=3": "k_hess_p0 (octave 0) + k_hess_w (octaves 1-2), writing the integral image, "
                 "row sums from k_hess_p0 + k_rowsum_p0",
    "octaves=5": P0W + ", writing the integral image, row sums from k_hess_p0 + k_rowsum_p0 + k_hessian (octave 4)",
    "max_batch=1": "k_hessian_t0 (octave 0) + k_hessian (octaves 1-3)",
}


def test_plan_text_unchanged(surf, monkeypatch):
    """make_plan, pinned exactly: the plan text of every plan the layout tests
    run, of the row-sum and gather switches, of 2, 3 and 5 octaves and of the
    one-frame detector that picks the gather plan by itself."""
    assert set(PLANS) <= set(PLAN_TEXT)
    got = {}
    for case in PLAN_TEXT:
        kind, _, val = case.partition("=")
        noct = int(val) if kind == "octaves" else 4
        for name in ("SURFHIP_ROWSUM", "SURFHIP_HESS_T0"):      # (set_plan clears the others)
            monkeypatch.delenv(name, raising=False)
        set_plan(monkeypatch, case if kind.startswith("SURFHIP_") else "")
        if kind == "max_batch":
            monkeypatch.delenv("SURFHIP_HESS_GATHER")
        w, h = (W5, H5) if noct == 5 else (W, H)
        gp = surf.make_param(noct, 4.0, upright=True, doubled=case == "doubled")
        det = surf.Detector(gp, w, h, max_batch=1 if kind == "max_batch" else N, max_pts=64)
        got[case] = det.hessian_kernels()
        det.close()
    print(got)
    assert got == PLAN_TEXT


# ------------------------------------------------------------------ schedules
_FRAMES = {}


def frames_on_gpu(surf, w, h):
    """Sets A (first=0) and B (first=100) of N frames on the device:
    (buffer, pitch) each, uploaded once per shape."""
    if (w, h) not in _FRAMES:
        sets = []
        for first in (0, 100):
            fr = surf.synth_frames(N, w, h, first=first)
            buf = surf.DeviceBuffer(fr.nbytes)
            buf.upload(fr)
            sets.append((buf, fr.shape[2]))
        _FRAMES[(w, h)] = sets
    return _FRAMES[(w, h)]


class Out:
    """One call's output buffers, so that a sequence of calls needs no host
    synchronisation until all of it is enqueued."""

    def __init__(self, surf, max_pts, nf=64, min_pts=50):
        self.surf, self.max_pts, self.nf, self.min_pts = surf, max_pts, nf, min_pts
        self.pb = surf.DeviceBuffer(48 * N * max_pts)
        self.db = surf.DeviceBuffer(4 * N * max_pts * nf)
        self.cb = surf.DeviceBuffer(4 * N)

    def args(self):
        return self.pb.ptr, self.db.ptr, self.cb.ptr

    def fetch(self):
        """(counts, points, descriptors) as bytes; call after synchronize."""
        c = self.cb.download(np.int32, N)
        assert (c >= self.min_pts).all() and (c < self.max_pts).all(), c
        p = self.pb.download(self.surf.POINT_DTYPE, N * self.max_pts).reshape(N, self.max_pts)
        d = self.db.download(np.float32, N * self.max_pts * self.nf).reshape(N, self.max_pts, self.nf)
        return (c.tobytes(), b"".join(p[f, :c[f]].tobytes() for f in range(N)),
                b"".join(d[f, :c[f]].tobytes() for f in range(N)))


def plain_results(surf, gp, w, h, max_pts, sets):
    """A fresh detector's detect_batch of sets A and B."""
    det = surf.Detector(gp, w, h, max_batch=N, max_pts=max_pts)
    want = []
    for buf, pitch in sets:
        out = Out(surf, max_pts)
        det.detect_batch(buf.ptr, N, pitch, h * pitch, *out.args())
        surf.synchronize()
        want.append(out.fetch())
    det.close()
    assert want[0] != want[1]
    return want


SCHEDULES = [("", 4), ("SURFHIP_ROWSUM=rowseg", 4), ("SURFHIP_II_FUSE=0", 4), ("SURFHIP_II_FUSE=0", 5),
             ("SURFHIP_HESS_GATHER=1", 4)]


@pytest.mark.parametrize("env,noct", SCHEDULES, ids=[f"{e or 'default'}-{n}oct" for e, n in SCHEDULES])
def test_timed_and_profiled_calls_match_plain(surf, monkeypatch, env, noct):
    """Fused (row sums from k_hess_p0, or prefetched from k_ii_rowseg), the
    u8 kernels beside the integral on the side stream (without and with
    integral-image Hessian kernels there) and integral first: a plain call,
    timed pipelined calls with and without a next batch, a stage-profiled call
    and a timed plain call, enqueued back to back on one detector, all give
    the bytes of a fresh detector's detect_batch; the in-step timer counts the
    unprofiled timed calls only."""
    set_plan(monkeypatch, env)
    w, h = (W5, H5) if noct == 5 else (W, H)
    max_pts = 16384 if noct == 5 else 4096
    gp = surf.make_param(noct, 4.0, upright=True)
    (a, pa), (b, pb) = sets = frames_on_gpu(surf, w, h)
    want = plain_results(surf, gp, w, h, max_pts, sets)
    det = surf.Detector(gp, w, h, max_batch=N, max_pts=max_pts)
    outs = [Out(surf, max_pts) for _ in range(5)]
    det.detect_batch(a.ptr, N, pa, h * pa, *outs[0].args())
    det.time_hessian(True)
    det.detect_batch_next(a.ptr, N, pa, h * pa, *outs[1].args(), b.ptr, N, pb, h * pb)
    det.detect_batch_next(b.ptr, N, pb, h * pb, *outs[2].args(), None, 0, 0, 0)
    det.set_profiling(True)
    det.detect_batch(a.ptr, N, pa, h * pa, *outs[3].args())
    stages = det.stage_times()
    det.set_profiling(False)
    det.detect_batch(b.ptr, N, pb, h * pb, *outs[4].args())
    surf.synchronize()
    times = det.hessian_times()
    again = det.hessian_times()
    for k, which in enumerate((0, 0, 1, 0, 1)):
        assert outs[k].fetch() == want[which], f"call {k}"
    print(f"{env or 'default'} {noct} octaves: hessian_times {times} stage_times {stages}")
    assert len(times) == 3, times
    assert all(math.isfinite(t) and t > 0 for t in times), times
    assert again == []
    assert len(stages) == 6 and all(math.isfinite(v) and v >= 0 for v in stages.values()), stages
    parts = sum(v for k, v in stages.items() if k != "total")
    assert stages["total"] >= 0.99 * parts, stages
    det.close()


def test_hessian_times_stop_at_capacity(surf, monkeypatch):
    """MAX_HESS_EV + 3 timed calls: the timer keeps the first MAX_HESS_EV and
    the calls past them still compute the same bytes."""
    set_plan(monkeypatch, "")
    w, h, max_pts = 256, 128, 1024
    gp = surf.make_param(4, 4.0, upright=True)
    (a, pa), _ = frames_on_gpu(surf, w, h)
    det = surf.Detector(gp, w, h, max_batch=N, max_pts=max_pts)
    first, last = Out(surf, max_pts, min_pts=1), Out(surf, max_pts, min_pts=1)
    det.time_hessian(True)
    for k in range(MAX_HESS_EV + 3):
        det.detect_batch(a.ptr, N, pa, h * pa, *(first if k == 0 else last).args())
    surf.synchronize()
    times = det.hessian_times()
    assert len(times) == MAX_HESS_EV
    assert all(math.isfinite(t) and t > 0 for t in times), times
    assert det.hessian_times() == []
    assert last.fetch() == first.fetch()
    det.close()
    ref = surf.Detector(gp, w, h, max_batch=N, max_pts=max_pts)
    out = Out(surf, max_pts, min_pts=1)
    ref.detect_batch(a.ptr, N, pa, h * pa, *out.args())
    surf.synchronize()
    assert out.fetch() == first.fetch()
    ref.close()


# ------------------------------------------------ SURFHIP_PREFETCH, per process
CHILD = r"""
import hashlib, importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
surf = importlib.import_module("cuda-surf_amd")
N, W, H, MAX_PTS = 9, 640, 480, 4096
gp = surf.make_param(4, 4.0, upright=True)
sets = []
for first in (0, 100):
    fr = surf.synth_frames(N, W, H, first=first)
    buf = surf.DeviceBuffer(fr.nbytes)
    buf.upload(fr)
    sets.append((buf, fr.shape[2]))
pb, db, cb = surf.DeviceBuffer(48 * N * MAX_PTS), surf.DeviceBuffer(4 * N * MAX_PTS * 64), surf.DeviceBuffer(4 * N)

def digest(hsh):
    surf.synchronize()
    c = cb.download(np.int32, N)
    assert (c >= 50).all() and (c < MAX_PTS).all(), c
    p = pb.download(surf.POINT_DTYPE, N * MAX_PTS).reshape(N, MAX_PTS)
    d = db.download(np.float32, N * MAX_PTS * 64).reshape(N, MAX_PTS, 64)
    hsh.update(c.tobytes())
    for f in range(N):
        hsh.update(p[f, :c[f]].tobytes())
        hsh.update(d[f, :c[f]].tobytes())

order = (0, 1, 0)
plain, piped = hashlib.sha256(), hashlib.sha256()
det = surf.Detector(gp, W, H, max_batch=N, max_pts=MAX_PTS)
print("plan", det.hessian_kernels())
for k in order:
    buf, pitch = sets[k]
    det.detect_batch(buf.ptr, N, pitch, H * pitch, pb.ptr, db.ptr, cb.ptr)
    digest(plain)
det.close()
det = surf.Detector(gp, W, H, max_batch=N, max_pts=MAX_PTS)
for i, k in enumerate(order):
    buf, pitch = sets[k]
    if i + 1 < len(order):
        nbuf, npitch = sets[order[i + 1]]
        det.detect_batch_next(buf.ptr, N, pitch, H * pitch, pb.ptr, db.ptr, cb.ptr, nbuf.ptr, N, npitch, H * npitch)
    else:
        det.detect_batch_next(buf.ptr, N, pitch, H * pitch, pb.ptr, db.ptr, cb.ptr, None, 0, 0, 0)
    digest(piped)
det.close()
print("plain", plain.hexdigest())
print("piped", piped.hexdigest())
"""


@pytest.mark.parametrize("plan", ["SURFHIP_ROWSUM=rowseg", "SURFHIP_II_FUSE=0"])
def test_prefetch_env_values(plan):
    """SURFHIP_PREFETCH (one child process per value) unset, nms, describe and an
    unlisted value, where the prefetch is the row-sum pass and where it is the
    integral: the pipelined sequence A -> B, B -> A, A -> none hashes like the
    same batches through detect_batch, in every child alike."""
    hashes = {}
    for value in (None, "nms", "describe", "tail"):
        # (SURFHIP_LIB_DIR names the build under test, no switch of it)
        env = {k: v for k, v in os.environ.items() if not k.startswith("SURFHIP_") or k == "SURFHIP_LIB_DIR"}
        env.update(SURFHIP_HESS_GATHER="0", SURFHIP_DESC_UR="0")
        name, _, val = plan.partition("=")
        env[name] = val
        if value is not None:
            env["SURFHIP_PREFETCH"] = value
        r = subprocess.run([sys.executable, "-c", CHILD, REPO], capture_output=True, text=True, timeout=120,
                           cwd=REPO, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.strip())
        print(value, out)
        assert ("k_ii_rowseg" in out["plan"]) == (plan == "SURFHIP_ROWSUM=rowseg"), out["plan"]
        assert "writing the integral image" not in out["plan"] or plan != "SURFHIP_II_FUSE=0", out["plan"]
        assert len(out["plain"]) == 64 and out["piped"] == out["plain"], (value, out)
        hashes[value] = out["plain"]
    assert len(set(hashes.values())) == 1, hashes
