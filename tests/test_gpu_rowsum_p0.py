"""k_hess_w's row sums from k_hess_p0's producers (plan.rsum, SURFHIP_ROWSUM).

With k_hess_w writing the integral image, its 480-column strips add S_k(r) =
the sum of pixel row r over the columns left of the strip's first halo column
X_k = 480 k - 144.  k_ii_rowseg computes them in a pass over the frames; the
default plan takes them from k_hess_p0's producers instead (own-column and
left-of-X sums per 128-column strip, added up by k_rowsum_p0).  Everything
here is integer arithmetic, so every comparison is for equality.

Shapes.  The plan needs two k_hess_w strips, i.e. a width of 481 (checked
against 480 below); the height does not enter the plan, so the frames are as
short as the existing integral-writer tests run them (37-71 rows: the first
epoch of k_hess_p0's producer ends at row 19, later ones every 36 rows, so
37, 40 and 71 all end inside an epoch whose last rows lie past the frame).
9 frames: the frame-to-XCD interleave (frame = 8 j + XCD) wraps.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 9
MAX_PTS = 2048
ST, HALO = 480, 144                      # k_hess_w's strips
# (width, height, all-255 frames)
SHAPES = [(481, 37, False), (1920, 40, False), (1003, 71, False), (1920, 40, True)]
IDS = ["481x37", "1920x40", "1003x71", "1920x40-white"]

_cache = {}


class _env:
    """Set / unset process environment variables for a block (the detector
    reads them when it is created)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _frames(surf, w, h, white):
    key = ("frames", w, h, white)
    if key not in _cache:
        fr = surf.synth_frames(N, w, h, first=700)
        if white:
            fr[:, :, :w] = 255
        fr.setflags(write=False)
        _cache[key] = fr
    return _cache[key]


def _np_rowsums(frames, w, h, ns, rows, st=ST, halo=HALO):
    """[n][ns][rows]: slab k row r = sum of frames[:, r, :st k - halo]."""
    cs = np.cumsum(frames[:, :, :w].astype(np.int64), axis=2)
    ref = np.zeros((frames.shape[0], ns, rows), np.uint32)
    for k in range(1, ns):
        ref[:, k, :h] = cs[:, :, st * k - halo - 1]
    return ref


def _np_integral(frame, w, h, ip):
    ii = np.zeros((h + 1, ip), np.int64)
    ii[1:, 1:w + 1] = np.cumsum(np.cumsum(frame[:, :w].astype(np.int64), axis=0), axis=1)
    return ii.astype(np.int32)


def _run(surf, w, h, white, mode, fuse=None):
    """One detect_batch of the 9 frames with SURFHIP_ROWSUM=mode: plan text,
    row-sum source and buffer, integral images, counts, points, descriptors."""
    key = ("run", w, h, white, mode, fuse)
    if key in _cache:
        return _cache[key]
    frames = _frames(surf, w, h, white)
    pitch = frames.shape[2]
    param = surf.make_param(4, 4.0, upright=True)
    with _env(SURFHIP_ROWSUM=mode, SURFHIP_II_FUSE=fuse):
        det = surf.Detector(param, w, h, max_batch=N, max_pts=MAX_PTS)
    fb = surf.DeviceBuffer(frames.nbytes)
    fb.upload(frames)
    pb = surf.DeviceBuffer(48 * N * MAX_PTS)
    db = surf.DeviceBuffer(4 * 64 * N * MAX_PTS)
    cb = surf.DeviceBuffer(4 * N)
    pb.zero()
    db.zero()
    det.detect_batch(fb.ptr, N, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.synchronize()
    out = {"plan": det.hessian_kernels()}
    ptr, ns, rows, src = det.rowsums()
    out["source"], out["ns"], out["rows"] = src, ns, rows
    out["rowseg"] = surf.download_ptr(ptr, np.uint32, N * ns * rows).reshape(N, ns, rows) if ptr else None
    ii, iis, _, _ = det.workspace()
    out["ii"] = surf.download_ptr(ii, np.int32, N * iis).reshape(N, -1)
    out["counts"] = cb.download(np.int32, N)
    out["points"] = pb.download(np.uint8, 48 * N * MAX_PTS)
    out["desc"] = db.download(np.uint8, 4 * 64 * N * MAX_PTS)
    det.close()
    for b in (fb, pb, db, cb):
        b.free()
    _cache[key] = out
    return out


def test_plan_selected_from_two_strips(surf):
    """The plan reports where the row sums come from; 480 columns (one
    k_hess_w strip) need none, 481 are the narrowest frames on the new path."""
    param = surf.make_param(4, 4.0, upright=True)
    with _env(SURFHIP_ROWSUM="p0", SURFHIP_II_FUSE=None):
        d480 = surf.Detector(param, 480, 37, max_batch=N, max_pts=64)
        d481 = surf.Detector(param, 481, 37, max_batch=N, max_pts=64)
    assert "row sums" not in d480.hessian_kernels() and d480.rowsums()[3] == 0
    assert "row sums from k_hess_p0" in d481.hessian_kernels() and d481.rowsums()[3] == 2
    assert "k_ii_rowseg" not in d481.hessian_kernels()
    d480.close()
    d481.close()


@pytest.mark.parametrize("w,h,white", SHAPES, ids=IDS)
def test_rowsums_equal_numpy_and_rowseg(surf, w, h, white):
    """The buffer k_hess_w reads, made by k_hess_p0 + k_rowsum_p0: bit-equal
    to numpy's cumulative sums of the frames and to k_ii_rowseg's buffer of
    the same detector configuration (slab 0 and the rows past H zero)."""
    new = _run(surf, w, h, white, "p0")
    old = _run(surf, w, h, white, "rowseg")
    assert new["source"] == 2 and "row sums from k_hess_p0" in new["plan"], new["plan"]
    assert old["source"] == 1 and "row sums from k_ii_rowseg" in old["plan"], old["plan"]
    assert (new["ns"], new["rows"]) == (old["ns"], old["rows"]) and new["ns"] == (w + ST - 1) // ST
    ref = _np_rowsums(_frames(surf, w, h, white), w, h, new["ns"], new["rows"])
    if white:
        assert ref.max() == 255 * (ST * (new["ns"] - 1) - HALO)
    bad = np.argwhere(new["rowseg"] != ref)
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    assert np.array_equal(old["rowseg"], ref)


@pytest.mark.parametrize("w,h,white", SHAPES, ids=IDS)
def test_integral_bit_exact(surf, w, h, white):
    """The integral image k_hess_w writes with the new row sums equals the
    numpy integral of every frame, pad columns included."""
    new = _run(surf, w, h, white, "p0")
    frames = _frames(surf, w, h, white)
    ip = surf.align_up(w + 1, 128)
    for f in range(N):
        ref = _np_integral(frames[f], w, h, ip)
        got = new["ii"][f][: (h + 1) * ip].reshape(h + 1, ip)
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (f, len(bad), bad[:4].tolist())


def test_switch_equality(surf):
    """Points, counts and descriptors byte-identical between
    SURFHIP_ROWSUM=p0 and rowseg on a 9-frame batch, through detect_batch and
    through two consecutive detect_batch_next calls (the second takes what the
    first prepared for it; with p0 nothing is prefetched)."""
    w, h = 1920, 256
    frames = surf.synth_frames(2 * N, w, h, first=40)
    pitch = frames.shape[2]
    param = surf.make_param(4, 4.0, upright=True)
    res = {}
    for mode in ("p0", "rowseg"):
        with _env(SURFHIP_ROWSUM=mode, SURFHIP_II_FUSE=None):
            det = surf.Detector(param, w, h, max_batch=N, max_pts=MAX_PTS)
        assert det.rowsums()[3] == (2 if mode == "p0" else 1)
        fb = [surf.DeviceBuffer(frames.nbytes // 2) for _ in range(2)]
        fb[0].upload(frames[:N])
        fb[1].upload(frames[N:])
        pb = surf.DeviceBuffer(48 * N * MAX_PTS)
        db = surf.DeviceBuffer(4 * 64 * N * MAX_PTS)
        cb = surf.DeviceBuffer(4 * N)

        def grab():
            surf.synchronize()
            out = (cb.download(np.int32, N), pb.download(np.uint8, 48 * N * MAX_PTS),
                   db.download(np.uint8, 4 * 64 * N * MAX_PTS))
            pb.zero()
            db.zero()
            return out

        pb.zero()
        db.zero()
        st = h * pitch
        runs = []
        det.detect_batch(fb[0].ptr, N, pitch, st, pb.ptr, db.ptr, cb.ptr)
        runs.append(grab())
        det.detect_batch_next(fb[0].ptr, N, pitch, st, pb.ptr, db.ptr, cb.ptr, fb[1].ptr, N, pitch, st)
        runs.append(grab())
        det.detect_batch_next(fb[1].ptr, N, pitch, st, pb.ptr, db.ptr, cb.ptr, None, 0, 0, 0)
        runs.append(grab())
        res[mode] = runs
        det.close()
        for b in fb + [pb, db, cb]:
            b.free()
    assert res["p0"][0][0].sum() > 0 and res["p0"][2][0].sum() > 0          # the frames have keypoints
    for a, b in zip(res["p0"], res["rowseg"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # the pipelined call of the first batch repeats detect_batch's result
    for x, y in zip(res["p0"][0], res["p0"][1]):
        assert np.array_equal(x, y)


def test_fallback_keeps_rowseg(surf, monkeypatch):
    """Plans the new path does not cover keep k_ii_rowseg and say so: the
    integral written by k_hess_p0 (SURFHIP_II_FUSE=2, 128-column strips), whose
    row sums and integral stay exact, and a 2-frame detector's default plan
    (the gather Hessian), which has no row sums at all."""
    w, h = 1003, 71
    r = _run(surf, w, h, False, "p0", fuse="2")
    assert r["source"] == 1 and "row sums from k_ii_rowseg" in r["plan"] and "k_rowsum_p0" not in r["plan"], r["plan"]
    frames = _frames(surf, w, h, False)
    assert r["ns"] == (w // 2 + 63) // 64
    assert np.array_equal(r["rowseg"], _np_rowsums(frames, w, h, r["ns"], r["rows"], 128, 16))
    ip = surf.align_up(w + 1, 128)
    for f in range(N):
        assert np.array_equal(r["ii"][f][: (h + 1) * ip].reshape(h + 1, ip), _np_integral(frames[f], w, h, ip))
    monkeypatch.delenv("SURFHIP_HESS_GATHER", raising=False)
    monkeypatch.setenv("SURFHIP_ROWSUM", "p0")
    det = surf.Detector(surf.make_param(4, 4.0, upright=True), 1920, 1080, max_batch=2, max_pts=64)
    assert det.rowsums() == (None, 0, 0, 0) and "row sums" not in det.hessian_kernels(), det.hessian_kernels()
    det.close()
