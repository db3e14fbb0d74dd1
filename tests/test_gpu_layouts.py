"""GPU parity along three axes of the detect_batch contract the rest of the
suite leaves at their defaults: the frame layout (pitch, frame stride, base
offset, non-zero pad bytes), the sampling step, and frames taller than 32767
rows.

Every comparison is against the CPU oracle at the project's bar (integral and
response planes bit-exact, candidate count equal, keypoint fields bit-exact,
ori bit-exact when rotated, descriptors within DESC_TOL); no tolerance of its
own.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import assert_points_equal
from test_gpu_parity import _plane_views, compare_frame, gpu_run, took    # compare_frame: descriptors within DESC_TOL

pytestmark = pytest.mark.gpu

TAIL = 4096
PLAN_VARS = ("SURFHIP_II_FUSE", "SURFHIP_HESS_W", "SURFHIP_Q01", "SURFHIP_P0")


def run_layout(surf, param, imgs, pitch, stride, lead, fill, max_pts=16384, desc=True):
    """detect_batch of imgs[n, h, w] laid out as

        lead | frame 0 | ... | frame n-1 | 4096-byte tail

    frame f at lead + f * stride, its rows `pitch` apart.  The whole array is
    first filled with `fill` (0xFF, or "rand": seeded random bytes) and only
    the [h, :w] pixels are copied in, so a byte read past a row, a frame or
    the batch changes a value instead of reading an allocator's zeros.
    Returns what gpu_run returns (workspace included) plus the plan text and
    the host array's per-frame [h, pitch] views, pad bytes and all."""
    n, h, w = imgs.shape
    assert stride >= h * pitch
    total = lead + n * stride + TAIL
    if isinstance(fill, str):
        arr = np.random.default_rng(0x1A70).integers(0, 256, total, dtype=np.uint8)
    else:
        arr = np.full(total, fill, np.uint8)
    views = []
    for f in range(n):
        v = arr[lead + f * stride: lead + f * stride + h * pitch].reshape(h, pitch)
        v[:, :w] = imgs[f]
        views.append(v)
    det = surf.Detector(param, w, h, max_batch=n, max_pts=max_pts)
    buf = surf.DeviceBuffer(total)
    buf.upload(arr)
    nf = param.nfeatures
    pb = surf.DeviceBuffer(48 * n * max_pts)
    db = surf.DeviceBuffer(4 * n * max_pts * nf) if desc else None
    cb = surf.DeviceBuffer(4 * n)
    det.detect_batch(buf.ptr + lead, n, pitch, stride, pb.ptr, db.ptr if desc else None, cb.ptr)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    ds = db.download(np.float32, n * max_pts * nf).reshape(n, max_pts, nf) if desc else None
    ii, iis, rs, rss = det.workspace()
    out = {"counts": counts, "pts": [pts[f, :counts[f]] for f in range(n)],
           "desc": [ds[f, :counts[f]] for f in range(n)] if desc else None,
           "cand": det.candidates(n), "truncated": det.truncated(), "capacity": det.capacity(),
           "ii": surf.download_ptr(ii, np.int32, n * iis).reshape(n, -1),
           "resp": surf.download_ptr(rs, np.float32, n * rss).reshape(n, -1),
           "geom": det.geometry(), "plan": det.hessian_kernels(), "switches": det.switches(), "frames": views}
    det.close()
    return out


def set_plan(monkeypatch, env):
    """The plan switches of `env` ("" = the default plan; read when a detector
    is created), every other one unset."""
    for name in PLAN_VARS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SURFHIP_HESS_GATHER", "0")
    for kv in filter(None, env.split(",")):
        name, _, val = kv.partition("=")
        monkeypatch.setenv(name, val)


def params(surf, orc, noct=4, **kw):
    return surf.make_param(noct, 4.0, **kw), orc.make_param(noct, 4.0, **kw)


_PIXELS = {}
_ORACLE = {}


def pixels(surf, n, w, h, first=40):
    key = (n, w, h, first)
    if key not in _PIXELS:
        px = np.ascontiguousarray(surf.synth_frames(n, w, h, first=first)[:, :, :w])
        px.setflags(write=False)
        _PIXELS[key] = px
    return _PIXELS[key]


def oracle_frame(orc, op, key, frame, w, h):
    """The oracle's (integral, planes, geometry, octaves, points, descriptors,
    candidates) of one frame, computed once per `key`."""
    if key not in _ORACLE:
        ii, resp, g, octs = orc.hessian(op, frame, w, h)
        pts, desc, nc = orc.detect(op, frame, w, h)
        _ORACLE[key] = (ii, resp, g, octs, pts, desc, nc)
    return _ORACLE[key]


def check_frame(res, f, ref, op, min_pts):
    ii, resp, g, octs, o_pts, o_desc, nc = ref
    assert len(o_pts) >= min_pts, f"oracle: {len(o_pts)} keypoints"
    # the integral with its zero pad columns (doubled: of the upsampled frame)
    got_ii = res["ii"][f]
    assert got_ii.size == ii.size
    bad = np.argwhere(got_ii.reshape(ii.shape) != ii)
    assert len(bad) == 0, f"frame {f}: integral differs in {len(bad)} cells, first {bad[:3].tolist()}"
    for (o, s, rp), (_, _, gp) in zip(_plane_views(resp, g, octs, op), _plane_views(res["resp"][f], g, octs, op)):
        same = rp.view(np.uint32) == gp.view(np.uint32)
        assert same.all(), f"frame {f} octave {o} scale {s}: {(~same).sum()} cells differ, first {np.argwhere(~same)[0]}"
    assert not res["truncated"]
    assert res["cand"][f] == nc
    compare_frame(res["pts"][f], res["desc"][f] if res["desc"] is not None else None, o_pts, o_desc,
                  bool(op.upright))


def padded(surf, imgs):
    """The usual layout: zero pad bytes, pitch align128(W), frames back to back."""
    n, h, w = imgs.shape
    fr = np.zeros((n, h, surf.align_up(w, 128)), np.uint8)
    fr[:, :, :w] = imgs
    return fr


# ---------------------------------------------------------------- A. layouts
# (W, H, pitch): W % 4 takes all four values; 482 is just over one 480-column
# k_hess_w strip, 1924 is 4 such strips / 15 k_hess_p0 strips of 128 plus 4;
# pitch 400 is no multiple of 128; 640 has no pad bytes at all
SHAPES = [(333, 211, 336), (482, 360, 496), (1003, 303, 1008), (1924, 270, 1936), (333, 211, 400), (640, 480, 640)]
# (gap bytes between frames, lead bytes before frame 0)
GAP, TIGHT = (48, 16), (0, 0)
COMBOS = [(GAP, "rand"), (TIGHT, 0xFF), (GAP, 0xFF), (TIGHT, "rand")]
# "doubled" is no switch: SurfParam.doubled at the default step (sampling 4:
# k_double reads the caller's layout, the gather kernels the upsampled frames)
PLANS = ["", "SURFHIP_II_FUSE=2", "SURFHIP_II_FUSE=0", "SURFHIP_HESS_W=0", "SURFHIP_HESS_W=0,SURFHIP_Q01=0",
         "SURFHIP_P0=0", "SURFHIP_HESS_GATHER=1", "doubled"]
PLAN_TEXT = {"": ("k_hess_p0", "k_hess_w", "writing the integral image"),
             "SURFHIP_II_FUSE=2": ("k_hess_w", "writing the integral image (k_hess_p0)"),
             "SURFHIP_II_FUSE=0": ("k_hess_p0", "k_hess_w"),
             "SURFHIP_HESS_W=0": ("k_hess_q01",),
             "SURFHIP_HESS_W=0,SURFHIP_Q01=0": ("k_hess_p0", "k_hess_q1"),
             "SURFHIP_P0=0": ("k_hess_q0", "k_hess_w"),
             "SURFHIP_HESS_GATHER=1": ("k_hessian_t0", "k_hessian"),
             "doubled": ("k_hessian",)}


def _layout_cases():
    """Every plan meets every W % 4 and both fills (and both layouts); the
    default plan gets all six shapes."""
    cases = []
    for pi, plan in enumerate(PLANS):
        shapes = [0, 1, 2, 3, 4, 5] if plan == "" else [4 if pi % 2 else 0, 1, 2, 3]
        for k, si in enumerate(shapes):
            (gap, lead), fill = COMBOS[(k + pi) % 4]
            if si == 5:
                (gap, lead) = GAP                     # no pad bytes: the gap is all there is
            cases.append(pytest.param(plan, si, gap, lead, fill,
                                      id=f"{plan or 'default'}-{SHAPES[si][0]}x{SHAPES[si][1]}p{SHAPES[si][2]}"
                                         f"-gap{gap}-{fill}"))
    return cases


_BASE = {}


@pytest.mark.parametrize("plan,si,gap,lead,fill", _layout_cases())
def test_layout_matrix(surf, orc, monkeypatch, plan, si, gap, lead, fill):
    """Tight pitches, wide pads, gaps between frames and an offset base, with
    0xFF or random bytes wherever no pixel lies, under every Hessian plan:
    integral, planes, candidates, keypoints and descriptors as the oracle's,
    and keypoints and descriptors byte-identical to the same pixels in the
    usual zero-padded align128 layout."""
    w, h, pitch = SHAPES[si]
    n = 3
    doubled = plan == "doubled"
    set_plan(monkeypatch, "" if doubled else plan)
    imgs = pixels(surf, n, w, h)
    gp, op = params(surf, orc, upright=True, doubled=doubled)
    res = run_layout(surf, gp, imgs, pitch, h * pitch + gap, lead, fill)
    assert took(res, "" if doubled else plan), res["switches"]
    for text in PLAN_TEXT[plan]:
        assert text in res["plan"], res["plan"]
    if plan == "SURFHIP_II_FUSE=0":
        assert "writing the integral image" not in res["plan"]
    for f in range(n):
        # the oracle reads the same host bytes, pad and all
        ref = oracle_frame(orc, op, ("A", w, h, doubled, f), res["frames"][f], w, h)
        check_frame(res, f, ref, op, 50)
    bkey = (plan, w, h)
    if bkey not in _BASE:
        _BASE[bkey] = gpu_run(surf, gp, padded(surf, imgs), w, h)
    base = _BASE[bkey]
    for f in range(n):
        assert res["pts"][f].tobytes() == base["pts"][f].tobytes(), f
        assert res["desc"][f].tobytes() == base["desc"][f].tobytes(), f


@pytest.mark.parametrize("plan", ["", "SURFHIP_II_FUSE=2"], ids=lambda p: p or "default")
def test_layout_batch17(surf, orc, monkeypatch, plan):
    """17 frames of the smallest shape, tight pitch, a gap between frames and
    random bytes around them: the fused integral writers address frames past
    the 16th differently (test_fused_integral_batch256)."""
    w, h, pitch = SHAPES[0]
    n = 17
    set_plan(monkeypatch, plan)
    imgs = pixels(surf, n, w, h)
    gp, op = params(surf, orc, upright=True)
    res = run_layout(surf, gp, imgs, pitch, h * pitch + 48, 16, "rand", max_pts=2048)
    assert took(res, plan), res["switches"]
    for text in PLAN_TEXT[plan]:
        assert text in res["plan"], res["plan"]
    for f in (0, 15, 16):
        ref = oracle_frame(orc, op, ("A17", w, h, f), res["frames"][f], w, h)
        check_frame(res, f, ref, op, 50)


@pytest.mark.parametrize("plan", ["", "SURFHIP_II_FUSE=0"], ids=lambda p: p or "default")
def test_detect_batch_next_other_layout(surf, monkeypatch, plan):
    """The pipelined entry point with a next batch laid out differently from
    the current one (pitch 336 tight, then pitch 400 with a gap and an offset
    base, then 336 again): the prefetched row sums (default plan) or integral
    (SURFHIP_II_FUSE=0) are used by the following call, and every batch is
    byte-identical to a plain detect_batch of the same frames."""
    w, h = 333, 211
    n, max_pts = 3, 2048
    set_plan(monkeypatch, plan)
    gp = surf.make_param(4, 4.0, upright=True)
    # (pitch, gap, lead, fill, first frame index)
    layouts = [(336, 0, 0, "rand", 40), (400, 48, 16, 0xFF, 50), (336, 0, 0, 0xFF, 60)]
    bufs = []
    for pitch, gap, lead, fill, first in layouts:
        imgs = pixels(surf, n, w, h, first=first)
        stride = h * pitch + gap
        total = lead + n * stride + TAIL
        arr = (np.random.default_rng(first).integers(0, 256, total, dtype=np.uint8) if isinstance(fill, str)
               else np.full(total, fill, np.uint8))
        for f in range(n):
            arr[lead + f * stride: lead + f * stride + h * pitch].reshape(h, pitch)[:, :w] = imgs[f]
        b = surf.DeviceBuffer(total)
        b.upload(arr)
        bufs.append((b, b.ptr + lead, pitch, stride))
    pb = surf.DeviceBuffer(48 * n * max_pts)
    db = surf.DeviceBuffer(4 * n * max_pts * 64)
    cb = surf.DeviceBuffer(4 * n)

    def fetch():
        surf.synchronize()
        c = cb.download(np.int32, n)
        p = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
        d = db.download(np.float32, n * max_pts * 64).reshape(n, max_pts, 64)
        assert (c >= 50).all(), c
        return [(p[f, :c[f]].tobytes(), d[f, :c[f]].tobytes()) for f in range(n)]

    ref = surf.Detector(gp, w, h, max_batch=n, max_pts=max_pts)
    want = []
    for _, ptr, pitch, stride in bufs:
        ref.detect_batch(ptr, n, pitch, stride, pb.ptr, db.ptr, cb.ptr)
        want.append(fetch())
    ref.close()
    assert want[0] != want[1] and want[1] != want[2]
    det = surf.Detector(gp, w, h, max_batch=n, max_pts=max_pts)
    for k in range(3):
        _, ptr, pitch, stride = bufs[k]
        if k < 2:
            _, nptr, npitch, nstride = bufs[k + 1]
            det.detect_batch_next(ptr, n, pitch, stride, pb.ptr, db.ptr, cb.ptr, nptr, n, npitch, nstride)
        else:
            det.detect_batch_next(ptr, n, pitch, stride, pb.ptr, db.ptr, cb.ptr, None, 0, 0, 0)
        assert fetch() == want[k], k
    det.close()


# --------------------------------------------------------- B. sampling steps
def run_sampling(surf, orc, monkeypatch, w, h, n, check, min_pts, noct=4, **kw):
    """Frames in the usual layout through a detector of the given parameters,
    frames `check` against the oracle; returns gpu_run's result."""
    set_plan(monkeypatch, "")
    imgs = pixels(surf, n, w, h)
    frames = padded(surf, imgs)
    gp, op = params(surf, orc, noct, **kw)
    res = gpu_run(surf, gp, frames, w, h, want_ws=True)
    for f in check:
        ref = oracle_frame(orc, op, ("B", w, h, noct, tuple(sorted(kw.items())), f), frames[f], w, h)
        check_frame(res, f, ref, op, min_pts)
    return res


# sampling step, W, H, octaves, least oracle keypoints of the frames checked
STEPS = [(1, 320, 240, 4, 93), (3, 333, 211, 4, 89), (3, 640, 480, 4, 427), (4, 640, 480, 4, 447)]


@pytest.mark.parametrize("mode", ["upright", "rotated"])
@pytest.mark.parametrize("step,w,h,noct,min_pts", STEPS)
def test_sampling_steps(surf, orc, monkeypatch, step, w, h, noct, min_pts, mode):
    """sampling_step 1, 3 and 4: every octave on the generic k_hessian, the
    NMS scan, the fit and makePoint with deltas other than 2, 4, 8, 16."""
    n = 1 if (w, step) == (640, 3) else 2
    run_sampling(surf, orc, monkeypatch, w, h, n, range(n), min_pts, noct, sampling_step=step,
                 upright=mode == "upright")


def test_sampling_step3_extended_rotated(surf, orc, monkeypatch):
    run_sampling(surf, orc, monkeypatch, 333, 211, 2, range(2), 89, sampling_step=3, upright=False, extend=True)


def test_sampling_step3_five_octaves(surf, orc, monkeypatch):
    run_sampling(surf, orc, monkeypatch, 640, 480, 1, range(1), 427, 5, sampling_step=3, upright=True)


@pytest.mark.parametrize("step,w,h,min_pts", [(1, 320, 240, 83), (3, 333, 211, 82)])
def test_sampling_steps_batch12(surf, orc, monkeypatch, step, w, h, min_pts):
    """The batched defaults (fit records from the scan, k_describe_u2 taking
    getTrace from the fit's stash) at sampling steps 1 and 3."""
    monkeypatch.delenv("SURFHIP_TRACE_DESC", raising=False)
    monkeypatch.setenv("SURFHIP_DESC_UR", "0")
    res = run_sampling(surf, orc, monkeypatch, w, h, 12, (0, 5, 11), min_pts, sampling_step=step, upright=True)
    assert took(res, "SURFHIP_DESC_UR=0") and "SURFHIP_TRACE_DESC" not in res["switches"], res["switches"]


def test_sampling_step3_doubled(surf, orc, monkeypatch):
    """doubled with step 3: sampling 6 on the upsampled frame."""
    run_sampling(surf, orc, monkeypatch, 640, 480, 1, range(1), 703, sampling_step=3, doubled=True, upright=True)


def test_single_octave(surf, orc, monkeypatch):
    """One octave: octave 0 alone on k_hess_p0 -- no k_hess_w, no k_hess_q1,
    no integral written by the Hessian stage."""
    set_plan(monkeypatch, "")
    w, h = 640, 480
    gp = surf.make_param(1, 4.0, upright=True)
    det = surf.Detector(gp, w, h, max_batch=1, max_pts=64)
    plan = det.hessian_kernels()
    det.close()
    assert "k_hess_p0" in plan and "k_hess_w" not in plan and "q1" not in plan and "writing" not in plan, plan
    run_sampling(surf, orc, monkeypatch, w, h, 1, range(1), 319, 1, upright=True)


@pytest.mark.parametrize("plan", ["", "SURFHIP_II_FUSE=2", "SURFHIP_II_FUSE=0", "SURFHIP_HESS_GATHER=1"], ids=lambda p: p or "default")
def test_doubled_step1_streaming_plan(surf, orc, monkeypatch, plan):
    """doubled with sampling_step 1 is sampling 2 with the default lobes: the
    only way k_hess_p0, k_hess_w, the fused integral writers and k_ii_rowseg
    see the upsampled frames (their own pitch and stride).  The caller's
    frames are tight (pitch 336 for 331 columns) between random bytes; the
    (2W-1) x (2H-1) integral and everything after it as the oracle's."""
    w, h, pitch = 331, 243, 336
    n = 2
    set_plan(monkeypatch, plan)
    imgs = pixels(surf, n, w, h)
    gp, op = params(surf, orc, sampling_step=1, doubled=True, upright=True)
    assert gp.sampling == 2
    res = run_layout(surf, gp, imgs, pitch, h * pitch + 48, 16, "rand")
    assert took(res, plan), res["switches"]
    if plan in ("", "SURFHIP_II_FUSE=2"):
        assert "k_hess_p0" in res["plan"] and "writing the integral image" in res["plan"], res["plan"]
        assert ("(k_hess_p0)" in res["plan"]) == (plan != "")
    assert res["geom"][0][:2] == (2 * w - 1, 2 * h - 1)
    for f in range(n):
        ref = oracle_frame(orc, op, ("B2", w, h, f), res["frames"][f], w, h)
        check_frame(res, f, ref, op, 208)


# -------------------------------------------------------------- C. tall frame
@pytest.mark.parametrize("trace_desc", [None, "0"])
def test_tall_frame_rows_past_32767(surf, orc, monkeypatch, trace_desc):
    """256 x 33500 at sampling_step 4: keypoints past row 32767.  With
    getTrace left to k_describe_u2 the fit stashes the box centre as two
    int16, so such a frame must keep the laplace sign in the fit (the default,
    SURFHIP_TRACE_DESC unset, has to decide that by itself); every point field
    equals the oracle's either way."""
    w, h = 256, 33500
    set_plan(monkeypatch, "")
    monkeypatch.setenv("SURFHIP_DESC_UR", "0")
    if trace_desc is None:
        monkeypatch.delenv("SURFHIP_TRACE_DESC", raising=False)
    else:
        monkeypatch.setenv("SURFHIP_TRACE_DESC", trace_desc)
    imgs = pixels(surf, 1, w, h)
    frames = padded(surf, imgs)
    gp, op = params(surf, orc, sampling_step=4, upright=True)
    if "C" not in _ORACLE:
        _ORACLE["C"] = orc.detect(op, frames[0], w, h)
    o_pts, o_desc, nc = _ORACLE["C"]
    low = o_pts[o_pts["y"] >= 32770]
    assert len(o_pts) >= 11000 and len(low) >= 200
    assert (low["laplace"] == 1).any() and (low["laplace"] == -1).any()
    res = gpu_run(surf, gp, frames, w, h, max_pts=16384)
    assert took(res, "SURFHIP_DESC_UR=0" + (f",SURFHIP_TRACE_DESC={trace_desc}" if trace_desc else "")), res["switches"]
    assert not res["truncated"] and res["cand"][0] == nc
    got = res["pts"][0]
    assert len(got) == len(o_pts)
    wrong = got["laplace"] != o_pts["laplace"]
    assert not wrong.any(), (f"{int(wrong.sum())} laplace signs differ, "
                             f"{int(wrong[o_pts['y'] >= 32768].sum())} of them past row 32767")
    assert_points_equal(got, o_pts, fields=("x", "y", "scale", "o", "strength", "laplace", "ori"))
    compare_frame(got, res["desc"][0], o_pts, o_desc, True)


# ------------------------------------------------------- D. argument checks
def test_frame_argument_checks(surf):
    """check_frames and the width limits answer with an argument error
    (SurfError of the C-ABI's own status), before any kernel is launched."""
    w, h, n = 100, 64, 2
    gp = surf.make_param(4, 4.0, upright=True)
    det = surf.Detector(gp, w, h, max_batch=n, max_pts=64)
    buf = surf.DeviceBuffer(n * h * 128 + 4096)
    pb, db, cb = surf.DeviceBuffer(48 * n * 64), surf.DeviceBuffer(4 * n * 64 * 64), surf.DeviceBuffer(4 * n)

    def call(ptr, pitch, stride, nframes=n):
        det.detect_batch(ptr, nframes, pitch, stride, pb.ptr, db.ptr, cb.ptr)

    for ptr, pitch, stride in [(buf.ptr, 120, h * 120),          # pitch no multiple of 16
                               (buf.ptr, 96, h * 96),            # pitch < W
                               (buf.ptr + 8, 112, h * 112),      # base not 16-byte aligned
                               (buf.ptr, 112, h * 112 - 16),     # frames overlap
                               (buf.ptr, 112, h * 112 + 8)]:     # stride no multiple of 16
        with pytest.raises(surf.SurfError, match="invalid argument"):
            call(ptr, pitch, stride)
    call(buf.ptr, 112, h * 112)                                 # the smallest legal layout runs
    surf.synchronize()
    det.close()
    with pytest.raises(surf.SurfError, match="unsupported option"):
        surf.Detector(gp, 8192, 64, max_batch=1, max_pts=64)
    surf.Detector(gp, 8191, 64, max_batch=1, max_pts=64).close()
    dp = surf.make_param(4, 4.0, doubled=True, upright=True)
    with pytest.raises(surf.SurfError, match="unsupported option"):
        surf.Detector(dp, 4097, 64, max_batch=1, max_pts=64)     # W becomes 8192
    surf.Detector(dp, 4096, 64, max_batch=1, max_pts=64).close()
