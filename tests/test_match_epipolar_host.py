"""CPU tests of surfhip_match_batch_epipolar's argument checks and scratch size
(no GPU call: every case returns before a launch), of its Python surface, and
of the numpy twin of the kernels' line-against-box test."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from epipolar_ref import RECTIFIED, ZERO, epipolar_lines, line_may_offer, pose_f, rot, translation_f

OK, INVALID = 0, -1
P = 0x1000          # a non-NULL, 16-B aligned pointer value; never dereferenced by a rejected call
INF, NAN = math.inf, math.nan
DEFAULT = object()


def call(surf, pts1=P, desc1=P, counts1=P, slots1=64, pts2=P, desc2=P, counts2=P, slots2=64, npairs=1,
         nf=64, flags=0, f=P, f_stride=16, band=1.5, window=DEFAULT, scratch=P):
    if window is DEFAULT:
        window = (-64.0, 0.0, -INF, INF)
    w = None if window is None else C.byref(surf.MatchWindow(*window))
    return surf.lib.surfhip_match_batch_epipolar(pts1, desc1, counts1, slots1, pts2, desc2, counts2, slots2, npairs,
                                                 nf, flags, f, f_stride, band, w, scratch, None)


def test_constants_and_binding(surf):
    assert surf.MATCH_FULL_TAIL == 1 and surf.MATCH_SAME_LAPLACE == 2 and surf.MATCH_MUTUAL == 4
    assert callable(surf.match_batch_epipolar) and callable(surf.match_batch_epipolar_scratch_bytes)
    assert "surfhip_match_batch_epipolar" in surf._sigs and "surfhip_match_batch_epipolar_scratch" in surf._sigs
    assert len(surf._sigs["surfhip_match_batch_epipolar"][1]) == 17
    assert surf._sigs["surfhip_match_batch_epipolar"][1][13] is C.c_float
    src = open(surf.REPO + "/include/surfhip.h").read()
    assert "int surfhip_match_batch_epipolar(" in src and "size_t surfhip_match_batch_epipolar_scratch(" in src
    assert "const float* d_f, int f_stride, float band," in src
    text = " ".join(src.replace("\n *", " ").split())             # the comment as running text
    for words in ("(x2, y2, 1) F (x1, y1, 1)^T = 0",
                  "lim = (band * band) * (a*a + b*b);",
                  "r = (x2*a + y2*b) + c; offered <=> r*r <= lim",
                  "that of surfhip_match_batch_window with the same window and flags",
                  "that of surfhip_match_batch_window with (dx_min, dx_max, -B, B)",
                  "A matrix that holds a NaN offers nothing",
                  "band = 0 is valid: only r*r == 0 is offered"):
        assert words in text, words
    # f_stride 16: the matrix is the first member of the 64-B record
    assert surf.FUNDAMENTAL_DTYPE.itemsize == 64 and surf.FUNDAMENTAL_DTYPE.fields["f"][1] == 0


BAD_BANDS = [NAN, INF, -INF, -1.0, -0.5]


@pytest.mark.parametrize("kw", [dict(npairs=-1), dict(slots1=0), dict(slots1=-4), dict(slots2=0), dict(slots2=-1),
                                dict(nf=0), dict(nf=2), dict(nf=66), dict(nf=1028), dict(nf=-64),
                                dict(flags=8), dict(flags=8 | 1), dict(flags=16 | 4), dict(flags=-1),
                                dict(pts1=None), dict(desc1=None), dict(counts1=None),
                                dict(pts2=None), dict(desc2=None), dict(counts2=None),
                                dict(scratch=None), dict(scratch=P + 8), dict(scratch=P + 4),
                                dict(window=None),
                                dict(window=(NAN, 1.0, -1.0, 1.0)), dict(window=(-1.0, NAN, -1.0, 1.0)),
                                dict(window=(-1.0, 1.0, NAN, 1.0)), dict(window=(-1.0, 1.0, -1.0, NAN)),
                                dict(window=(1.0, -1.0, -1.0, 1.0)), dict(window=(-1.0, 1.0, 1.0, -1.0)),
                                dict(window=(INF, -INF, -1.0, 1.0)), dict(window=(-1.0, 1.0, INF, -INF)),
                                dict(f_stride=-1), dict(f_stride=1), dict(f_stride=8), dict(f_stride=-16),
                                dict(f=None), dict(f=P + 2), dict(f=None, f_stride=0), dict(f=P + 2, f_stride=9)]
                         + [dict(band=b) for b in BAD_BANDS])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(slots1=0), dict(nf=6), dict(flags=16), dict(flags=8), dict(window=None),
                                dict(window=(NAN, 1.0, -1.0, 1.0)), dict(window=(2.0, 1.0, -1.0, 1.0)),
                                dict(f_stride=-1), dict(f_stride=1), dict(f_stride=8), dict(f_stride=-16)]
                         + [dict(band=b) for b in BAD_BANDS])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, npairs=0, **kw) == INVALID
    assert call(surf, npairs=0, f=None, **kw) == INVALID


@pytest.mark.parametrize("f_stride", [0, 9, 16, 1000])
def test_valid_strides(surf, f_stride):
    """Accepted (zero pairs: the call returns before it would touch the GPU)
    where the neighbouring values are rejected."""
    assert call(surf, npairs=0, f_stride=f_stride) == OK
    assert call(surf, npairs=0, f_stride=f_stride, f=None) == OK
    assert call(surf, npairs=0, f_stride=f_stride, f=P + 2) == OK     # d_f is checked with npairs > 0 only
    # with a pair, the stride passes the scalar checks: the call is then rejected for its NULL d_pts1 alone
    assert call(surf, f_stride=f_stride, pts1=None) == INVALID


@pytest.mark.parametrize("band", [0.0, 1e6, 1.5, 1e-30])
def test_valid_bands(surf, band):
    assert call(surf, npairs=0, band=band) == OK
    assert call(surf, band=band, pts1=None) == INVALID               # (rejected for the NULL d_pts1 alone)


@pytest.mark.parametrize("flags", range(8))
def test_zero_pairs_is_ok(surf, flags):
    assert call(surf, npairs=0, flags=flags) == OK
    assert call(surf, npairs=0, flags=flags, pts1=None, desc1=None, counts1=None, pts2=None, desc2=None,
                counts2=None, f=None, scratch=None) == OK
    surf.match_batch_epipolar(None, None, None, 16, None, None, None, 16, 0, 128, flags, None, 16, 1.5,
                              (-1, 1, -2, 2), None)
    surf.match_batch_epipolar(None, None, None, 16, None, None, None, 16, 0, 128, flags, None, 0, 0.0,
                              surf.MatchWindow(-INF, INF, -INF, INF), None)


@pytest.mark.parametrize("window", [(-INF, INF, -INF, INF), (0.0, 0.0, 0.0, 0.0), (-64.0, 0.0, -1.5, 1.5),
                                    (-INF, -INF, INF, INF), (5.0, INF, -INF, -5.0)])
def test_infinite_and_degenerate_windows_are_valid(surf, window):
    assert call(surf, npairs=0, window=window) == OK


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 1, 64, 0, P, 16, 1.5, (-1, 1, -1, 1), None)
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 1, 64, 0, None, 16, 1.5, (-1, 1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 8, 1.5, (-1, 1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 16, 1.5, (1, -1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 16, -1.0, (-1, 1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_epipolar(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 16, NAN, (-1, 1, -1, 1), P)


def test_scratch_size(surf):
    size, window_size = surf.match_batch_epipolar_scratch_bytes, surf.match_batch_window_scratch_bytes
    for flags in (0, 4, 7):
        for args in ((0, 64, 64), (-1, 64, 64), (3, 64, 0), (3, 64, -5), (3, 0, 64), (3, -1, 64)):
            assert size(*args, flags) == 0 == window_size(*args, flags), (args, flags)
    for npairs, slots1, slots2 in ((1, 1, 1), (3, 160, 192), (255, 3000, 3000), (65536, 8, 40), (2, 64, 33)):
        boxes = 16 * npairs * ((slots2 + 31) // 32)
        for flags in (0, 1, 2, 3):
            assert size(npairs, slots1, slots2, flags) == boxes == window_size(npairs, slots1, slots2, flags)
            assert size(npairs, 16 * slots1, slots2, flags) == boxes          # set 1 does not count
            assert size(npairs, slots1, slots2, flags | 4) == boxes + 8 * npairs * slots2   # MUTUAL: + the keys
            assert size(npairs, slots1, slots2, flags | 4) == window_size(npairs, slots1, slots2, flags | 4)
        assert size(npairs, slots1, slots2) == boxes                          # flags default to 0
    assert size(2 ** 20, 8, 2 ** 11, 4) >= 8 * 2 ** 31                        # no 32-bit wrap
    assert size(2 ** 20, 8, 2 ** 11, 4) == window_size(2 ** 20, 8, 2 ** 11, 4)


def test_the_old_calls_still_reject_what_they_rejected(surf):
    assert surf.lib.surfhip_match_batch(P, P, P, 64, P, P, P, 64, 1, 64, 4, None) == INVALID
    assert surf.lib.surfhip_match_batch_cross(P, P, P, 64, P, P, P, 64, 1, 64, 4, P, None) == INVALID
    assert surf.lib.surfhip_match_batch(P, P, P, 64, P, P, P, 64, 1, 64, 8, None) == INVALID
    assert surf.lib.surfhip_match_batch_cross(P, P, P, 64, P, P, P, 64, 1, 64, 8, P, None) == INVALID
    w = C.byref(surf.MatchWindow(-1.0, 1.0, -1.0, 1.0))
    assert surf.lib.surfhip_match_batch_window(P, P, P, 64, P, P, P, 64, 1, 64, 8, w, P, None) == INVALID
    assert surf.lib.surfhip_match_batch_window(P, P, P, 64, P, P, P, 64, 1, 64, 0, w, None, None) == INVALID
    assert surf.lib.surfhip_match_batch_guided(P, P, P, 64, P, P, P, 64, 1, 64, 0, P, 8, w, P, None) == INVALID
    assert surf.lib.surfhip_match_batch_guided(P, P, P, 64, P, P, P, 64, 1, 64, 0, None, 16, w, P, None) == INVALID
    assert surf.lib.surfhip_match_batch_guided(P, P, P, 64, P, P, P, 64, 0, 64, 0, None, 16, w, None, None) == OK
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 2, P, None) == INVALID
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 4, P, None) == INVALID


# ------------------------------------------------ the corner bound, in numpy

def test_the_corner_test_never_drops_an_offered_point():
    """Random lines (rectified, near-horizontal, steep, from camera poses, all
    zero) against random boxes: wherever the fp32 band test offers a point of
    the box, line_may_offer keeps the box; and it does drop boxes."""
    rng = np.random.default_rng(5)
    pt = np.dtype([("x", "<f4"), ("y", "<f4")])
    mats = [RECTIFIED, ZERO, translation_f(1.0, 0.0625), translation_f(0.0625, 1.0), translation_f(-1.0, 0.5),
            pose_f(rot(0.5, -3.0, 0.3), np.array([-0.8, 0.02, 0.05])),
            pose_f(rot(-1.5, 2.0, -2.5), np.array([0.25, -0.1, -0.75]))]
    dropped = offered = 0
    for k in range(400):
        f = mats[k % len(mats)]
        band = float(rng.choice([0.0, 0.5, 1.5, 6.0, 40.0]))
        p1 = np.zeros(16, pt)
        p1["x"], p1["y"] = rng.uniform(0, 1920, 16), rng.uniform(0, 1080, 16)
        a, b, c, lim = epipolar_lines(p1, f, band)
        x0, y0 = rng.uniform(0, 1900), rng.uniform(0, 1060)
        w, h = rng.choice([0.0, 3.0, 40.0, 1900.0]), rng.choice([0.0, 2.0, 30.0, 300.0])
        x2 = rng.uniform(x0, x0 + w, 64).astype(np.float32)
        y2 = rng.uniform(y0, y0 + h, 64).astype(np.float32)
        if k % 3 == 0:                                                # points exactly on a line of the set
            y2[:16] = (p1["y"] + np.float32(0.0625) * (x2[:16] - p1["x"])).astype(np.float32)
        bx = (x2.min(), x2.max(), y2.min(), y2.max())
        keep = line_may_offer(a, b, c, lim, bx)
        r = (x2[None, :] * a[:, None] + y2[None, :] * b[:, None]) + c[:, None]
        assert r.dtype == np.float32
        off = (r * r <= lim[:, None]).any(axis=1)
        assert (keep | ~off).all(), (k, f, band)
        dropped += int((~keep).sum())
        offered += int(off.sum())
    assert dropped >= 500 and offered >= 500


def test_the_corner_test_keeps_on_nan_and_on_the_zero_matrix():
    pt = np.dtype([("x", "<f4"), ("y", "<f4")])
    p1 = np.zeros(3, pt)
    p1["x"], p1["y"] = [10.0, NAN, 30.0], [5.0, 6.0, INF]
    bx = (np.float32(0), np.float32(100), np.float32(500), np.float32(600))
    keep = line_may_offer(*epipolar_lines(p1, RECTIFIED, 1.5), bx)
    # y1 = 5 +- 1.5 misses rows 500 .. 600; a NaN x1 and an infinite y1 (a = 0 * inf) give NaN lines, which keep
    assert [bool(k) for k in keep] == [False, True, True]
    assert line_may_offer(*epipolar_lines(p1[:1], ZERO, 1.5), bx).all()
    nan_f = RECTIFIED.copy()
    nan_f[0] = NAN
    assert line_may_offer(*epipolar_lines(p1[:1], nan_f, 1.5), bx).all()
    empty = (np.float32(INF), np.float32(-INF), np.float32(INF), np.float32(-INF))   # a tile of NaN points
    assert line_may_offer(*epipolar_lines(p1[:1], RECTIFIED, 1.5), empty).all()      # inf * 0: NaN keeps
