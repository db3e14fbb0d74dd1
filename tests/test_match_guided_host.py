"""CPU tests of surfhip_match_batch_guided's argument checks and scratch size
(no GPU call: every case returns before a launch) and of its Python
surface."""
from __future__ import annotations

import ctypes as C
import math

import pytest

OK, INVALID = 0, -1
P = 0x1000          # a non-NULL, 16-B aligned pointer value; never dereferenced by a rejected call
INF, NAN = math.inf, math.nan
DEFAULT = object()


def call(surf, pts1=P, desc1=P, counts1=P, slots1=64, pts2=P, desc2=P, counts2=P, slots2=64, npairs=1,
         nf=64, flags=0, h=P, h_stride=16, window=DEFAULT, scratch=P):
    if window is DEFAULT:
        window = (-32.0, 32.0, -32.0, 32.0)
    w = None if window is None else C.byref(surf.MatchWindow(*window))
    return surf.lib.surfhip_match_batch_guided(pts1, desc1, counts1, slots1, pts2, desc2, counts2, slots2, npairs,
                                               nf, flags, h, h_stride, w, scratch, None)


def test_constants_and_binding(surf):
    assert surf.MATCH_FULL_TAIL == 1 and surf.MATCH_SAME_LAPLACE == 2 and surf.MATCH_MUTUAL == 4
    assert callable(surf.match_batch_guided) and callable(surf.match_batch_guided_scratch_bytes)
    assert "surfhip_match_batch_guided" in surf._sigs and "surfhip_match_batch_guided_scratch" in surf._sigs
    assert len(surf._sigs["surfhip_match_batch_guided"][1]) == 16
    src = open(surf.REPO + "/include/surfhip.h").read()
    assert "int surfhip_match_batch_guided(" in src and "size_t surfhip_match_batch_guided_scratch(" in src
    assert "const float* d_h, int h_stride," in src
    text = " ".join(src.replace("\n *", " ").split())             # the comment as running text
    for words in ("that of surfhip_match_batch_window with the same window and flags",
                  "that of surfhip_match_batch / surfhip_match_batch_cross, for points with W > 0"):
        assert words in text, words
    # h_stride 16: the matrix is the first member of the 64-B record
    assert surf.HOMOGRAPHY_DTYPE.itemsize == 64 and surf.HOMOGRAPHY_DTYPE.fields["h"][1] == 0


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
                                dict(h_stride=-1), dict(h_stride=1), dict(h_stride=8), dict(h_stride=-16),
                                dict(h=None), dict(h=P + 2), dict(h=None, h_stride=0), dict(h=P + 2, h_stride=9)])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(slots1=0), dict(nf=6), dict(flags=16), dict(flags=8), dict(window=None),
                                dict(window=(NAN, 1.0, -1.0, 1.0)), dict(window=(2.0, 1.0, -1.0, 1.0)),
                                dict(h_stride=-1), dict(h_stride=1), dict(h_stride=8), dict(h_stride=-16)])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, npairs=0, **kw) == INVALID
    assert call(surf, npairs=0, h=None, **kw) == INVALID


@pytest.mark.parametrize("h_stride", [0, 9, 16, 1000])
def test_valid_strides(surf, h_stride):
    """Accepted (zero pairs: the call returns before it would touch the GPU)
    where the neighbouring values are rejected."""
    assert call(surf, npairs=0, h_stride=h_stride) == OK
    assert call(surf, npairs=0, h_stride=h_stride, h=None) == OK
    assert call(surf, npairs=0, h_stride=h_stride, h=P + 2) == OK     # d_h is checked with npairs > 0 only
    # with a pair, the stride passes the scalar checks: the call is then rejected for its NULL d_pts1 alone
    assert call(surf, h_stride=h_stride, pts1=None) == INVALID


@pytest.mark.parametrize("flags", range(8))
def test_zero_pairs_is_ok(surf, flags):
    assert call(surf, npairs=0, flags=flags) == OK
    assert call(surf, npairs=0, flags=flags, pts1=None, desc1=None, counts1=None, pts2=None, desc2=None,
                counts2=None, h=None, scratch=None) == OK
    surf.match_batch_guided(None, None, None, 16, None, None, None, 16, 0, 128, flags, None, 16, (-1, 1, -2, 2), None)
    surf.match_batch_guided(None, None, None, 16, None, None, None, 16, 0, 128, flags, None, 0,
                            surf.MatchWindow(-INF, INF, -INF, INF), None)


@pytest.mark.parametrize("window", [(-INF, INF, -INF, INF), (0.0, 0.0, 0.0, 0.0), (-64.0, 0.0, -1.5, 1.5),
                                    (-INF, -INF, INF, INF), (5.0, INF, -INF, -5.0)])
def test_infinite_and_degenerate_windows_are_valid(surf, window):
    assert call(surf, npairs=0, window=window) == OK


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.match_batch_guided(P, P, P, 16, P, P, P, 16, 1, 64, 0, P, 16, (-1, 1, -1, 1), None)
    with pytest.raises(surf.SurfError):
        surf.match_batch_guided(P, P, P, 16, P, P, P, 16, 1, 64, 0, None, 16, (-1, 1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_guided(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 8, (-1, 1, -1, 1), P)
    with pytest.raises(surf.SurfError):
        surf.match_batch_guided(P, P, P, 16, P, P, P, 16, 0, 64, 0, P, 16, (1, -1, -1, 1), P)


def test_scratch_size(surf):
    size, window_size = surf.match_batch_guided_scratch_bytes, surf.match_batch_window_scratch_bytes
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
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 2, P, None) == INVALID
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 4, P, None) == INVALID
