"""CPU tests of surfhip_match_batch_window's argument checks and scratch size
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
         nf=64, flags=0, window=DEFAULT, scratch=P):
    if window is DEFAULT:
        window = (-32.0, 32.0, -32.0, 32.0)
    w = None if window is None else C.byref(surf.MatchWindow(*window))
    return surf.lib.surfhip_match_batch_window(pts1, desc1, counts1, slots1, pts2, desc2, counts2, slots2, npairs,
                                               nf, flags, w, scratch, None)


def test_constants_and_binding(surf):
    assert surf.MATCH_FULL_TAIL == 1 and surf.MATCH_SAME_LAPLACE == 2 and surf.MATCH_MUTUAL == 4
    assert callable(surf.match_batch_window) and callable(surf.match_batch_window_scratch_bytes)
    assert "surfhip_match_batch_window" in surf._sigs and "surfhip_match_batch_window_scratch" in surf._sigs
    assert C.sizeof(surf.MatchWindow) == 16
    assert [f[0] for f in surf.MatchWindow._fields_] == ["dx_min", "dx_max", "dy_min", "dy_max"]
    src = open(surf.REPO + "/include/surfhip.h").read()
    assert "int surfhip_match_batch_window(" in src and "size_t surfhip_match_batch_window_scratch(" in src
    assert "#define SURFHIP_MATCH_MUTUAL 4" in src
    assert "typedef struct surfhip_match_window { float dx_min, dx_max, dy_min, dy_max; } surfhip_match_window;" in src


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
                                dict(window=(INF, -INF, -1.0, 1.0)), dict(window=(-1.0, 1.0, INF, -INF))])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(slots1=0), dict(nf=6), dict(flags=16), dict(flags=8), dict(window=None),
                                dict(window=(NAN, 1.0, -1.0, 1.0)), dict(window=(2.0, 1.0, -1.0, 1.0))])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, npairs=0, **kw) == INVALID


@pytest.mark.parametrize("flags", range(8))
def test_zero_pairs_is_ok(surf, flags):
    assert call(surf, npairs=0, flags=flags) == OK
    assert call(surf, npairs=0, flags=flags, pts1=None, desc1=None, counts1=None, pts2=None, desc2=None,
                counts2=None, scratch=None) == OK
    surf.match_batch_window(None, None, None, 16, None, None, None, 16, 0, 128, flags, (-1, 1, -2, 2), None)
    surf.match_batch_window(None, None, None, 16, None, None, None, 16, 0, 128, flags,
                            surf.MatchWindow(-INF, INF, -INF, INF), None)


@pytest.mark.parametrize("window", [(-INF, INF, -INF, INF), (0.0, 0.0, 0.0, 0.0), (-64.0, 0.0, -1.5, 1.5),
                                    (-INF, -INF, INF, INF), (5.0, INF, -INF, -5.0)])
def test_infinite_and_degenerate_windows_are_valid(surf, window):
    assert call(surf, npairs=0, window=window) == OK


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.match_batch_window(P, P, P, 16, P, P, P, 16, 1, 64, 0, (-1, 1, -1, 1), None)
    with pytest.raises(surf.SurfError):
        surf.match_batch_window(P, P, P, 16, P, P, P, 16, 0, 64, 0, (1, -1, -1, 1), P)


def test_scratch_size(surf):
    size = surf.match_batch_window_scratch_bytes
    for flags in (0, 4, 7):
        for args in ((0, 64, 64), (-1, 64, 64), (3, 64, 0), (3, 64, -5), (3, 0, 64), (3, -1, 64)):
            assert size(*args, flags) == 0, (args, flags)
    for npairs, slots1, slots2 in ((1, 1, 1), (3, 160, 192), (255, 3000, 3000), (65536, 8, 40), (2, 64, 33)):
        boxes = 16 * npairs * ((slots2 + 31) // 32)
        for flags in (0, 1, 2, 3):
            assert size(npairs, slots1, slots2, flags) == boxes, (npairs, slots1, slots2, flags)
            assert size(npairs, 16 * slots1, slots2, flags) == boxes          # set 1 does not count
            assert size(npairs, slots1, slots2, flags | 4) == boxes + 8 * npairs * slots2   # MUTUAL: + the keys
        assert size(npairs, slots1, slots2) == boxes                          # flags default to 0
    assert size(2 ** 20, 8, 2 ** 11, 4) >= 8 * 2 ** 31                        # no 32-bit wrap


def test_the_old_calls_still_reject_the_new_flag_bit(surf):
    assert surf.lib.surfhip_match_batch(P, P, P, 64, P, P, P, 64, 1, 64, 4, None) == INVALID
    assert surf.lib.surfhip_match_batch_cross(P, P, P, 64, P, P, P, 64, 1, 64, 4, P, None) == INVALID
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 2, P, None) == INVALID
    assert surf.lib.surfhip_match(P, P, P, P, 64, 64, 64, 4, P, None) == INVALID
