"""CPU tests of surfhip_match_batch_cross's argument checks and scratch size
(no GPU call: every case returns before a launch) and of its Python
surface."""
from __future__ import annotations

import pytest

OK, INVALID = 0, -1
P = 0x1000          # a non-NULL, 16-B aligned pointer value; never dereferenced by a rejected call


def call(surf, pts1=P, desc1=P, counts1=P, slots1=64, pts2=P, desc2=P, counts2=P, slots2=64, npairs=1,
         nf=64, flags=0, scratch=P):
    return surf.lib.surfhip_match_batch_cross(pts1, desc1, counts1, slots1, pts2, desc2, counts2, slots2, npairs,
                                              nf, flags, scratch, None)


def test_constants_and_binding(surf):
    assert callable(surf.match_batch_cross) and callable(surf.match_batch_cross_scratch_bytes)
    assert "surfhip_match_batch_cross" in surf._sigs and "surfhip_match_batch_cross_scratch" in surf._sigs
    src = open(surf.REPO + "/include/surfhip.h").read()
    assert "int surfhip_match_batch_cross(" in src and "size_t surfhip_match_batch_cross_scratch(" in src


@pytest.mark.parametrize("kw", [dict(npairs=-1), dict(slots1=0), dict(slots1=-4), dict(slots2=0), dict(slots2=-1),
                                dict(nf=0), dict(nf=2), dict(nf=66), dict(nf=1028), dict(nf=-64),
                                dict(flags=4), dict(flags=8 | 1), dict(flags=-1),
                                dict(pts1=None), dict(desc1=None), dict(counts1=None),
                                dict(pts2=None), dict(desc2=None), dict(counts2=None),
                                dict(scratch=None), dict(scratch=P + 8)])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(npairs=0, slots1=0), dict(npairs=0, nf=6), dict(npairs=0, flags=16),
                                dict(npairs=0, flags=4)])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_zero_pairs_is_ok(surf, flags):
    assert call(surf, npairs=0, flags=flags) == OK
    assert call(surf, npairs=0, flags=flags, pts1=None, desc1=None, counts1=None, pts2=None, desc2=None,
                counts2=None, scratch=None) == OK
    surf.match_batch_cross(None, None, None, 16, None, None, None, 16, 0, 128, None, flags)   # the wrapper: no raise


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.match_batch_cross(P, P, P, 16, P, P, P, 16, 1, 64, None)


def test_scratch_size(surf):
    size = surf.match_batch_cross_scratch_bytes
    for args in ((0, 64, 64), (-1, 64, 64), (3, 64, 0), (3, 64, -5), (3, 0, 64)):
        assert size(*args) == 0, args
    for npairs, slots1, slots2 in ((1, 1, 1), (3, 160, 192), (255, 3000, 3000), (65536, 8, 40)):
        n = size(npairs, slots1, slots2)
        assert 8 * npairs * slots2 <= n <= 8 * npairs * slots2 + 256, (npairs, slots1, slots2, n)
        assert size(npairs, 16 * slots1, slots2) <= n           # one word per set-2 slot: set 1 does not count
    assert size(2 ** 20, 8, 2 ** 11) >= 8 * 2 ** 31             # no 32-bit wrap


def test_the_old_call_still_rejects_new_flag_bits(surf):
    assert surf.lib.surfhip_match_batch(P, P, P, 64, P, P, P, 64, 1, 64, 4, None) == INVALID
