"""CPU tests of surfhip_match_batch's argument checks (no GPU call: every
case returns before a launch) and of its Python surface."""
from __future__ import annotations

import pytest

OK, INVALID = 0, -1
P = 0x1000          # a non-NULL pointer value; never dereferenced by a rejected call


def call(surf, pts1=P, desc1=P, counts1=P, slots1=64, pts2=P, desc2=P, counts2=P, slots2=64, npairs=1,
         nf=64, flags=0):
    return surf.lib.surfhip_match_batch(pts1, desc1, counts1, slots1, pts2, desc2, counts2, slots2, npairs, nf,
                                        flags, None)


def test_constants_and_binding(surf):
    assert surf.MATCH_FULL_TAIL == 1 and surf.MATCH_SAME_LAPLACE == 2
    assert callable(surf.match_batch)
    assert "surfhip_match_batch" in surf._sigs
    src = open(surf.REPO + "/include/surfhip.h").read()
    assert "#define SURFHIP_MATCH_SAME_LAPLACE 2" in src


@pytest.mark.parametrize("kw", [dict(npairs=-1), dict(slots1=0), dict(slots1=-4), dict(slots2=0), dict(slots2=-1),
                                dict(nf=0), dict(nf=2), dict(nf=66), dict(nf=1028), dict(nf=-64),
                                dict(flags=4), dict(flags=8 | 1), dict(flags=-1),
                                dict(pts1=None), dict(desc1=None), dict(counts1=None),
                                dict(pts2=None), dict(desc2=None), dict(counts2=None)])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(npairs=0, slots1=0), dict(npairs=0, nf=6), dict(npairs=0, flags=16)])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_zero_pairs_is_ok(surf, flags):
    assert call(surf, npairs=0, flags=flags) == OK
    assert call(surf, npairs=0, flags=flags, pts1=None, desc1=None, counts1=None, pts2=None, desc2=None,
                counts2=None) == OK
    surf.match_batch(None, None, None, 16, None, None, None, 16, 0, 128, flags)      # the wrapper: no raise


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.match_batch(P, P, P, 16, P, P, P, 16, -1, 64)


def test_single_pair_call_keeps_rejecting_the_laplace_flag(surf):
    assert surf.lib.surfhip_match(P, P, P, P, 4, 4, 64, surf.MATCH_SAME_LAPLACE, None, None) == INVALID
