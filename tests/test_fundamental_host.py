"""CPU tests of surfhip_fundamental_batch's argument checks (no GPU call:
every case returns before a launch), its struct layout and its Python
surface."""
from __future__ import annotations

import re
import subprocess

import pytest

OK, INVALID = 0, -1
P = 0x1000          # a non-NULL pointer value; never dereferenced by a rejected call
NAN, INF = float("nan"), float("inf")


def call(surf, pts=P, counts=P, slots=64, npairs=1, amb=0.95, thr=3.0, nhyp=256, seed=0, out=P, inlier=P):
    return surf.lib.surfhip_fundamental_batch(pts, counts, slots, npairs, amb, thr, nhyp, seed, out, inlier, None)


def test_struct_is_64_bytes_with_the_homography_offsets(surf):
    assert surf.FUNDAMENTAL_DTYPE.itemsize == 64
    assert surf.FUNDAMENTAL_DTYPE.names == ("f", "status", "ncand", "ninliers", "rms", "reserved")
    offsets = [surf.FUNDAMENTAL_DTYPE.fields[n][1] for n in surf.FUNDAMENTAL_DTYPE.names]
    assert offsets == [0, 36, 40, 44, 48, 52]
    assert offsets == [surf.HOMOGRAPHY_DTYPE.fields[n][1] for n in surf.HOMOGRAPHY_DTYPE.names]
    src = ('#include <stddef.h>\n#include "surfhip.h"\n'
           "_Static_assert(sizeof(surfhip_fundamental) == 64, \"size\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, f) == 0, \"f\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, status) == 36, \"status\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, ncand) == 40, \"ncand\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, ninliers) == 44, \"ninliers\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, rms) == 48, \"rms\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, reserved) == 52, \"reserved\");\n"
           "_Static_assert(offsetof(surfhip_fundamental, status) == offsetof(surfhip_homography, status), \"same\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", surf.REPO + "/include", "-x", "c", "-"], input=src,
                   text=True, check=True)


def test_constants_and_binding(surf):
    src = open(surf.REPO + "/include/surfhip.h").read()
    for name, value in (("OK", surf.FUND_OK), ("TOO_FEW", surf.FUND_TOO_FEW), ("DEGENERATE", surf.FUND_DEGENERATE)):
        m = re.search(rf"#define\s+SURFHIP_FUND_{name}\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert (surf.FUND_OK, surf.FUND_TOO_FEW, surf.FUND_DEGENERATE) == (0, 1, 2)
    assert callable(surf.fundamental_batch)
    assert "surfhip_fundamental_batch" in surf._sigs and "surfhip_fundamental_lds_capacity" in surf._sigs
    assert surf.FUNDAMENTAL_LDS_CAPACITY == surf.lib.surfhip_fundamental_lds_capacity() >= 2048


@pytest.mark.parametrize("kw", [dict(npairs=-1), dict(slots=0), dict(slots=-8),
                                dict(nhyp=0), dict(nhyp=-1), dict(nhyp=4097),
                                dict(thr=0.0), dict(thr=-3.0), dict(thr=NAN), dict(thr=INF), dict(thr=-INF),
                                dict(amb=0.0), dict(amb=-0.5), dict(amb=NAN), dict(amb=INF),
                                dict(pts=None), dict(counts=None), dict(out=None)])
def test_invalid_arguments(surf, kw):
    assert call(surf, **kw) == INVALID


@pytest.mark.parametrize("kw", [dict(slots=0), dict(nhyp=0), dict(nhyp=5000), dict(thr=NAN), dict(thr=0.0),
                                dict(amb=INF), dict(amb=-1.0)])
def test_invalid_scalars_are_rejected_for_zero_pairs_too(surf, kw):
    assert call(surf, npairs=0, **kw) == INVALID


@pytest.mark.parametrize("nhyp", [1, 1024, 4096])
def test_zero_pairs_is_ok(surf, nhyp):
    assert call(surf, npairs=0, nhyp=nhyp) == OK
    assert call(surf, npairs=0, nhyp=nhyp, pts=None, counts=None, out=None, inlier=None) == OK
    surf.fundamental_batch(None, None, 16, 0, None, None, nhyp=nhyp)          # the wrapper: no raise


def test_wrapper_raises_on_invalid(surf):
    with pytest.raises(surf.SurfError):
        surf.fundamental_batch(P, P, 16, -1, P)
    with pytest.raises(surf.SurfError):
        surf.fundamental_batch(P, P, 16, 0, P, inlier_thresh=0.0)
    with pytest.raises(surf.SurfError):
        surf.fundamental_batch(None, P, 16, 1, P)
