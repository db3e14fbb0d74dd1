"""`select_strongest`, the host restatement of SURFHIP_KEEP_STRONGEST's rule, on hand-made arrays
(no GPU): strengths ordered by the order-preserving map of their IEEE bits, the earlier point on ties,
the kept indices ascending."""
from __future__ import annotations

import numpy as np
import pytest


def points(surf, strengths):
    pts = np.zeros(len(strengths), surf.POINT_DTYPE)
    pts["strength"] = np.asarray(strengths, np.float32)
    pts["x"] = np.arange(len(strengths))
    return pts


def test_constants_and_binding(surf):
    assert surf.KEEP_FIRST == 0 and surf.KEEP_STRONGEST == 1
    assert callable(surf.Detector.set_keep) and callable(surf.Detector.keep)
    for name in ("surfhip_detector_set_keep", "surfhip_detector_get_keep"):
        getattr(surf.lib, name)
    hdr = open(surf.REPO + "/include/surfhip.h").read()
    assert "#define SURFHIP_KEEP_FIRST     0" in hdr and "#define SURFHIP_KEEP_STRONGEST 1" in hdr


def test_null_detector_is_invalid(surf):
    import ctypes as C
    m, n = C.c_int(), C.c_int()
    assert surf.lib.surfhip_detector_set_keep(None, surf.KEEP_STRONGEST, 4) == -1
    assert surf.lib.surfhip_detector_get_keep(None, C.byref(m), C.byref(n)) == -1


def test_distinct_strengths(surf):
    pts = points(surf, [5.0, 9.0, 1.0, 7.0, 3.0, 8.0])
    assert surf.select_strongest(pts, 3).tolist() == [1, 3, 5]
    assert surf.select_strongest(pts, 4).tolist() == [0, 1, 3, 5]


def test_equal_strengths_across_the_cut(surf):
    pts = points(surf, [6.0, 4.0, 9.0, 4.0, 4.0, 4.0, 2.0])
    assert surf.select_strongest(pts, 4).tolist() == [0, 1, 2, 3]     # of the four 4.0s the two earliest
    assert surf.select_strongest(pts, 3).tolist() == [0, 1, 2]
    assert surf.select_strongest(pts, 5).tolist() == [0, 1, 2, 3, 4]


def test_negative_strengths(surf):
    pts = points(surf, [-3.0, -1.0, -2.0, 0.5, -0.25])
    assert surf.select_strongest(pts, 1).tolist() == [3]
    assert surf.select_strongest(pts, 2).tolist() == [3, 4]
    assert surf.select_strongest(pts, 4).tolist() == [1, 2, 3, 4]     # -1 and -2 beat -3


def test_negative_zero_is_below_positive_zero(surf):
    pts = points(surf, [-0.0, 0.0, -0.0, 0.0])
    assert np.signbit(pts["strength"]).tolist() == [True, False, True, False]
    assert surf.select_strongest(pts, 2).tolist() == [1, 3]
    assert surf.select_strongest(pts, 3).tolist() == [0, 1, 3]


def test_nan_has_a_defined_place(surf):
    """A NaN sorts by its bits: the positive quiet NaN above +inf, the one with the sign bit set below -inf."""
    pos = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    neg = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    pts = points(surf, [np.inf, pos, 1.0, neg, -np.inf])
    assert pts["strength"].view(np.uint32)[[1, 3]].tolist() == [0x7FC00000, 0xFFC00000]
    assert surf.select_strongest(pts, 1).tolist() == [1]
    assert surf.select_strongest(pts, 2).tolist() == [0, 1]
    assert surf.select_strongest(pts, 4).tolist() == [0, 1, 2, 4]
    assert surf.select_strongest(pts, 4).tolist() == surf.select_strongest(pts, 4).tolist()


def test_n_at_least_len_keeps_all(surf):
    pts = points(surf, [2.0, 1.0, 3.0])
    assert surf.select_strongest(pts, 3).tolist() == [0, 1, 2]
    assert surf.select_strongest(pts, 100).tolist() == [0, 1, 2]


def test_n_one(surf):
    pts = points(surf, [2.0, 7.0, 7.0, 3.0])
    assert surf.select_strongest(pts, 1).tolist() == [1]
    with pytest.raises(ValueError):
        surf.select_strongest(pts, 0)


def test_empty_array(surf):
    got = surf.select_strongest(np.zeros(0, surf.POINT_DTYPE), 5)
    assert got.shape == (0,) and got.dtype.kind == "i"


def test_result_is_ascending_and_matches_a_plain_restatement(surf):
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 500, dtype=np.uint64).astype(np.uint32)
    bits[::7] = bits[3]                                                 # ties
    pts = points(surf, np.zeros(500))
    pts["strength"] = bits.view(np.float32)
    assert pts["strength"].view(np.uint32).tolist() == bits.tolist()
    m = [int(u) ^ (0xFFFFFFFF if int(u) >> 31 else 0x80000000) for u in bits]
    for n in (1, 37, 250, 499):
        got = surf.select_strongest(pts, n)
        assert (np.diff(got) > 0).all() and len(got) == n
        want = sorted(sorted(range(500), key=lambda i: (-m[i], i))[:n])
        assert got.tolist() == want
