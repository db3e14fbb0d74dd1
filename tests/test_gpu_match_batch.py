"""GPU tests of surfhip_match_batch (batched matching on the f32 matrix
instruction): every comparison is bitwise on the five match fields against
the CPU oracle's or_match run per pair on the host copies."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from match_ref import (CANARY, COUNTS1, COUNTS2, FULL_TAIL, KEPT_FIELDS, MATCH_FIELDS, SAME_LAPLACE, assert_match_equal,
                       make_points, ragged_data, run_batch, with_canary)

pytestmark = pytest.mark.gpu


def check_batch(surf, orc, p1, f1, c1, p2, f2, c2, flags, got=None, ref_fn=None):
    """One batch call against the oracle per pair + the nothing-else-written
    properties (canary past the counts, detect fields, descriptors)."""
    if got is None:
        got, d1, d2 = run_batch(surf, p1, f1, c1, p2, f2, c2, flags)
        assert d1.tobytes() == f1.tobytes() and d2.tobytes() == f2.tobytes()
    s1, s2 = p1.shape[1], p2.shape[1]
    for i in range(len(p1)):
        n1, n2 = min(max(int(c1[i]), 0), s1), min(max(int(c2[i]), 0), s2)
        if ref_fn is None:
            ref = orc.match(p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2], full_tail=bool(flags & FULL_TAIL))
        else:
            ref = ref_fn(i, n1, n2)
        assert_match_equal(got[i, :n1], ref, f"pair {i} (n1 {n1}, n2 {n2}): ")
        for f in MATCH_FIELDS:                                    # slots at or past n1: untouched
            assert (got[i, n1:][f].view(np.uint32) == p1[i, n1:][f].view(np.uint32)).all(), (i, f)
        for f in KEPT_FIELDS:
            assert (got[i][f].view(np.uint32) == p1[i][f].view(np.uint32)).all(), (i, f)
    return got


@functools.lru_cache(maxsize=None)
def ragged_result(surf, orc, nf, flags):
    p1, f1, p2, f2 = ragged_data(surf, nf)
    got = check_batch(surf, orc, p1, f1, COUNTS1, p2, f2, COUNTS2, flags)
    got.setflags(write=False)
    return got


def test_operand_map_exact_integers(surf, orc):
    """One-hot set-1 rows pick single elements of an asymmetric integer set
    2: a swapped operand, row/column or k order changes the scores."""
    n, nf = 96, 64
    f1 = np.zeros((1, n, nf), np.float32)
    f1[0, np.arange(n), (5 * np.arange(n)) % nf] = 1.0
    p2i, d = np.meshgrid(np.arange(n), np.arange(nf), indexing="ij")
    f2 = (1 + ((7 * p2i + 3 * d) % 251)).astype(np.float32)[None]
    rng = np.random.default_rng(1)
    p1 = with_canary(make_points(rng, 1, n, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n, surf.POINT_DTYPE)
    got = check_batch(surf, orc, p1, f1, [n], p2, f2, [n], 0)
    want = f2[0][:, (5 * np.arange(n)) % nf].max(axis=0)          # the best score is one element of f2, exactly
    np.testing.assert_array_equal(got[0]["score"], want)


@pytest.mark.parametrize("flags", [0, FULL_TAIL])
@pytest.mark.parametrize("nf", [64, 128, 36, 392])
def test_ragged_batch(surf, orc, nf, flags):
    ragged_result(surf, orc, nf, flags)


@pytest.mark.parametrize("flags", [0, FULL_TAIL])
def test_ties_and_sign(surf, orc, flags):
    nf, s1, s2 = 64, 64, 96
    rng = np.random.default_rng(33)
    f1 = np.abs(rng.standard_normal((3, s1, nf))).astype(np.float32)
    f2 = np.abs(rng.standard_normal((3, s2, nf))).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    # pair 0: one descriptor at two positions of thread row 1 in tiles 0 and 1
    # (the earlier index wins inside the row), another in rows 2 and 4 (the
    # row merge keeps the lower row's index and takes the equal score as second)
    f2[0, 5] = f2[0, 37] = f1[0, 3]
    f2[0, 10] = f2[0, 50] = f1[0, 7]
    # pair 1: every score negative
    perm = rng.permutation(s1)
    f2[1, :s1] = -f1[1, perm]
    c1, c2 = [40, s1, 50], [s2, s1, 31]
    p1 = with_canary(make_points(rng, 3, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, s2, surf.POINT_DTYPE)
    got = check_batch(surf, orc, p1, f1, c1, p2, f2, c2, flags)
    assert got[0, 3]["match"] == 5 and got[0, 7]["match"] == 10
    assert got[0, 7]["ambiguity"] > 0.99                          # the twin in row 4 is the second
    empty = [got[1, :s1]] + ([got[2, :50]] if not flags else [])  # n2 = 31: nothing scanned without FULL_TAIL
    for g in empty:
        assert (g["match"] == -1).all() and (g["score"] == 0).all()
        assert (g["match_x"] == 0).all() and (g["match_y"] == 0).all() and (g["ambiguity"] == 0).all()
    if flags:
        assert (got[2, :50]["match"] >= 0).all()


def test_counts_are_clamped(surf, orc):
    nf, s1, s2 = 64, 70, 100
    rng = np.random.default_rng(44)
    f1 = rng.standard_normal((3, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((3, s2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 3, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, s2, surf.POINT_DTYPE)
    got = check_batch(surf, orc, p1, f1, [s1 + 5, 40, -3], p2, f2, [s2 + 5, -3, 64], FULL_TAIL)
    assert (got[0]["match"] >= 0).all()                           # all 70 slots matched against all 100
    assert (got[1, :40]["match"] == -1).all()                     # n2 = 0
    assert (got[2]["match"] == CANARY["match"]).all()             # n1 = 0: nothing written


@pytest.mark.parametrize("flags", [0, FULL_TAIL])
def test_same_result_as_per_pair_call(surf, orc, flags):
    p1, f1, p2, f2 = ragged_data(surf, 64)
    batch = ragged_result(surf, orc, 64, flags)
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        if n1 == 0:
            continue
        bufs = []
        for a in (p1[i, :n1], p2[i, :max(n2, 1)], f1[i, :n1], f2[i, :max(n2, 1)]):
            b = surf.DeviceBuffer(a.nbytes)
            b.upload(a)
            bufs.append(b)
        surf.match_points(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n1, n2, 64, flags)
        surf.synchronize()
        single = bufs[0].download(surf.POINT_DTYPE, n1)
        assert_match_equal(batch[i, :n1], single, f"pair {i}: ")
        for b in bufs:
            b.free()


@pytest.mark.parametrize("flags", [SAME_LAPLACE, SAME_LAPLACE | FULL_TAIL])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_same_laplace_flag(surf, orc, nf, flags):
    """A set-2 point of the other sign is not offered to the scan: the same
    as scoring a zero row in its place (+-0 never passes the strict '>'
    against a state >= 0), which the oracle can do."""
    p1, f1, p2, f2 = ragged_data(surf, nf)
    assert set(np.unique(p1["laplace"])) == {-1, 1} and set(np.unique(p2["laplace"])) == {-1, 1}

    def ref_fn(i, n1, n2):
        ref = p1[i, :n1].copy()
        for v in (-1, 1):
            fz = f2[i, :n2].copy()
            fz[p2[i, :n2]["laplace"] != v] = 0.0
            r = orc.match(p1[i, :n1], p2[i, :n2], f1[i, :n1], fz, full_tail=bool(flags & FULL_TAIL))
            rows = p1[i, :n1]["laplace"] == v
            ref[rows] = r[rows]
        return ref

    got = check_batch(surf, orc, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, ref_fn=ref_fn)
    plain = ragged_result(surf, orc, nf, flags & FULL_TAIL)
    assert any((got[i, :n]["match"] != plain[i, :n]["match"]).any() for i, n in enumerate(COUNTS1))
    for i, n1 in enumerate(COUNTS1):                               # every match has the point's own sign
        m = got[i, :n1]["match"]
        ok = m >= 0
        assert (p2[i]["laplace"][m[ok]] == p1[i, :n1]["laplace"][ok]).all()


def test_detect_then_match_without_host_round_trip(surf, orc):
    """detect_batch, then match_batch of consecutive frames on the detector's
    own output buffers and device counts (set 2 = set 1 advanced one frame),
    enqueued without reading anything back in between."""
    n, w, h, max_pts = 4, 640, 480, 1024
    frames = surf.synth_frames(n, w, h)
    pitch = frames.shape[2]
    param = surf.make_param(4, 4.0, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    det = surf.Detector(param, w, h, max_batch=n, max_pts=max_pts)
    fb = surf.DeviceBuffer(frames.nbytes)
    fb.upload(frames)
    pb = surf.DeviceBuffer(48 * n * max_pts)
    db = surf.DeviceBuffer(4 * n * max_pts * nf)
    cb = surf.DeviceBuffer(4 * n)
    pb.zero()
    for flags in (0, FULL_TAIL):
        det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
        surf.match_batch(pb.ptr, db.ptr, cb.ptr, max_pts, pb.ptr + 48 * max_pts, db.ptr + 4 * max_pts * nf,
                         cb.ptr + 4, max_pts, n - 1, nf, flags)
        surf.synchronize()
        counts = cb.download(np.int32, n)
        assert counts.min() >= 64 and counts.max() <= max_pts and (counts % 32 != 0).all()
        pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
        desc = db.download(np.float32, n * max_pts * nf).reshape(n, max_pts, nf)
        for i in range(n - 1):
            a, b = counts[i], counts[i + 1]
            ref = orc.match(pts[i, :a], pts[i + 1, :b], desc[i, :a], desc[i + 1, :b], full_tail=bool(flags))
            assert_match_equal(pts[i, :a], ref, f"flags {flags} pair {i}: ")
            assert (ref["match"] >= 0).mean() > 0.5
    det.close()
