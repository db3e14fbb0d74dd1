"""GPU tests of surfhip_match_batch_epipolar (batched matching inside a window
around each set-1 point and a band along its epipolar line under a per-pair
fundamental matrix): every comparison is bitwise on the five match fields.

The model needs no new oracle.  The offered mask is computed in numpy float32
with exactly the kernel's operations (epipolar_ref.epipolar_mask); the forward
match per group of equal mask rows and the MUTUAL clearing rest on or_match
alone, through match_ref.  Only the five match fields are compared with that
model; everything else is compared with the original upload."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from epipolar_ref import (RECTIFIED, ZERO, epipolar_census, epipolar_lines, epipolar_mask, epipolar_model,
                          line_may_offer, mask_forward, pack_f, pose_f, rot, run_epipolar, translation_f)
from match_ref import (CANARY, COUNTS1, COUNTS2, EVERYWHERE, FULL_TAIL, INF, KEPT_FIELDS, MATCH_FIELDS, MUTUAL,
                       SAME_LAPLACE, SYMMETRIC, assert_match_equal, box, clamp, make_points, matrices, may_offer,
                       ragged_matrices, run_window, score_column, small_batch, window_data, with_canary)

pytestmark = pytest.mark.gpu

BAND = 1.5                                                            # |d| <= 1.5 <=> d d <= 2.25 in fp32
WINDOW_SETS = {"symmetric": SYMMETRIC, "everywhere": EVERYWHERE}


def check_epipolar(orc, got, p1, f1, c1, p2, f2, c2, flags, win, mats, fs, bands, knowns=None):
    """got against the model per pair (fs[i], bands[i]: the pair's matrix and
    band) + the nothing-else-written properties against the upload.  Returns
    the per-pair (expected, forward, offered mask)."""
    s1, s2 = p1.shape[1], p2.shape[1]
    refs = []
    for i in range(len(p1)):
        n1, n2 = clamp(c1[i], s1), clamp(c2[i], s2)
        ref, fwd, m = epipolar_model(orc, mats[i], p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2], flags, win,
                                     fs[i], bands[i], knowns[i] if knowns is not None else None)
        assert_match_equal(got[i, :n1], ref, f"flags {flags} window {win} pair {i} (n1 {n1}, n2 {n2}): ")
        for f in MATCH_FIELDS:                                    # slots at or past n1: untouched
            assert (got[i, n1:][f].view(np.uint32) == p1[i, n1:][f].view(np.uint32)).all(), (i, f)
        for f in KEPT_FIELDS:
            assert (got[i][f].view(np.uint32) == p1[i][f].view(np.uint32)).all(), (i, f)
        refs.append((ref, fwd, m))
    return refs


def assert_nothing(g):
    assert (g["match"] == -1).all()
    for f in ("score", "match_x", "match_y", "ambiguity"):
        assert (g[f].view(np.uint32) == 0).all(), f


# ------------------------------------------------- 1. the all-zero matrix

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["symmetric", "everywhere"])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_zero_matrix_is_the_window_call(surf, nf, name, flags):
    """What a failed fundamental record holds: the band test passes everywhere
    (0 <= 0) and the call writes the bytes of match_batch_window, GPU to GPU,
    plain and with MUTUAL, at f_stride 0 and inside junk-filled records."""
    win = WINDOW_SETS[name]
    p1, f1, p2, f2 = window_data(surf, nf)
    for fl in (flags, flags | MUTUAL):
        want = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, win)
        for stride in (0, 16):
            fbuf = pack_f([ZERO] * (1 if stride == 0 else len(p1)), stride)
            got = run_epipolar(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, win, fbuf, stride, BAND)
            assert got.tobytes() == want.tobytes(), (fl, stride)


# ------------------------------------------------ 2. the rectified matrix

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["symmetric", "everywhere"])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_rectified_matrix_is_a_window_of_rows(surf, nf, name, flags):
    """r = -(y2 - y1) exactly: band 1.5 with the window open in y writes the
    bytes of match_batch_window with (dx_min, dx_max, -1.5, 1.5).  (y lies on
    a half-pixel grid: points sit on the band's edge.)"""
    dx_min, dx_max = WINDOW_SETS[name][:2]
    p1, f1, p2, f2 = window_data(surf, nf)
    on_edge = sum(int((np.abs(p2["y"][i, None, :COUNTS2[i]] - p1["y"][i, :COUNTS1[i], None]) == 1.5).sum())
                  for i in range(len(p1)))
    assert on_edge >= 10
    for fl in (flags, flags | MUTUAL):
        want = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, (dx_min, dx_max, -BAND, BAND))
        for stride in (0, 16):
            fbuf = pack_f([RECTIFIED] * (1 if stride == 0 else len(p1)), stride)
            got = run_epipolar(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, (dx_min, dx_max, -INF, INF), fbuf, stride,
                               BAND)
            assert got.tobytes() == want.tobytes(), (fl, stride)
        if fl == 0 and name == "everywhere":
            assert (want["match"][np.array(COUNTS1) > 100] >= 0).sum() >= 8      # ... and it does match


# ------------------------------------------- 3. ragged batch, a matrix per pair

STEEP = translation_f(0.0625, 1.0)                                    # x2 - x1 = (y2 - y1) / 16: near-vertical lines
POSES = pose_f(rot(0.5, -3.0, 0.3), np.array([-0.8, 0.02, 0.05]))      # a verged stereo rig, norm 1
KINDS = (RECTIFIED, POSES, STEEP, ZERO)
KIND_BANDS = (6.0, 30.0, 4.0, 2.0)                                    # (the zero matrix ignores its band)
RAGGED_F = [KINDS[i % 4] for i in range(len(COUNTS1))]
RAGGED_BAND = [KIND_BANDS[i % 4] for i in range(len(COUNTS1))]


@functools.lru_cache(maxsize=None)
def ragged_forwards(surf, orc, nf, flags):
    """Per pair of window_data: (forward points, offered mask) inside SYMMETRIC
    and the pair's band."""
    p1, f1, p2, f2 = window_data(surf, nf)
    return [mask_forward(orc, p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2], flags,
                         epipolar_mask(p1[i, :n1], p2[i, :n2], flags, SYMMETRIC, RAGGED_F[i], RAGGED_BAND[i]))
            for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2))]


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_ragged_batch_with_a_matrix_per_pair(surf, orc, nf, flags):
    """The ragged batch (empty sets, partial tiles, dead waves, two blocks,
    the any-length kernel) with the rectified matrix, one from two camera
    poses, one with steep lines and the zero matrix cycling over the pairs, at
    strides 9, 16 and 20, plain and with MUTUAL.  Every kind has its own band
    and a call has one: the batch runs once per band value, and a pair is
    compared in the run that had its kind's band."""
    p1, f1, p2, f2 = window_data(surf, nf)
    mats = ragged_matrices(surf, orc, nf)
    fwds = ragged_forwards(surf, orc, nf, flags)
    dropped = partial = matches = not_next = 0
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        fwd, m = fwds[i]
        nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
        if n1 and nscan:                                          # both offered and not-offered columns
            assert m[:, :nscan].any() and not m[:, :nscan].all(), i
        for group in (128, 32):
            total, kept, part = epipolar_census(p1[i, :n1], p2[i, :n2], flags, SYMMETRIC, RAGGED_F[i],
                                                RAGGED_BAND[i], m, group)
            dropped += total - kept
            partial += part
        rows = np.nonzero(fwd["match"] >= 0)[0]
        cols = fwd["match"][rows]
        matches += len(rows)
        j = (i + 1) % len(COUNTS1)
        nxt = epipolar_mask(p1[i, :n1], p2[i, :n2], flags, SYMMETRIC, RAGGED_F[j], RAGGED_BAND[i])
        not_next += int((~nxt[rows, cols]).sum())
    print(f"nf {nf} flags {flags}: dropped (group, tile) {dropped}, partly offered {partial}, matches {matches}, "
          f"outside the next pair's band {not_next}")
    assert dropped >= 1 and partial >= 1 and matches >= 50
    assert not_next >= 1                                              # fails for a wrong stride
    for stride in (9, 16, 20):
        fbuf = pack_f(RAGGED_F, stride)
        for fl in (flags, flags | MUTUAL):
            gots = {band: run_epipolar(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, SYMMETRIC, fbuf, stride, band)
                    for band in sorted(set(RAGGED_BAND))}
            got = np.stack([gots[RAGGED_BAND[i]][i] for i in range(len(p1))])
            check_epipolar(orc, got, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, SYMMETRIC, mats, RAGGED_F, RAGGED_BAND,
                           fwds)
            if fl & MUTUAL:
                for i, n1 in enumerate(COUNTS1):
                    kept = got[i, :n1]["match"][got[i, :n1]["match"] >= 0]
                    assert len(np.unique(kept)) == len(kept), f"pair {i}: the kept matches share partners"


# ------------------------------------------------------------------ 4. edges

def edge_pair(surf, seed=191):
    nf, n1, n2 = 64, 40, 96
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p1["laplace"] = 1
    p2["laplace"] = 1
    for p in (p1, p2):                                                # integer rows, far apart unless planted
        p["x"] = rng.integers(0, 200, p.shape)
        p["y"] = 8.0 * rng.permutation(p.shape[1])[None, :]
    return rng, nf, n1, n2, p1, f1, p2, f2


def test_edges(surf, orc):
    """The rectified matrix and band 1.5: partners planted at dy = +-1.5 are
    offered (the exact-descriptor copy wins), at +-1.75 and at the next float
    past 1.5 not; NaN and infinite coordinates on either side are offered
    nothing and are never offered."""
    rng, nf, n1, n2, p1, f1, p2, f2 = edge_pair(surf)
    p1["y"][0] = 1000.0 + 16.0 * np.arange(n1)                        # nobody near anybody ...
    p2["y"][0] = 5000.0 + 16.0 * np.arange(n2)
    p1["y"][0, 4] = 0.0                                               # (where y1 + nextafter(1.5) is exact)
    f32 = np.float32
    up = f32(INF)
    # (set-1 point, set-2 slot, dy, offered): ... but these
    edges = [(0, 1, f32(1.5), True), (1, 2, f32(-1.5), True), (2, 3, f32(1.75), False), (3, 4, f32(-1.75), False),
             (4, 5, np.nextafter(f32(1.5), up), False), (5, 33, f32(0.0), True), (6, 34, f32(1.0), True),
             (7, 35, f32(-1.25), True)]
    for k, j, dy, _ in edges:
        p2["y"][0, j] = p1["y"][0, k] + dy
        assert p2["y"][0, j] - p1["y"][0, k] == dy                    # (exact)
        f2[0, j] = f1[0, k]
    # point 8: the exact copy at dy = 1.5 (slot 43) wins over a double-score one at 1.75 ahead of it in its thread
    # row (slot 40); the second is a half-score copy at dy = 0 in another row (slot 44)
    p2["y"][0, [43, 44, 40]] = p1["y"][0, 8] + np.array([1.5, 0.0, 1.75], np.float32)
    f2[0, 43], f2[0, 44], f2[0, 40] = f1[0, 8], 0.5 * f1[0, 8], 2.0 * f1[0, 8]
    # set-1 points with NaN and infinite coordinates, each with an exact partner on its (finite) row
    p1["x"][0, 20] = np.nan
    p1["y"][0, 21] = np.nan
    p1["x"][0, 22] = INF
    p1["y"][0, 23] = -INF
    for k in (20, 21, 22, 23):
        f2[0, 50 + k] = f1[0, k]
        p2["y"][0, 50 + k] = p1["y"][0, k] if np.isfinite(p1["y"][0, k]) else -500.0
    # set-2 points with NaN and infinite coordinates on the rows of set-1 points 24 .. 27, with their descriptors
    for k, (x, y) in zip((24, 25, 26, 27), ((np.nan, None), (None, np.nan), (INF, None), (None, -INF))):
        p2["x"][0, 60 + k] = x if x is not None else p2["x"][0, 60 + k]
        p2["y"][0, 60 + k] = y if y is not None else p1["y"][0, k]
        f2[0, 60 + k] = f1[0, k]
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL, 0, SAME_LAPLACE | MUTUAL):
        got = run_epipolar(surf, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, pack_f([RECTIFIED], 9), 9, BAND)
        (ref, fwd, m), = check_epipolar(orc, got, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, mats, [RECTIFIED],
                                        [BAND])
        for k, j, dy, offered in edges:
            assert m[k, j] == offered, (k, j)
            assert (fwd["match"][k] == j) == offered, (k, j, fwd["match"][k])
        assert m[8, 43] and m[8, 44] and not m[8, 40]
        assert fwd["match"][8] == 43 and got[0, 8]["match"] == 43
        assert abs(float(fwd["ambiguity"][8]) - 0.5) < 0.05           # the second is the half score, not the double
        assert not m[20:24].any() and not m[:, 84:88].any()
        assert_nothing(got[0, 20:24])
        assert (got[0, 24:28]["match"] == -1).all()
        # band 0: only dy == 0
        zero = run_epipolar(surf, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, pack_f([RECTIFIED], 9), 9, 0.0)
        (_, fwd0, m0), = check_epipolar(orc, zero, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, mats, [RECTIFIED],
                                        [0.0])
        assert m0.sum() == 2 and m0[5, 33] and m0[8, 44]
        assert fwd0["match"][5] == 33 and fwd0["match"][8] == 44 and (fwd0["match"] >= 0).sum() == 2


def test_unusable_and_wide_open(surf, orc):
    """A matrix holding a NaN matches nothing; band 1e6 under a matrix from two
    camera poses (norm 1: lim is about 1e12 (a^2 + b^2), far above every r r
    of this data) gives the window call's bits."""
    p1, f1, p2, f2 = window_data(surf, 64)
    for k in range(9):
        nan_f = POSES.copy()
        nan_f[k] = np.nan
        for flags in (FULL_TAIL, FULL_TAIL | SAME_LAPLACE | MUTUAL):
            got = run_epipolar(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, EVERYWHERE, pack_f([nan_f], 0), 0, BAND)
            for i, n1 in enumerate(COUNTS1):
                assert_nothing(got[i, :n1])
                assert (got[i, n1:]["match"] == CANARY["match"]).all()
    for flags in (0, FULL_TAIL | MUTUAL):
        for win in (SYMMETRIC, EVERYWHERE):
            for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
                assert epipolar_mask(p1[i, :n1], p2[i, :n2], 0, EVERYWHERE, POSES, 1e6).all()
            want = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, win)
            got = run_epipolar(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, win, pack_f([POSES], 0), 0, 1e6)
            assert got.tobytes() == want.tobytes(), (flags, win)


# ------------------------------------------------------------ 5. three blocks

TILTED = translation_f(1.0, 0.0625)                                   # y2 - y1 = (x2 - x1) / 16: lines tilted by 3.6 degrees


def test_three_blocks_under_tilted_lines(surf, orc):
    """n1 = 300 against n2 = 320, both sorted by y over 1000 rows, x over 1600
    columns: a line climbs up to 100 rows across the frame.  The planted exact
    partners of points of block 0 lie in a set-2 tile that block 0's rows
    alone (the rectified matrix, the same band) would drop and the tilted
    lines keep; with MUTUAL the planted back best in another block clears the
    noisy copy."""
    nf, n1, n2 = 64, 300, 320
    win = (-INF, INF, -150.0, 150.0)
    rng = np.random.default_rng(179)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p1["x"], p2["x"] = rng.integers(0, 1600, (1, n1)), rng.integers(0, 1600, (1, n2))
    p1["y"] = (np.arange(n1) * (1000.0 / n1)).astype(np.float32)
    p2["y"] = (np.arange(n2) * (1000.0 / n2)).astype(np.float32)
    # block 0's points 120 .. 127 (rows 400 .. 423) at x = 0; their exact partners at x = 1600, 100 rows further
    # down their lines: set-2 slots of tile 5 (rows 500 .. 597)
    planted = []
    for k in range(8):
        i = 120 + k
        j = int(np.ceil((p1["y"][0, i] + 100.0) / (1000.0 / n2)))
        assert j // 32 == 5 and (i, j) not in planted
        planted.append((i, j))
        p1["x"][0, i] = 0.0
        p2["x"][0, j] = np.float32(16.0 * (p2["y"][0, j] - p1["y"][0, i]))    # on the line, to the rounding of x
        f2[0, j] = f1[0, i]
        p2["laplace"][0, j] = p1["laplace"][0, i]
    # set-2 point 136 (row 425): its exact copy in block 1, a noisy copy in block 0, both with their line through it
    j, exact, noisy = 136, 130, 117
    p2["x"][0, j] = 800.0
    for i in (exact, noisy):
        p1["x"][0, i] = np.float32(800.0 - 16.0 * (p2["y"][0, j] - p1["y"][0, i]))
        p1["laplace"][0, i] = p2["laplace"][0, j]
    f1[0, exact] = f2[0, j]
    nv = f2[0, j] + 0.05 * rng.standard_normal(nf).astype(np.float32)
    f1[0, noisy] = nv / np.linalg.norm(nv)
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    tile5 = box(p2["x"][0, 160:192], p2["y"][0, 160:192])
    block0 = slice(0, 128)
    for flags in (0, FULL_TAIL | SAME_LAPLACE):
        got = run_epipolar(surf, p1, f1, [n1], p2, f2, [n2], flags, win, pack_f([TILTED], 0), 0, BAND)
        (ref, fwd, m), = check_epipolar(orc, got, p1, f1, [n1], p2, f2, [n2], flags, win, mats, [TILTED], [BAND])
        for i, pj in planted:
            assert m[i, pj] and fwd["match"][i] == pj and got[0, i]["match"] == pj and fwd["score"][i] > 0.99
        assert may_offer(box(p1["x"][0, block0], p1["y"][0, block0]), tile5, win)     # the window keeps the tile,
        a, b, c, lim = epipolar_lines(p1[0, block0], TILTED, BAND)
        assert line_may_offer(a, b, c, lim, tile5).any()                              # the tilted lines keep it,
        a, b, c, lim = epipolar_lines(p1[0, block0], RECTIFIED, BAND)
        assert not line_may_offer(a, b, c, lim, tile5).any()                          # the block's rows would not
        total, kept, part = epipolar_census(p1[0], p2[0], flags, win, TILTED, BAND, m)
        wtotal, wkept, wpart = epipolar_census(p1[0], p2[0], flags, win, TILTED, BAND, m, 32)
        print(f"flags {flags}: blocks kept {kept} of {total} ({part} partly offered), waves {wkept} of {wtotal} "
              f"({wpart}), offered pairs {int(m.sum())}")
        assert total == 30 and kept < total and part >= 1
        assert wtotal == 100 and wkept < wtotal and wpart >= 1
        mut = run_epipolar(surf, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, win, pack_f([TILTED], 0), 0, BAND)
        check_epipolar(orc, mut, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, win, mats, [TILTED], [BAND])
        assert fwd["match"][exact] == j and fwd["match"][noisy] == j and exact // 128 != noisy // 128
        assert mut[0, exact]["match"] == j and mut[0, noisy]["match"] == -1


# ------------------------------------------------------ 6. chunked tile list

def test_more_tiles_than_one_list_chunk(surf, orc):
    """n2 = 8300: 260 tiles, the kept-tile list is built in two chunks of 256
    tile boxes.  One wave's lines run near the first rows and one's near the
    last: both chunks hold offered pairs, and the waves score a small share
    of the tiles."""
    nf, n1, n2 = 64, 64, 8300
    rng = np.random.default_rng(224)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p2["x"] = rng.integers(0, 100, (1, n2))
    p2["y"] = np.arange(n2, dtype=np.float32)[None, :]           # a tile: 32 rows
    p1["x"][0] = rng.integers(0, 100, n1)
    p1["y"][0] = np.concatenate([rng.integers(0, 150, 32), rng.integers(8250, 8299, 32)])
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
        m = epipolar_mask(p1[0], p2[0], flags, EVERYWHERE, TILTED, BAND)
        s = np.zeros((n1, n2), np.float32)                        # the columns somebody is offered; 0 elsewhere
        if flags & MUTUAL:
            for j in np.nonzero(m.any(axis=0))[0]:
                s[:, j] = score_column(orc, p1[0], f1[0], f2[0, j])
        got = run_epipolar(surf, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, pack_f([TILTED], 9), 9, BAND)
        (ref, fwd, m2), = check_epipolar(orc, got, p1, f1, [n1], p2, f2, [n2], flags, EVERYWHERE, [s], [TILTED],
                                         [BAND])
        total, kept, part = epipolar_census(p1[0], p2[0], flags, EVERYWHERE, TILTED, BAND, m2)
        wave_total, wave_kept, _ = epipolar_census(p1[0], p2[0], flags, EVERYWHERE, TILTED, BAND, m2, 32)
        print(f"flags {flags}: block keeps {kept} of {total}, waves {wave_kept} of {wave_total}, offered "
              f"{int(m2.sum())}, matches {int((got[0]['match'] >= 0).sum())}")
        # rows 0 .. 149 +- 8 and 8250 .. 8298 +- 8 (the lines climb 100 / 16 rows over the x range): 6 + 3 tiles
        assert total == 260 and kept <= 10
        assert wave_total == 520 and wave_kept <= 10
        assert m2[:, :256 * 32].any() and m2[:, 256 * 32:].any()
        assert (got[0, :32]["match"] >= 0).any() and (got[0, 32:]["match"] >= 8192).any()
        assert (got[0]["match"] >= 0).sum() >= 16


# ------------------------------------------------------------ 7. robustness

ROBUST_F = [TILTED, translation_f(1.0, -0.125), POSES]
ROBUST_BAND = 6.0
ROBUST_WIN = (-INF, INF, -60.0, 60.0)


def test_scratch_full_of_ff(surf, orc):
    """The scratch may hold anything: all-0xFF first, then its own leftovers."""
    s1, s2 = 160, 96
    rng, p1, f1, p2, f2 = small_batch(surf, 157, 2, s1, s2)
    fs = ROBUST_F[:2]
    flags = FULL_TAIL | MUTUAL
    c1, c2 = [s1, 150], [s2, 90]
    scratch = surf.DeviceBuffer(surf.match_batch_epipolar_scratch_bytes(2, s1, s2, flags))
    scratch.upload(np.full(scratch.nbytes, 0xFF, np.uint8))
    mats = matrices(orc, p1, f1, c1, f2, c2)
    runs = []
    for _ in range(2):
        got = run_epipolar(surf, p1, f1, c1, p2, f2, c2, flags, ROBUST_WIN, pack_f(fs, 9), 9, ROBUST_BAND,
                           scratch=scratch)
        check_epipolar(orc, got, p1, f1, c1, p2, f2, c2, flags, ROBUST_WIN, mats, fs, [ROBUST_BAND] * 2)
        runs.append(got)
    scratch.free()
    assert runs[0].tobytes() == runs[1].tobytes()
    assert (runs[0]["match"][0] >= 0).sum() >= 4


def test_position_independence(surf, orc):
    """The same pair and matrix at positions 0, 5 and 11 of a batch of
    unrelated pairs, and over two runs: the same bits."""
    nf, src = 64, 10                                              # 159 x 192: two blocks
    rp1, rf1, rp2, rf2 = window_data(surf, nf)
    p1, f1, p2, f2 = rp1.copy(), rf1.copy(), rp2.copy(), rf2.copy()
    c1, c2, fs = list(COUNTS1), list(COUNTS2), list(RAGGED_F)
    where = (0, 5, 11)
    for k in where:
        p1[k], f1[k], p2[k], f2[k], c1[k], c2[k] = rp1[src], rf1[src], rp2[src], rf2[src], COUNTS1[src], COUNTS2[src]
        fs[k] = STEEP
    mats = ragged_matrices(surf, orc, nf)
    mats = [mats[src] if k in where else mats[k] for k in range(12)]
    for flags in (0, FULL_TAIL | SAME_LAPLACE | MUTUAL):
        got = run_epipolar(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_f(fs, 16), 16, ROBUST_BAND)
        again = run_epipolar(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_f(fs, 16), 16, ROBUST_BAND)
        assert got.tobytes() == again.tobytes(), flags
        for k in where[1:]:
            assert got[k].tobytes() == got[where[0]].tobytes(), (flags, k)
        check_epipolar(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, mats, fs, [ROBUST_BAND] * 12)
        assert (got[where[0], :COUNTS1[src]]["match"] >= 0).sum() >= 4


def test_counts_are_clamped(surf, orc):
    s1, s2 = 70, 100
    rng, p1, f1, p2, f2 = small_batch(surf, 146, 3, s1, s2)
    c1, c2 = [s1 + 9, 40, -3], [s2 + 9, -3, 64]
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
        got = run_epipolar(surf, p1, f1, c1, p2, f2, c2, flags, ROBUST_WIN, pack_f(ROBUST_F, 9), 9, ROBUST_BAND)
        check_epipolar(orc, got, p1, f1, c1, p2, f2, c2, flags, ROBUST_WIN, matrices(orc, p1, f1, c1, f2, c2),
                       ROBUST_F, [ROBUST_BAND] * 3)
        assert (got[0]["match"] >= 0).sum() >= 12                 # all 70 slots against all 100
        assert (got[1, :40]["match"] == -1).all()                 # n2 = 0
        assert (got[2]["match"] == CANARY["match"]).all()         # n1 = 0: nothing written


def test_consecutive_frames_overlap(surf, orc):
    """Set 2 = set 1 advanced one frame in the same buffers (nframes 4,
    npairs 3): only match fields of set-1 points are written, only x, y,
    laplace of set 2 are read."""
    nf, n, slots = 64, 4, 96
    rng, pts, desc, _, _ = small_batch(surf, 147, n, slots, 32)
    counts = np.array([96, 70, 64, 33], np.int32)
    for i in reversed(range(n - 1)):                              # frame i + 1's first 64 points: frame i's, moved
        pts["x"][i, :64] = pts["x"][i + 1, :64] + rng.integers(-20, 21, 64)        # ... along TILTED's lines
        pts["y"][i, :64] = pts["y"][i + 1, :64] + (pts["x"][i, :64] - pts["x"][i + 1, :64]) * np.float32(0.0625)
        desc[i, :64] = desc[i + 1, :64] + 0.03 * rng.standard_normal((64, nf)).astype(np.float32)
    fs = [TILTED] * (n - 1)
    for flags in (0, FULL_TAIL | SAME_LAPLACE | MUTUAL):
        pb = surf.DeviceBuffer(pts.nbytes)
        db = surf.DeviceBuffer(desc.nbytes)
        cb = surf.DeviceBuffer(counts.nbytes)
        hb = surf.DeviceBuffer(4 * 9)
        sb = surf.DeviceBuffer(surf.match_batch_epipolar_scratch_bytes(n - 1, slots, slots, flags))
        for b, a in ((pb, pts), (db, desc), (cb, counts), (hb, pack_f(fs[:1], 0))):
            b.upload(a)
        surf.match_batch_epipolar(pb.ptr, db.ptr, cb.ptr, slots, pb.ptr + 48 * slots, db.ptr + 4 * slots * nf,
                                  cb.ptr + 4, slots, n - 1, nf, flags, hb.ptr, 0, BAND, ROBUST_WIN, sb.ptr)
        surf.synchronize()
        got = pb.download(surf.POINT_DTYPE, n * slots).reshape(n, slots)
        assert db.download(np.float32, desc.size).tobytes() == desc.tobytes()
        for b in (pb, db, cb, hb, sb):
            b.free()
        assert got[n - 1].tobytes() == pts[n - 1].tobytes()       # the last frame is set 2 only
        mats = matrices(orc, pts[:-1], desc[:-1], counts[:-1], desc[1:], counts[1:])
        check_epipolar(orc, got[:-1], pts[:-1], desc[:-1], counts[:-1], pts[1:], desc[1:], counts[1:], flags,
                       ROBUST_WIN, mats, fs, [BAND] * (n - 1))
        assert min((got[i, :counts[i]]["match"] >= 0).sum() for i in range(n - 1)) >= 8


# ------------------------------------------------------ 8. no host round trip

# Half of the 1466 kept matches of the first MI355X run (first pass 709 inliers of 804 candidates; second pass 870 of
# 947): a guard against a silent collapse, not against a slowdown.
KEPT_FLOOR = 733


def test_real_stereo_pair_without_host_round_trip(surf, orc):
    """The left / right keypoints and descriptors of a real 1280 x 960 stereo
    pair as one pair: match_batch -> fundamental_batch (nhyp 1024) ->
    match_batch_epipolar (MUTUAL) reading the fundamental record where it
    lies, at f_stride 16, band = twice the RANSAC threshold, the infinite
    window -> fundamental_batch, enqueued with one synchronise at the end."""
    thr, amb, nf = 3.0, np.float32(0.95), 64
    band = 2.0 * thr
    za = np.load(os.path.join(GOLDEN, "left_1280x960_upright.npz"))
    zb = np.load(os.path.join(GOLDEN, "right_1280x960_upright.npz"))
    p1 = za["points"].view(surf.POINT_DTYPE).copy().reshape(-1)
    p2 = zb["points"].view(surf.POINT_DTYPE).copy().reshape(-1)
    f1, f2 = np.ascontiguousarray(za["desc"], np.float32), np.ascontiguousarray(zb["desc"], np.float32)
    n1, n2 = len(p1), len(p2)
    assert f1.shape == (n1, nf) and f2.shape == (n2, nf)
    bufs = []
    for a in (p1, f1, np.array([n1], np.int32), p2, f2, np.array([n2], np.int32)):
        b = surf.DeviceBuffer(a.nbytes)
        b.upload(a)
        bufs.append(b)
    ob1, ob2 = surf.DeviceBuffer(64), surf.DeviceBuffer(64)
    sb = surf.DeviceBuffer(surf.match_batch_epipolar_scratch_bytes(1, n1, n2, MUTUAL))
    sets = (bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, n2)
    surf.match_batch(*sets, 1, nf, 0)
    surf.fundamental_batch(bufs[0].ptr, bufs[2].ptr, n1, 1, ob1.ptr, None, float(amb), thr, 1024, 0)
    surf.match_batch_epipolar(*sets, 1, nf, MUTUAL, ob1.ptr, 16, band, EVERYWHERE, sb.ptr)
    surf.fundamental_batch(bufs[0].ptr, bufs[2].ptr, n1, 1, ob2.ptr, None, float(amb), thr, 1024, 0)
    surf.synchronize()
    g = bufs[0].download(surf.POINT_DTYPE, n1)
    first = ob1.download(surf.FUNDAMENTAL_DTYPE, 1)[0]
    second = ob2.download(surf.FUNDAMENTAL_DTYPE, 1)[0]
    assert bufs[3].download(surf.POINT_DTYPE, n2).tobytes() == p2.tobytes()
    for b in bufs + [ob1, ob2, sb]:
        b.free()
    assert first["status"] == surf.FUND_OK
    fm = first["f"]
    fwd, m = mask_forward(orc, p1, p2, f1, f2, 0, epipolar_mask(p1, p2, 0, EVERYWHERE, fm, band))
    ref = fwd.copy()
    for j in np.unique(fwd["match"][fwd["match"] >= 0]):              # B only where a forward match names the column
        col = np.where(m[:, j], score_column(orc, p1, f1, f2[j]), np.float32(0))
        rows = np.nonzero(fwd["match"] == j)[0]
        assert col.max() > 0 and (col[rows].view(np.uint32) == fwd["score"][rows].view(np.uint32)).all()
        lose = rows[rows != int(col.argmax())]
        ref["match"][lose] = -1
        ref["match_x"][lose] = 0.0
        ref["match_y"][lose] = 0.0
    assert_match_equal(g, ref, "real pair: ")
    for f in KEPT_FIELDS:
        assert (g[f].view(np.uint32) == p1[f].view(np.uint32)).all(), f
    kept = g["match"] >= 0
    f64 = fm.astype(np.float64).reshape(3, 3)
    x, y, u, v = (g[k][kept].astype(np.float64) for k in ("x", "y", "match_x", "match_y"))
    a = f64[0, 0] * x + f64[0, 1] * y + f64[0, 2]
    b = f64[1, 0] * x + f64[1, 1] * y + f64[1, 2]
    c = f64[2, 0] * x + f64[2, 1] * y + f64[2, 2]
    dist = np.abs(u * a + v * b + c) / np.hypot(a, b)
    assert (dist <= band + 1e-3).all(), dist.max()
    assert (g["match_x"][kept] == p2["x"][g["match"][kept]]).all()
    assert len(np.unique(g["match"][kept])) == kept.sum()             # injective
    print(f"real pair {n1} x {n2}: first pass ncand {first['ncand']} ninliers {first['ninliers']} rms "
          f"{first['rms']:.4f}; epipolar kept {kept.sum()} (largest line distance {dist.max():.3f} px), second pass "
          f"status {second['status']} ncand {second['ncand']} ninliers {second['ninliers']} rms {second['rms']:.4f}")
    assert int(second["ncand"]) == int((kept & (g["ambiguity"] <= amb)).sum())
    assert kept.sum() >= KEPT_FLOOR
