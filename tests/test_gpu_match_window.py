"""GPU tests of surfhip_match_batch_window (batched matching inside a search
window, optionally with the mutual-best test): every comparison is bitwise on
the five match fields against a host model built from the CPU oracle's
or_match alone.

The model.  "Offered" is evaluated in numpy with the kernel's own fp32
subtractions.  Forward, for set-1 point p1: or_match of p1 against the pair's
set 2 with the descriptor rows of the points not offered to p1 set to zero
(the zero-row construction of test_gpu_match_batch.test_same_laplace_flag,
here per point; points with one and the same offered set share one or_match
call, which treats its set-1 points independently).  Back: the column maxima
of the score matrix of match_ref.score_column, masked by
"offered"."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from match_ref import (CANARY, COUNTS1, COUNTS2, EVERYWHERE, FULL_TAIL, INF, KEPT_FIELDS, MATCH_FIELDS, MUTUAL,
                       SAME_LAPLACE, SYMMETRIC, WINDOWS, assert_match_equal, box, clamp, cross_model, forward_ref,
                       make_points, matrices, may_offer, offered_mask, ragged_data, ragged_matrices, ragged_plain,
                       run_cross, run_window, score_column, tile_census, window_data, window_forward, window_model,
                       with_canary)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- checking

def check_window(orc, got, p1, f1, c1, p2, f2, c2, flags, win, mats, fwds=None):
    """got against the model per pair + the nothing-else-written properties of
    check_batch (canary past the counts, detect fields).  mats[i]: the pair's
    score matrix; fwds[i]: its (forward points, mask) where already known.
    Returns the per-pair (expected, forward, mask)."""
    s1, s2 = p1.shape[1], p2.shape[1]
    refs = []
    for i in range(len(p1)):
        n1, n2 = clamp(c1[i], s1), clamp(c2[i], s2)
        a, b, fa, fb = p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2]
        ref, fwd, m = window_model(orc, mats[i], a, b, fa, fb, flags, win, fwds[i] if fwds is not None else None)
        assert_match_equal(got[i, :n1], ref, f"flags {flags} window {win} pair {i} (n1 {n1}, n2 {n2}): ")
        for f in MATCH_FIELDS:                                    # slots at or past n1: untouched
            assert (got[i, n1:][f].view(np.uint32) == p1[i, n1:][f].view(np.uint32)).all(), (i, f)
        for f in KEPT_FIELDS:
            assert (got[i][f].view(np.uint32) == p1[i][f].view(np.uint32)).all(), (i, f)
        refs.append((ref, fwd, m))
    return refs


@functools.lru_cache(maxsize=None)
def window_forwards(surf, orc, nf, flags, name):
    """Per pair of window_data: (forward points, offered mask)."""
    p1, f1, p2, f2 = window_data(surf, nf)
    return [window_forward(orc, p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2], flags, WINDOWS[name])
            for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2))]


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_infinite_window(surf, orc, nf, flags):
    """The window (-inf, inf, -inf, inf) gives the bits of match_batch and,
    with MUTUAL, of match_batch_cross: GPU against GPU and against the model."""
    p1, f1, p2, f2 = ragged_data(surf, nf)
    mats = ragged_matrices(surf, orc, nf)
    got = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, EVERYWHERE)
    mut = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags | MUTUAL, surf.MatchWindow(*EVERYWHERE))
    assert got.tobytes() == ragged_plain(surf, nf, flags).tobytes()
    assert mut.tobytes() == run_cross(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags).tobytes()
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        a, b, fa, fb = p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2]
        assert_match_equal(got[i, :n1], forward_ref(orc, a, b, fa, fb, flags), f"pair {i}: ")
        assert_match_equal(mut[i, :n1], cross_model(orc, mats[i], a, b, fa, fb, flags)[0], f"MUTUAL, pair {i}: ")
    check_window(orc, got, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, EVERYWHERE, mats)
    check_window(orc, mut, p1, f1, COUNTS1, p2, f2, COUNTS2, flags | MUTUAL, EVERYWHERE, mats)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["symmetric", "stereo"])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_ragged_batch(surf, orc, nf, name, flags):
    """The ragged batch (empty sets, partial tiles, dead waves, two blocks,
    the any-length kernel) inside +-40 px and inside a stereo-like window,
    plain and with MUTUAL."""
    win = WINDOWS[name]
    p1, f1, p2, f2 = window_data(surf, nf)
    mats = ragged_matrices(surf, orc, nf)                         # (the descriptors are those of ragged_data)
    fwds = window_forwards(surf, orc, nf, flags, name)
    got = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, win)
    check_window(orc, got, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, win, mats, fwds)
    mut = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags | MUTUAL, win)
    refs = check_window(orc, mut, p1, f1, COUNTS1, p2, f2, COUNTS2, flags | MUTUAL, win, mats, fwds)

    # what the data exercise, from the model
    nothing = dropped = partial = differs = cleared = 0
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        a, b = p1[i, :n1], p2[i, :n2]
        fwd, m = fwds[i]
        nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
        if nscan:
            nothing += int((~m[:, :nscan].any(axis=1)).sum())
        for group in (128, 32):                                   # blocks and waves
            total, kept, part = tile_census(a, b, flags, win, m, group)
            dropped += total - kept
            partial += part
        plain = forward_ref(orc, a, b, f1[i, :n1], f2[i, :n2], flags)
        differs += int((plain["match"] != fwd["match"]).sum())
        hit = fwd["match"] >= 0
        assert m[np.nonzero(hit)[0], fwd["match"][hit]].all()     # every match lies in the window
        none = ~m[:, :nscan].any(axis=1)
        for f in MATCH_FIELDS:
            assert (got[i, :n1][f][none] == (-1 if f == "match" else 0)).all(), (i, f)
        cleared += int((hit & (refs[i][0]["match"] < 0)).sum())
        g = mut[i, :n1]
        kept_m = g["match"][g["match"] >= 0]
        assert len(np.unique(kept_m)) == len(kept_m), f"pair {i}: the kept matches share partners"
    print(f"nf {nf} {name} flags {flags}: nothing offered {nothing}, dropped (group, tile) {dropped}, "
          f"partly offered {partial}, matches other than unwindowed {differs}, cleared by MUTUAL {cleared}")
    assert nothing >= 1 and dropped >= 1 and partial >= 1
    assert differs >= 1                                           # fails for a call that ignores the window


def test_edges(surf, orc):
    """Inclusive bounds and their next floats, NaN and infinite coordinates on
    both sides, a tile of NaN points, and a stronger point outside the window
    ahead of the winner in its tile."""
    nf, n1, n2 = 64, 40, 96
    rng = np.random.default_rng(91)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p1["laplace"] = 1
    p2["laplace"] = 1
    win = (-3.0, 5.0, -2.0, 7.0)
    p1["x"], p1["y"] = 100.0, 100.0
    p2["x"][0, :64] = 100 + rng.integers(-5, 8, 64) + 0.25        # around the window: some in, some out
    p2["y"][0, :64] = 100 + rng.integers(-4, 10, 64) + 0.25
    up, down = np.float32(INF), np.float32(-INF)
    f32 = np.float32
    # (set-2 slot, x, y, offered): exactly on each bound, and the next float outside
    edges = [(1, f32(105), f32(100), True), (2, np.nextafter(f32(105), up), f32(100), False),
             (3, f32(97), f32(100), True), (4, np.nextafter(f32(97), down), f32(100), False),
             (5, f32(100), f32(107), True), (6, f32(100), np.nextafter(f32(107), up), False),
             (7, f32(100), f32(98), True), (8, f32(100), np.nextafter(f32(98), down), False),
             (33, f32(105), f32(107), True), (34, f32(97), f32(98), True),          # the corners
             (35, f32(np.nan), f32(100), False), (36, f32(100), f32(np.nan), False),
             (37, f32(INF), f32(100), False), (38, f32(100), f32(-INF), False)]
    for k, (j, x, y, _) in enumerate(edges):                      # set-1 point k would choose slot j: its own row
        p2["x"][0, j], p2["y"][0, j] = x, y
        f1[0, k] = f2[0, j]
    # set-1 points with NaN and infinite coordinates
    p1["x"][0, 20] = np.nan
    p1["y"][0, 21] = np.nan
    p1["x"][0, 22] = INF
    p1["y"][0, 23] = -INF
    # tile 2: NaN points with rows that would win everything
    p2["x"][0, 64:] = np.nan
    p2["y"][0, 64:] = np.nan
    f2[0, 64:] = 3.0 * f1[0, 8:40]
    # point 30: the stronger slot 40 lies outside, the winner 43 in the same
    # thread row of the same tile inside, a second inside in tile 0
    p2["x"][0, [40, 43, 12]], p2["y"][0, [40, 43, 12]] = [120.0, 101.0, 102.0], [100.0, 101.0, 99.0]
    f2[0, 40], f2[0, 43], f2[0, 12] = 2.0 * f1[0, 30], f1[0, 30], 0.5 * f1[0, 30]
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL, 0, SAME_LAPLACE | MUTUAL):
        got = run_window(surf, p1, f1, [n1], p2, f2, [n2], flags, win)
        (ref, fwd, m), = check_window(orc, got, p1, f1, [n1], p2, f2, [n2], flags, win, mats)
        for k, (j, x, y, offered) in enumerate(edges):
            assert m[k, j] == offered, (k, j)
            assert (fwd["match"][k] == j) == offered, (k, j, fwd["match"][k])
        assert not m[:, 64:].any() and not m[20].any() and not m[21].any() and not m[22].any() and not m[23].any()
        for k in (20, 21, 22, 23):
            assert got[0, k]["match"] == -1 and got[0, k]["score"] == 0 and got[0, k]["ambiguity"] == 0
        assert not m[30, 40] and m[30, 43] and m[30, 12]
        assert fwd["match"][30] == 43 and fwd["score"][30] == mats[0][30, 43]
        assert abs(float(fwd["ambiguity"][30]) - 0.5) < 0.05      # the second is slot 12's half score, not slot 40
        assert got[0, 30]["match"] == 43
    # half-infinite windows: an infinite coordinate is offered, inf - inf and NaN are not
    p2["x"][0, 39], p2["y"][0, 39] = -INF, 100.0
    for w in ((-INF, INF, -2.0, 7.0), (-INF, 5.0, -INF, INF)):
        for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
            got = run_window(surf, p1, f1, [n1], p2, f2, [n2], flags, w)
            (ref, fwd, m), = check_window(orc, got, p1, f1, [n1], p2, f2, [n2], flags, w, mats)
            assert m[0, 39] and not m[22, 37] and not m[:, 35].any() and not m[:, 64:].any()
            assert m[22, 39] == (w[0] == -INF and w[2] <= 0)      # -inf - inf = -inf
            assert m[0, 37] == (w[1] == INF)


def test_three_blocks(surf, orc):
    """n1 = 300 against n2 = 320, both sorted by y: the best partners of
    points of block 2 lie in tiles block 0 drops; with MUTUAL the back best of
    a planted set-2 point sits in another block than the other point that
    chose it."""
    nf, n1, n2 = 64, 300, 320
    rng = np.random.default_rng(78)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p1["x"], p2["x"] = rng.uniform(0, 50, (1, n1)), rng.uniform(0, 50, (1, n2))
    p1["y"] = (np.arange(n1) * (1000.0 / n1)).astype(np.float32)
    p2["y"] = (np.arange(n2) * (1000.0 / n2)).astype(np.float32)
    # block 2's points 270 .. 279 and their exact partners in tile 9
    for k in range(10):
        f2[0, 288 + k] = f1[0, 270 + k]
        p2["x"][0, 288 + k] = p1["x"][0, 270 + k]
    # (set-2 point, its exact copy in set 1, a noisy copy in the block before)
    plants = [(136, 130, 125), (271, 258, 250)]
    for j, exact, noisy in plants:
        f1[0, exact] = f2[0, j]
        v = f2[0, j] + 0.05 * rng.standard_normal(nf).astype(np.float32)
        f1[0, noisy] = v / np.linalg.norm(v)
        p1["x"][0, [exact, noisy]] = p2["x"][0, j]
        p1["laplace"][0, [exact, noisy]] = p2["laplace"][0, j]
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    for flags in (0, FULL_TAIL | SAME_LAPLACE):
        got = run_window(surf, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC)
        (ref, fwd, m), = check_window(orc, got, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC, mats)
        block0 = box(p1["x"][0, :128], p1["y"][0, :128])
        for k in range(10):
            j = 288 + k
            if flags & SAME_LAPLACE and p1["laplace"][0, 270 + k] != p2["laplace"][0, j]:
                continue
            assert fwd["match"][270 + k] == j and got[0, 270 + k]["match"] == j
            assert not may_offer(block0, box(p2["x"][0, 32 * (j // 32):][:32], p2["y"][0, 32 * (j // 32):][:32]),
                                 SYMMETRIC)
        total, kept, part = tile_census(p1[0], p2[0], flags, SYMMETRIC, m)
        assert total == 30 and kept < 20 and part >= 3
        mut = run_window(surf, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, SYMMETRIC)
        check_window(orc, mut, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, SYMMETRIC, mats)
        for j, exact, noisy in plants:
            assert fwd["match"][exact] == j and fwd["match"][noisy] == j and exact // 128 != noisy // 128
            assert mut[0, exact]["match"] == j and mut[0, noisy]["match"] == -1


def test_more_tiles_than_one_list_chunk(surf, orc):
    """n2 = 8300: 260 tiles, so the kept-tile list is built in two chunks of
    256 tile boxes.  Pair 0: one wave near the first rows and one near the
    last, the block's box covers everything (a full first chunk, every tile
    staged, the waves skip most); pair 1: both waves near the last rows (an
    empty first chunk, then a few tiles); pair 2: near the first rows only."""
    nf, n1, n2 = 64, 64, 8300
    rng = np.random.default_rng(123)
    f1 = rng.standard_normal((3, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((3, n2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 3, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, n2, surf.POINT_DTYPE)
    p2["x"] = rng.uniform(0, 100, (3, n2))
    p2["y"] = np.arange(n2, dtype=np.float32)[None, :]           # a tile: 32 rows
    p1["x"] = rng.uniform(0, 100, (3, n1))
    top, bottom = rng.uniform(0, 150, (3, 32)), rng.uniform(8250, 8299, (3, 32))
    p1["y"][0] = np.concatenate([top[0], bottom[0]])
    p1["y"][1] = np.concatenate([bottom[1], bottom[2]])
    p1["y"][2] = np.concatenate([top[1], top[2]])
    c1, c2 = [n1, n1, n1], [n2, n2, n2]
    mats = None
    for flags in (0, FULL_TAIL | MUTUAL):
        if flags & MUTUAL:                                        # the columns somebody is offered; 0 elsewhere
            mats = []
            for i in range(3):
                m = offered_mask(p1[i], p2[i], flags, SYMMETRIC)
                s = np.zeros((n1, n2), np.float32)
                for j in np.nonzero(m.any(axis=0))[0]:
                    s[:, j] = score_column(orc, p1[i], f1[i], f2[i, j])
                mats.append(s)
        got = run_window(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC)
        refs = check_window(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, mats or [None] * 3)
        census = [tile_census(p1[i], p2[i], flags, SYMMETRIC, refs[i][2]) for i in range(3)]
        ntile = census[0][0]
        assert ntile == (260 if flags & FULL_TAIL else 259)
        assert census[0][1] == ntile and 2 <= census[1][1] <= 9 and 2 <= census[2][1] <= 9
        for i in range(3):
            m = refs[i][2]
            assert (m[:, :256 * 32].any() and m[:, 256 * 32:].any()) == (i == 0)
            assert m[:, 256 * 32:].any() == (i != 2)
            assert (got[i]["match"] >= 0).sum() >= 16


def test_scratch_reuse(surf, orc):
    """The scratch may hold anything: all-0xFF first, then the boxes and keys
    of another call (more points, stronger scores, other coordinates)."""
    nf, s1, s2 = 64, 160, 96
    rng = np.random.default_rng(56)
    f1 = rng.standard_normal((2, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((2, s2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    strong = (4.0 * f1).astype(np.float32)
    weak = np.ascontiguousarray(f1[:, ::-1])
    p1 = with_canary(make_points(rng, 2, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 2, s2, surf.POINT_DTYPE)
    for p in (p1, p2):
        p["x"] = rng.uniform(0, 120, p.shape)
        p["y"] = np.sort(rng.uniform(0, 300, p.shape), axis=1)
    q2 = p2.copy()
    q2["y"] = q2["y"][:, ::-1]                                    # the second call: other boxes, fewer tiles
    flags = FULL_TAIL | MUTUAL
    scratch = surf.DeviceBuffer(surf.match_batch_window_scratch_bytes(2, s1, s2, flags))
    scratch.upload(np.full(scratch.nbytes, 0xFF, np.uint8))
    runs = []
    for fa, b, c1, c2 in ((strong, p2, [s1, 150], [s2, 90]), (weak, q2, [150, s1], [60, 33]),
                          (weak, q2, [150, s1], [60, 33])):
        got = run_window(surf, p1, fa, c1, b, f2, c2, flags, SYMMETRIC, scratch=scratch)
        check_window(orc, got, p1, fa, c1, b, f2, c2, flags, SYMMETRIC, matrices(orc, p1, fa, c1, f2, c2))
        runs.append(got)
    scratch.free()
    assert runs[1].tobytes() == runs[2].tobytes()
    assert (runs[0]["match"][0] >= 0).sum() >= 4 and (runs[1]["match"][0, :150] >= 0).sum() >= 4


def test_position_independence(surf, orc):
    """One pair at positions 0, 5 and 11 of a batch of unrelated pairs, and
    over two runs: the same bits."""
    nf, src = 64, 10                                              # 159 x 192: two blocks
    rp1, rf1, rp2, rf2 = window_data(surf, nf)
    p1, f1, p2, f2 = rp1.copy(), rf1.copy(), rp2.copy(), rf2.copy()
    c1, c2 = list(COUNTS1), list(COUNTS2)
    where = (0, 5, 11)
    for k in where:
        p1[k], f1[k], p2[k], f2[k], c1[k], c2[k] = rp1[src], rf1[src], rp2[src], rf2[src], COUNTS1[src], COUNTS2[src]
    mats = ragged_matrices(surf, orc, nf)
    mats = [mats[src] if k in where else mats[k] for k in range(12)]
    for flags in (0, FULL_TAIL | SAME_LAPLACE | MUTUAL):
        got = run_window(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC)
        again = run_window(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC)
        assert got.tobytes() == again.tobytes(), flags
        for k in where[1:]:
            assert got[k].tobytes() == got[where[0]].tobytes(), (flags, k)
        check_window(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, mats)


def test_counts_are_clamped(surf, orc):
    nf, s1, s2 = 64, 70, 100
    rng = np.random.default_rng(45)
    f1 = rng.standard_normal((3, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((3, s2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 3, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, s2, surf.POINT_DTYPE)
    for p in (p1, p2):
        p["x"] = rng.uniform(0, 100, p.shape)
        p["y"] = np.sort(rng.uniform(0, 200, p.shape), axis=1)
    c1, c2 = [s1 + 9, 40, -3], [s2 + 9, -3, 64]
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
        got = run_window(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC)
        check_window(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, matrices(orc, p1, f1, c1, f2, c2))
        assert (got[0]["match"] >= 0).sum() >= 12                 # all 70 slots against all 100
        assert (got[1, :40]["match"] == -1).all()                 # n2 = 0
        assert (got[2]["match"] == CANARY["match"]).all()         # n1 = 0: nothing written


def test_detect_window_match_homography_without_host_round_trip(surf, orc):
    """detect_batch -> match_batch_window with MUTUAL of consecutive frames on
    the detector's own buffers (set 2 = set 1 advanced one frame) ->
    homography_batch, enqueued without reading anything back in between."""
    n, w, h, max_pts = 4, 640, 480, 1024
    win = (-48.0, 48.0, -48.0, 48.0)
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
    ob = surf.DeviceBuffer(64 * (n - 1))
    sb = surf.DeviceBuffer(surf.match_batch_window_scratch_bytes(n - 1, max_pts, max_pts, MUTUAL))
    pb.zero()
    set2 = (pb.ptr + 48 * max_pts, db.ptr + 4 * max_pts * nf, cb.ptr + 4, max_pts)
    det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.match_batch_window(pb.ptr, db.ptr, cb.ptr, max_pts, *set2, n - 1, nf, MUTUAL, win, sb.ptr)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob.ptr)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    assert counts.min() >= 64 and counts.max() <= max_pts
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    desc = db.download(np.float32, n * max_pts * nf).reshape(n, max_pts, nf)
    res = ob.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    for b in (fb, pb, db, cb, ob, sb):
        b.free()
    det.close()
    for i in range(n - 1):
        a, b = counts[i], counts[i + 1]
        p1, p2, f1, f2 = pts[i, :a], pts[i + 1, :b], desc[i, :a], desc[i + 1, :b]
        fwd, m = window_forward(orc, p1, p2, f1, f2, 0, win)
        ref = fwd.copy()
        for j in np.unique(fwd["match"][fwd["match"] >= 0]):      # B only where a forward match names the column
            col = np.where(m[:, j], score_column(orc, p1, f1, f2[j]), np.float32(0))
            rows = np.nonzero(fwd["match"] == j)[0]
            assert col.max() > 0 and (col[rows].view(np.uint32) == fwd["score"][rows].view(np.uint32)).all()
            lose = rows[rows != int(col.argmax())]
            ref["match"][lose] = -1
            ref["match_x"][lose] = 0.0
            ref["match_y"][lose] = 0.0
        assert_match_equal(pts[i, :a], ref, f"pair {i}: ")
        g = pts[i, :a]
        kept = g["match"] >= 0
        dx, dy = g["match_x"][kept] - g["x"][kept], g["match_y"][kept] - g["y"][kept]
        assert kept.sum() >= 16 and (np.abs(dx) <= 48).all() and (np.abs(dy) <= 48).all()
        assert (g["match_x"][kept] == p2["x"][g["match"][kept]]).all()
        unwindowed = orc.match(p1, p2, f1, f2, full_tail=False)
        print(f"pair {i}: {a} x {b}, kept {kept.sum()}, forward {int((fwd['match'] >= 0).sum())}, "
              f"other than unwindowed {int((unwindowed['match'] != fwd['match']).sum())}")
        assert (unwindowed["match"] != fwd["match"]).any()
        assert int(res[i]["ncand"]) == int((kept & (g["ambiguity"] <= np.float32(0.95))).sum())
