"""GPU tests of surfhip_match_batch_guided (batched matching inside a window
around each set-1 point's predicted position under a per-pair homography):
every comparison is bitwise on the five match fields.

The model needs no new oracle.  (u, v, W) of every set-1 point are computed
in numpy float32 with exactly the kernel's operations; a copy of the set-1
points with x, y replaced by u, v (NaN where W > 0 is false) goes to
window_model / window_forward of match_ref, which rest on
or_match alone.  Only the five match fields are compared with that model;
everything else is compared with the original upload."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from match_ref import (CANARY, COUNTS1, COUNTS2, EVERYWHERE, FULL_TAIL, INF, KEPT_FIELDS, MATCH_FIELDS, MUTUAL,
                       SAME_LAPLACE, SYMMETRIC, WINDOWS, assert_match_equal, box, clamp, make_points, matrices,
                       may_offer, offered_mask, ragged_data, ragged_matrices, ragged_plain, run_cross, run_guided,
                       run_window, score_column, small_batch, tile_census, window_data, window_forward, window_model,
                       with_canary)

pytestmark = pytest.mark.gpu

IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
TIGHT = (-8.0, 8.0, -8.0, 8.0)


# ------------------------------------------------------------------ model

def predict(p1, h):
    """(u, v, W) of the set-1 points under the row-major matrix h: float32,
    one rounding per written operation, u = v = NaN where W > 0 is false."""
    h = np.asarray(h, np.float32).reshape(9)
    x, y = p1["x"], p1["y"]
    with np.errstate(all="ignore"):
        X = (h[0] * x + h[1] * y) + h[2]
        Y = (h[3] * x + h[4] * y) + h[5]
        W = (h[6] * x + h[7] * y) + h[8]
        u, v = X / W, Y / W
    for a in (X, Y, W, u, v):
        assert a.dtype == np.float32
    front = W > 0
    nan = np.float32(np.nan)
    return np.where(front, u, nan), np.where(front, v, nan), W


def projected(p1, h):
    """The set-1 points with their predicted positions for coordinates."""
    q = p1.copy()
    q["x"], q["y"], _ = predict(p1, h)
    return q


def inverse_points(h, x, y):
    """The fp64 inverse map of (x, y) under h, rounded to fp32."""
    inv = np.linalg.inv(np.asarray(h, np.float32).astype(np.float64).reshape(3, 3))
    x, y = x.astype(np.float64), y.astype(np.float64)
    w = inv[2, 0] * x + inv[2, 1] * y + inv[2, 2]
    return (((inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]) / w).astype(np.float32),
            ((inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]) / w).astype(np.float32))


def similarity(deg, zoom, tx, ty):
    a, b = zoom * np.cos(np.radians(deg)), zoom * np.sin(np.radians(deg))
    return np.array([a, -b, tx, b, a, ty, 0, 0, 1], np.float32)


def pack_h(hs, stride):
    """The matrix argument as a flat float32 array: one matrix (stride 0),
    packed (9), inside 64-B homography records whose other fields hold junk,
    status = 2 included (16), or with other gaps of junk."""
    hs = np.asarray(hs, np.float32).reshape(-1, 9)
    if stride == 0:
        assert len(hs) == 1
        return hs.reshape(-1).copy()
    out = np.full((len(hs), stride), -3.0e38, np.float32)
    out[:, :9] = hs
    if stride == 16:
        out[:, 9:].view(np.int32)[:] = (2, -5, 123456, 0x7FC00000, -1, 0x7F800000, 77)   # status, ncand, ..., NaN, inf
    return out.reshape(-1)


# ---------------------------------------------------------------- running

def check_guided(orc, got, p1, f1, c1, p2, f2, c2, flags, win, mats, hs, fwds=None):
    """got against the model per pair (hs[i]: the pair's matrix) + the
    nothing-else-written properties against the upload.  Returns the per-pair
    (expected, forward, offered mask, projected set 1)."""
    s1, s2 = p1.shape[1], p2.shape[1]
    refs = []
    for i in range(len(p1)):
        n1, n2 = clamp(c1[i], s1), clamp(c2[i], s2)
        q = projected(p1[i, :n1], hs[i])
        ref, fwd, m = window_model(orc, mats[i], q, p2[i, :n2], f1[i, :n1], f2[i, :n2], flags, win,
                                   fwds[i] if fwds is not None else None)
        assert_match_equal(got[i, :n1], ref, f"flags {flags} window {win} pair {i} (n1 {n1}, n2 {n2}): ")
        for f in MATCH_FIELDS:                                    # slots at or past n1: untouched
            assert (got[i, n1:][f].view(np.uint32) == p1[i, n1:][f].view(np.uint32)).all(), (i, f)
        for f in KEPT_FIELDS:
            assert (got[i][f].view(np.uint32) == p1[i][f].view(np.uint32)).all(), (i, f)
        refs.append((ref, fwd, m, q))
    return refs


def assert_nothing(g):
    assert (g["match"] == -1).all()
    for f in ("score", "match_x", "match_y", "ambiguity"):
        assert (g[f].view(np.uint32) == 0).all(), f


# ----------------------------------------------------------- 1. identity

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["symmetric", "stereo"])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_identity_is_the_window_call(surf, nf, name, flags):
    """The identity at h_stride 0, 9 and 16 gives the bytes of
    match_batch_window, GPU to GPU, plain and with MUTUAL."""
    win = WINDOWS[name]
    p1, f1, p2, f2 = window_data(surf, nf)
    for fl in (flags, flags | MUTUAL):
        want = run_window(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, win)
        for stride in (0, 9, 16):
            hbuf = pack_h([IDENTITY] * (1 if stride == 0 else len(p1)), stride)
            got = run_guided(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, win, hbuf, stride)
            assert got.tobytes() == want.tobytes(), (fl, stride)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_identity_and_infinite_window(surf, nf, flags):
    """... and with the infinite window those of match_batch / match_batch_cross."""
    p1, f1, p2, f2 = ragged_data(surf, nf)
    for stride in (0, 16):
        hbuf = pack_h([IDENTITY] * (1 if stride == 0 else len(p1)), stride)
        got = run_guided(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, EVERYWHERE, hbuf, stride)
        mut = run_guided(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags | MUTUAL, EVERYWHERE, hbuf, stride)
        assert got.tobytes() == ragged_plain(surf, nf, flags).tobytes()
        assert mut.tobytes() == run_cross(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags).tobytes()


# ------------------------------------------- 2. ragged batch, a matrix per pair

KINDS = (np.array([1, 0, 37.5, 0, 1, -210, 0, 0, 1], np.float32),             # a pure translation
         similarity(5.0, 1.05, 20.0, -30.0),                                  # roll 5 degrees, zoom 1.05
         np.array([0, 1, 0, 1, 0, 0, 0, 0, 1], np.float32),                   # u = y, v = x
         np.array([1, 0.02, 5, -0.01, 1, -8, 1e-4, -2e-4, 1], np.float32))    # a mild perspective
RAGGED_H = [KINDS[i % 4] for i in range(len(COUNTS1))]


@functools.lru_cache(maxsize=None)
def guided_data(surf, nf):
    """window_data with the set-1 coordinates mapped back through each pair's
    matrix (fp64, rounded to fp32), so the predictions land where that data
    has partners."""
    wp1, f1, p2, f2 = window_data(surf, nf)
    p1 = wp1.copy()
    for i, h in enumerate(RAGGED_H):
        p1["x"][i], p1["y"][i] = inverse_points(h, wp1["x"][i], wp1["y"][i])
    p1.setflags(write=False)
    return p1, f1, p2, f2


@functools.lru_cache(maxsize=None)
def guided_forwards(surf, orc, nf, flags):
    """Per pair of guided_data: (forward points, offered mask) inside SYMMETRIC."""
    p1, f1, p2, f2 = guided_data(surf, nf)
    return [window_forward(orc, projected(p1[i, :n1], RAGGED_H[i]), p2[i, :n2], f1[i, :n1], f2[i, :n2], flags,
                           SYMMETRIC) for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2))]


def ragged_census(surf, orc, nf, flags):
    """What guided_data exercises, from the model alone: (points with nothing
    offered, (group, tile) combinations the box test on the predictions
    drops, partly offered ones, matches the window call on the raw
    coordinates cannot give, matches the next pair's matrix cannot give)."""
    p1, f1, p2, f2 = guided_data(surf, nf)
    fwds = guided_forwards(surf, orc, nf, flags)
    nothing = dropped = partial = not_raw = not_next = 0
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        a, b = p1[i, :n1], p2[i, :n2]
        fwd, m = fwds[i]
        q = projected(a, RAGGED_H[i])
        assert (predict(a, RAGGED_H[i])[2] > 0).all()             # W > 0 on all points
        nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
        if nscan:
            nothing += int((~m[:, :nscan].any(axis=1)).sum())
        for group in (128, 32):                                   # blocks and waves; asserts: none dropped that offers
            total, kept, part = tile_census(q, b, flags, SYMMETRIC, m, group)
            dropped += total - kept
            partial += part
        rows = np.nonzero(fwd["match"] >= 0)[0]
        cols = fwd["match"][rows]
        assert m[rows, cols].all()                                # every match lies in the window of its prediction
        raw = offered_mask(a, b, flags, SYMMETRIC)                # the window call: around (x1, y1)
        nxt = offered_mask(projected(a, RAGGED_H[(i + 1) % len(RAGGED_H)]), b, flags, SYMMETRIC)
        not_raw += int((~raw[rows, cols]).sum())
        not_next += int((~nxt[rows, cols]).sum())
    return nothing, dropped, partial, not_raw, not_next


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_ragged_batch_with_a_matrix_per_pair(surf, orc, nf, flags):
    """The ragged batch (empty sets, partial tiles, dead waves, two blocks,
    the any-length kernel) with a translation, a similarity, an axis swap and
    a perspective cycling over the pairs, at strides 9 and 16, plain and with
    MUTUAL."""
    p1, f1, p2, f2 = guided_data(surf, nf)
    mats = ragged_matrices(surf, orc, nf)                         # (the descriptors are those of ragged_data)
    fwds = guided_forwards(surf, orc, nf, flags)
    nothing, dropped, partial, not_raw, not_next = ragged_census(surf, orc, nf, flags)
    print(f"nf {nf} flags {flags}: nothing offered {nothing}, dropped (group, tile) {dropped}, partly offered "
          f"{partial}, matches outside the raw window {not_raw}, outside the next pair's prediction {not_next}")
    assert nothing >= 1 and dropped >= 1 and partial >= 1
    assert not_raw >= 1                                           # fails for a call that ignores d_h
    assert not_next >= 1                                          # fails for a wrong stride
    for stride in (9, 16):
        hbuf = pack_h(RAGGED_H, stride)
        for fl in (flags, flags | MUTUAL):
            got = run_guided(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, SYMMETRIC, hbuf, stride)
            check_guided(orc, got, p1, f1, COUNTS1, p2, f2, COUNTS2, fl, SYMMETRIC, mats, RAGGED_H, fwds)
            if fl & MUTUAL:
                for i, n1 in enumerate(COUNTS1):
                    kept = got[i, :n1]["match"][got[i, :n1]["match"] >= 0]
                    assert len(np.unique(kept)) == len(kept), f"pair {i}: the kept matches share partners"


# ------------------------------------------------------------------ 3. edges

def edge_pair(surf, seed=91):
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
    return rng, nf, n1, n2, p1, f1, p2, f2


def test_edges(surf, orc):
    """Dyadic coordinates and the matrix {2, 0, 0.5; 0, 2, -0.5; 0, 0, 2}
    (W = 2, u = x + 0.25, v = y - 0.25, every operation exact): inclusive
    bounds and their next floats around the prediction, NaN and infinite
    coordinates, a tile of NaN points, a stronger point outside the window
    ahead of the winner in its thread row."""
    rng, nf, n1, n2, p1, f1, p2, f2 = edge_pair(surf)
    h = np.array([2, 0, 0.5, 0, 2, -0.5, 0, 0, 2], np.float32)
    win = (-3.0, 5.0, -2.0, 7.0)
    p1["x"], p1["y"] = 99.75, 100.25                              # predicted at (100, 100)
    u, v, w = predict(p1[0], h)
    assert (u == 100).all() and (v == 100).all() and (w == 2).all()
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
        got = run_guided(surf, p1, f1, [n1], p2, f2, [n2], flags, win, pack_h([h], 9), 9)
        (ref, fwd, m, q), = check_guided(orc, got, p1, f1, [n1], p2, f2, [n2], flags, win, mats, [h])
        for k, (j, x, y, offered) in enumerate(edges):
            assert m[k, j] == offered, (k, j)
            assert (fwd["match"][k] == j) == offered, (k, j, fwd["match"][k])
        assert not m[:, 64:].any() and not m[20].any() and not m[21].any() and not m[22].any() and not m[23].any()
        assert_nothing(got[0, [20, 21, 22, 23]])
        assert not m[30, 40] and m[30, 43] and m[30, 12]
        assert fwd["match"][30] == 43 and fwd["score"][30] == mats[0][30, 43]
        assert abs(float(fwd["ambiguity"][30]) - 0.5) < 0.05      # the second is slot 12's half score, not slot 40
        assert got[0, 30]["match"] == 43


def test_w_zero_negative_and_positive(surf, orc):
    """h6 = 1/64, h8 = -1: set-1 points at W = 0 exactly, W < 0 and W > 0.
    The first two get -1 and zeros with the infinite window too; the third
    matches."""
    rng, nf, n1, n2, p1, f1, p2, f2 = edge_pair(surf, 92)
    h = np.array([1, 0, 0, 0, 1, 0, 1 / 64, 0, -1], np.float32)
    kind = np.arange(n1) % 3                                      # W = 0, -0.5, 1
    p1["x"][0] = np.array([64.0, 32.0, 128.0], np.float32)[kind]
    p1["y"][0] = 8.0 * np.arange(n1)
    u, v, w = predict(p1[0], h)
    assert (w[kind == 0] == 0).all() and (w[kind == 1] == -0.5).all() and (w[kind == 2] == 1).all()
    assert np.isnan(u[kind != 2]).all() and (u[kind == 2] == 128).all()
    assert (v[kind == 2] == p1["y"][0][kind == 2]).all()
    p2["x"][0] = 128.0 + rng.integers(-6, 7, n2)
    p2["y"][0] = 4.0 * np.arange(n2)
    for k in range(n1):                                           # everyone has an exact partner at its raw row
        f2[0, 2 * k] = f1[0, k]
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    for win in (EVERYWHERE, TIGHT):
        for flags in (FULL_TAIL, FULL_TAIL | MUTUAL, SAME_LAPLACE):
            got = run_guided(surf, p1, f1, [n1], p2, f2, [n2], flags, win, pack_h([h], 16), 16)
            (ref, fwd, m, q), = check_guided(orc, got, p1, f1, [n1], p2, f2, [n2], flags, win, mats, [h])
            assert not m[kind != 2].any() and m[kind == 2].any(axis=1).all()
            assert_nothing(got[0, :n1][kind != 2])
            assert (got[0, :n1]["match"][kind == 2] == 2 * np.nonzero(kind == 2)[0]).all()


def test_unusable_matrices_match_nothing(surf, orc):
    """A 4-pair batch: a matrix with a NaN, a good one, an all-zero one and one
    with +inf in h2.  The bad pairs' points match nothing; the good pair is
    the bytes of its own one-pair call."""
    rng, nf, n1, n2, ep1, ef1, ep2, ef2 = edge_pair(surf, 93)
    good = np.array([2, 0, 0.5, 0, 2, -0.5, 0, 0, 2], np.float32)
    nan_h = np.array(IDENTITY, np.float32)
    nan_h[4] = np.nan
    inf_h = np.array(IDENTITY, np.float32)
    inf_h[2] = INF
    hs = [nan_h, good, np.zeros(9, np.float32), inf_h]
    p1, f1, p2, f2 = (np.repeat(a, 4, axis=0) for a in (ep1, ef1, ep2, ef2))
    for p in (p1, p2):
        p["x"] = rng.integers(0, 64, p.shape)
        p["y"] = np.sort(rng.integers(0, 64, p.shape), axis=1)
    p1["x"] -= 0.25
    p1["y"] += 0.25
    f2[:, :n1] = f1                                               # partners for everybody, if offered
    p2["x"][:, :n1], p2["y"][:, :n1] = p1["x"] + 0.25, p1["y"] - 0.25
    c1, c2 = [n1] * 4, [n2] * 4
    mats = matrices(orc, p1, f1, c1, f2, c2)
    for win in (TIGHT, EVERYWHERE):
        for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
            for stride in (9, 16):
                got = run_guided(surf, p1, f1, c1, p2, f2, c2, flags, win, pack_h(hs, stride), stride)
                refs = check_guided(orc, got, p1, f1, c1, p2, f2, c2, flags, win, mats, hs)
                assert_nothing(got[0, :n1])
                assert_nothing(got[2, :n1])
                assert not refs[0][2].any() and not refs[2][2].any()
                if win is TIGHT:
                    assert_nothing(got[3, :n1])
                assert (got[1, :n1]["match"] >= 0).sum() >= n1 // 2
                alone = run_guided(surf, p1[1:2], f1[1:2], c1[:1], p2[1:2], f2[1:2], c2[:1], flags, win,
                                   pack_h([good], stride), stride)
                assert alone[0].tobytes() == got[1].tobytes()


# ------------------------------------------- 4. boxes are boxes of the predictions

def test_three_blocks_under_a_translation(surf, orc):
    """n1 = 300 against n2 = 320, both sorted by y, and a translation by +400
    rows: the planted exact partners of points of block 0 lie in a set-2 tile
    that the box of block 0's raw coordinates would drop; with MUTUAL the
    planted back best in another block clears the noisy copy."""
    nf, n1, n2 = 64, 300, 320
    h = np.array([1, 0, 0, 0, 1, 400, 0, 0, 1], np.float32)
    rng = np.random.default_rng(79)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p1["x"], p2["x"] = rng.uniform(0, 50, (1, n1)), rng.uniform(0, 50, (1, n2))
    p1["y"] = (np.arange(n1) * (1000.0 / n1)).astype(np.float32)
    p2["y"] = (np.arange(n2) * (1000.0 / n2)).astype(np.float32)
    # block 0's points 100 .. 109 (rows 333 .. 363, predicted at 733 .. 763) and their exact partners in tile 7
    for k in range(10):
        f2[0, 235 + k] = f1[0, 100 + k]
        p2["x"][0, 235 + k] = p1["x"][0, 100 + k]
        p2["laplace"][0, 235 + k] = p1["laplace"][0, 100 + k]
    # set-2 point 264 (row 825): its exact copy in block 1, a noisy copy in block 0
    j, exact, noisy = 264, 130, 125
    f1[0, exact] = f2[0, j]
    nv = f2[0, j] + 0.05 * rng.standard_normal(nf).astype(np.float32)
    f1[0, noisy] = nv / np.linalg.norm(nv)
    p1["x"][0, [exact, noisy]] = p2["x"][0, j]
    p1["laplace"][0, [exact, noisy]] = p2["laplace"][0, j]
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    raw_block0 = box(p1["x"][0, :128], p1["y"][0, :128])
    for flags in (0, FULL_TAIL | SAME_LAPLACE):
        got = run_guided(surf, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC, pack_h([h], 0), 0)
        (ref, fwd, m, q), = check_guided(orc, got, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC, mats, [h])
        for k in range(10):
            t = (235 + k) // 32
            assert fwd["match"][100 + k] == 235 + k and got[0, 100 + k]["match"] == 235 + k
            tile = box(p2["x"][0, 32 * t:][:32], p2["y"][0, 32 * t:][:32])
            assert not may_offer(raw_block0, tile, SYMMETRIC)     # the raw block box would drop the tile ...
            assert may_offer(box(q["x"][:128], q["y"][:128]), tile, SYMMETRIC)      # ... the predictions' keeps it
        total, kept, part = tile_census(q, p2[0], flags, SYMMETRIC, m)
        assert total == 30 and kept < 20 and part >= 3
        assert not m[200:].any()                                  # predicted below the last row: nothing offered
        assert_nothing(got[0, 200:n1])
        mut = run_guided(surf, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, SYMMETRIC, pack_h([h], 0), 0)
        check_guided(orc, mut, p1, f1, [n1], p2, f2, [n2], flags | MUTUAL, SYMMETRIC, mats, [h])
        assert fwd["match"][exact] == j and fwd["match"][noisy] == j and exact // 128 != noisy // 128
        assert mut[0, exact]["match"] == j and mut[0, noisy]["match"] == -1


# ------------------------------------------------------ 5. chunked tile list

def test_more_tiles_than_one_list_chunk(surf, orc):
    """n2 = 8300: 260 tiles, the kept-tile list is built in two chunks of 256
    tile boxes.  One wave is predicted near the first rows and one near the
    last, so the block's box covers everything and both chunks hold offered
    pairs."""
    nf, n1, n2 = 64, 64, 8300
    h = similarity(2.0, 1.03, 15.0, -25.0)
    rng = np.random.default_rng(124)
    f1 = rng.standard_normal((1, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    p2["x"] = rng.uniform(0, 100, (1, n2))
    p2["y"] = np.arange(n2, dtype=np.float32)[None, :]           # a tile: 32 rows
    tx = rng.uniform(0, 100, n1).astype(np.float32)
    ty = np.concatenate([rng.uniform(0, 150, 32), rng.uniform(8250, 8299, 32)]).astype(np.float32)
    p1["x"][0], p1["y"][0] = inverse_points(h, tx, ty)
    q = projected(p1[0], h)
    assert np.abs(q["x"] - tx).max() < 0.01 and np.abs(q["y"] - ty).max() < 0.01
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
        m = offered_mask(q, p2[0], flags, SYMMETRIC)
        s = np.zeros((n1, n2), np.float32)                        # the columns somebody is offered; 0 elsewhere
        if flags & MUTUAL:
            for j in np.nonzero(m.any(axis=0))[0]:
                s[:, j] = score_column(orc, p1[0], f1[0], f2[0, j])
        got = run_guided(surf, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC, pack_h([h], 9), 9)
        (ref, fwd, m2, _), = check_guided(orc, got, p1, f1, [n1], p2, f2, [n2], flags, SYMMETRIC, [s], [h])
        total, kept, part = tile_census(q, p2[0], flags, SYMMETRIC, m2)
        assert total == 260 and kept == 260                       # the block stages every tile, the waves skip most
        wave_total, wave_kept, _ = tile_census(q, p2[0], flags, SYMMETRIC, m2, 32)
        assert wave_total == 520 and wave_kept <= 24
        assert m2[:, :256 * 32].any() and m2[:, 256 * 32:].any()
        assert (got[0]["match"] >= 0).sum() >= 16


# ------------------------------------------------------------ 6. robustness

def test_scratch_full_of_ff(surf, orc):
    """The scratch may hold anything: all-0xFF first, then its own leftovers."""
    s1, s2 = 160, 96
    rng, p1, f1, p2, f2 = small_batch(surf, 57, 2, s1, s2)
    hs = [similarity(3.0, 0.97, 4.0, 9.0), KINDS[3]]
    for i in range(2):
        p1["x"][i], p1["y"][i] = inverse_points(hs[i], p1["x"][i], p1["y"][i])
    flags = FULL_TAIL | MUTUAL
    c1, c2 = [s1, 150], [s2, 90]
    scratch = surf.DeviceBuffer(surf.match_batch_guided_scratch_bytes(2, s1, s2, flags))
    scratch.upload(np.full(scratch.nbytes, 0xFF, np.uint8))
    mats = matrices(orc, p1, f1, c1, f2, c2)
    runs = []
    for _ in range(2):
        got = run_guided(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_h(hs, 9), 9, scratch=scratch)
        check_guided(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, mats, hs)
        runs.append(got)
    scratch.free()
    assert runs[0].tobytes() == runs[1].tobytes()
    assert (runs[0]["match"][0] >= 0).sum() >= 4


def test_position_independence(surf, orc):
    """The same pair and matrix at positions 0, 5 and 11 of a batch of
    unrelated pairs, and over two runs: the same bits."""
    nf, src = 64, 10                                              # 159 x 192: two blocks
    rp1, rf1, rp2, rf2 = guided_data(surf, nf)
    p1, f1, p2, f2 = rp1.copy(), rf1.copy(), rp2.copy(), rf2.copy()
    c1, c2, hs = list(COUNTS1), list(COUNTS2), list(RAGGED_H)
    where = (0, 5, 11)
    for k in where:
        p1[k], f1[k], p2[k], f2[k], c1[k], c2[k] = rp1[src], rf1[src], rp2[src], rf2[src], COUNTS1[src], COUNTS2[src]
        hs[k] = RAGGED_H[src]
    mats = ragged_matrices(surf, orc, nf)
    mats = [mats[src] if k in where else mats[k] for k in range(12)]
    for flags in (0, FULL_TAIL | SAME_LAPLACE | MUTUAL):
        got = run_guided(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_h(hs, 16), 16)
        again = run_guided(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_h(hs, 16), 16)
        assert got.tobytes() == again.tobytes(), flags
        for k in where[1:]:
            assert got[k].tobytes() == got[where[0]].tobytes(), (flags, k)
        check_guided(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, mats, hs)
        assert (got[where[0], :COUNTS1[src]]["match"] >= 0).sum() >= 4


def test_counts_are_clamped(surf, orc):
    s1, s2 = 70, 100
    rng, p1, f1, p2, f2 = small_batch(surf, 46, 3, s1, s2)
    hs = [KINDS[1], KINDS[3], KINDS[0]]
    for i in range(3):
        p1["x"][i], p1["y"][i] = inverse_points(hs[i], p1["x"][i], p1["y"][i])
    c1, c2 = [s1 + 9, 40, -3], [s2 + 9, -3, 64]
    for flags in (FULL_TAIL, FULL_TAIL | MUTUAL):
        got = run_guided(surf, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, pack_h(hs, 9), 9)
        check_guided(orc, got, p1, f1, c1, p2, f2, c2, flags, SYMMETRIC, matrices(orc, p1, f1, c1, f2, c2), hs)
        assert (got[0]["match"] >= 0).sum() >= 12                 # all 70 slots against all 100
        assert (got[1, :40]["match"] == -1).all()                 # n2 = 0
        assert (got[2]["match"] == CANARY["match"]).all()         # n1 = 0: nothing written


def test_consecutive_frames_overlap(surf, orc):
    """Set 2 = set 1 advanced one frame in the same buffers (nframes 4,
    npairs 3): only match fields of set-1 points are written, only x, y,
    laplace of set 2 are read."""
    nf, n, slots = 64, 4, 96
    rng, pts, desc, _, _ = small_batch(surf, 47, n, slots, 32)
    counts = np.array([96, 70, 64, 33], np.int32)
    hs = [KINDS[1], similarity(-2.0, 1.02, -6.0, 11.0), KINDS[3]]
    for i in reversed(range(n - 1)):                              # frame i: where frame i + 1's points come from
        pts["x"][i], pts["y"][i] = inverse_points(hs[i], pts["x"][i + 1], pts["y"][i + 1])
        desc[i, :64] = desc[i + 1, :64] + 0.03 * rng.standard_normal((64, nf)).astype(np.float32)
    for flags in (0, FULL_TAIL | SAME_LAPLACE | MUTUAL):
        pb = surf.DeviceBuffer(pts.nbytes)
        db = surf.DeviceBuffer(desc.nbytes)
        cb = surf.DeviceBuffer(counts.nbytes)
        hb = surf.DeviceBuffer(4 * 9 * (n - 1))
        sb = surf.DeviceBuffer(surf.match_batch_guided_scratch_bytes(n - 1, slots, slots, flags))
        for b, a in ((pb, pts), (db, desc), (cb, counts), (hb, pack_h(hs, 9))):
            b.upload(a)
        surf.match_batch_guided(pb.ptr, db.ptr, cb.ptr, slots, pb.ptr + 48 * slots, db.ptr + 4 * slots * nf, cb.ptr + 4,
                                slots, n - 1, nf, flags, hb.ptr, 9, SYMMETRIC, sb.ptr)
        surf.synchronize()
        got = pb.download(surf.POINT_DTYPE, n * slots).reshape(n, slots)
        assert db.download(np.float32, desc.size).tobytes() == desc.tobytes()
        for b in (pb, db, cb, hb, sb):
            b.free()
        assert got[n - 1].tobytes() == pts[n - 1].tobytes()       # the last frame is set 2 only
        mats = matrices(orc, pts[:-1], desc[:-1], counts[:-1], desc[1:], counts[1:])
        check_guided(orc, got[:-1], pts[:-1], desc[:-1], counts[:-1], pts[1:], desc[1:], counts[1:], flags, SYMMETRIC,
                     mats, hs)
        assert min((got[i, :counts[i]]["match"] >= 0).sum() for i in range(n - 1)) >= 8


# ------------------------------------------------------ 7. no host round trip

def moved_frame(img, deg, tx, ty):
    """img's content rolled by deg about the centre and shifted by (tx, ty):
    bilinear, edge pixels repeated."""
    hh, ww = img.shape
    y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    dx, dy = x - tx - ww / 2, y - ty - hh / 2                     # the source position of every output pixel
    sx = np.clip(c * dx + s * dy + ww / 2, 0, ww - 1)
    sy = np.clip(-s * dx + c * dy + hh / 2, 0, hh - 1)
    x0, y0 = np.minimum(sx.astype(int), ww - 2), np.minimum(sy.astype(int), hh - 2)
    fx, fy = sx - x0, sy - y0
    a = img.astype(np.float64)
    out = ((1 - fy) * ((1 - fx) * a[y0, x0] + fx * a[y0, x0 + 1])
           + fy * ((1 - fx) * a[y0 + 1, x0] + fx * a[y0 + 1, x0 + 1]))
    return np.rint(out).astype(np.uint8)


def test_detect_match_homography_guided_without_host_round_trip(surf, orc):
    """A synthetic frame and the same content shifted and slightly rolled:
    detect_batch -> match_batch_window (MUTUAL) -> homography_batch ->
    match_batch_guided (MUTUAL) reading the homography records where they lie,
    at h_stride 16 -> homography_batch, on the detector's own buffers (set 2 =
    set 1 advanced one frame), enqueued with one synchronise at the end."""
    n, w, h, max_pts = 2, 640, 480, 1024
    wide, tight = (-48.0, 48.0, -48.0, 48.0), TIGHT
    frames = surf.synth_frames(n, w, h).copy()
    frames[1, :, :w] = moved_frame(frames[0, :, :w], 1.5, 12.0, -7.0)
    pitch = frames.shape[2]
    param = surf.make_param(4, 4.0, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    det = surf.Detector(param, w, h, max_batch=n, max_pts=max_pts)
    fb = surf.DeviceBuffer(frames.nbytes)
    fb.upload(frames)
    pb = surf.DeviceBuffer(48 * n * max_pts)
    db = surf.DeviceBuffer(4 * n * max_pts * nf)
    cb = surf.DeviceBuffer(4 * n)
    ob1 = surf.DeviceBuffer(64 * (n - 1))
    ob2 = surf.DeviceBuffer(64 * (n - 1))
    sb = surf.DeviceBuffer(surf.match_batch_guided_scratch_bytes(n - 1, max_pts, max_pts, MUTUAL))
    pb.zero()
    sets = (pb.ptr, db.ptr, cb.ptr, max_pts, pb.ptr + 48 * max_pts, db.ptr + 4 * max_pts * nf, cb.ptr + 4, max_pts)
    det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.match_batch_window(*sets, n - 1, nf, MUTUAL, wide, sb.ptr)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob1.ptr)
    surf.match_batch_guided(*sets, n - 1, nf, MUTUAL, ob1.ptr, 16, tight, sb.ptr)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob2.ptr)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    assert counts.min() >= 64 and counts.max() <= max_pts
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    desc = db.download(np.float32, n * max_pts * nf).reshape(n, max_pts, nf)
    first = ob1.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    second = ob2.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    for b in (fb, pb, db, cb, ob1, ob2, sb):
        b.free()
    det.close()
    for i in range(n - 1):
        a, b = counts[i], counts[i + 1]
        p1, p2, f1, f2 = pts[i, :a], pts[i + 1, :b], desc[i, :a], desc[i + 1, :b]
        q = projected(p1, first[i]["h"])                          # the model, with the downloaded matrix
        fwd, m = window_forward(orc, q, p2, f1, f2, 0, tight)
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
        dx, dy = g["match_x"][kept] - q["x"][kept], g["match_y"][kept] - q["y"][kept]
        assert kept.sum() >= 16 and (np.abs(dx) <= 8).all() and (np.abs(dy) <= 8).all()
        assert (g["match_x"][kept] == p2["x"][g["match"][kept]]).all()
        assert len(np.unique(g["match"][kept])) == kept.sum()     # injective
        print(f"pair {i}: {a} x {b}, first pass status {first[i]['status']} ninliers {first[i]['ninliers']} "
              f"rms {first[i]['rms']:.4f}; guided kept {kept.sum()}, second pass status {second[i]['status']} "
              f"ninliers {second[i]['ninliers']} rms {second[i]['rms']:.4f}")
        assert int(second[i]["ncand"]) == int((kept & (g["ambiguity"] <= np.float32(0.95))).sum())
