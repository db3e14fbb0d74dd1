"""What the GPU tests of the batched match calls share (surfhip_match_batch,
_cross, _window, _guided): the ragged batch and its cached derivatives, the
runners, and the host models built from the CPU oracle's or_match alone.  Not a
test module."""
from __future__ import annotations

import functools

import numpy as np

MATCH_FIELDS = ("score", "match", "match_x", "match_y", "ambiguity")
KEPT_FIELDS = ("x", "y", "scale", "o", "strength", "laplace", "ori")
CANARY = {"score": np.float32(-77.5), "match": np.int32(-12345), "match_x": np.float32(3.0e30),
          "match_y": np.float32(-4.0e30), "ambiguity": np.float32(55.25)}
FULL_TAIL, SAME_LAPLACE, MUTUAL = 1, 2, 4
COUNTS1 = (0, 1, 31, 32, 33, 63, 64, 65, 97, 128, 159, 160)
COUNTS2 = (100, 0, 31, 32, 33, 64, 65, 95, 96, 191, 192, 7)
SLOTS1, SLOTS2 = 160, 192
INF = float("inf")
EVERYWHERE = (-INF, INF, -INF, INF)
SYMMETRIC = (-40.0, 40.0, -40.0, 40.0)
STEREO = (-64.0, 0.0, -1.5, 1.5)
WINDOWS = {"symmetric": SYMMETRIC, "stereo": STEREO}


def assert_match_equal(got, ref, what=""):
    for f in MATCH_FIELDS:
        g, r = got[f], ref[f]
        if g.dtype == np.float32:
            g, r = g.view(np.uint32), r.view(np.uint32)
        bad = np.nonzero(g != r)[0]
        assert len(bad) == 0, f"{what}{f} differs at {bad[:5]}: {got[f][bad[:5]]} vs {ref[f][bad[:5]]}"


def with_canary(pts):
    out = pts.copy()
    for f, v in CANARY.items():
        out[f] = v
    return out


def make_points(rng, npairs, slots, dtype):
    p = np.zeros((npairs, slots), dtype)
    p["x"] = rng.uniform(0, 1920, (npairs, slots))
    p["y"] = rng.uniform(0, 1080, (npairs, slots))
    p["scale"] = rng.uniform(1, 9, (npairs, slots))
    p["strength"] = rng.uniform(4, 900, (npairs, slots))
    p["laplace"] = rng.choice(np.array([-1, 1], np.int32), (npairs, slots))
    return p


def clamp(c, slots):
    return min(max(int(c), 0), slots)


def run_batch(surf, p1, f1, c1, p2, f2, c2, flags=0):
    """Upload [npairs][slots] arrays, one surfhip_match_batch call; returns
    the downloaded (pts1, desc1, desc2)."""
    npairs, s1 = p1.shape
    s2 = p2.shape[1]
    nf = f1.shape[2]
    bufs = []
    for a in (p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32)):
        b = surf.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
    surf.match_batch(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, s2, npairs,
                     nf, flags)
    surf.synchronize()
    got = bufs[0].download(surf.POINT_DTYPE, npairs * s1).reshape(npairs, s1)
    d1 = bufs[1].download(np.float32, f1.size).reshape(f1.shape)
    d2 = bufs[4].download(np.float32, f2.size).reshape(f2.shape)
    for b in bufs:
        b.free()
    return got, d1, d2


def run_cross(surf, p1, f1, c1, p2, f2, c2, flags=0, scratch=None, plain=False):
    """Upload [npairs][slots] arrays, one call (match_batch_cross, or
    match_batch with plain); returns the downloaded set-1 points after the
    checks that neither descriptor array nor set 2 changed."""
    npairs, s1 = p1.shape
    s2 = p2.shape[1]
    nf = f1.shape[2]
    bufs = []
    for a in (p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32)):
        b = surf.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
    args = (bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, s2, npairs, nf)
    if plain:
        surf.match_batch(*args, flags)
    else:
        own = scratch is None
        if own:
            scratch = surf.DeviceBuffer(surf.match_batch_cross_scratch_bytes(npairs, s1, s2))
        assert scratch.nbytes >= surf.match_batch_cross_scratch_bytes(npairs, s1, s2)
        surf.match_batch_cross(*args, scratch.ptr, flags)
    surf.synchronize()
    got = bufs[0].download(surf.POINT_DTYPE, npairs * s1).reshape(npairs, s1)
    assert bufs[1].download(np.float32, f1.size).tobytes() == f1.tobytes()
    assert bufs[4].download(np.float32, f2.size).tobytes() == f2.tobytes()
    assert bufs[3].download(surf.POINT_DTYPE, npairs * s2).tobytes() == p2.tobytes()
    for b in bufs:
        b.free()
    if not plain and own:
        scratch.free()
    return got


def run_window(surf, p1, f1, c1, p2, f2, c2, flags, win, scratch=None):
    """Upload [npairs][slots] arrays, one match_batch_window call; returns the
    downloaded set-1 points after the checks that neither descriptor array
    nor set 2 changed."""
    npairs, s1 = p1.shape
    s2 = p2.shape[1]
    nf = f1.shape[2]
    bufs = []
    for a in (p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32)):
        b = surf.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
    own = scratch is None
    need = surf.match_batch_window_scratch_bytes(npairs, s1, s2, flags)
    if own:
        scratch = surf.DeviceBuffer(need)
    assert scratch.nbytes >= need
    surf.match_batch_window(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, s2,
                            npairs, nf, flags, win, scratch.ptr)
    surf.synchronize()
    got = bufs[0].download(surf.POINT_DTYPE, npairs * s1).reshape(npairs, s1)
    assert bufs[1].download(np.float32, f1.size).tobytes() == f1.tobytes()
    assert bufs[4].download(np.float32, f2.size).tobytes() == f2.tobytes()
    assert bufs[3].download(surf.POINT_DTYPE, npairs * s2).tobytes() == p2.tobytes()
    for b in bufs:
        b.free()
    if own:
        scratch.free()
    return got


def run_guided(surf, p1, f1, c1, p2, f2, c2, flags, win, hbuf, stride, scratch=None):
    """Upload [npairs][slots] arrays and the matrices, one match_batch_guided
    call; returns the downloaded set-1 points after the checks that neither
    descriptor array, nor set 2, nor the matrices changed."""
    npairs, s1 = p1.shape
    s2 = p2.shape[1]
    nf = f1.shape[2]
    hbuf = np.ascontiguousarray(hbuf, np.float32)
    bufs = []
    for a in (p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32), hbuf):
        b = surf.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
    own = scratch is None
    need = surf.match_batch_guided_scratch_bytes(npairs, s1, s2, flags)
    assert need == surf.match_batch_window_scratch_bytes(npairs, s1, s2, flags)
    if own:
        scratch = surf.DeviceBuffer(need)
    assert scratch.nbytes >= need
    surf.match_batch_guided(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, s2,
                            npairs, nf, flags, bufs[6].ptr, stride, win, scratch.ptr)
    surf.synchronize()
    got = bufs[0].download(surf.POINT_DTYPE, npairs * s1).reshape(npairs, s1)
    assert bufs[1].download(np.float32, f1.size).tobytes() == f1.tobytes()
    assert bufs[4].download(np.float32, f2.size).tobytes() == f2.tobytes()
    assert bufs[3].download(surf.POINT_DTYPE, npairs * s2).tobytes() == p2.tobytes()
    assert bufs[6].download(np.float32, hbuf.size).tobytes() == hbuf.tobytes()
    for b in bufs:
        b.free()
    if own:
        scratch.free()
    return got


def score_column(orc, p1, f1, f2row):
    """S(p1, j) for every p1 against the one set-2 descriptor f2row, where
    positive (0 elsewhere, NaN scores included)."""
    zero = np.zeros(1, p1.dtype)
    return orc.match(p1, zero, f1, f2row[None], full_tail=True)["score"]


def score_matrix(orc, p1, f1, f2):
    s = np.zeros((len(p1), len(f2)), np.float32)
    for j in range(len(f2)):
        s[:, j] = score_column(orc, p1, f1, f2[j])
    return s


def forward_ref(orc, p1, p2, f1, f2, flags):
    full = bool(flags & FULL_TAIL)
    if not flags & SAME_LAPLACE:
        return orc.match(p1, p2, f1, f2, full_tail=full)
    ref = p1.copy()
    for v in np.unique(p1["laplace"]):
        fz = f2.copy()
        fz[p2["laplace"] != v] = 0.0
        rows = p1["laplace"] == v
        ref[rows] = orc.match(p1, p2, f1, fz, full_tail=full)[rows]
    return ref


def back_best(s, p1, p2, flags):
    """B(p2) for p2 < nscan from the score matrix s[n1][>= nscan]."""
    n2 = len(p2)
    nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
    m = s[:, :nscan].copy()
    if flags & SAME_LAPLACE:
        m[p1["laplace"][:, None] != p2["laplace"][None, :nscan]] = 0.0
    if m.shape[0] == 0 or nscan == 0:
        return np.full(nscan, -1, np.int64)
    return np.where(m.max(axis=0) > 0, m.argmax(axis=0), -1)


def cross_model(orc, s, p1, p2, f1, f2, flags):
    """(expected points, forward points) of one pair; s: its score matrix."""
    fwd = forward_ref(orc, p1, p2, f1, f2, flags)
    b = back_best(s, p1, p2, flags)
    m = fwd["match"]
    hit = m >= 0
    rows = np.nonzero(hit)[0]
    # the model agrees with itself: a forward score is the matrix entry, bitwise
    assert (fwd["score"][rows].view(np.uint32) == s[rows, m[rows]].view(np.uint32)).all()
    clear = hit.copy()
    clear[rows] = b[m[rows]] != rows
    out = fwd.copy()
    out["match"][clear] = -1
    out["match_x"][clear] = 0.0
    out["match_y"][clear] = 0.0
    return out, fwd


def matrices(orc, p1, f1, c1, f2, c2):
    s1, s2 = p1.shape[1], f2.shape[1]
    return [score_matrix(orc, p1[i, :clamp(c1[i], s1)], f1[i, :clamp(c1[i], s1)], f2[i, :clamp(c2[i], s2)])
            for i in range(len(p1))]


def offered_mask(p1, p2, flags, win):
    """[n1][n2]: set-2 point p2 is offered to set-1 point p1 (the scan limit
    nscan apart, which or_match applies itself)."""
    w = np.asarray(win, np.float32)
    with np.errstate(invalid="ignore"):
        dx = p2["x"][None, :] - p1["x"][:, None]                  # one fp32 subtraction each
        dy = p2["y"][None, :] - p1["y"][:, None]
        m = (dx >= w[0]) & (dx <= w[1]) & (dy >= w[2]) & (dy <= w[3])
    assert dx.dtype == np.float32
    if flags & SAME_LAPLACE:
        m &= p1["laplace"][:, None] == p2["laplace"][None, :]
    return m


def window_forward(orc, p1, p2, f1, f2, flags, win):
    """(forward points, offered mask) of one pair."""
    m = offered_mask(p1, p2, flags, win)
    ref = p1.copy()
    if len(p1) == 0:
        return ref, m
    groups, inv = np.unique(m, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for g in range(len(groups)):
        fz = f2.copy()
        fz[~groups[g]] = 0.0
        rows = inv == g
        ref[rows] = orc.match(p1[rows], p2, f1[rows], fz, full_tail=bool(flags & FULL_TAIL))
    return ref, m


def window_model(orc, s, p1, p2, f1, f2, flags, win, known=None):
    """(expected points, forward points, offered mask) of one pair; s: its
    score matrix (needed with MUTUAL only); known: its window_forward result
    where there is one already."""
    fwd, m = known if known is not None else window_forward(orc, p1, p2, f1, f2, flags, win)
    if not flags & MUTUAL:
        return fwd, fwd, m
    n2 = len(p2)
    nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
    ms = np.where(m[:, :nscan], s[:, :nscan], np.float32(0))
    if ms.shape[0] == 0 or nscan == 0:
        b = np.full(nscan, -1, np.int64)
    else:
        b = np.where(ms.max(axis=0) > 0, ms.argmax(axis=0), -1)
    hit = fwd["match"] >= 0
    rows = np.nonzero(hit)[0]
    cols = fwd["match"][rows]
    assert m[rows, cols].all()                                    # a match is an offered point ...
    assert (fwd["score"][rows].view(np.uint32) == s[rows, cols].view(np.uint32)).all()   # ... with the matrix's score
    clear = hit.copy()
    clear[rows] = b[cols] != rows
    out = fwd.copy()
    out["match"][clear] = -1
    out["match_x"][clear] = 0.0
    out["match_y"][clear] = 0.0
    return out, fwd, m


def box(x, y):
    """(xmin, xmax, ymin, ymax), NaN ignored; of nothing: (inf, -inf, inf, -inf)."""
    return (np.fmin.reduce(x, initial=np.float32(INF)), np.fmax.reduce(x, initial=np.float32(-INF)),
            np.fmin.reduce(y, initial=np.float32(INF)), np.fmax.reduce(y, initial=np.float32(-INF)))


def may_offer(a, b, win):
    """The conservative fp32 box test: may a point of box a (set 1) be
    offered a point of box b (set 2)?"""
    w = np.asarray(win, np.float32)
    with np.errstate(invalid="ignore"):
        return bool(not b[0] - a[1] > w[1] and not b[1] - a[0] < w[0] and not b[2] - a[3] > w[3]
                    and not b[3] - a[2] < w[2])


def tile_census(p1, p2, flags, win, m, group=128):
    """Over the (group of set-1 points, set-2 tile) combinations of one pair:
    (combinations, kept by the box test, kept with some but not all pairs
    offered).  Asserts the box test's promise: a dropped one offers nothing."""
    n2 = len(p2)
    nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
    total = kept = partial = 0
    for g0 in range(0, len(p1), group):
        a = box(p1["x"][g0:g0 + group], p1["y"][g0:g0 + group])
        for t0 in range(0, nscan, 32):
            t1 = min(t0 + 32, nscan)
            sub = m[g0:g0 + group, t0:t1]
            keep = may_offer(a, box(p2["x"][t0:t1], p2["y"][t0:t1]), win)
            assert keep or not sub.any()
            total += 1
            kept += keep
            partial += bool(keep and sub.any() and not sub.all())
    return total, kept, partial


@functools.lru_cache(maxsize=None)
def ragged_data(surf, nf):
    """Case 2's batch: random normalised descriptors with a planted perfect
    partner per pair; slots past the counts hold large descriptors that would
    win every scan if they were read as points."""
    rng = np.random.default_rng(1000 + nf)
    npairs = len(COUNTS1)
    f1 = rng.standard_normal((npairs, SLOTS1, nf)).astype(np.float32)
    f2 = rng.standard_normal((npairs, SLOTS2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        if n1 and n2:
            f2[i, n2 // 2] = f1[i, 0]                             # a perfect partner (ties across rows)
        f1[i, n1:] = 1000.0
        f2[i, n2:] = 1000.0
    p1 = with_canary(make_points(rng, npairs, SLOTS1, surf.POINT_DTYPE))
    p2 = make_points(rng, npairs, SLOTS2, surf.POINT_DTYPE)
    for a in (f1, f2, p1, p2):
        a.setflags(write=False)
    return p1, f1, p2, f2


def small_batch(surf, seed, npairs, s1, s2, nf=64):
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((npairs, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((npairs, s2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    p1 = with_canary(make_points(rng, npairs, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, npairs, s2, surf.POINT_DTYPE)
    for p in (p1, p2):
        p["x"] = rng.uniform(0, 120, p.shape)
        p["y"] = np.sort(rng.uniform(0, 300, p.shape), axis=1)
    return rng, p1, f1, p2, f2


@functools.lru_cache(maxsize=None)
def ragged_matrices(surf, orc, nf):
    p1, f1, p2, f2 = ragged_data(surf, nf)
    return matrices(orc, p1, f1, COUNTS1, f2, COUNTS2)


@functools.lru_cache(maxsize=None)
def ragged_plain(surf, nf, flags):
    p1, f1, p2, f2 = ragged_data(surf, nf)
    return run_cross(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, plain=True)


@functools.lru_cache(maxsize=None)
def window_data(surf, nf):
    """The ragged batch of test_gpu_match_batch with coordinates for windows:
    set 2 sorted by y inside every pair (32 consecutive points: a band of
    about 100 rows), set 1 sorted in the even pairs and in random order in the
    odd ones (a block of those covers everything: nothing to skip)."""
    rp1, f1, rp2, f2 = ragged_data(surf, nf)
    rng = np.random.default_rng(2000 + nf)
    p1, p2 = rp1.copy(), rp2.copy()
    for p, slots in ((p1, SLOTS1), (p2, SLOTS2)):
        p["x"] = rng.uniform(0, 160, (len(p), slots)).astype(np.float32)
        p["y"] = np.sort(np.round(rng.uniform(0, 600, (len(p), slots)) * 2) / 2, axis=1).astype(np.float32)
    for i in range(1, len(p1), 2):
        p1["y"][i] = p1["y"][i][rng.permutation(SLOTS1)]
    for a in (p1, p2):
        a.setflags(write=False)
    return p1, f1, p2, f2
