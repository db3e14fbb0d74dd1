"""What the tests of surfhip_match_batch_epipolar share: the fp32 numpy model
of "offered" (window around the raw point + band along its epipolar line),
the forward and MUTUAL models over a given mask (or_match alone, through
match_ref), the numpy twin of the kernels' line-against-box test with its
census, matrices, and the runner.  Not a test module."""
from __future__ import annotations

import numpy as np

from match_ref import FULL_TAIL, box, may_offer, offered_mask, window_model

RECTIFIED = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)       # a = 0, b = -1, c = y1: r = -(y2 - y1)
ZERO = np.zeros(9, np.float32)                                       # what a failed fundamental record holds
K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1.0]])


def rot(rx, ry, rz):
    """Rotation by rx, ry, rz degrees about x, then y, then z."""
    a, b, c = np.radians([rx, ry, rz])
    mx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    my = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    mz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return mz @ my @ mx


def cross_matrix(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def pose_f(r, t, k=K):
    """The fundamental matrix of camera 2 seeing X2 = r X1 + t, both cameras
    with the intrinsics k: (x2, y2, 1) F (x1, y1, 1)^T = 0, Frobenius norm 1,
    rounded to fp32."""
    ki = np.linalg.inv(k)
    f = ki.T @ cross_matrix(t) @ r @ ki
    return (f / np.linalg.norm(f)).astype(np.float32).reshape(9)


def translation_f(tx, ty):
    """F of a pure image-plane translation direction (tx, ty): every epipolar
    line passes through its own point, along (tx, ty).  Exact in fp32 for
    dyadic tx, ty."""
    return np.array([0, 0, ty, 0, 0, -tx, -ty, tx, 0], np.float32)


# ------------------------------------------------------------------ model

def epipolar_lines(p1, f, band):
    """(a, b, c, lim) of every set-1 point: float32, one rounding per written
    operation, in the kernel's order."""
    f = np.asarray(f, np.float32).reshape(9)
    x, y = p1["x"], p1["y"]
    bb = np.float32(band) * np.float32(band)
    with np.errstate(all="ignore"):
        a = (f[0] * x + f[1] * y) + f[2]
        b = (f[3] * x + f[4] * y) + f[5]
        c = (f[6] * x + f[7] * y) + f[8]
        lim = bb * (a * a + b * b)
    for v in (a, b, c, lim):
        assert v.dtype == np.float32
    return a, b, c, lim


def epipolar_mask(p1, p2, flags, win, f, band):
    """[n1][n2]: set-2 point p2 is offered to set-1 point p1 (the scan limit
    nscan apart, which or_match applies itself): same laplace with
    SAME_LAPLACE, the window around the raw (x1, y1), and r r <= lim."""
    a, b, c, lim = epipolar_lines(p1, f, band)
    with np.errstate(all="ignore"):
        r = (p2["x"][None, :] * a[:, None] + p2["y"][None, :] * b[:, None]) + c[:, None]
        inband = r * r <= lim[:, None]                                # NaN: False
    assert r.dtype == np.float32
    return offered_mask(p1, p2, flags, win) & inband


def mask_forward(orc, p1, p2, f1, f2, flags, m):
    """The forward points of one pair under the offered mask m (the shape of
    match_ref.window_forward): per group of set-1 points with the same row of
    m, or_match against set 2 with the descriptors that are not offered
    zeroed."""
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


def epipolar_model(orc, s, p1, p2, f1, f2, flags, win, f, band, known=None):
    """(expected points, forward points, offered mask) of one pair; s: its
    score matrix (needed with MUTUAL only); known: its (forward, mask) where
    there is one already.  The MUTUAL clearing is match_ref.window_model's over
    this mask."""
    if known is None:
        known = mask_forward(orc, p1, p2, f1, f2, flags, epipolar_mask(p1, p2, flags, win, f, band))
    return window_model(orc, s, p1, p2, f1, f2, flags, win, known)


# --------------------------------------------------------- line against box

def line_may_offer(a, b, c, lim, bx):
    """The kernels' conservative test, for arrays of lines against one box
    (xmin, xmax, ymin, ymax): r at the four corners with r's own expression;
    False only when all four lie on one side of 0 with r r > lim.  A NaN
    corner or lim fails its comparisons: True."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        xa0, xa1, yb0, yb1 = f32(bx[0]) * a, f32(bx[1]) * a, f32(bx[2]) * b, f32(bx[3]) * b
        rs = [(xa0 + yb0) + c, (xa1 + yb0) + c, (xa0 + yb1) + c, (xa1 + yb1) + c]
        far = np.logical_and.reduce([r * r > lim for r in rs])
        above = np.logical_and.reduce([r > 0 for r in rs])
        below = np.logical_and.reduce([r < 0 for r in rs])
    assert rs[0].dtype == np.float32
    return ~(far & (above | below))


def epipolar_census(p1, p2, flags, win, f, band, m, group=128):
    """Over the (group of set-1 points, set-2 tile) combinations of one pair:
    (combinations, kept by the box test and the line test, kept with some but
    not all pairs offered).  Asserts the promise of both tests: a dropped one
    offers nothing."""
    n2 = len(p2)
    nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
    a, b, c, lim = epipolar_lines(p1, f, band)
    total = kept = partial = 0
    for g0 in range(0, len(p1), group):
        g = slice(g0, g0 + group)
        gbox = box(p1["x"][g], p1["y"][g])
        for t0 in range(0, nscan, 32):
            t1 = min(t0 + 32, nscan)
            sub = m[g, t0:t1]
            tb = box(p2["x"][t0:t1], p2["y"][t0:t1])
            keep = may_offer(gbox, tb, win) and bool(line_may_offer(a[g], b[g], c[g], lim[g], tb).any())
            assert keep or not sub.any(), (g0, t0)
            total += 1
            kept += keep
            partial += bool(keep and sub.any() and not sub.all())
    return total, kept, partial


# ---------------------------------------------------------------- running

def pack_f(fs, stride):
    """The matrix argument as a flat float32 array: one matrix (stride 0),
    packed (9), inside 64-B fundamental records whose other fields hold junk,
    status = 2 included (16), or with other gaps of junk."""
    fs = np.asarray(fs, np.float32).reshape(-1, 9)
    if stride == 0:
        assert len(fs) == 1
        return fs.reshape(-1).copy()
    out = np.full((len(fs), stride), -3.0e38, np.float32)
    out[:, :9] = fs
    if stride == 16:
        out[:, 9:].view(np.int32)[:] = (2, -5, 123456, 0x7FC00000, -1, 0x7F800000, 77)   # status, ncand, ..., NaN, inf
    return out.reshape(-1)


def run_epipolar(surf, p1, f1, c1, p2, f2, c2, flags, win, fbuf, stride, band, scratch=None):
    """Upload [npairs][slots] arrays and the matrices, one
    match_batch_epipolar call; returns the downloaded set-1 points after the
    checks that neither descriptor array, nor set 2, nor the matrices
    changed."""
    npairs, s1 = p1.shape
    s2 = p2.shape[1]
    nf = f1.shape[2]
    fbuf = np.ascontiguousarray(fbuf, np.float32)
    bufs = []
    for a in (p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32), fbuf):
        b = surf.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
    own = scratch is None
    need = surf.match_batch_epipolar_scratch_bytes(npairs, s1, s2, flags)
    assert need == surf.match_batch_window_scratch_bytes(npairs, s1, s2, flags)
    if own:
        scratch = surf.DeviceBuffer(need)
    assert scratch.nbytes >= need
    surf.match_batch_epipolar(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s1, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, s2,
                              npairs, nf, flags, bufs[6].ptr, stride, band, win, scratch.ptr)
    surf.synchronize()
    got = bufs[0].download(surf.POINT_DTYPE, npairs * s1).reshape(npairs, s1)
    assert bufs[1].download(np.float32, f1.size).tobytes() == f1.tobytes()
    assert bufs[4].download(np.float32, f2.size).tobytes() == f2.tobytes()
    assert bufs[3].download(surf.POINT_DTYPE, npairs * s2).tobytes() == p2.tobytes()
    assert bufs[6].download(np.float32, fbuf.size).tobytes() == fbuf.tobytes()
    for b in bufs:
        b.free()
    if own:
        scratch.free()
    return got

