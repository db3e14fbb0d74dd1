"""The describe kernels on planted keypoints, path by path.

`surfhip_run_describe` hands the describe stage a point list, so these tests
choose each keypoint's position, scale, border distance and queue neighbours
instead of taking whatever `detect_batch` finds.  `geometry()` restates the
public per-keypoint formulas of `or_describe` / `k_worklist` (step, hs,
iradius, side, cs, W4, the border tests) and `classes()` names the code path
each planted keypoint takes in k_describe_u2 / k_describe_ur; every test
first asserts that the classes it names are populated, so it cannot pass
without the path it names.  Reference: `or_orientation` / `or_describe` of
the CPU oracle on the same integral image; bar: `ori` bit for bit,
descriptors within DESC_TOL L2 (the project's existing bar).

Frames are 256 x 192 (pitch 256).  Keypoint scales stay within what the
detector's octaves can emit: makePoint's scale is 1.2 ns divisor with ns =
(init_lobe + (octave - 1) max_scale + 2 octave (s + off)) / 3, 1 <= s <=
max_scale - 2, |off| <= 1.5 (the fit's limit), i.e. `scale_bounds()`: 0.8 ..
44 for 4 octaves, .. 88.8 for 5 (x 0.5 doubled, 6 octaves: .. 89.2).  The
random points use 1.6 .. 24; the few-rows / one-column points need windows
about as large as the frame, up to scale 58 (5 octaves; doubled: 6).
`worklist_fits` (step < 2^10, hs < 2^12, iradius < 2^10) holds for all of
them, and side = 2 iradius + 1 <= 45 <= 64 lanes.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import desc_l2
from test_gpu_parity import DESC_TOL, _extreme_frame, took

pytestmark = pytest.mark.gpu

W, H, PITCH = 256, 192, 256
MAX_PTS = 2048
F32 = np.float32
KINDS = ("noise", "hbands", "vbands", "checker")
DROP_CAP = 0.05            # non-finite oracle results dropped per frame kind, at most
# 1.65f * scale == 5, 9, 13, 17, 21 exactly in fp32 (hs = 2 step + 1); doubled: 3.3f * scale == 5, 9
HALF_SCALES = (3.0303030014038086, 5.454545497894287, 7.878787994384766, 10.303030014038086, 12.727272987365723)
HALF_SCALES_DOUBLED = (1.5151515007019043, 2.7272727489471436)
# launch_describe: 2,048 persistent workgroups of 4 waves, 8 XCDs x kDescQ = 16 queues
DESC_GRID_WAVES, DESC_XCDS, DESC_Q = 2048 * 4, 8, 16
CANARY_U8 = 0xA7


def scale_bounds(noct, doubled=False, init_lobe=3, max_scale=5):
    """The scales makePoint can emit (see the module docstring)."""
    octave = 1 << (noct - 1)
    div = 0.5 if doubled else 1.0
    lo = 1.2 * (init_lobe + 2.0 * (1 - 1.5)) / 3.0 * div
    hi = 1.2 * (init_lobe + (octave - 1) * max_scale + 2.0 * octave * (max_scale - 2 + 1.5)) / 3.0 * div
    return lo, hi


def test_half_way_scales_are_exact():
    for s, want in zip(HALF_SCALES, (5, 9, 13, 17, 21)):
        assert F32(1.65) * F32(s) == F32(want)
    for s, want in zip(HALF_SCALES_DOUBLED, (5, 9)):
        assert F32(3.3) * F32(s) == F32(want)


# ------------------------------------------------------------ classifier

def geometry(pts, wi, hi, doubled=False, wsz=4, rotated=False):
    """Per-keypoint window geometry on a wi x hi frame (the frame the integral is taken of: doubled
    2w - 2 x 2h - 2), with the float operations of or_describe / k_worklist."""
    sc = pts["scale"].astype(F32)
    x, y = pts["x"].astype(F32), pts["y"].astype(F32)
    if doubled:
        S, x, y = F32(3.3) * sc, x + x, y + y
    else:
        S = F32(1.65) * sc
    step = np.maximum(np.rint(S * F32(0.5)).astype(np.int64), 1)
    hs = S.astype(np.int64)
    ix, iy = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    spacing = S * F32(12 // wsz)
    reach = F32(1.4) * spacing if rotated else spacing
    iradius = np.rint(((reach * F32(wsz + 1)) * F32(0.5)) / step.astype(F32)).astype(np.int64)
    side = 2 * iradius + 1
    cs = (ix + (-2 - iradius) * step) & ~3
    w4 = (ix + (side + 1 - iradius) * step + 2 - cs + 3) >> 2
    g = dict(S=S, step=step, hs=hs, ix=ix, iy=iy, iradius=iradius, side=side, cs=cs, w4=w4, hmode=hs - 2 * step,
             fx=x - ix.astype(F32), fy=y - iy.astype(F32), spacing=spacing)
    # the upright grid is separable: grid row / column t is valid when it is inside the window
    # (rx in (-1, wsz)) and its Haar boxes are inside the integral image
    t = np.arange(64)[None, :]
    si = t - iradius[:, None]
    wofs, fw = F32(wsz) * F32(0.5) - F32(0.5), F32(wsz)
    for ax, frac, centre, lim in (("r", g["fy"], iy, hi + 1), ("c", g["fx"], ix, wi + 1)):
        pos = ((step[:, None] * si).astype(F32) - frac[:, None]) / spacing[:, None]
        rx = pos + wofs
        inwin = (t < side[:, None]) & (rx > -1) & (rx < fw)
        r = centre[:, None] + si * step[:, None]
        low, high = r < 1 + hs[:, None], r >= lim - 1 - hs[:, None]
        g["n" + ax] = (inwin & ~low & ~high).sum(1)
        g[ax + "_low"], g[ax + "_high"] = (inwin & low).any(1), (inwin & high).any(1)
    # rotated windows: the square of half-width 2.5 spacing turned by any angle contains the grid
    # samples of its centre row / column up to 2.4 spacing, so these are clipped whatever `ori` is
    far = np.floor(F32(2.4) * spacing / step.astype(F32)).astype(np.int64) * step
    g["rot_top"], g["rot_bottom"] = iy - far < 1 + hs, iy + far >= hi - hs
    g["rot_left"], g["rot_right"] = ix - far < 1 + hs, ix + far >= wi - hs
    # assignOrientationApprox: the 19 x 19 samples at pixsi2 apart, boxes of +-pixsi; the samples at
    # (0, +-9), (+-9, 0) are inside its radius (81 < 81.5)
    so = sc + sc if doubled else sc
    pixsi, pixsi2 = (F32(2) * so + F32(1.6)).astype(np.int64), (so + F32(0.8)).astype(np.int64)
    g["ori_top"], g["ori_bottom"] = iy - 9 * pixsi2 - pixsi <= -1, iy + 9 * pixsi2 + pixsi + 2 >= hi + 1
    g["ori_left"], g["ori_right"] = ix - 9 * pixsi2 - pixsi <= -1, ix + 9 * pixsi2 + pixsi + 2 >= wi + 1
    return g


def classes(pts, wi, hi, doubled=False):
    """Boolean masks of the code-path classes of the upright wsz-4 kernels."""
    g = geometry(pts, wi, hi, doubled)
    step, hm, w4, side = g["step"], g["hmode"], g["w4"], g["side"]
    share = (hm == 0) | (hm == -1)
    ring = share & (w4 <= 32) & (step <= 3)                      # k_describe_u2's LDS-DMA ring
    dual = side <= 32
    c = {"mode_2step": hm == 0, "mode_2step-1": hm == -1, "mode_half": hm == 1,
         "sparse_4to7": share & ~ring & (step >= 4) & (step <= 7), "sparse_ge8": share & ~ring & (step >= 8),
         "span_le16": w4 <= 16, "span_17to32": (w4 >= 17) & (w4 <= 32), "span_gt32": w4 > 32,
         "waves_dual": dual, "waves_single": ~dual,
         # k_describe_ur's staged-segment path (step <= 3, its 448-word row buffer large enough)
         "ur_seg": share & (step <= 3) & (2 * np.where(dual, 2, 1) * w4 <= 128)
                   & (2 * np.where(dual, 2, 1) * 4 * w4 <= 448)}
    for s in (1, 2, 3):
        c[f"ring_step{s}"] = ring & (step == s)
        for k in range(4):
            c[f"ring_step{s}_ix{k}"] = ring & (step == s) & (g["ix"] % 4 == k)
    x, y = pts["x"].astype(F32), pts["y"].astype(F32)
    if doubled:
        x, y = x + x, y + y
    fx, fy = x - np.floor(x), y - np.floor(y)
    c["pos_integer"] = (fx == 0) & (fy == 0)
    half = (fx == 0.5) & (fy == 0.5)
    c["pos_half_even"] = half & (np.floor(x) % 2 == 0) & (np.floor(y) % 2 == 0)
    c["pos_half_odd"] = half & (np.floor(x) % 2 == 1) & (np.floor(y) % 2 == 1)
    c["pos_generic"] = (fx != 0) & (fx != 0.5) & (fy != 0) & (fy != 0.5)
    top, bottom, left, right = g["r_low"], g["r_high"], g["c_low"], g["c_high"]
    some = (g["nr"] > 0) & (g["nc"] > 0)
    c["clip_none"] = ~(top | bottom | left | right)
    c["clip_top"], c["clip_bottom"] = top & ~bottom & some, bottom & ~top & some
    c["clip_left"], c["clip_right"] = left & ~right & some, right & ~left & some
    c["clip_top_left"], c["clip_top_right"] = top & left & some, top & right & some
    c["clip_bottom_left"], c["clip_bottom_right"] = bottom & left & some, bottom & right & some
    c["clip_top_and_bottom"], c["clip_left_and_right"] = top & bottom & some, left & right & some
    for k in (1, 2, 3):
        c[f"rows_{k}"] = (g["nr"] == k) & (g["nc"] > 0)
    c["cols_1"] = (g["nc"] == 1) & (g["nr"] > 0)
    c["heavy_clip"] = some & ((g["nr"] <= 3) | (g["nc"] <= 3) | (top & bottom) | (left & right))
    c["ring_narrow"], c["ring_wide"] = ring & (w4 <= 16), ring & (w4 > 16)
    c["sparse"] = share & ~ring
    return c


UPRIGHT_CLASSES = (["mode_2step", "mode_2step-1", "mode_half", "sparse_4to7", "sparse_ge8", "span_le16",
                    "span_17to32", "span_gt32", "waves_dual", "waves_single", "pos_integer", "pos_half_even",
                    "pos_half_odd", "pos_generic", "clip_none", "clip_top", "clip_bottom", "clip_left", "clip_right",
                    "clip_top_left", "clip_top_right", "clip_bottom_left", "clip_bottom_right",
                    "clip_top_and_bottom", "clip_left_and_right", "rows_1", "rows_2", "rows_3", "cols_1"]
                   + [f"ring_step{s}" for s in (1, 2, 3)]
                   + [f"ring_step{s}_ix{k}" for s in (1, 2, 3) for k in range(4)])


def need(name):
    return 2 if name == "mode_half" else 8


# ------------------------------------------------------------ planted set

def pts_dtype():
    from conftest import load_surf_amd
    return load_surf_amd().POINT_DTYPE


def make_points(x, y, scale, doubled=False):
    """Points at (x, y, scale) of the integral's frame (doubled: the caller's frame is half of it).  The
    other fields are filled so that a kernel writing one of them shows."""
    n = len(x)
    p = np.zeros(n, pts_dtype())
    div = F32(0.5) if doubled else F32(1)
    p["x"], p["y"], p["scale"] = F32(x) * div, F32(y) * div, F32(scale) * div
    p["o"], p["strength"], p["laplace"] = 3, 17.25, -1
    p["ori"], p["score"], p["match"] = 123.5, 0.375, 77
    p["match_x"], p["match_y"], p["ambiguity"] = 5.5, 6.5, 0.625
    return p


def planted_set(wi, hi, doubled=False, few=True, seed=1):
    """MAX_PTS keypoints on a wi x hi frame: the special cases named in `classes`, then random ones
    (uniform position, log-uniform scale 1.6 .. 24).  few: with the few-rows / one-column windows, whose
    scales (up to 0.5 hi / 1.65) need the detector's fifth (doubled: sixth) octave."""
    rng = np.random.default_rng(seed)
    xs, ys, ss = [], [], []

    def add(x, y, s):
        x, y, s = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(s, np.float64))
        xs.append(x.ravel()); ys.append(y.ravel()); ss.append(s.ravel())

    cx, cy = wi / 2.0, hi / 2.0
    half = [2 * s for s in HALF_SCALES_DOUBLED] if doubled else list(HALF_SCALES)
    # (doubled: scale / 2 is exact, so 3.3f * (2 s / 2) is the half-way product again)
    near = [(cx + 0.3, cy + 0.7), (cx, cy), (cx + 0.5, cy + 1.5), (3.2, cy), (wi - 3.6, cy), (cx, 2.7), (cx, hi - 3.1),
            (2.0, 3.0), (wi - 2.5, 2.5), (4.4, hi - 3.0), (wi - 4.0, hi - 2.2), (cx + 1.25, cy - 2.75)]
    for s in half:
        for (x, y) in near:
            add(x, y, s)
    # positions: integers, exact .5 with even / odd integer parts
    n = 64
    sc = np.exp(rng.uniform(np.log(1.6), np.log(24.0), 3 * n))
    add(rng.integers(0, wi, n), rng.integers(0, hi, n), sc[:n])
    add(2 * rng.integers(0, wi // 2, n) + 0.5, 2 * rng.integers(0, hi // 2, n) + 0.5, sc[n:2 * n])
    add(2 * rng.integers(0, wi // 2 - 1, n) + 1.5, 2 * rng.integers(0, hi // 2 - 1, n) + 1.5, sc[2 * n:])
    # borders and corners, at scales of every row class
    for s in (1.7, 2.1, 2.6, 3.3, 4.1, 5.2, 6.6, 9.0, 14.0, 20.0):
        for d in (0.0, 2.3, 5.5):
            add([d, wi - 1 - d, cx + d, cx - d], [cy - d, cy + d, d, hi - 1 - d], s)
            add([d, wi - 1 - d, d + 0.4, wi - 1.2 - d], [d + 0.6, d, hi - 1 - d, hi - 1.7 - d], s)
    # windows larger than the frame (7.5 S > hi / 2, > wi / 2)
    for s in (hi / 14.0, hi / 12.0, wi / 14.0, wi / 11.0, wi / 9.0):
        add(cx + rng.uniform(-6, 6, 6), cy + rng.uniform(-6, 6, 6), s)
    if few:
        # 1, 2, 3 valid grid rows, one valid column: windows about as large as the frame, found with
        # the classifier among candidate scales and positions
        for names, S_lo, S_hi, lim in ((("rows_1", "rows_2", "rows_3"), 0.30 * hi, 0.497 * hi, hi),
                                       (("cols_1",), 0.485 * hi, 0.497 * hi, wi)):
            S = np.repeat(np.linspace(S_lo, S_hi, 160), 64)
            if names[0] == "cols_1":
                cand = make_points(rng.uniform(0, wi - 1, S.size), cy + rng.uniform(-2, 2, S.size), S / 1.65, doubled)
            else:
                cand = make_points(cx + rng.uniform(-9, 9, S.size), rng.uniform(0, hi - 1, S.size), S / 1.65, doubled)
            c = classes(cand, wi, hi, doubled)
            for nm in names:
                idx = np.nonzero(c[nm])[0]
                idx = idx[rng.permutation(len(idx))[:12]]
                k = 2.0 if doubled else 1.0
                add(cand["x"][idx] * k, cand["y"][idx] * k, cand["scale"][idx] * k)
    have = sum(len(a) for a in xs)
    assert have < MAX_PTS - 900, have
    m = MAX_PTS - have
    add(rng.uniform(0, wi - 1, m), rng.uniform(0, hi - 1, m), np.exp(rng.uniform(np.log(1.6), np.log(24.0), m)))
    p = make_points(np.concatenate(xs), np.concatenate(ys), np.concatenate(ss), doubled)
    return p[rng.permutation(MAX_PTS)]


def image(kind, seed=5, w=W, h=H, pitch=PITCH):
    if kind == "noise" and seed != 5:
        f = np.zeros((h, pitch), np.uint8)
        f[:, :w] = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
        return f
    return _extreme_frame(kind, w, h, pitch)


_REF = {}


def oracle_ref(orc, key, img, pts, doubled=False, **par):
    """(ori, desc, finite) of the oracle for `pts` on `img`, computed once per key."""
    k = (key, doubled, tuple(sorted(par.items())))
    if k not in _REF:
        p = orc.make_param(4, 4.0, doubled=doubled, **par)
        g, _ = orc.geometry(p, W, H)
        ii = orc.integral(orc.double_image(img, W, H), 2 * W - 2, 2 * H - 2) if doubled else orc.integral(img, W, H)
        with np.errstate(all="ignore"):
            ori, desc = orc.describe_points(p, g, ii, pts)
        fin = np.isfinite(ori) & np.isfinite(desc).all(axis=1)
        _REF[k] = (ori, desc, fin)
    return _REF[k]


def build_batch(orc, base, keys, imgs, perm_seeds, doubled=False, orders=None, **par):
    """Per frame: the planted set in its own order, a point whose oracle result is not finite on that
    frame's pixels replaced by the set's first finite generic one; the oracle's (ori, desc) alongside.
    Returns (pts[n, MAX_PTS], ori, desc, dropped per image key)."""
    n = len(keys)
    pts = np.zeros((n, MAX_PTS), base.dtype)
    ori = np.zeros((n, MAX_PTS), F32)
    desc = None
    dropped = {}
    wi, hi = (2 * W - 2, 2 * H - 2) if doubled else (W, H)
    generic = classes(base, wi, hi, doubled)
    generic = generic["pos_generic"] & generic["clip_none"]
    for f, key in enumerate(keys):
        o, d, fin = oracle_ref(orc, key, imgs[key], base, doubled, **par)
        dropped[key] = int((~fin).sum())
        filler = int(np.nonzero(fin & generic)[0][0])
        src = np.where(fin, np.arange(MAX_PTS), filler)
        order = orders[f] if orders is not None else np.random.default_rng(perm_seeds[f]).permutation(MAX_PTS)
        src = src[order]
        pts[f], ori[f] = base[src], o[src]
        if desc is None:
            desc = np.zeros((n, MAX_PTS, d.shape[1]), F32)
        desc[f] = d[src]
    return pts, ori, desc, dropped


def assert_drop_cap(dropped):
    print("dropped non-finite per frame kind (of %d, cap %d):" % (MAX_PTS, int(DROP_CAP * MAX_PTS)), dropped)
    for key, k in dropped.items():
        assert k <= DROP_CAP * MAX_PTS, (key, k)


# ------------------------------------------------------------ GPU side

class Planted:
    """A detector with a resident integral of `frames`, and canary-guarded point / descriptor / count
    buffers for run_describe."""

    TAIL = 4096

    def __init__(self, surf, param, frames, max_batch=None, via_detect=False):
        self.surf, self.n = surf, frames.shape[0]
        self.nf = param.nfeatures
        self.det = surf.Detector(param, W, H, max_batch=max_batch or self.n, max_pts=MAX_PTS)
        self.fb = surf.DeviceBuffer(frames.nbytes)
        self.fb.upload(frames)
        self.resident = False
        self.frames, self.via_detect = frames, via_detect

    def make_resident(self):
        surf, n = self.surf, self.n
        if self.via_detect:
            pb, db, cb = surf.DeviceBuffer(48 * n * MAX_PTS), surf.DeviceBuffer(4 * n * MAX_PTS * self.nf), \
                surf.DeviceBuffer(4 * n)
            self.det.detect_batch(self.fb.ptr, n, PITCH, H * PITCH, pb.ptr, db.ptr, cb.ptr)
            surf.synchronize()
        else:
            self.det.run_integral(self.fb.ptr, n, PITCH, H * PITCH)
        self.resident = True

    def switches(self):
        return {"switches": self.det.switches()}

    def run(self, pts, counts, rotated):
        """run_describe of pts[n, MAX_PTS] with the given counts; checks containment (test 5 of the
        issue) and returns (points, desc) of the device afterwards."""
        surf, n, nf = self.surf, self.n, self.nf
        if not self.resident:
            self.make_resident()
        counts = np.asarray(counts, np.int32)
        eff = np.clip(counts, 0, MAX_PTS)
        T = self.TAIL
        h_pts = np.full(48 * n * MAX_PTS + T, CANARY_U8, np.uint8)
        slots = h_pts[:48 * n * MAX_PTS].view(pts.dtype).reshape(n, MAX_PTS)
        for f in range(n):
            slots[f, :eff[f]] = pts[f, :eff[f]]
        h_desc = np.full(4 * n * MAX_PTS * nf + T, CANARY_U8, np.uint8)
        h_cnt = np.full(4 * n + T, CANARY_U8, np.uint8)
        h_cnt[:4 * n].view(np.int32)[:] = counts
        pb, db, cb = surf.DeviceBuffer(h_pts.nbytes), surf.DeviceBuffer(h_desc.nbytes), surf.DeviceBuffer(h_cnt.nbytes)
        pb.upload(h_pts)
        db.upload(h_desc)
        cb.upload(h_cnt)
        self.det.run_describe(pb.ptr, cb.ptr, n, db.ptr)
        surf.synchronize()
        g_pts, g_desc, g_cnt = pb.download(np.uint8, h_pts.nbytes), db.download(np.uint8, h_desc.nbytes), \
            cb.download(np.uint8, h_cnt.nbytes)
        for b in (pb, db, cb):
            b.free()
        # containment: counts and tails untouched; slots at or past the count untouched; described
        # points byte-identical to their input but for `ori` of a rotated detector
        assert g_cnt.tobytes() == h_cnt.tobytes(), "counts buffer changed"
        assert (g_pts[-T:] == CANARY_U8).all() and (g_desc[-T:] == CANARY_U8).all(), "canary tail changed"
        gp = g_pts[:-T].view(pts.dtype).reshape(n, MAX_PTS)
        gd = g_desc[:-T].view(F32).reshape(n, MAX_PTS, nf)
        hp = h_pts[:-T].view(pts.dtype).reshape(n, MAX_PTS)
        for f in range(n):
            k = eff[f]
            assert gp[f, k:].tobytes() == hp[f, k:].tobytes(), f"frame {f}: point slots past the count changed"
            assert (gd[f, k:].view(np.uint8) == CANARY_U8).all(), f"frame {f}: descriptors past the count changed"
            a, b = gp[f, :k].copy(), hp[f, :k].copy()
            if rotated:
                a["ori"], b["ori"] = 0, 0
            assert a.tobytes() == b.tobytes(), f"frame {f}: a described point's other fields changed"
            assert not (gd[f, :k].view(np.uint8) == CANARY_U8).all(axis=1).any(), f"frame {f}: a slot was not described"
        return gp, gd, eff

    def close(self):
        self.det.close()
        self.fb.free()


def check_batch(tag, got_pts, got_desc, eff, pts, ori, desc, masks, names, rotated):
    """Every described slot against the oracle; prints the largest L2 error per class, then asserts."""
    n = len(eff)
    live = np.arange(MAX_PTS)[None, :] < eff[:, None]
    err = np.zeros((n, MAX_PTS))
    for f in range(n):
        err[f, :eff[f]] = desc_l2(got_desc[f, :eff[f]], desc[f, :eff[f]])
    assert np.isfinite(err).all(), f"{tag}: non-finite descriptor at {np.argwhere(~np.isfinite(err))[:4]}"
    print(f"{tag}: {int(live.sum())} keypoints, max descriptor L2 {err.max():.3g}")
    for nm in names:
        m = masks[nm] & live
        print(f"  {nm:22s} n={int(m.sum()):6d}  max L2 {err[m].max() if m.any() else float('nan'):.3g}")
    if rotated:
        same = (got_pts["ori"].view(np.uint32) == ori.view(np.uint32)) | ~live
        assert same.all(), f"{tag}: ori differs at {np.argwhere(~same)[:4]}"
    worst = np.unravel_index(err.argmax(), err.shape)
    assert err.max() <= DESC_TOL, f"{tag}: descriptor L2 {err.max():.3g} at frame/slot {worst}: {pts[worst]}"


def populated(masks, eff, names):
    live = np.arange(MAX_PTS)[None, :] < np.asarray(eff)[:, None]
    for nm in names:
        k = int((masks[nm] & live).sum())
        assert k >= need(nm), f"class {nm} holds {k} keypoints"


def batch_classes(pts, doubled=False):
    wi, hi = (2 * W - 2, 2 * H - 2) if doubled else (W, H)
    per = [classes(pts[f], wi, hi, doubled) for f in range(pts.shape[0])]
    return {k: np.stack([c[k] for c in per]) for k in per[0]}


def with_env(monkeypatch, env):
    for kv in filter(None, env.split(",")):
        name, _, val = kv.partition("=")
        monkeypatch.setenv(name, val)


# 1 ------------------------------------------------------------ upright paths

COUNTS_12 = [MAX_PTS, 0, 1, MAX_PTS - 1, MAX_PTS, 1500, 777, MAX_PTS + 9, -3, 64, MAX_PTS, 2000]


@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("env", ["SURFHIP_DESC_UR=0", "SURFHIP_DESC_UR=1"])
def test_upright_paths(surf, orc, monkeypatch, env, extend):
    """k_describe_u2<extend> (SURFHIP_DESC_UR=0) and k_describe_ur<extend> (=1) on every class of
    UPRIGHT_CLASSES: 12 frames (ten on one noise image, one checker, one other noise, so a kernel
    reading another frame's integral fails), each the planted set in its own permutation, ragged
    counts (0, 1, max_pts - 1, max_pts, and counts to clamp)."""
    with_env(monkeypatch, env)
    keys = ["noise"] * 12
    keys[4], keys[9] = "checker", "noise2"
    imgs = {"noise": image("noise"), "checker": image("checker"), "noise2": image("noise", seed=11)}
    base = planted_set(W, H)
    lo, hi = scale_bounds(5)
    assert lo <= base["scale"].min() and base["scale"].max() <= hi
    pts, ori, desc, dropped = build_batch(orc, base, keys, imgs, list(range(100, 112)), upright=True, extend=extend)
    assert_drop_cap(dropped)
    masks = batch_classes(pts)
    eff = np.clip(COUNTS_12, 0, MAX_PTS)
    populated(masks, eff, UPRIGHT_CLASSES + ["ur_seg"])
    frames = np.stack([imgs[k] for k in keys])
    run = Planted(surf, surf.make_param(5, 4.0, upright=True, extend=extend), frames)
    assert took(run.switches(), env), run.switches()
    gp, gd, eff = run.run(pts, COUNTS_12, rotated=False)
    run.close()
    check_batch(f"{env} extend={int(extend)}", gp, gd, eff, pts, ori, desc, masks, UPRIGHT_CLASSES + ["ur_seg"], False)


# 2 ------------------------------------------------------------ several keypoints per wave

PAIR_CLASSES = ("ring_narrow", "ring_wide", "sparse", "mode_half", "heavy_clip")


def euler_cycle(k):
    """A cyclic sequence over range(k) in which every ordered pair (a, b), a == b included, is adjacent
    once: an Euler circuit of the complete digraph with loops (Hierholzer)."""
    nxt = {a: list(range(k)) for a in range(k)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            out.append(stack.pop())
    return out[::-1][:-1]


@pytest.mark.parametrize("extend", [False, True])
def test_keypoints_back_to_back(surf, orc, monkeypatch, extend):
    """16 x 2,048 keypoints on 8,192 persistent waves: waves describe keypoints back to back (the ring
    is refilled while the previous keypoint's reduction rows are live).  A wave's keypoints come from
    one queue -- every DESC_Q-th keypoint of its XCD's contiguous eighth of the batch -- so the set is
    ordered such that along every queue all ordered pairs of PAIR_CLASSES are adjacent.  Two runs must
    be byte-identical."""
    with_env(monkeypatch, "SURFHIP_DESC_UR=0")
    n = 16
    total = n * MAX_PTS
    assert total > 2 * DESC_GRID_WAVES and total % (DESC_XCDS * DESC_Q) == 0
    keys = ["noise"] * n
    keys[3], keys[12] = "checker", "noise2"
    imgs = {"noise": image("noise"), "checker": image("checker"), "noise2": image("noise", seed=11)}
    base = planted_set(W, H)
    bc = classes(base, W, H)
    # one label per keypoint: the first four classes are disjoint, heavy_clip (last) overrides them
    label = np.full(MAX_PTS, -1)
    for i, nm in enumerate(PAIR_CLASSES):
        label[bc[nm]] = i
    pools = [np.nonzero(label == i)[0] for i in range(len(PAIR_CLASSES))]
    assert all(len(p) >= need(nm) for p, nm in zip(pools, PAIR_CLASSES)), [len(p) for p in pools]
    cyc = euler_cycle(len(PAIR_CLASSES))
    # batch index k = queue position (k // DESC_Q) within its XCD chunk, queue k % DESC_Q
    k = np.arange(total)
    want = np.array(cyc)[(k % (total // DESC_XCDS)) // DESC_Q % len(cyc)]
    rng = np.random.default_rng(3)
    flat = np.array([pools[c][rng.integers(len(pools[c]))] for c in want])
    orders = flat.reshape(n, MAX_PTS)
    pts, ori, desc, dropped = build_batch(orc, base, keys, imgs, None, orders=orders, upright=True, extend=extend)
    assert_drop_cap(dropped)
    masks = batch_classes(pts)
    # the adjacency the docstring claims, from the classes of the points actually uploaded
    lab = np.full(total, -1)
    for i, nm in enumerate(PAIR_CLASSES):
        lab[masks[nm].ravel()] = i
    chunk = total // DESC_XCDS
    for xcd in (0, DESC_XCDS - 1):
        for q in (0, DESC_Q - 1):
            seq = lab[xcd * chunk + q:(xcd + 1) * chunk:DESC_Q]
            pairs = set(zip(seq[:-1], seq[1:]))
            # (a replaced non-finite point may break single pairs; each pair occurs ~10 times)
            assert {(a, b) for a in range(5) for b in range(5)} <= pairs, (xcd, q)
    eff = np.full(n, MAX_PTS)
    populated(masks, eff, PAIR_CLASSES)
    frames = np.stack([imgs[kk] for kk in keys])
    run = Planted(surf, surf.make_param(5, 4.0, upright=True, extend=extend), frames)
    assert took(run.switches(), "SURFHIP_DESC_UR=0"), run.switches()
    gp, gd, eff = run.run(pts, eff, rotated=False)
    _, gd2, _ = run.run(pts, eff, rotated=False)
    run.close()
    check_batch(f"back-to-back extend={int(extend)}", gp, gd, eff, pts, ori, desc, masks, PAIR_CLASSES, False)
    assert gd.tobytes() == gd2.tobytes(), "k_describe_u2 did not repeat byte for byte"


# 3 ------------------------------------------------------------ rotated and generic kernels

ROT_CONFIGS = {
    "rot4": (dict(upright=False, extend=False, desc_wsz=4), "", True),              # k_describe_rot<4>
    "rot8": (dict(upright=False, extend=True, desc_wsz=4), "", True),               # k_describe_rot<8>
    "rot_atomic": (dict(upright=False, extend=False, desc_wsz=4), "SURFHIP_ROT_ATOMIC=1", False),
    "wsz3_upright": (dict(upright=True, extend=False, desc_wsz=3), "", False),      # k_describe<true, 128>
    "wsz3_rotated": (dict(upright=False, extend=False, desc_wsz=3), "", False),     # k_describe<false, 128>
    "wsz5_upright": (dict(upright=True, extend=False, desc_wsz=5), "", False),
    "wsz5_rotated": (dict(upright=False, extend=False, desc_wsz=5), "", False),
    "wsz6_ext_upright": (dict(upright=True, extend=True, desc_wsz=6), "", False),   # k_describe<true, 512>
    "wsz6_ext_rotated": (dict(upright=False, extend=True, desc_wsz=6), "", False),  # k_describe<false, 512>
}
COUNTS_4 = [MAX_PTS, MAX_PTS - 1, 1500, MAX_PTS]


@pytest.mark.parametrize("name", list(ROT_CONFIGS))
def test_rotated_and_generic_kernels(surf, orc, monkeypatch, name):
    """The rotated wsz-4 kernels (atomic-free, and the LDS-atomic one), the generic kernel at desc_wsz
    3 and 5 and its 512-feature instance at desc_wsz 6 extended, on one frame of each kind: `ori` bit
    for bit, descriptors within DESC_TOL; windows (and the orientation's sample disc) clipped at each
    side, and oracle orientations of exactly 0 and exactly pi (vbands: dy == 0 everywhere)."""
    par, env, deterministic = ROT_CONFIGS[name]
    monkeypatch.delenv("SURFHIP_ROT_ATOMIC", raising=False)
    with_env(monkeypatch, env)
    rotated = not par["upright"]
    imgs = {k: image(k) for k in KINDS}
    base = planted_set(W, H, few=False)
    lo, hi = scale_bounds(4)
    assert lo <= base["scale"].min() and base["scale"].max() <= hi
    pts, ori, desc, dropped = build_batch(orc, base, list(KINDS), imgs, [7, 8, 9, 10], **par)
    assert_drop_cap(dropped)
    eff = np.clip(COUNTS_4, 0, MAX_PTS)
    live = np.arange(MAX_PTS)[None, :] < eff[:, None]
    geo = [geometry(pts[f], W, H, wsz=par["desc_wsz"], rotated=rotated) for f in range(4)]
    masks = {}
    if rotated:
        for side in ("top", "bottom", "left", "right"):
            masks["window_" + side] = np.stack([g["rot_" + side] for g in geo])
            masks["ori_disc_" + side] = np.stack([g["ori_" + side] for g in geo])
        vb = np.zeros((4, MAX_PTS), bool)
        vb[KINDS.index("vbands")] = True
        masks["ori_exactly_0"] = vb & (ori == 0)
        masks["ori_exactly_pi"] = vb & (ori == F32(np.pi))
    else:
        for side, k in (("top", "r_low"), ("bottom", "r_high"), ("left", "c_low"), ("right", "c_high")):
            masks["window_" + side] = np.stack([g[k] & (g["nr"] > 0) & (g["nc"] > 0) for g in geo])
    masks["unclipped"] = ~np.any([masks["window_" + s] for s in ("top", "bottom", "left", "right")], axis=0)
    for k, kind in enumerate(KINDS):
        masks["kind_" + kind] = np.zeros((4, MAX_PTS), bool)
        masks["kind_" + kind][k] = True
    names = list(masks)
    for nm in names:
        assert int((masks[nm] & live).sum()) >= 8, f"class {nm} holds {int((masks[nm] & live).sum())} keypoints"
    frames = np.stack([imgs[k] for k in KINDS])
    run = Planted(surf, surf.make_param(4, 4.0, **par), frames)
    assert took(run.switches(), env), run.switches()
    assert ("SURFHIP_ROT_ATOMIC" in run.switches()["switches"]) == bool(env)
    gp, gd, eff = run.run(pts, COUNTS_4, rotated)
    if deterministic:
        gp2, gd2, _ = run.run(pts, COUNTS_4, rotated)
        assert gd.tobytes() == gd2.tobytes() and gp.tobytes() == gp2.tobytes(), "did not repeat byte for byte"
    run.close()
    check_batch(name, gp, gd, eff, pts, ori, desc, masks, names, rotated)


# 4 ------------------------------------------------------------ doubled

def test_doubled_upright_paths(surf, orc, monkeypatch):
    """A doubled detector (integral of the 510 x 382 upsampled frames, windows of 3.3 scale at (2x,
    2y)), its integral left resident by a detect_batch: the upright classes, both half-way scales of
    3.3f included."""
    with_env(monkeypatch, "SURFHIP_DESC_UR=0")
    keys = ["noise", "checker", "noise2", "noise"]
    imgs = {"noise": image("noise"), "checker": image("checker"), "noise2": image("noise", seed=11)}
    wi, hi = 2 * W - 2, 2 * H - 2
    base = planted_set(wi, hi, doubled=True)
    lo, hi_s = scale_bounds(6, doubled=True)
    assert lo <= base["scale"].min() and base["scale"].max() <= hi_s
    assert sum(int((base["scale"] == F32(s)).sum()) for s in HALF_SCALES_DOUBLED) >= 16
    pts, ori, desc, dropped = build_batch(orc, base, keys, imgs, [21, 22, 23, 24], doubled=True, upright=True)
    assert_drop_cap(dropped)
    masks = batch_classes(pts, doubled=True)
    eff = np.clip(COUNTS_4, 0, MAX_PTS)
    populated(masks, eff, UPRIGHT_CLASSES)
    frames = np.stack([imgs[k] for k in keys])
    run = Planted(surf, surf.make_param(6, 4.0, doubled=True, upright=True), frames, via_detect=True)
    assert took(run.switches(), "SURFHIP_DESC_UR=0"), run.switches()
    gp, gd, eff = run.run(pts, COUNTS_4, rotated=False)
    run.close()
    check_batch("doubled", gp, gd, eff, pts, ori, desc, masks, UPRIGHT_CLASSES, False)


# 6 ------------------------------------------------------------ argument checks

def test_run_describe_argument_checks(surf):
    frames = image("noise")[None]
    run = Planted(surf, surf.make_param(4, 4.0, upright=True), frames, max_batch=2)
    pb, db, cb = surf.DeviceBuffer(48 * 2 * MAX_PTS), surf.DeviceBuffer(4 * 2 * MAX_PTS * 64), surf.DeviceBuffer(8)
    cb.upload(np.zeros(2, np.int32))
    with pytest.raises(surf.SurfError, match="invalid argument"):          # no integral resident yet
        run.det.run_describe(pb.ptr, cb.ptr, 1, db.ptr)
    run.make_resident()
    surf.synchronize()
    for args in ((pb.ptr, cb.ptr, 0, db.ptr), (pb.ptr, cb.ptr, 3, db.ptr), (pb.ptr, cb.ptr, -1, db.ptr),
                 (None, cb.ptr, 1, db.ptr), (pb.ptr, None, 1, db.ptr), (pb.ptr, cb.ptr, 1, None)):
        with pytest.raises(surf.SurfError, match="invalid argument"):
            run.det.run_describe(*args)
    with pytest.raises(surf.SurfError, match="invalid argument"):
        surf.check(surf.lib.surfhip_run_describe(None, pb.ptr, cb.ptr, 1, db.ptr), "run_describe")
    run.det.run_describe(pb.ptr, cb.ptr, 1, db.ptr)                         # and a valid call goes through
    surf.synchronize()
    run.close()
