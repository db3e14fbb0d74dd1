#!/usr/bin/env python3
"""Time surfhip_match (Surfor::match) on one GPU: n x n points, nf-D
descriptors, caller-provided scratch, HIP events via torch on the null
stream.  Prints one JSON line per case.

    python tools/match_bench.py [--n 3000] [--iters 50]

--batch NPAIRS instead times NPAIRS pairs of n x n points (flags 0, nf 64
then 128) two ways on the same data, alternating in one run: a loop of NPAIRS
surfhip_match calls with caller scratch, and one surfhip_match_batch call.
It checks that both write the same bits and prints, per nf, one JSON line
with both times in ms (median and range over --reps), their ratio and the
batch call's fp32 TFLOP/s.

    python tools/match_bench.py --batch 255 [--n 3000] [--reps 7]

--batch NPAIRS --cross times one surfhip_match_batch call against one
surfhip_match_batch_cross call (the same match with the mutual-best test) on
the same data, alternating in one run, and prints both medians with their
ranges and the ratio cross / batch.

--window R detects 256 synthetic 1920 x 1080 frames (random points have no
canonical order and would show nothing) and matches the 255 consecutive pairs
on the detector's buffers, alternating in one run: surfhip_match_batch,
surfhip_match_batch_window with +-R px on both axes, with the infinite window
and with a window that holds no pair (the box pre-pass, the list building and
the launches alone).  It also prints the share of (128-point block, tile) and
(wave, tile) combinations the box tests keep, computed in numpy from the
downloaded points: the factor the kernel can at best reach.  --cross does the
same against surfhip_match_batch_cross (SURFHIP_MATCH_MUTUAL).

    python tools/match_bench.py --window 32 [--cross] [--reps 7] [--inner 4]

--guided R times surfhip_match_batch_guided on the same detected frames, all
calls alternating in one run.  (1) The 255 consecutive pairs:
surfhip_match_batch_window with +-R px against the guided call with +-R px and
the identity matrix (h_stride 0); the two must write the same bytes (exit
status 1 if not).  (2) A moving camera: set 2 is each frame's own keypoints
mapped through a known similarity (roll 3 degrees, zoom 1.02, pan (120, -40) px
about the frame centre; fp64, rounded to fp32, re-sorted by row and column
inside every (octave, level) group, descriptors travelling with their points):
the guided call with +-R px around the prediction under that matrix against the
window call opened just wide enough to hold every true displacement.  It
prints times, matches (and how many are the true partner) and the kept (block,
tile) and (wave, tile) shares of both.  --cross adds SURFHIP_MATCH_MUTUAL.

    python tools/match_bench.py --guided 32 [--cross] [--reps 7] [--inner 4]

--epipolar B times surfhip_match_batch_epipolar with a band of B px on the same
detected frames, all calls alternating in one run.  (1) The 255 consecutive
pairs: the all-zero matrix with the window +-32 px against
surfhip_match_batch_window with +-32 px; the two must write the same bytes
(exit status 1 if not).  (2) Rectified stereo: set 2 is each frame's own
keypoints moved by a per-point disparity in [-64, 0] px along their row
(re-sorted as for --guided): the epipolar call with the rectified matrix and
the window (-64, 0, -inf, inf) against the window call with (-64, 0, -B, B);
the same bytes again.  (3) The same disparities along lines tilted by 3
degrees: the epipolar call under that matrix against the window call opened
just tall enough to hold every true partner.  It prints times, matches (and how
many are the true partner) and the kept (block, tile) and (wave, tile) shares,
computed in numpy.  --cross adds SURFHIP_MATCH_MUTUAL.

    python tools/match_bench.py --epipolar 1.5 [--cross] [--reps 7] [--inner 4]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_surf():
    pkg = os.path.join(REPO, "cuda-surf_amd")
    spec = importlib.util.spec_from_file_location("surf_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["surf_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def bench_batch(surf, torch, npairs, n, reps, inner):
    for nf in (64, 128):
        torch.manual_seed(nf)
        ft = torch.randn((2, npairs, n, nf), device="cuda")
        ft /= ft.norm(dim=3, keepdim=True)
        pts = torch.zeros((2, npairs, n, 48), dtype=torch.uint8, device="cuda")
        pts_b = torch.zeros((npairs, n, 48), dtype=torch.uint8, device="cuda")
        counts = torch.full((2, npairs), n, dtype=torch.int32, device="cuda")
        scratch = torch.empty(max(surf.match_scratch_bytes(n, n, 0), 4), dtype=torch.uint8, device="cuda")

        def loop():
            for i in range(npairs):
                surf.match_points(pts[0, i].data_ptr(), pts[1, i].data_ptr(), ft[0, i].data_ptr(),
                                  ft[1, i].data_ptr(), n, n, nf, 0, scratch.data_ptr())

        def batch():
            surf.match_batch(pts_b.data_ptr(), ft[0].data_ptr(), counts[0].data_ptr(), n, pts[1].data_ptr(),
                             ft[1].data_ptr(), counts[1].data_ptr(), n, npairs, nf, 0)

        loop()
        batch()
        torch.cuda.synchronize()
        same = bool(torch.equal(pts[0], pts_b))
        t_loop, t_batch = [], []
        for _ in range(reps):                       # alternate the two in the same run
            for fn, k, out in ((loop, 1, t_loop), (batch, inner, t_batch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / k)
        lm, bm = float(np.median(t_loop)), float(np.median(t_batch))
        fma = npairs * n * (32 * (n // 32)) * nf
        print(json.dumps({"case": f"match {npairs} pairs of {n}x{n} nf={nf} flags=0",
                          "loop_ms": round(lm, 4), "loop_ms_range": [round(min(t_loop), 4), round(max(t_loop), 4)],
                          "batch_ms": round(bm, 4),
                          "batch_ms_range": [round(min(t_batch), 4), round(max(t_batch), 4)],
                          "ratio": round(lm / bm, 3), "batch_fp32_tflops": round(2 * fma / bm / 1e9, 2),
                          "loop_fp32_tflops": round(2 * fma / lm / 1e9, 2), "reps": reps,
                          "bit_identical": same}), flush=True)
        if not same:
            raise SystemExit("surfhip_match_batch and the surfhip_match loop disagree")
        del ft, pts, pts_b, scratch


def bench_cross(surf, torch, npairs, n, reps, inner):
    """surfhip_match_batch against surfhip_match_batch_cross on the same
    data, alternating in one run.  The cost of composing the mutual test by
    hand is two match_batch calls (before the caller's own filter kernel and
    slab copy), so cross_over_batch below 2 is the library doing better."""
    for nf in (64, 128):
        torch.manual_seed(nf)
        ft = torch.randn((2, npairs, n, nf), device="cuda")
        ft /= ft.norm(dim=3, keepdim=True)
        pts = torch.zeros((2, npairs, n, 48), dtype=torch.uint8, device="cuda")
        pts_c = torch.zeros((npairs, n, 48), dtype=torch.uint8, device="cuda")
        counts = torch.full((2, npairs), n, dtype=torch.int32, device="cuda")
        nbytes = surf.match_batch_cross_scratch_bytes(npairs, n, n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        tail = (counts[0].data_ptr(), n, pts[1].data_ptr(), ft[1].data_ptr(), counts[1].data_ptr(), n, npairs, nf)

        def batch():
            surf.match_batch(pts[0].data_ptr(), ft[0].data_ptr(), *tail, 0)

        def cross():
            surf.match_batch_cross(pts_c.data_ptr(), ft[0].data_ptr(), *tail, scratch.data_ptr(), 0)

        batch()
        cross()
        torch.cuda.synchronize()
        a = pts[0].cpu().numpy().reshape(-1).view(surf.POINT_DTYPE)
        c = pts_c.cpu().numpy().reshape(-1).view(surf.POINT_DTYPE)
        kept = c["match"] >= 0
        ok = bool((a["score"] == c["score"]).all() and (a["ambiguity"] == c["ambiguity"]).all()
                  and (a["match"][kept] == c["match"][kept]).all())
        partners = c["match"].reshape(npairs, n)
        injective = all(len(np.unique(r[r >= 0])) == int((r >= 0).sum()) for r in partners)
        t_batch, t_cross = [], []
        for _ in range(reps):                       # alternate the two in the same run
            for fn, out in ((batch, t_batch), (cross, t_cross)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / inner)
        bm, cm = float(np.median(t_batch)), float(np.median(t_cross))
        nscan = 32 * (n // 32)
        atomic_bytes = 8 * npairs * nscan * ((n + 127) // 128)     # one key per (128-point block, scanned p2)
        print(json.dumps({"case": f"cross match {npairs} pairs of {n}x{n} nf={nf} flags=0",
                          "batch_ms": round(bm, 4),
                          "batch_ms_range": [round(min(t_batch), 4), round(max(t_batch), 4)],
                          "cross_ms": round(cm, 4),
                          "cross_ms_range": [round(min(t_cross), 4), round(max(t_cross), 4)],
                          "cross_over_batch": round(cm / bm, 3), "reps": reps,
                          "forward_matches": int((a["match"] >= 0).sum()), "kept": int(kept.sum()),
                          "atomic_mbytes": round(atomic_bytes / 1e6, 2), "scratch_mbytes": round(nbytes / 1e6, 2),
                          "consistent": ok and injective}), flush=True)
        if not (ok and injective):
            raise SystemExit("surfhip_match_batch_cross disagrees with surfhip_match_batch")
        del ft, pts, pts_c, scratch


def kept_tile_shares(surf, pts, counts, win):
    """The share of (128-point block, 32-point tile) and of (32-point wave,
    tile) combinations of consecutive frame pairs that the windowed kernel's
    fp32 box tests keep, computed from the downloaded points (flags 0: full
    tiles only).  Random points would keep nearly all; detect_batch's order
    (octave, level, row, column) is what makes the boxes narrow."""
    return kept_pair_shares(pts[:-1], counts[:-1], pts[1:], counts[1:], win)


def kept_pair_shares(pts1, counts1, pts2, counts2, win, f=None, band=0.0):
    """The same for pair i = pts1[i] (its x, y: the positions the window is
    measured from) against pts2[i].  f, band: the matrix and band of
    surfhip_match_batch_epipolar, whose kernels also drop a combination when
    none of the group's epipolar lines can come within the band of the tile's
    box (r at the box's four corners, fp32)."""
    w = np.asarray(win, np.float32)
    inf = np.float32(np.inf)

    def boxes(p, n, group):
        g = (n + group - 1) // group
        x = np.full(g * group, np.nan, np.float32)
        y = np.full(g * group, np.nan, np.float32)
        x[:n], y[:n] = p["x"][:n], p["y"][:n]
        x, y = x.reshape(g, group), y.reshape(g, group)
        return (np.fmin.reduce(x, axis=1, initial=inf), np.fmax.reduce(x, axis=1, initial=-inf),
                np.fmin.reduce(y, axis=1, initial=inf), np.fmax.reduce(y, axis=1, initial=-inf))

    tot = {128: 0, 32: 0}
    kept = {128: 0, 32: 0}
    for i in range(len(counts1)):
        n1, nscan = int(counts1[i]), 32 * (int(counts2[i]) // 32)
        if n1 == 0 or nscan == 0:
            continue
        b = boxes(pts2[i], nscan, 32)
        for group in (128, 32):
            a = boxes(pts1[i], n1, group)
            with np.errstate(invalid="ignore"):
                keep = (~(b[0][None] - a[1][:, None] > w[1]) & ~(b[1][None] - a[0][:, None] < w[0])
                        & ~(b[2][None] - a[3][:, None] > w[3]) & ~(b[3][None] - a[2][:, None] < w[2]))
            if f is not None:
                keep &= lines_reach(pts1[i], n1, group, b, f, band)
            tot[group] += keep.size
            kept[group] += int(keep.sum())
    return kept[128] / max(tot[128], 1), kept[32] / max(tot[32], 1)


def epipolar_lines_f32(f, band, x, y):
    """surfhip_match_batch_epipolar's (a, b, c, lim) of the set-1 points, its
    fp32 operations."""
    f = np.asarray(f, np.float32)
    bb = np.float32(band) * np.float32(band)
    with np.errstate(all="ignore"):
        a = (f[0] * x + f[1] * y) + f[2]
        b = (f[3] * x + f[4] * y) + f[5]
        c = (f[6] * x + f[7] * y) + f[8]
        return a, b, c, bb * (a * a + b * b)


def lines_reach(p, n, group, boxes, f, band):
    """[groups of `group` set-1 points][tiles]: one of the group's lines may
    offer a point of the tile's box (xmin, xmax, ymin, ymax arrays): not all
    four corner values of r on one side of 0 with r r > lim."""
    g = (n + group - 1) // group
    x = np.zeros(g * group, np.float32)
    y = np.zeros(g * group, np.float32)
    x[:n], y[:n] = p["x"][:n], p["y"][:n]
    live = (np.arange(g * group) < n).reshape(g, group, 1)
    a, b, c, lim = (v.reshape(g, group, 1) for v in epipolar_lines_f32(f, band, x, y))
    with np.errstate(all="ignore"):
        xa = [boxes[0][None, None, :] * a, boxes[1][None, None, :] * a]
        yb = [boxes[2][None, None, :] * b, boxes[3][None, None, :] * b]
        rs = [(xa[i] + yb[j]) + c for j in (0, 1) for i in (0, 1)]
        far = np.logical_and.reduce([r * r > lim for r in rs])
        side = np.logical_and.reduce([r > 0 for r in rs]) | np.logical_and.reduce([r < 0 for r in rs])
    return (~(far & side) & live).any(axis=1)


def bench_window(surf, torch, radius, cross, frames_n, reps, inner, width=1920, height=1080, thresh=4.0,
                 slots=8192):
    """surfhip_match_batch (or, with cross, surfhip_match_batch_cross) against
    surfhip_match_batch_window with +-radius px, with the infinite window and
    with a window no pair lies in (the cost of the box pre-pass, the list
    building and the launches), alternating in one run, on the consecutive
    pairs of one detected batch of synthetic frames in the detector's own
    buffers."""
    dev = torch.device("cuda", 0)
    surf.set_device(0)
    B, npairs = frames_n, frames_n - 1
    pitch = surf.align_up(width, 128)
    d_frames = torch.from_numpy(surf.synth_frames(B, width, height, pitch)).to(dev)
    param = surf.make_param(4, thresh, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    stream = torch.cuda.current_stream(dev).cuda_stream
    det = surf.Detector(param, width, height, max_batch=B, max_pts=slots, stream=stream)
    d_pts = torch.zeros(B * slots * 48, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(B * slots * nf, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    det.detect_batch(d_frames.data_ptr(), B, pitch, height * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                     d_cnt.data_ptr())
    mutual = surf.MATCH_MUTUAL if cross else 0
    d_scratch = torch.empty(max(surf.match_batch_window_scratch_bytes(npairs, slots, slots, mutual),
                                surf.match_batch_cross_scratch_bytes(npairs, slots, slots), 16),
                            dtype=torch.uint8, device=dev)
    sets = (d_pts.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
            d_pts.data_ptr() + 48 * slots, d_desc.data_ptr() + 4 * slots * nf, d_cnt.data_ptr() + 4, slots)
    inf = float("inf")
    windows = {"window": (-radius, radius, -radius, radius), "infinite": (-inf, inf, -inf, inf),
               "empty": (1e30, 1e30, 1e30, 1e30)}

    def plain():
        if cross:
            surf.match_batch_cross(*sets, npairs, nf, d_scratch.data_ptr(), 0, stream)
        else:
            surf.match_batch(*sets, npairs, nf, 0, stream)

    def windowed(name):
        return lambda: surf.match_batch_window(*sets, npairs, nf, mutual, windows[name], d_scratch.data_ptr(), stream)

    calls = {"plain": plain, "window": windowed("window"), "infinite": windowed("infinite"),
             "empty": windowed("empty")}
    out = {}
    for name, fn in calls.items():                  # warm-up, and the results to compare
        fn()
        torch.cuda.synchronize()
        out[name] = d_pts.cpu().numpy().view(surf.POINT_DTYPE).reshape(B, slots).copy()
    counts = d_cnt.cpu().numpy()
    same = out["infinite"].tobytes() == out["plain"].tobytes()
    times = {name: [] for name in calls}
    for _ in range(reps):                           # the calls alternate inside one run
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    block_share, wave_share = kept_tile_shares(surf, out["plain"], counts, windows["window"])
    live = np.arange(slots)[None, :] < counts[:-1, None]
    res = {"case": f"{npairs} consecutive pairs of {B} {width}x{height} frames, nf={nf} flags=0, "
                   f"window +-{radius} px" + (", mutual-best" if cross else ""),
           "reps": reps, "inner": inner, "keypoints_mean": round(float(counts.mean()), 1),
           "keypoints_max": int(counts.max()),
           "matches_plain": int((out["plain"]["match"][:-1][live] >= 0).sum()),
           "matches_window": int((out["window"]["match"][:-1][live] >= 0).sum()),
           "kept_block_tile_share": round(block_share, 4), "kept_wave_tile_share": round(wave_share, 4),
           "infinite_window_bit_identical": same}
    for name, t in times.items():
        res[f"{name}_ms"] = round(float(np.median(t)), 4)
        res[f"{name}_ms_range"] = [round(min(t), 4), round(max(t), 4)]
    res["window_over_plain"] = round(res["window_ms"] / res["plain_ms"], 4)
    res["infinite_over_plain"] = round(res["infinite_ms"] / res["plain_ms"], 4)
    print(json.dumps(res), flush=True)
    det.close()
    if not same:
        raise SystemExit("the infinite window disagrees with the unwindowed call")


def predict_f32(h, x, y):
    """surfhip_match_batch_guided's predicted position, its fp32 operations."""
    h = np.asarray(h, np.float32)
    with np.errstate(all="ignore"):
        xx = (h[0] * x + h[1] * y) + h[2]
        yy = (h[3] * x + h[4] * y) + h[5]
        ww = (h[6] * x + h[7] * y) + h[8]
        nan = np.float32(np.nan)
        return np.where(ww > 0, xx / ww, nan), np.where(ww > 0, yy / ww, nan)


def moved_set(pts, counts, h64, height, init_sample=2):
    """Every frame's own keypoints mapped through the 3 x 3 matrix h64 (fp64,
    rounded to fp32) and re-sorted as detect_batch would have written them:
    inside each (octave, level) group by row, then column.  The groups are
    read off the canonical order of the input: a new one starts where the
    octave changes or y falls by more than a quarter of the frame height; a
    row is the octave's sampling step, init_sample << octave, of the new y.
    Returns (moved points, perm) with moved[i, j] = map(pts[i, perm[i, j]])."""
    def through(x, y):
        w = h64[2, 0] * x + h64[2, 1] * y + h64[2, 2]
        return (h64[0, 0] * x + h64[0, 1] * y + h64[0, 2]) / w, (h64[1, 0] * x + h64[1, 1] * y + h64[1, 2]) / w

    return moved_by(pts, counts, lambda i, x, y: through(x, y), height, init_sample)


def moved_by(pts, counts, move, height, init_sample=2):
    """moved_set for any map: move(i, x, y) gives frame i's new fp64
    coordinates."""
    moved = pts.copy()
    perm = np.tile(np.arange(pts.shape[1]), (len(pts), 1))
    for i, n in enumerate(counts):
        p = pts[i, :n]
        mx, my = (v.astype(np.float32) for v in move(i, p["x"].astype(np.float64), p["y"].astype(np.float64)))
        start = np.zeros(n, bool)
        start[1:] = (p["o"][1:] != p["o"][:-1]) | (p["y"][1:] < p["y"][:-1] - 0.25 * height)
        group = np.cumsum(start)
        row = np.floor(my / (init_sample * 2.0 ** p["o"])).astype(np.int64)
        order = np.lexsort((mx, row, group))
        perm[i, :n] = order
        moved[i, :n] = p[order]
        moved["x"][i, :n], moved["y"][i, :n] = mx[order], my[order]
    return moved, perm


def bench_guided(surf, torch, radius, cross, frames_n, reps, inner, width=1920, height=1080, thresh=4.0,
                 slots=8192):
    """surfhip_match_batch_guided against surfhip_match_batch_window, all four
    calls alternating in one run on one detected batch of synthetic frames:
    the identity on the consecutive pairs (the same bytes, the cost of the
    guided mode itself), and a moving camera (see the module docstring)."""
    dev = torch.device("cuda", 0)
    surf.set_device(0)
    B, npairs = frames_n, frames_n - 1
    pitch = surf.align_up(width, 128)
    d_frames = torch.from_numpy(surf.synth_frames(B, width, height, pitch)).to(dev)
    param = surf.make_param(4, thresh, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    stream = torch.cuda.current_stream(dev).cuda_stream
    det = surf.Detector(param, width, height, max_batch=B, max_pts=slots, stream=stream)
    d_pts = torch.zeros(B * slots * 48, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(B * slots * nf, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    det.detect_batch(d_frames.data_ptr(), B, pitch, height * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                     d_cnt.data_ptr())
    torch.cuda.synchronize()
    flags = surf.MATCH_MUTUAL if cross else 0
    d_scratch = torch.empty(max(surf.match_batch_guided_scratch_bytes(npairs, slots, slots, flags), 16),
                            dtype=torch.uint8, device=dev)
    counts = d_cnt.cpu().numpy()
    pts = d_pts.cpu().numpy().view(surf.POINT_DTYPE).reshape(B, slots).copy()

    # the moving camera: roll 3 degrees, zoom 1.02, pan (120, -40) about the frame centre
    a, b = 1.02 * np.cos(np.radians(3.0)), 1.02 * np.sin(np.radians(3.0))
    cx, cy = width / 2.0, height / 2.0
    h32 = np.array([a, -b, cx - a * cx + b * cy + 120.0, b, a, cy - b * cx - a * cy - 40.0, 0, 0, 1], np.float32)
    moved, perm = moved_set(pts[:npairs], counts[:npairs], h32.astype(np.float64).reshape(3, 3), height)
    live = np.arange(slots)[None, :] < counts[:npairs, None]
    with np.errstate(invalid="ignore"):
        # the true displacements, as the window call measures them: one fp32 subtraction per axis
        back = np.argsort(perm, axis=1)                            # set-1 point k lies at set-2 index back[i, k]
        tx = np.take_along_axis(moved["x"], back, axis=1) - pts[:npairs]["x"]
        ty = np.take_along_axis(moved["y"], back, axis=1) - pts[:npairs]["y"]
    wide = (float(tx[live].min()), float(tx[live].max()), float(ty[live].min()), float(ty[live].max()))
    tight = (-radius, radius, -radius, radius)
    d_moved = torch.from_numpy(moved.view(np.uint8).reshape(-1)).to(dev)
    d_perm = torch.from_numpy(perm).to(dev)
    d_mdesc = torch.take_along_dim(d_desc.view(B, slots, nf)[:npairs], d_perm[:, :, None], dim=1).contiguous()
    d_h = torch.from_numpy(np.concatenate([np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32), h32])).to(dev)
    d_out = torch.zeros(npairs * slots * 48, dtype=torch.uint8, device=dev)      # set 1 of the moving-camera calls

    consecutive = (d_pts.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
                   d_pts.data_ptr() + 48 * slots, d_desc.data_ptr() + 4 * slots * nf, d_cnt.data_ptr() + 4, slots)
    camera = (d_out.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
              d_moved.data_ptr(), d_mdesc.data_ptr(), d_cnt.data_ptr(), slots)
    sp = d_scratch.data_ptr()
    calls = {
        "window": lambda: surf.match_batch_window(*consecutive, npairs, nf, flags, tight, sp, stream),
        "guided_identity": lambda: surf.match_batch_guided(*consecutive, npairs, nf, flags, d_h.data_ptr(), 0, tight,
                                                           sp, stream),
        "wide_window": lambda: surf.match_batch_window(*camera, npairs, nf, flags, wide, sp, stream),
        "guided_camera": lambda: surf.match_batch_guided(*camera, npairs, nf, flags, d_h.data_ptr() + 36, 0, tight,
                                                         sp, stream),
    }
    out = {}
    for name, fn in calls.items():                  # warm-up, and the results to compare
        if name in ("wide_window", "guided_camera"):
            d_out.copy_(d_pts[:npairs * slots * 48])
        fn()
        torch.cuda.synchronize()
        src = d_out if name in ("wide_window", "guided_camera") else d_pts
        out[name] = src.cpu().numpy().view(surf.POINT_DTYPE).reshape(-1, slots)[:npairs].copy()
    same = out["window"].tobytes() == out["guided_identity"].tobytes()
    times = {name: [] for name in calls}
    for _ in range(reps):                           # the calls alternate inside one run
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    res = {"case": f"{npairs} pairs of {B} {width}x{height} frames, nf={nf} flags={flags}, guided +-{radius} px"
                   + (", mutual-best" if cross else ""),
           "reps": reps, "inner": inner, "keypoints_mean": round(float(counts.mean()), 1),
           "set1_points": int(live.sum()), "identity_bit_identical": same,
           "camera_matrix": [round(float(v), 6) for v in h32], "wide_window": [round(v, 3) for v in wide]}
    for name, t in times.items():
        res[f"{name}_ms"] = round(float(np.median(t)), 4)
        res[f"{name}_ms_range"] = [round(min(t), 4), round(max(t), 4)]
    res["guided_identity_over_window"] = round(res["guided_identity_ms"] / res["window_ms"], 4)
    res["guided_camera_over_wide_window"] = round(res["guided_camera_ms"] / res["wide_window_ms"], 4)
    res["matches_window"] = int((out["window"]["match"][live] >= 0).sum())
    pred = pts[:npairs].copy()
    pred["x"], pred["y"] = predict_f32(h32, pts[:npairs]["x"], pts[:npairs]["y"])
    for name, p1, win in (("wide_window", pts[:npairs], wide), ("guided_camera", pred, tight)):
        m = out[name]["match"]
        res[f"matches_{name}"] = int((m[live] >= 0).sum())
        res[f"true_partner_{name}"] = int((m[live] == back[live]).sum())
        block_share, wave_share = kept_pair_shares(p1, counts[:npairs], moved, counts[:npairs], win)
        res[f"kept_block_tile_share_{name}"] = round(block_share, 4)
        res[f"kept_wave_tile_share_{name}"] = round(wave_share, 4)
    block_share, wave_share = kept_tile_shares(surf, pts, counts, tight)
    res["kept_block_tile_share_window"] = round(block_share, 4)
    res["kept_wave_tile_share_window"] = round(wave_share, 4)
    print(json.dumps(res), flush=True)
    det.close()
    if not same:
        raise SystemExit("surfhip_match_batch_guided with the identity disagrees with surfhip_match_batch_window")


def bench_epipolar(surf, torch, band, cross, frames_n, reps, inner, width=1920, height=1080, thresh=4.0, slots=8192,
                   radius=32.0, disparity=64.0, tilt_deg=3.0):
    """surfhip_match_batch_epipolar against surfhip_match_batch_window, all six
    calls alternating in one run on one detected batch of synthetic frames
    (see the module docstring): the zero matrix (the same bytes: the cost of
    the mode itself), rectified stereo (the same bytes: the cost of the line
    test and the list build on the same offered set) and tilted lines (what
    only this call can prune)."""
    dev = torch.device("cuda", 0)
    surf.set_device(0)
    B, npairs = frames_n, frames_n - 1
    pitch = surf.align_up(width, 128)
    d_frames = torch.from_numpy(surf.synth_frames(B, width, height, pitch)).to(dev)
    param = surf.make_param(4, thresh, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    stream = torch.cuda.current_stream(dev).cuda_stream
    det = surf.Detector(param, width, height, max_batch=B, max_pts=slots, stream=stream)
    d_pts = torch.zeros(B * slots * 48, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(B * slots * nf, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    det.detect_batch(d_frames.data_ptr(), B, pitch, height * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                     d_cnt.data_ptr())
    torch.cuda.synchronize()
    flags = surf.MATCH_MUTUAL if cross else 0
    d_scratch = torch.empty(max(surf.match_batch_epipolar_scratch_bytes(npairs, slots, slots, flags), 16),
                            dtype=torch.uint8, device=dev)
    counts = d_cnt.cpu().numpy()
    pts = d_pts.cpu().numpy().view(surf.POINT_DTYPE).reshape(B, slots).copy()
    live = np.arange(slots)[None, :] < counts[:npairs, None]
    inf = float("inf")

    # the stereo sets: a disparity per point, along its row and along a line tilted by tilt_deg
    rng = np.random.default_rng(2024)
    disp = [-disparity * rng.random(int(n)) for n in counts[:npairs]]
    slope = float(np.float32(np.tan(np.radians(tilt_deg))))
    f_zero = np.zeros(9, np.float32)
    f_rect = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
    f_tilt = np.array([0, 0, slope, 0, 0, -1, -slope, 1, 0], np.float32)      # y2 - y1 = slope (x2 - x1)
    sets2 = {}
    for name, k in (("rect", 0.0), ("tilt", slope)):
        moved, perm = moved_by(pts[:npairs], counts[:npairs], lambda i, x, y: (x + disp[i], y + k * disp[i]), height)
        back = np.argsort(perm, axis=1)                            # set-1 point k lies at set-2 index back[i, k]
        d_perm = torch.from_numpy(perm).to(dev)
        sets2[name] = (moved, back, torch.from_numpy(moved.view(np.uint8).reshape(-1)).to(dev),
                       torch.take_along_dim(d_desc.view(B, slots, nf)[:npairs], d_perm[:, :, None], dim=1).contiguous())
    with np.errstate(invalid="ignore"):
        moved, back = sets2["tilt"][:2]
        ty = np.take_along_axis(moved["y"], back, axis=1) - pts[:npairs]["y"]       # one fp32 subtraction, as the call's
    tall = (-disparity, 0.0, float(ty[live].min()), float(ty[live].max()))
    tight = (-radius, radius, -radius, radius)
    rows = (-disparity, 0.0, -band, band)
    open_y = (-disparity, 0.0, -inf, inf)
    d_f = torch.from_numpy(np.concatenate([f_zero, f_rect, f_tilt])).to(dev)
    d_out = torch.zeros(npairs * slots * 48, dtype=torch.uint8, device=dev)          # set 1 of the stereo calls

    consecutive = (d_pts.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
                   d_pts.data_ptr() + 48 * slots, d_desc.data_ptr() + 4 * slots * nf, d_cnt.data_ptr() + 4, slots)

    def stereo(name):
        return (d_out.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
                sets2[name][2].data_ptr(), sets2[name][3].data_ptr(), d_cnt.data_ptr(), slots)

    sp, fp = d_scratch.data_ptr(), d_f.data_ptr()
    calls = {
        "window": lambda: surf.match_batch_window(*consecutive, npairs, nf, flags, tight, sp, stream),
        "epipolar_zero": lambda: surf.match_batch_epipolar(*consecutive, npairs, nf, flags, fp, 0, band, tight, sp,
                                                           stream),
        "window_rows": lambda: surf.match_batch_window(*stereo("rect"), npairs, nf, flags, rows, sp, stream),
        "epipolar_rect": lambda: surf.match_batch_epipolar(*stereo("rect"), npairs, nf, flags, fp + 36, 0, band,
                                                           open_y, sp, stream),
        "window_tall": lambda: surf.match_batch_window(*stereo("tilt"), npairs, nf, flags, tall, sp, stream),
        "epipolar_tilt": lambda: surf.match_batch_epipolar(*stereo("tilt"), npairs, nf, flags, fp + 72, 0, band,
                                                           open_y, sp, stream),
    }
    out = {}
    for name, fn in calls.items():                  # warm-up, and the results to compare
        on_out = name not in ("window", "epipolar_zero")
        if on_out:
            d_out.copy_(d_pts[:npairs * slots * 48])
        fn()
        torch.cuda.synchronize()
        out[name] = (d_out if on_out else d_pts).cpu().numpy().view(surf.POINT_DTYPE).reshape(-1, slots)[:npairs].copy()
    same_zero = out["window"].tobytes() == out["epipolar_zero"].tobytes()
    same_rect = out["window_rows"].tobytes() == out["epipolar_rect"].tobytes()
    times = {name: [] for name in calls}
    for _ in range(reps):                           # the calls alternate inside one run
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    res = {"case": f"{npairs} pairs of {B} {width}x{height} frames, nf={nf} flags={flags}, epipolar band {band} px"
                   + (", mutual-best" if cross else ""),
           "reps": reps, "inner": inner, "keypoints_mean": round(float(counts.mean()), 1),
           "set1_points": int(live.sum()), "zero_matrix_bit_identical": same_zero,
           "rectified_bit_identical": same_rect, "tilt_deg": tilt_deg, "tall_window": [round(v, 3) for v in tall]}
    for name, t in times.items():
        res[f"{name}_ms"] = round(float(np.median(t)), 4)
        res[f"{name}_ms_range"] = [round(min(t), 4), round(max(t), 4)]
    res["epipolar_zero_over_window"] = round(res["epipolar_zero_ms"] / res["window_ms"], 4)
    res["epipolar_rect_over_window_rows"] = round(res["epipolar_rect_ms"] / res["window_rows_ms"], 4)
    res["epipolar_tilt_over_window_tall"] = round(res["epipolar_tilt_ms"] / res["window_tall_ms"], 4)
    p1 = pts[:npairs]
    shares = {"window": (p1, pts[1:], counts[1:], tight, None),
              "epipolar_zero": (p1, pts[1:], counts[1:], tight, f_zero),
              "window_rows": (p1, sets2["rect"][0], counts[:npairs], rows, None),
              "epipolar_rect": (p1, sets2["rect"][0], counts[:npairs], open_y, f_rect),
              "window_tall": (p1, sets2["tilt"][0], counts[:npairs], tall, None),
              "epipolar_tilt": (p1, sets2["tilt"][0], counts[:npairs], open_y, f_tilt)}
    for name, (a, b, c2, win, f) in shares.items():
        m = out[name]["match"]
        res[f"matches_{name}"] = int((m[live] >= 0).sum())
        if name not in ("window", "epipolar_zero"):
            back = sets2["rect" if name in ("window_rows", "epipolar_rect") else "tilt"][1]
            res[f"true_partner_{name}"] = int((m[live] == back[live]).sum())
        block_share, wave_share = kept_pair_shares(a, counts[:npairs], b, c2, win, f, band)
        res[f"kept_block_tile_share_{name}"] = round(block_share, 4)
        res[f"kept_wave_tile_share_{name}"] = round(wave_share, 4)
    print(json.dumps(res), flush=True)
    det.close()
    if not same_zero:
        raise SystemExit("surfhip_match_batch_epipolar with the zero matrix disagrees with surfhip_match_batch_window")
    if not same_rect:
        raise SystemExit("surfhip_match_batch_epipolar with the rectified matrix disagrees with the window of rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=0, metavar="NPAIRS",
                    help="time NPAIRS surfhip_match calls against one surfhip_match_batch call")
    ap.add_argument("--reps", type=int, default=7, help="--batch: timed repeats of each side")
    ap.add_argument("--inner", type=int, default=4, help="--batch: batch calls per timed window")
    ap.add_argument("--cross", action="store_true",
                    help="--batch: time surfhip_match_batch against surfhip_match_batch_cross instead")
    ap.add_argument("--window", type=float, default=0.0, metavar="R",
                    help="time surfhip_match_batch_window with +-R px on detected frames (--cross: with MUTUAL)")
    ap.add_argument("--guided", type=float, default=0.0, metavar="R",
                    help="time surfhip_match_batch_guided with +-R px against the window call (--cross: with MUTUAL)")
    ap.add_argument("--epipolar", type=float, default=0.0, metavar="B",
                    help="time surfhip_match_batch_epipolar with a band of B px against the window call "
                         "(--cross: with MUTUAL)")
    ap.add_argument("--frames", type=int, default=256,
                    help="--window, --guided, --epipolar: synthetic 1920x1080 frames to detect")
    args = ap.parse_args()
    import torch
    surf = load_surf()
    if args.epipolar > 0:
        bench_epipolar(surf, torch, args.epipolar, args.cross, args.frames, args.reps, args.inner)
        return
    if args.guided > 0:
        bench_guided(surf, torch, args.guided, args.cross, args.frames, args.reps, args.inner)
        return
    if args.window > 0:
        bench_window(surf, torch, args.window, args.cross, args.frames, args.reps, args.inner)
        return
    if args.batch > 0 and args.cross:
        bench_cross(surf, torch, args.batch, args.n, args.reps, args.inner)
        return
    if args.batch > 0:
        bench_batch(surf, torch, args.batch, args.n, args.reps, args.inner)
        return
    for nf in (64, 128):
        for flags in (0, 1):
            n = args.n
            rng = np.random.default_rng(nf)
            f = rng.standard_normal((2, n, nf)).astype(np.float32)
            f /= np.linalg.norm(f, axis=2, keepdims=True)
            ft = torch.from_numpy(f).cuda()
            pts = torch.zeros((2, n, 48), dtype=torch.uint8, device="cuda")
            scratch = torch.empty(max(surf.match_scratch_bytes(n, n, flags), 4), dtype=torch.uint8, device="cuda")
            args_ = (pts[0].data_ptr(), pts[1].data_ptr(), ft[0].data_ptr(), ft[1].data_ptr(), n, n, nf, flags,
                     scratch.data_ptr())
            for _ in range(3):
                surf.match_points(*args_)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                surf.match_points(*args_)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            fma = n * (n if flags else 32 * (n // 32)) * nf
            print(json.dumps({"case": f"match {n}x{n} nf={nf} full_tail={flags}", "ms": round(ms, 4),
                              "pairs_per_s": round(n * n / ms * 1e3, 1),
                              "fp32_tflops": round(2 * fma / ms / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
