"""GPU tests of surfhip_homography_batch (batched RANSAC homographies from
the match fields of the set-1 points).  The host reference is numpy float64,
in ransac_ref.py: the transfer error, the candidate filter and the documented
least-squares cost (inhomogeneous Hartley-normalised DLT)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ransac_ref import AMB, AMB_ABOVE, THR, candidate_mask, fit_dlt, project, transfer_err

pytestmark = pytest.mark.gpu

FRAME_W, FRAME_H = 1920.0, 1080.0
SLOTS = 160
COUNTS = (0, 1, 3, 4, 5, 31, 32, 33, 64, 65, 159, 160)
TWO_MODEL_PAIR = 11                                    # 30 % of its candidates follow H1

H_IDENTITY = np.eye(3)
H_TRANSLATION = np.array([[1, 0, 37.25], [0, 1, -12.5], [0, 0, 1.0]])
H_ROT90_SCALE = np.array([[0, -1.2, 1300.0], [1.2, 0, 10.0], [0, 0, 1.0]])
H_PERSPECTIVE = np.array([[1.1, 0.05, 20.0], [0.02, 0.95, -15.0], [2.0e-4, 1.0e-4, 1.0]])
# close to what the committed left/right 1280x960 pair gives (tests/golden, ambiguity <= 0.95, 3 px)
H_REAL_LIKE = np.array([[1.3, -0.01, -718.0], [0.124, 1.2085, -93.8], [2.297e-4, -6.6e-6, 1.0]])
H_KINDS = (H_IDENTITY, H_TRANSLATION, H_ROT90_SCALE, H_PERSPECTIVE, H_REAL_LIKE)
H1 = np.array([[0.98, 0.03, 150.0], [-0.03, 0.98, 140.0], [1.0e-5, -2.0e-5, 1.0]])      # the smaller consensus
H2 = np.array([[1.05, -0.08, -70.0], [0.08, 1.05, 90.0], [-3.0e-5, 4.0e-5, 1.0]])     # what must never be read


# ------------------------------------------------------- float64 reference

def corner_displacement(ha, hb):
    cx, cy = np.array([0, FRAME_W, FRAME_W, 0]), np.array([0, 0, FRAME_H, FRAME_H])
    ax, ay, _ = project(ha, cx, cy)
    bx, by, _ = project(hb, cx, cy)
    return float(np.hypot(ax - bx, ay - by).max())


def band_recheck(pts, count, res, mask, thr=THR, amb=AMB):
    """The mask agrees with a float64 recount under the GPU's h for every
    candidate whose float64 error lies outside [0.99, 1.01] thr; at most 2 %
    of the candidates lie inside; nothing else is set."""
    cand = candidate_mask(pts, count, amb)
    assert int(res["ncand"]) == int(cand.sum())
    assert not mask[~cand].any()
    e = transfer_err(res["h"], pts["x"], pts["y"], pts["match_x"], pts["match_y"])
    inside = cand & (e >= 0.99 * thr) & (e <= 1.01 * thr)
    assert inside.sum() <= 0.02 * cand.sum(), (int(inside.sum()), int(cand.sum()))
    sure = cand & ~inside
    bad = np.nonzero(sure & (mask.astype(bool) != (e < thr)))[0]
    assert len(bad) == 0, (bad[:5], e[bad[:5]], mask[bad[:5]])
    assert abs(int(res["ninliers"]) - int((cand & (e < thr)).sum())) <= int(inside.sum())
    assert int(res["ninliers"]) == int(mask.sum())


# --------------------------------------------------------------- planting

def min_height_ratio(x, y):
    """Smallest (triangle height / longest side) over all triples."""
    best, n = np.inf, len(x)
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                cr = abs((x[j] - x[i]) * (y[k] - y[i]) - (y[j] - y[i]) * (x[k] - x[i]))
                l2 = max((x[j] - x[i]) ** 2 + (y[j] - y[i]) ** 2, (x[k] - x[i]) ** 2 + (y[k] - y[i]) ** 2,
                         (x[k] - x[j]) ** 2 + (y[k] - y[j]) ** 2)
                best = min(best, cr / l2)
    return best


def f32_project(h, x, y):
    px, py, w = project(h, x, y)
    assert (w > 0).all()
    return px.astype(np.float32), py.astype(np.float32)


def plant_pair(rng, dtype, slots, count, h0, out_frac=0.4, h1_frac=0.0, sigma=0.0, sprinkle=True, thr=THR):
    """One pair's slots: inliers of h0 (match_xy = fp32(h0 xy), plus noise),
    outliers at least 2 thr away under h0, non-candidates inside the count and
    every slot past it carrying H2 correspondences that look like candidates
    apart from the one thing that excludes them.  Returns (points, planted
    inlier mask)."""
    while True:
        x = rng.uniform(20, FRAME_W - 20, slots).astype(np.float32)
        y = rng.uniform(20, FRAME_H - 20, slots).astype(np.float32)
        if count > 8 or count < 4 or min_height_ratio(x[:count].astype(float), y[:count].astype(float)) > 0.1:
            break
    p = np.zeros(slots, dtype)
    p["x"], p["y"] = x, y
    p["scale"], p["strength"], p["laplace"] = 2.0, 100.0, 1
    p["match_x"], p["match_y"] = f32_project(H2, x, y)
    p["match"] = np.arange(slots) % 7
    p["score"] = 0.9
    p["ambiguity"] = rng.uniform(0.2, 0.9, slots).astype(np.float32)
    idx = np.arange(count)
    non = idx[2::8] if (sprinkle and count >= 5) else idx[:0]
    p["match"][non[0::2]] = -1
    p["ambiguity"][non[1::2]] = AMB_ABOVE
    cand = np.setdiff1d(idx, non)
    if len(cand):
        p["ambiguity"][cand[0]] = AMB                                   # `<=` keeps the cut itself
    order = rng.permutation(cand)
    n_h1 = int(h1_frac * len(cand))
    n_out = int(out_frac * len(cand)) if len(cand) >= 12 else 0
    assert n_h1 + n_out <= 0.5 * len(cand)
    i_h1, i_out, i_in = order[:n_h1], order[n_h1:n_h1 + n_out], order[n_h1 + n_out:]
    u, v = f32_project(h0, x[i_in], y[i_in])
    if sigma:
        u = (u + rng.normal(0, sigma, len(i_in))).astype(np.float32)
        v = (v + rng.normal(0, sigma, len(i_in))).astype(np.float32)
    p["match_x"][i_in], p["match_y"][i_in] = u, v
    p["match_x"][i_h1], p["match_y"][i_h1] = f32_project(H1, x[i_h1], y[i_h1])
    for i in i_out:
        while True:
            uu, vv = np.float32(rng.uniform(0, FRAME_W)), np.float32(rng.uniform(0, FRAME_H))
            if transfer_err(h0, x[i], y[i], uu, vv) >= 4 * thr:
                break
        p["match_x"][i], p["match_y"][i] = uu, vv
    wrong = np.concatenate([i_h1, i_out]).astype(int)
    assert (transfer_err(h0, x[wrong], y[wrong], p["match_x"][wrong], p["match_y"][wrong]) >= 2 * thr).all()
    planted = np.zeros(slots, bool)
    planted[i_in] = True
    return p, planted


def run(surf, pts, counts, thr=THR, amb=float(AMB), nhyp=256, seed=0):
    """Upload, one surfhip_homography_batch call, download; checks the
    canaries behind both outputs and that the points are untouched."""
    npairs, slots = pts.shape
    pb, cb = surf.DeviceBuffer(pts.nbytes), surf.DeviceBuffer(4 * npairs)
    ob, mb = surf.DeviceBuffer(64 * (npairs + 1)), surf.DeviceBuffer(npairs * slots + 64)
    pb.upload(pts)
    cb.upload(np.asarray(counts, np.int32))
    ob.upload(np.full(64 * (npairs + 1), 0xA5, np.uint8))
    mb.upload(np.full(npairs * slots + 64, 0xA5, np.uint8))
    surf.homography_batch(pb.ptr, cb.ptr, slots, npairs, ob.ptr, mb.ptr, amb, thr, nhyp, seed)
    surf.synchronize()
    out = ob.download(np.uint8, 64 * (npairs + 1))
    mask = mb.download(np.uint8, npairs * slots + 64)
    back = pb.download(surf.POINT_DTYPE, npairs * slots)
    for b in (pb, cb, ob, mb):
        b.free()
    assert (out[64 * npairs:] == 0xA5).all() and (mask[npairs * slots:] == 0xA5).all()
    assert back.tobytes() == pts.tobytes()
    res = out[:64 * npairs].view(surf.HOMOGRAPHY_DTYPE)
    assert np.isfinite(res["h"]).all() and np.isfinite(res["rms"]).all()
    assert (res["reserved"] == 0).all()
    assert set(np.unique(mask[:npairs * slots])) <= {0, 1}
    return res, mask[:npairs * slots].reshape(npairs, slots)


def assert_failed(surf, res, mask, status):
    assert res["status"] == status
    assert res["h"].tobytes() == np.eye(3, dtype=np.float32).tobytes()
    assert res["ninliers"] == 0 and res["rms"] == 0 and not mask.any()


def assert_planted(surf, res, mask, pts, count, planted, thr=THR):
    assert res["ncand"] == candidate_mask(pts, count).sum()
    if res["ncand"] < 4:
        assert_failed(surf, res, mask, surf.HOMOG_TOO_FEW)
        return
    assert res["status"] == surf.HOMOG_OK
    assert res["ninliers"] == planted.sum()
    assert (mask.astype(bool) == planted).all(), np.nonzero(mask.astype(bool) != planted)[0][:8]
    e = transfer_err(res["h"], pts["x"], pts["y"], pts["match_x"], pts["match_y"])
    assert (e[planted] < thr).all()
    assert res["h"][8] == np.float32(1.0)
    assert 0 <= res["rms"] < thr


@functools.lru_cache(maxsize=None)
def ragged_data(surf):
    rng = np.random.default_rng(20240)
    pts, planted = [], []
    for i, c in enumerate(COUNTS):
        two = i == TWO_MODEL_PAIR
        p, m = plant_pair(rng, surf.POINT_DTYPE, SLOTS, c, H_KINDS[i % len(H_KINDS)],
                          out_frac=0.1 if two else 0.4, h1_frac=0.3 if two else 0.0)
        pts.append(p)
        planted.append(m)
    pts, planted = np.stack(pts), np.stack(planted)
    pts.setflags(write=False)
    planted.setflags(write=False)
    return pts, planted


@functools.lru_cache(maxsize=None)
def ragged_result(surf, seed=0):
    pts, _ = ragged_data(surf)
    res, mask = run(surf, pts, COUNTS, seed=seed)
    res.setflags(write=False)
    mask.setflags(write=False)
    return res, mask


# ------------------------------------------------------------------ tests

def test_planted_noise_free_ragged_batch(surf):
    pts, planted = ragged_data(surf)
    assert {i % len(H_KINDS) for i, c in enumerate(COUNTS) if c >= 4} == set(range(len(H_KINDS)))
    res, mask = ragged_result(surf)
    for i, c in enumerate(COUNTS):
        assert_planted(surf, res[i], mask[i], pts[i], c, planted[i])
    assert [int(s) for s in res["status"][:3]] == [surf.HOMOG_TOO_FEW] * 3
    assert [int(n) for n in res["ncand"][:3]] == [0, 1, 3]
    # the two-model pair: the smaller consensus is large enough to have won
    two = candidate_mask(pts[TWO_MODEL_PAIR], COUNTS[TWO_MODEL_PAIR])
    e1 = transfer_err(H1, *(pts[TWO_MODEL_PAIR][k] for k in ("x", "y", "match_x", "match_y")))
    assert (two & (e1 < THR)).sum() >= 0.29 * two.sum()


def test_accuracy_with_noise(surf):
    slots = 150
    for s in range(100):                      # a seed for which H0 itself leaves nobody in the 1 % band
        rng = np.random.default_rng(7000 + s)
        p, planted = plant_pair(rng, surf.POINT_DTYPE, slots, slots, H_PERSPECTIVE, out_frac=0.4, sigma=0.5,
                                sprinkle=False)
        e0 = transfer_err(H_PERSPECTIVE, p["x"], p["y"], p["match_x"], p["match_y"])
        if not ((e0 >= 0.98 * THR) & (e0 <= 1.02 * THR)).any() and (e0[planted] < 0.9 * THR).all():
            break
    else:
        raise AssertionError("no usable seed")
    assert planted.sum() == 90
    res, mask = run(surf, p[None], [slots])
    res, mask = res[0], mask[0]
    assert res["status"] == surf.HOMOG_OK and res["ncand"] == slots and res["h"][8] == np.float32(1.0)
    band_recheck(p, slots, res, mask)
    m = mask.astype(bool)
    fit = fit_dlt(p["x"][m], p["y"][m], p["match_x"][m], p["match_y"][m])
    d_num = corner_displacement(res["h"], fit)
    d_stat = corner_displacement(fit, H_PERSPECTIVE)
    print(f"homography accuracy: d_num {d_num:.3e} px, d_stat {d_stat:.3e} px, inliers {int(m.sum())}")
    assert d_num <= 0.1 * d_stat, (d_num, d_stat)
    rms = np.sqrt((transfer_err(res["h"], p["x"][m], p["y"][m], p["match_x"][m], p["match_y"][m]) ** 2).mean())
    assert abs(float(res["rms"]) - rms) <= 1e-3


def test_degenerate_inputs(surf):
    rng = np.random.default_rng(31)
    slots = 64
    good, planted = plant_pair(rng, surf.POINT_DTYPE, slots, slots, H_TRANSLATION)
    line = good.copy()                        # every candidate on one line of image 1
    t = np.linspace(0, 1, slots)
    line["x"], line["y"] = (100 + 1500 * t).astype(np.float32), (200 + 700 * t).astype(np.float32)
    line["match"], line["ambiguity"] = 1, 0.5
    line["match_x"], line["match_y"] = f32_project(H_TRANSLATION, line["x"], line["y"])
    same = line.copy()                        # every candidate the same correspondence
    same["x"], same["y"], same["match_x"], same["match_y"] = 400.0, 300.0, 410.0, 290.0
    four = good.copy()                        # 4 candidates, 3 of them on a line
    four["match"] = -1
    four["x"][:4], four["y"][:4] = (100, 500, 900, 300), (100, 300, 500, 800)
    four["match"][:4], four["ambiguity"][:4] = 2, 0.5
    four["match_x"][:4], four["match_y"][:4] = f32_project(H_TRANSLATION, four["x"][:4], four["y"][:4])
    pts = np.stack([line, same, four, good])
    res, mask = run(surf, pts, [slots] * 4)
    for i in range(3):
        assert res[i]["ncand"] == (slots, slots, 4)[i]
        assert_failed(surf, res[i], mask[i], surf.HOMOG_DEGENERATE)
    assert_planted(surf, res[3], mask[3], good, slots, planted)


def test_determinism_and_batch_independence(surf):
    pts, planted = ragged_data(surf)
    res, mask = ragged_result(surf)
    again, mask2 = run(surf, pts, COUNTS)
    assert again.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
    for i, c in enumerate(COUNTS):            # a pair alone = its row of the batch
        one, m = run(surf, pts[i:i + 1], [c])
        assert one.tobytes() == res[i:i + 1].tobytes() and m.tobytes() == mask[i:i + 1].tobytes(), i
    other, mask3 = ragged_result(surf, seed=12345)
    assert mask3.tobytes() == mask.tobytes()
    assert (other["ninliers"] == res["ninliers"]).all() and (other["status"] == res["status"]).all()


def test_above_the_lds_capacity(surf):
    cap = surf.HOMOGRAPHY_LDS_CAPACITY
    ncand = cap + 33
    slots = ncand + 40
    rng = np.random.default_rng(55)
    p, planted = plant_pair(rng, surf.POINT_DTYPE, slots, ncand, H_PERSPECTIVE, out_frac=0.3, sprinkle=False)
    assert candidate_mask(p, ncand).sum() == ncand and planted.sum() == ncand - int(0.3 * ncand)
    assert planted[cap:ncand].any() and not planted[cap:ncand].all()
    res, mask = run(surf, p[None], [ncand])
    assert_planted(surf, res[0], mask[0], p, ncand, planted)
    # with sprinkled non-candidates the candidate of rank `cap` sits further back
    q, planted_q = plant_pair(rng, surf.POINT_DTYPE, slots + 600, slots + 560, H_ROT90_SCALE, out_frac=0.3)
    assert candidate_mask(q, slots + 560).sum() > cap
    res, mask = run(surf, q[None], [slots + 560], seed=3)
    assert_planted(surf, res[0], mask[0], q, slots + 560, planted_q)


def test_real_pair(surf):
    a = np.load(os.path.join(GOLDEN, "left_1280x960_upright.npz"))
    z = np.load(os.path.join(GOLDEN, "match_left_right_upright.npz"))
    p = a["points"].view(surf.POINT_DTYPE).copy().reshape(-1)
    for f in ("score", "match", "match_x", "match_y", "ambiguity"):
        p[f] = z[f"ref_{f}"]
    n = len(p)
    assert candidate_mask(p, n).sum() == 804
    res, mask = run(surf, p[None], [n])
    res, mask = res[0], mask[0]
    print(f"real pair: ncand {res['ncand']}, inliers {res['ninliers']}, rms {res['rms']:.3f} px, h {res['h']}")
    assert res["status"] == surf.HOMOG_OK and res["ncand"] == 804
    assert res["ninliers"] >= 620
    band_recheck(p, n, res, mask)


def test_detect_match_homography_without_host_round_trip(surf):
    """detect_batch -> match_batch of consecutive frames -> homography_batch,
    all on the detector's own buffers and device counts, enqueued before
    anything is read back."""
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
    ob = surf.DeviceBuffer(64 * (n - 1))
    mb = surf.DeviceBuffer((n - 1) * max_pts)
    pb.zero()
    det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.match_batch(pb.ptr, db.ptr, cb.ptr, max_pts, pb.ptr + 48 * max_pts, db.ptr + 4 * max_pts * nf, cb.ptr + 4,
                     max_pts, n - 1, nf, 0)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob.ptr, mb.ptr)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    res = ob.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    mask = mb.download(np.uint8, (n - 1) * max_pts).reshape(n - 1, max_pts)
    det.close()
    assert counts.min() >= 64
    again, mask2 = run(surf, pts[:n - 1], counts[:n - 1])
    assert again.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
    assert np.isfinite(res["h"]).all()
    for i in range(n - 1):
        print(f"pair {i}: status {res[i]['status']}, ncand {res[i]['ncand']}, inliers {res[i]['ninliers']}")
        if res[i]["status"] == surf.HOMOG_OK:
            band_recheck(pts[i], counts[i], res[i], mask[i])
        else:
            assert not mask[i].any()
