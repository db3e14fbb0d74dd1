"""GPU tests of surfhip_fundamental_batch (batched RANSAC fundamental matrices
from the match fields of the set-1 points).  The host reference is numpy
float64, in ransac_ref.py: the Sampson distance, the candidate filter, the
sampling hash, the normalised 8-point fit with its rank-2 projection, and a
restatement of the whole call (the same samples, unprojected hypotheses, two
refits) that has to recover a planted scene on the CPU before the GPU's
result is compared with it."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ransac_ref import AMB, AMB_ABOVE, THR, candidate_mask, fit_8pt, restate, sampson

pytestmark = pytest.mark.gpu

FRAME_W, FRAME_H = 1920.0, 1080.0
SLOTS = 160
COUNTS = (0, 1, 7, 8, 9, 31, 64, 65, 96, 159, 160)
TWO_MODEL_PAIR = 10                                    # 30 % of its candidates follow CAM_SECOND
OUTLIER_PX = 60.0                                      # outliers: at least this far from their epipolar line
K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1.0]])


def rot(rx, ry, rz):
    """Rotation by rx, ry, rz degrees about x, then y, then z."""
    a, b, c = np.radians([rx, ry, rz])
    mx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    my = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    mz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return mz @ my @ mx


# camera 2 sees X2 = R X1 + t; depth 4 .. 20 units
CAM_STEREO = (rot(0.5, -3.0, 0.3), np.array([-0.8, 0.02, 0.05]))         # a verged stereo rig, baseline 0.8
CAM_FORWARD = (rot(-1.5, 2.0, -2.5), np.array([0.25, -0.1, -0.75]))      # mostly forward motion
CAM_VERTICAL = (rot(2.5, 1.0, 4.0), np.array([0.1, 0.8, 0.1]))           # a vertical baseline and a roll
CAM_KINDS = (CAM_STEREO, CAM_FORWARD, CAM_VERTICAL)
CAM_SECOND = (rot(3.0, 4.0, -3.0), np.array([0.5, 0.6, -0.3]))           # the smaller consensus
CAM_DECOY = (rot(-4.0, -2.0, 5.0), np.array([-0.3, -0.7, 0.4]))          # what must never be read


# ------------------------------------------------------- float64 reference

def true_f(cam):
    r, t = cam
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    ki = np.linalg.inv(K)
    f = ki.T @ tx @ r @ ki
    return f / np.linalg.norm(f)


def line_distance(f, x, y, u, v):
    """Distance of (u, v) from the epipolar line of (x, y), px."""
    f = np.asarray(f, np.float64).reshape(3, 3)
    a = f[0, 0] * x + f[0, 1] * y + f[0, 2]
    b = f[1, 0] * x + f[1, 1] * y + f[1, 2]
    c = f[2, 0] * x + f[2, 1] * y + f[2, 2]
    return np.abs(u * a + v * b + c) / np.hypot(a, b)


def restatement_recovers(pts, count, planted, thr=THR, nhyp=256, seed=0):
    """The float64 restatement finds exactly the planted inliers, all of them
    below 0.5 thr and every other candidate above 2 thr under its model."""
    status, f, mask = restate(pts, count, thr, AMB, nhyp, seed)
    assert status == 0
    assert (mask == planted).all(), np.nonzero(mask != planted)[0][:8]
    e = np.abs(sampson(f, pts["x"], pts["y"], pts["match_x"], pts["match_y"]))
    others = candidate_mask(pts, count) & ~planted
    assert (e[planted] < 0.5 * thr).all() and (e[others] > 2 * thr).all(), (e[planted].max(), e[others].min())
    return f


def band_recheck(pts, count, res, mask, thr=THR, amb=AMB):
    """The mask agrees with a float64 recount under the GPU's f for every
    candidate whose float64 distance lies outside [0.99, 1.01] thr; at most
    2 % of the candidates lie inside; nothing else is set."""
    cand = candidate_mask(pts, count, amb)
    assert int(res["ncand"]) == int(cand.sum())
    assert not mask[~cand].any()
    e = np.abs(sampson(res["f"], pts["x"], pts["y"], pts["match_x"], pts["match_y"]))
    inside = cand & (e >= 0.99 * thr) & (e <= 1.01 * thr)
    assert inside.sum() <= 0.02 * cand.sum(), (int(inside.sum()), int(cand.sum()))
    sure = cand & ~inside
    bad = np.nonzero(sure & (mask.astype(bool) != (e < thr)))[0]
    assert len(bad) == 0, (bad[:5], e[bad[:5]], mask[bad[:5]])
    assert abs(int(res["ninliers"]) - int((cand & (e < thr)).sum())) <= int(inside.sum())
    assert int(res["ninliers"]) == int(mask.sum())


def assert_model_shape(f):
    """Frobenius norm 1, rank 2, the sign rule, for the fp32 f."""
    f = np.asarray(f)
    assert f.dtype == np.float32
    f64 = f.astype(np.float64)
    assert abs(np.linalg.norm(f64) - 1.0) <= 1e-6
    s = np.linalg.svd(f64.reshape(3, 3), compute_uv=False)
    assert s[2] <= 1e-6 * s[0], s
    assert f[np.argmax(np.abs(f))] > 0


# --------------------------------------------------------------- planting

def view_pair(rng, cam, n):
    """n points of image 1 (fp32) and their fp32 images in camera 2: 3-D
    points at depth 4 .. 20 in front of camera 1, inside both frames."""
    r, t = cam
    ki = np.linalg.inv(K)
    x, y, u, v = (np.zeros(n, np.float32) for _ in range(4))
    for i in range(n):
        while True:
            xi, yi = np.float32(rng.uniform(20, FRAME_W - 20)), np.float32(rng.uniform(20, FRAME_H - 20))
            p = K @ (r @ (rng.uniform(4, 20) * (ki @ np.array([xi, yi, 1.0]))) + t)
            if p[2] > 1 and 20 <= p[0] / p[2] <= FRAME_W - 20 and 20 <= p[1] / p[2] <= FRAME_H - 20:
                break
        x[i], y[i], u[i], v[i] = xi, yi, p[0] / p[2], p[1] / p[2]
    return x, y, u, v


def plant_pair(rng, dtype, slots, count, cam, out_frac=0.4, second_frac=0.0, sigma=0.0, sprinkle=True):
    """One pair's slots: inliers of `cam` (plus noise), outliers at least
    OUTLIER_PX from their epipolar line, non-candidates inside the count and
    every slot past it carrying CAM_DECOY correspondences that look like
    candidates apart from the one thing that excludes them.  Pairs with fewer
    than 64 candidates get no outliers.  Returns (points, planted mask)."""
    f0 = true_f(cam)
    x, y, du, dv = view_pair(rng, CAM_DECOY, slots)
    p = np.zeros(slots, dtype)
    p["x"], p["y"] = x, y
    p["scale"], p["strength"], p["laplace"] = 2.0, 100.0, 1
    p["match_x"], p["match_y"] = du, dv
    p["match"] = np.arange(slots) % 7
    p["score"] = 0.9
    p["ambiguity"] = rng.uniform(0.2, 0.9, slots).astype(np.float32)
    idx = np.arange(count)
    non = idx[2::8] if (sprinkle and count >= 16) else idx[:0]
    p["match"][non[0::2]] = -1
    p["ambiguity"][non[1::2]] = AMB_ABOVE
    cand = np.setdiff1d(idx, non)
    if len(cand):
        p["ambiguity"][cand[0]] = AMB                                   # `<=` keeps the cut itself
    order = rng.permutation(cand)
    n_second = int(second_frac * len(cand))
    n_out = int(out_frac * len(cand)) if len(cand) >= 64 else 0
    assert n_second + n_out <= 0.5 * len(cand)
    i_second, i_out, i_in = order[:n_second], order[n_second:n_second + n_out], order[n_second + n_out:]
    ki = np.linalg.inv(K)
    for group, c, noise in ((i_in, cam, sigma), (i_second, CAM_SECOND, 0.0)):
        for i in group:
            while True:                                 # a depth whose image lies inside frame 2
                q = K @ (c[0] @ (rng.uniform(4, 20) * (ki @ np.array([x[i], y[i], 1.0]))) + c[1])
                if q[2] > 1 and 0 <= q[0] / q[2] <= FRAME_W and 0 <= q[1] / q[2] <= FRAME_H and (
                        c is cam or line_distance(f0, float(x[i]), float(y[i]), q[0] / q[2], q[1] / q[2]) >= OUTLIER_PX):
                    break
                x[i], y[i] = np.float32(rng.uniform(20, FRAME_W - 20)), np.float32(rng.uniform(20, FRAME_H - 20))
            p["x"][i], p["y"][i] = x[i], y[i]
            p["match_x"][i] = np.float32(q[0] / q[2] + (rng.normal(0, noise) if noise else 0.0))
            p["match_y"][i] = np.float32(q[1] / q[2] + (rng.normal(0, noise) if noise else 0.0))
    for i in i_out:
        while True:
            uu, vv = np.float32(rng.uniform(0, FRAME_W)), np.float32(rng.uniform(0, FRAME_H))
            if line_distance(f0, float(x[i]), float(y[i]), float(uu), float(vv)) >= OUTLIER_PX:
                break
        p["match_x"][i], p["match_y"][i] = uu, vv
    planted = np.zeros(slots, bool)
    planted[i_in] = True
    return p, planted


def run(surf, pts, counts, thr=THR, amb=float(AMB), nhyp=256, seed=0):
    """Upload, one surfhip_fundamental_batch call, download; checks the
    canaries behind both outputs and that the points are untouched."""
    npairs, slots = pts.shape
    pb, cb = surf.DeviceBuffer(pts.nbytes), surf.DeviceBuffer(4 * npairs)
    ob, mb = surf.DeviceBuffer(64 * (npairs + 1)), surf.DeviceBuffer(npairs * slots + 64)
    pb.upload(pts)
    cb.upload(np.asarray(counts, np.int32))
    ob.upload(np.full(64 * (npairs + 1), 0xA5, np.uint8))
    mb.upload(np.full(npairs * slots + 64, 0xA5, np.uint8))
    surf.fundamental_batch(pb.ptr, cb.ptr, slots, npairs, ob.ptr, mb.ptr, amb, thr, nhyp, seed)
    surf.synchronize()
    out = ob.download(np.uint8, 64 * (npairs + 1))
    mask = mb.download(np.uint8, npairs * slots + 64)
    back = pb.download(surf.POINT_DTYPE, npairs * slots)
    for b in (pb, cb, ob, mb):
        b.free()
    assert (out[64 * npairs:] == 0xA5).all() and (mask[npairs * slots:] == 0xA5).all()
    assert back.tobytes() == pts.tobytes()
    res = out[:64 * npairs].view(surf.FUNDAMENTAL_DTYPE)
    assert np.isfinite(res["f"]).all() and np.isfinite(res["rms"]).all()
    assert (res["reserved"] == 0).all()
    assert set(np.unique(mask[:npairs * slots])) <= {0, 1}
    return res, mask[:npairs * slots].reshape(npairs, slots)


def assert_failed(surf, res, mask, status):
    assert res["status"] == status
    assert res["f"].tobytes() == np.zeros(9, np.float32).tobytes()
    assert res["ninliers"] == 0 and res["rms"] == 0 and not mask.any()


def assert_planted(surf, res, mask, pts, count, planted, thr=THR):
    assert res["ncand"] == candidate_mask(pts, count).sum()
    if res["ncand"] < 8:
        assert_failed(surf, res, mask, surf.FUND_TOO_FEW)
        return
    assert res["status"] == surf.FUND_OK
    assert res["ninliers"] == planted.sum()
    assert (mask.astype(bool) == planted).all(), np.nonzero(mask.astype(bool) != planted)[0][:8]
    e = np.abs(sampson(res["f"], pts["x"], pts["y"], pts["match_x"], pts["match_y"]))
    assert (e[planted] < thr).all()
    assert_model_shape(res["f"])
    assert 0 <= res["rms"] < thr


RAGGED_SEED = 20250
SEEDS = (0, 12345)                                     # the call's `seed` values the ragged batch is run with


@functools.lru_cache(maxsize=None)
def ragged_data(surf):
    rng = np.random.default_rng(RAGGED_SEED)
    pts, planted = [], []
    for i, c in enumerate(COUNTS):
        two = i == TWO_MODEL_PAIR
        p, m = plant_pair(rng, surf.POINT_DTYPE, SLOTS, c, CAM_KINDS[i % len(CAM_KINDS)],
                          out_frac=0.1 if two else 0.4, second_frac=0.3 if two else 0.0)
        pts.append(p)
        planted.append(m)
    pts, planted = np.stack(pts), np.stack(planted)
    for seed in SEEDS:                                 # the restatement first, on the CPU
        for i, c in enumerate(COUNTS):
            if candidate_mask(pts[i], c).sum() >= 8:
                restatement_recovers(pts[i], c, planted[i], seed=seed)
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
    assert {i % len(CAM_KINDS) for i, c in enumerate(COUNTS) if c >= 8} == set(range(len(CAM_KINDS)))
    res, mask = ragged_result(surf)
    for i, c in enumerate(COUNTS):
        assert_planted(surf, res[i], mask[i], pts[i], c, planted[i])
    assert [int(s) for s in res["status"][:3]] == [surf.FUND_TOO_FEW] * 3
    assert [int(n) for n in res["ncand"][:3]] == [0, 1, 7]
    assert (res["status"][3:] == surf.FUND_OK).all()
    # the two-model pair: the smaller consensus is large enough to have won
    two = candidate_mask(pts[TWO_MODEL_PAIR], COUNTS[TWO_MODEL_PAIR])
    e1 = np.abs(sampson(true_f(CAM_SECOND), *(pts[TWO_MODEL_PAIR][k] for k in ("x", "y", "match_x", "match_y"))))
    assert (two & (e1 < THR)).sum() >= 0.29 * two.sum()


def test_mask_consistency(surf):
    pts, _ = ragged_data(surf)
    res, mask = ragged_result(surf)
    for i, c in enumerate(COUNTS):
        band_recheck(pts[i], c, res[i], mask[i])
        assert int(res[i]["ninliers"]) == int(mask[i].sum())


NOISE_SEED = 7000


def test_accuracy_with_noise(surf):
    slots = 150
    f0 = true_f(CAM_STEREO)
    for s in range(100):                      # a seed for which F0 itself leaves nobody in the 1 % band
        rng = np.random.default_rng(NOISE_SEED + s)
        p, planted = plant_pair(rng, surf.POINT_DTYPE, slots, slots, CAM_STEREO, out_frac=0.4, sigma=0.5,
                                sprinkle=False)
        e0 = np.abs(sampson(f0, p["x"], p["y"], p["match_x"], p["match_y"]))
        if not ((e0 >= 0.98 * THR) & (e0 <= 1.02 * THR)).any() and (e0[planted] < 0.9 * THR).all():
            break
    else:
        raise AssertionError("no usable seed")
    assert planted.sum() == 90
    status, f_cpu, mask_cpu = restate(p, slots)
    assert status == 0 and (mask_cpu == planted).all()
    res, mask = run(surf, p[None], [slots])
    res, mask = res[0], mask[0]
    assert res["status"] == surf.FUND_OK and res["ncand"] == slots
    assert_model_shape(res["f"])
    band_recheck(p, slots, res, mask)
    m = mask.astype(bool)
    xs = tuple(p[k][m] for k in ("x", "y", "match_x", "match_y"))
    fit = fit_8pt(*xs)
    f_gpu = res["f"].astype(np.float64)
    f_gpu = f_gpu if f_gpu @ fit >= 0 else -f_gpu      # signed distances need one common sign
    f_true = f0.reshape(9) if f0.reshape(9) @ fit >= 0 else -f0.reshape(9)
    d_num = float(np.abs(sampson(f_gpu, *xs) - sampson(fit, *xs)).max())
    d_stat = float(np.abs(sampson(fit, *xs) - sampson(f_true, *xs)).max())
    print(f"fundamental accuracy: d_num {d_num:.3e} px, d_stat {d_stat:.3e} px, inliers {int(m.sum())}")
    assert d_num <= 0.1 * d_stat, (d_num, d_stat)
    rms = np.sqrt((sampson(res["f"], *xs) ** 2).mean())
    assert abs(float(res["rms"]) - rms) <= 1e-3


def test_degenerate_inputs(surf):
    rng = np.random.default_rng(31)
    slots = 64
    good, planted = plant_pair(rng, surf.POINT_DTYPE, slots, slots, CAM_FORWARD, sprinkle=False)
    restatement_recovers(good, slots, planted)
    ki = np.linalg.inv(K)
    line = good.copy()                        # every candidate on one line of image 1
    t = np.linspace(0, 1, slots)
    line["x"], line["y"] = (100 + 1500 * t).astype(np.float32), (200 + 700 * t).astype(np.float32)
    line["match"], line["ambiguity"] = 1, 0.5
    for i in range(slots):
        q = K @ (CAM_FORWARD[0] @ (rng.uniform(4, 20) * (ki @ np.array([line["x"][i], line["y"][i], 1.0])))
                 + CAM_FORWARD[1])
        line["match_x"][i], line["match_y"][i] = q[0] / q[2], q[1] / q[2]
    same = line.copy()                        # every candidate the same correspondence
    same["x"], same["y"], same["match_x"], same["match_y"] = 400.0, 300.0, 410.0, 290.0
    eight = good.copy()                       # 8 candidates, 7 of them on a line of image 1
    eight["match"] = -1
    eight["x"][:8] = (100, 300, 500, 700, 900, 1100, 1300, 640)
    eight["y"][:8] = (100, 200, 300, 400, 500, 600, 700, 900)
    eight["match"][:8], eight["ambiguity"][:8] = 2, 0.5
    for i in range(8):
        q = K @ (CAM_FORWARD[0] @ (rng.uniform(4, 20) * (ki @ np.array([eight["x"][i], eight["y"][i], 1.0])))
                 + CAM_FORWARD[1])
        eight["match_x"][i], eight["match_y"][i] = q[0] / q[2], q[1] / q[2]
    pts = np.stack([line, same, eight, good])
    res, mask = run(surf, pts, [slots] * 4)
    for i in range(3):
        assert res[i]["ncand"] == (slots, slots, 8)[i]
        assert_failed(surf, res[i], mask[i], surf.FUND_DEGENERATE)
    assert_planted(surf, res[3], mask[3], good, slots, planted)


def test_determinism_and_batch_independence(surf):
    pts, planted = ragged_data(surf)
    res, mask = ragged_result(surf)
    again, mask2 = run(surf, pts, COUNTS)
    assert again.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
    for i, c in enumerate(COUNTS):            # a pair alone = its row of the batch
        one, m = run(surf, pts[i:i + 1], [c])
        assert one.tobytes() == res[i:i + 1].tobytes() and m.tobytes() == mask[i:i + 1].tobytes(), i
    other, mask3 = ragged_result(surf, seed=SEEDS[1])
    assert mask3.tobytes() == mask.tobytes()
    assert (other["ninliers"] == res["ninliers"]).all() and (other["status"] == res["status"]).all()


CAPACITY_SEED = 55


def test_above_the_lds_capacity(surf):
    cap = surf.FUNDAMENTAL_LDS_CAPACITY
    ncand = cap + 33
    slots = ncand + 40
    rng = np.random.default_rng(CAPACITY_SEED)
    p, planted = plant_pair(rng, surf.POINT_DTYPE, slots, ncand, CAM_VERTICAL, out_frac=0.3, sprinkle=False)
    assert candidate_mask(p, ncand).sum() == ncand and planted.sum() == ncand - int(0.3 * ncand)
    assert planted[cap:ncand].any() and not planted[cap:ncand].all() and planted[:cap].any()
    restatement_recovers(p, ncand, planted)
    res, mask = run(surf, p[None], [ncand])
    assert_planted(surf, res[0], mask[0], p, ncand, planted)
    # with sprinkled non-candidates the candidate of rank `cap` sits further back
    q, planted_q = plant_pair(rng, surf.POINT_DTYPE, slots + 600, slots + 560, CAM_STEREO, out_frac=0.3)
    cq = candidate_mask(q, slots + 560)
    assert cq.sum() > cap
    tail = np.nonzero(cq)[0][cap]
    assert tail > cap and planted_q[tail:].any() and not planted_q[tail:][cq[tail:]].all()
    restatement_recovers(q, slots + 560, planted_q, seed=3)
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
    res, mask = run(surf, p[None], [n], nhyp=1024)
    res, mask = res[0], mask[0]
    print(f"real pair: ncand {res['ncand']}, inliers {res['ninliers']}, rms {res['rms']:.3f} px, f {res['f']}")
    assert res["status"] == surf.FUND_OK and res["ncand"] == 804
    assert res["ninliers"] >= 620
    assert_model_shape(res["f"])
    band_recheck(p, n, res, mask)


def test_detect_match_fundamental_without_host_round_trip(surf):
    """detect_batch -> match_batch of consecutive frames -> fundamental_batch,
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
    surf.fundamental_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob.ptr, mb.ptr, nhyp=256)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    res = ob.download(surf.FUNDAMENTAL_DTYPE, n - 1)
    mask = mb.download(np.uint8, (n - 1) * max_pts).reshape(n - 1, max_pts)
    det.close()
    assert counts.min() >= 64
    again, mask2 = run(surf, pts[:n - 1], counts[:n - 1])
    assert again.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
    assert np.isfinite(res["f"]).all()
    for i in range(n - 1):
        print(f"pair {i}: status {res[i]['status']}, ncand {res[i]['ncand']}, inliers {res[i]['ninliers']}")
        if res[i]["status"] == surf.FUND_OK:
            band_recheck(pts[i], counts[i], res[i], mask[i])
        else:
            assert not mask[i].any()
