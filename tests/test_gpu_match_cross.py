"""GPU tests of surfhip_match_batch_cross (batched matching with the
mutual-best test): every comparison is bitwise on the five match fields
against a host model built from the CPU oracle's or_match alone.

The model.  Forward: or_match per pair (SAME_LAPLACE: the zero-row
construction of test_gpu_match_batch.test_same_laplace_flag).  Scores: column
j of the score matrix is or_match against set-2 point j alone with the full
tail on, which returns S(p1, j) where that is positive and 0 elsewhere -- the
oracle's own fp32 FMA chain, so the bits are the kernel's.  Back best: the
first maximum of a column where that maximum is positive."""
from __future__ import annotations

import numpy as np
import pytest

from match_ref import (CANARY, COUNTS1, COUNTS2, FULL_TAIL, KEPT_FIELDS, MATCH_FIELDS, SAME_LAPLACE, assert_match_equal,
                       back_best, clamp, cross_model, make_points, matrices, ragged_data, ragged_matrices, ragged_plain,
                       run_cross, score_column, with_canary)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- checking

def check_cross(orc, got, p1, f1, c1, p2, f2, c2, flags, mats):
    """got against the model per pair + the nothing-else-written properties
    (canary past the counts, detect fields); mats[i]: the pair's score matrix
    (its clamped counts).  Returns the per-pair (expected, forward) points."""
    s1, s2 = p1.shape[1], p2.shape[1]
    refs = []
    for i in range(len(p1)):
        n1, n2 = clamp(c1[i], s1), clamp(c2[i], s2)
        ref, fwd = cross_model(orc, mats[i], p1[i, :n1], p2[i, :n2], f1[i, :n1], f2[i, :n2], flags)
        assert_match_equal(got[i, :n1], ref, f"flags {flags} pair {i} (n1 {n1}, n2 {n2}): ")
        for f in MATCH_FIELDS:                                    # slots at or past n1: untouched
            assert (got[i, n1:][f].view(np.uint32) == p1[i, n1:][f].view(np.uint32)).all(), (i, f)
        for f in KEPT_FIELDS:
            assert (got[i][f].view(np.uint32) == p1[i][f].view(np.uint32)).all(), (i, f)
        refs.append((ref, fwd))
    return refs


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nf", [64, 128, 36])
def test_ragged_batch(surf, orc, nf, flags):
    """Empty sets, partial point tiles, a live block with dead waves (33),
    two blocks per pair (160: the maximum across blocks), the any-length
    kernel (36), n1 >> n2 (160 against 7 with the full tail)."""
    p1, f1, p2, f2 = ragged_data(surf, nf)
    got = run_cross(surf, p1, f1, COUNTS1, p2, f2, COUNTS2, flags)
    refs = check_cross(orc, got, p1, f1, COUNTS1, p2, f2, COUNTS2, flags, ragged_matrices(surf, orc, nf))
    plain = ragged_plain(surf, nf, flags)
    for i, (n1, n2) in enumerate(zip(COUNTS1, COUNTS2)):
        g, (ref, fwd) = got[i, :n1], refs[i]
        assert_match_equal(plain[i, :n1], fwd, f"match_batch, pair {i}: ")
        kept = g["match"] >= 0
        cleared = (fwd["match"] >= 0) & ~kept
        print(f"nf {nf} flags {flags} pair {i} ({n1} x {n2}): kept {kept.sum()}, cleared {cleared.sum()}")
        nscan = n2 if flags & FULL_TAIL else 32 * (n2 // 32)
        if n1 >= 31 and nscan >= 32:
            assert kept.sum() >= 12 and cleared.sum() >= 12, (i, kept.sum(), cleared.sum())
        m = g["match"][kept]
        assert len(np.unique(m)) == len(m), f"pair {i}: the kept matches share partners"
        for f in ("score", "ambiguity"):                          # a cleared point keeps the forward values
            assert (g[f].view(np.uint32) == plain[i, :n1][f].view(np.uint32)).all(), (i, f)
        assert_match_equal(g[kept], plain[i, :n1][kept], f"kept points, pair {i}: ")
        assert (g["match_x"][cleared] == 0).all() and (g["match_y"][cleared] == 0).all()


def test_ties_sign_and_nan(surf, orc):
    """Pair 0 (128 x 191 of the ragged data): three bitwise equal set-1 rows
    choose one partner with one score, the lowest index keeps it; a row with a
    NaN is never anybody's best.  Pair 1 (the same against |set 2|): a row
    without a positive score neither matches nor is a back best."""
    nf, n1, n2 = 64, 128, 191
    i = COUNTS1.index(n1)
    assert COUNTS2[i] == n2
    rp1, rf1, rp2, rf2 = ragged_data(surf, nf)
    p1 = np.stack([rp1[i], rp1[i]])
    p2 = np.stack([rp2[i], rp2[i]])
    f1 = np.stack([rf1[i], rf1[i]])
    f2 = np.stack([rf2[i], np.abs(rf2[i])])
    f1[0, 40] = f1[0, 100] = f1[0, 7]
    f1[:, 77, 5] = np.nan
    f1[1, 50] = -np.abs(f1[1, 50])
    c1, c2 = [n1, n1], [n2, n2]
    mats = matrices(orc, p1, f1, c1, f2, c2)
    assert (mats[1][50] == 0).all() and (mats[0][77] == 0).all() and (mats[1][77] == 0).all()
    for flags in (0, FULL_TAIL):
        got = run_cross(surf, p1, f1, c1, p2, f2, c2, flags)
        refs = check_cross(orc, got, p1, f1, c1, p2, f2, c2, flags, mats)
        fwd = refs[0][1]
        trio = [7, 40, 100]
        assert len(set(fwd["match"][trio])) == 1 and fwd["match"][7] >= 0
        assert len(set(fwd["score"][trio].view(np.uint32))) == 1
        assert got[0, 7]["match"] == fwd["match"][7] and got[0, 40]["match"] == -1 and got[0, 100]["match"] == -1
        for k in (0, 1):
            assert got[k, 77]["match"] == -1 and got[k, 77]["score"] == 0
            assert back_best(mats[k], p1[k, :n1], p2[k, :n2], flags).tolist().count(77) == 0
        assert got[1, 50]["match"] == -1 and got[1, 50]["score"] == 0
        assert back_best(mats[1], p1[1, :n1], p2[1, :n2], flags).tolist().count(50) == 0


def test_three_blocks(surf, orc):
    """n1 = 290 of 300 slots (three 128-point blocks) against 64: for the
    planted set-2 points the back best sits in another block than the forward
    points that chose them, so the maximum has to cross blocks."""
    nf, s1, n1, n2 = 64, 300, 290, 64
    rng = np.random.default_rng(77)
    f1 = rng.standard_normal((1, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((1, n2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    # (set-2 point, its exact copy in set 1, a noisy copy in another block)
    plants = [(3, 270, 5), (17, 10, 200), (40, 130, 280), (41, 289, 127), (63, 0, 256)]
    for j, exact, noisy in plants:
        f1[0, exact] = f2[0, j]
        v = f2[0, j] + 0.05 * rng.standard_normal(nf).astype(np.float32)
        f1[0, noisy] = v / np.linalg.norm(v)
    f1[0, n1:] = 1000.0
    p1 = with_canary(make_points(rng, 1, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)
    mats = matrices(orc, p1, f1, [n1], f2, [n2])
    for flags in (0, SAME_LAPLACE):
        if flags:
            for j, exact, noisy in plants:                        # the planted trios share a sign
                p1["laplace"][0, [exact, noisy]] = p2["laplace"][0, j]
        got = run_cross(surf, p1, f1, [n1], p2, f2, [n2], flags)
        (ref, fwd), = check_cross(orc, got, p1, f1, [n1], p2, f2, [n2], flags, mats)
        b = back_best(mats[0], p1[0, :n1], p2[0], flags)
        for j, exact, noisy in plants:
            assert fwd["match"][exact] == j and fwd["match"][noisy] == j and b[j] == exact
            assert exact // 128 != noisy // 128
            assert got[0, exact]["match"] == j and got[0, noisy]["match"] == -1


def test_scratch_reuse(surf, orc):
    """The scratch may hold anything: all-0xFF first, then the keys of a
    call with stronger scores (a stale maximum would win every column)."""
    nf, s1, s2 = 64, 160, 96
    rng = np.random.default_rng(55)
    f1 = rng.standard_normal((2, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((2, s2, nf)).astype(np.float32)
    f1 /= np.linalg.norm(f1, axis=2, keepdims=True)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    strong = (4.0 * f1).astype(np.float32)
    weak = np.ascontiguousarray(f1[:, ::-1])                      # other pairings, a quarter of the scores
    p1 = with_canary(make_points(rng, 2, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 2, s2, surf.POINT_DTYPE)
    c1, c2 = [s1, 150], [s2, 90]
    scratch = surf.DeviceBuffer(surf.match_batch_cross_scratch_bytes(2, s1, s2))
    scratch.upload(np.full(scratch.nbytes, 0xFF, np.uint8))
    runs = []
    for fa in (strong, weak, weak):
        got = run_cross(surf, p1, fa, c1, p2, f2, c2, FULL_TAIL, scratch=scratch)
        check_cross(orc, got, p1, fa, c1, p2, f2, c2, FULL_TAIL, matrices(orc, p1, fa, c1, f2, c2))
        runs.append(got)
    scratch.free()
    assert runs[1].tobytes() == runs[2].tobytes()
    assert runs[0]["score"][0, :s1].min() > runs[1]["score"][0, :s1].max()


def test_position_independence(surf, orc):
    """One pair at positions 0, 5 and 11 of a batch of unrelated pairs."""
    nf, src = 64, 10                                              # 159 x 192: two blocks
    rp1, rf1, rp2, rf2 = ragged_data(surf, nf)
    p1, f1, p2, f2 = rp1.copy(), rf1.copy(), rp2.copy(), rf2.copy()
    c1, c2 = list(COUNTS1), list(COUNTS2)
    where = (0, 5, 11)
    for k in where:
        p1[k], f1[k], p2[k], f2[k], c1[k], c2[k] = rp1[src], rf1[src], rp2[src], rf2[src], COUNTS1[src], COUNTS2[src]
    for flags in (0, FULL_TAIL | SAME_LAPLACE):
        got = run_cross(surf, p1, f1, c1, p2, f2, c2, flags)
        for k in where[1:]:
            assert got[k].tobytes() == got[where[0]].tobytes(), (flags, k)
        mats = ragged_matrices(surf, orc, nf)
        check_cross(orc, got, p1, f1, c1, p2, f2, c2, flags, [mats[src] if k in where else mats[k] for k in range(12)])


def test_counts_are_clamped(surf, orc):
    nf, s1, s2 = 64, 70, 100
    rng = np.random.default_rng(44)
    f1 = rng.standard_normal((3, s1, nf)).astype(np.float32)
    f2 = rng.standard_normal((3, s2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 3, s1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, s2, surf.POINT_DTYPE)
    c1, c2 = [s1 + 9, 40, -3], [s2 + 9, -3, 64]
    got = run_cross(surf, p1, f1, c1, p2, f2, c2, FULL_TAIL)
    check_cross(orc, got, p1, f1, c1, p2, f2, c2, FULL_TAIL, matrices(orc, p1, f1, c1, f2, c2))
    assert (got[0]["match"] >= 0).sum() >= 12                     # all 70 slots against all 100
    assert (got[1, :40]["match"] == -1).all()                     # n2 = 0
    assert (got[2]["match"] == CANARY["match"]).all()             # n1 = 0: nothing written


def test_detect_cross_match_homography_without_host_round_trip(surf, orc):
    """detect_batch -> match_batch_cross of consecutive frames on the
    detector's own buffers (set 2 = set 1 advanced one frame) ->
    homography_batch, enqueued without reading anything back in between; then
    the plain match_batch -> homography_batch on the same buffers."""
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
    sb = surf.DeviceBuffer(surf.match_batch_cross_scratch_bytes(n - 1, max_pts, max_pts))
    pb.zero()
    set2 = (pb.ptr + 48 * max_pts, db.ptr + 4 * max_pts * nf, cb.ptr + 4, max_pts)
    det.detect_batch(fb.ptr, n, pitch, h * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.match_batch_cross(pb.ptr, db.ptr, cb.ptr, max_pts, *set2, n - 1, nf, sb.ptr)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob.ptr)
    surf.synchronize()
    counts = cb.download(np.int32, n)
    assert counts.min() >= 64 and counts.max() <= max_pts
    pts = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    desc = db.download(np.float32, n * max_pts * nf).reshape(n, max_pts, nf)
    res = ob.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    surf.match_batch(pb.ptr, db.ptr, cb.ptr, max_pts, *set2, n - 1, nf, 0)
    surf.homography_batch(pb.ptr, cb.ptr, max_pts, n - 1, ob.ptr)
    surf.synchronize()
    pts_plain = pb.download(surf.POINT_DTYPE, n * max_pts).reshape(n, max_pts)
    res_plain = ob.download(surf.HOMOGRAPHY_DTYPE, n - 1)
    for b in (fb, pb, db, cb, ob, sb):
        b.free()
    det.close()

    def ncand(p):
        return int(((p["match"] >= 0) & (p["ambiguity"] <= np.float32(0.95))).sum())

    fewer = 0
    for i in range(n - 1):
        a, b = counts[i], counts[i + 1]
        p1, f1, f2 = pts[i, :a], desc[i, :a], desc[i + 1, :b]
        fwd = orc.match(p1, pts[i + 1, :b], f1, f2, full_tail=False)
        assert_match_equal(pts_plain[i, :a], fwd, f"match_batch, pair {i}: ")
        ref = fwd.copy()
        for j in np.unique(fwd["match"][fwd["match"] >= 0]):      # B only where a forward match names the column
            col = score_column(orc, p1, f1, f2[j])
            rows = np.nonzero(fwd["match"] == j)[0]
            assert col.max() > 0 and (col[rows].view(np.uint32) == fwd["score"][rows].view(np.uint32)).all()
            lose = rows[rows != int(col.argmax())]
            ref["match"][lose] = -1
            ref["match_x"][lose] = 0.0
            ref["match_y"][lose] = 0.0
        assert_match_equal(pts[i, :a], ref, f"pair {i}: ")
        assert int(res[i]["ncand"]) == ncand(pts[i, :a]) and int(res_plain[i]["ncand"]) == ncand(pts_plain[i, :a])
        print(f"pair {i}: ncand {res[i]['ncand']} with the mutual test, {res_plain[i]['ncand']} without")
        assert res[i]["ncand"] <= res_plain[i]["ncand"]
        fewer += int(res[i]["ncand"] < res_plain[i]["ncand"])
    assert fewer >= 1
