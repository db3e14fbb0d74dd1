"""The per-frame keypoint budget (surfhip_detector_set_keep): SURFHIP_KEEP_STRONGEST's selection kernel
(k_keep_strongest) ahead of k_sort_rank (batches of <= 8 frames) and k_sort (more), and SURFHIP_KEEP_FIRST
with a budget below max_pts.

Reference in every test: the oracle's points of the frame with room for all of them, in canonical order
(`or_find_points` on the planted planes, `or_detect_and_compute` on frames), and `select_strongest` on
them; every field bit for bit (`assert_points_equal`) and the counts.  The class a test names (a frame
over its budget, a tie across the cut, octaves KEEP_FIRST drops, ...) is decided on the reference side and
asserted populated before the GPU result is looked at.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_points_equal, desc_l2
from test_gpu_nms_planted import (BIG_PTS, F32, GEOMS, SORT_CAP, Campaign, Frame, Rig, cached, dense_set, fit_set,
                                  geo_of, peaks_set, same_points, sparse_frame, spikes_frame)
from test_gpu_parity import DESC_TOL

pytestmark = pytest.mark.gpu

RANK, BITONIC = 2, 9                    # batch sizes: k_sort_rank (<= 8 frames), k_sort (more)
MID_PTS = 8192                          # holds every frame here but the dense one


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def kept(surf, fr, n):
    """The oracle's points of a planted frame that KEEP_STRONGEST with budget n keeps, and all of them."""
    ref, cnt = fr.ref()
    assert cnt == len(ref)
    return ref[surf.select_strongest(ref, n)], ref


def cycle(frames, n):
    return [frames[i % len(frames)] for i in range(n)]


def check_strongest(surf, rig, frames, n, what):
    """One run_nms under (KEEP_STRONGEST, n): every frame equals the reference selection; candidates are
    the raw counts and nothing is reported truncated.  Returns the points' bytes per frame."""
    rig.det.set_keep(surf.KEEP_STRONGEST, n)
    assert rig.det.keep() == (surf.KEEP_STRONGEST, n if n else rig.max_pts)
    pts, counts, cand, trunc, total = rig.run(frames)
    for f, fr in enumerate(frames):
        want, ref = kept(surf, fr, n if n else rig.max_pts)
        tag = f"{what} frame {f} ({fr.name}), n {n}"
        assert counts[f] == len(want) == min(len(ref), n if n else rig.max_pts), (tag, counts[f], len(want))
        assert cand[f] == len(ref), (tag, cand[f], len(ref))
        same_points(pts[f], want, tag)
    assert not trunc, what
    return [p.tobytes() for p in pts]


def pool_over(orc, gname, n):
    """Frames of more than n points: the isolated peaks of every octave and level, and the noise frames."""
    frames = [peaks_set(orc, gname)[0][0]] + fit_set(orc, gname)[0][:4]
    assert all(fr.ref()[1] > n for fr in frames)
    return frames


# ------------------------------------------------------------ 1: frames within the budget

@pytest.mark.parametrize("nframes", [RANK, BITONIC])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_frames_within_budget_equal_keep_first(surf, orc, gname, nframes):
    geo = geo_of(orc, gname)
    frames = cycle(peaks_set(orc, gname)[0] + [sparse_frame(geo, 0), sparse_frame(geo, 2)], nframes)
    n = max(fr.ref()[1] for fr in frames)
    assert 0 < n < MID_PTS and min(fr.ref()[1] for fr in frames) < n        # at the budget and below it
    rig = Rig(surf, geo, nframes, max_pts=MID_PTS)
    first = [p.tobytes() for p in rig.run(frames)[0]]
    for budget in (n, n + 1, 0):
        assert check_strongest(surf, rig, frames, budget, "within budget") == first
    rig.close()


# ------------------------------------------------------------ 2: distinct strengths over the budget

@pytest.mark.parametrize("nframes", [RANK, BITONIC])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_strongest_of_distinct_strengths(surf, orc, gname, nframes):
    geo = geo_of(orc, gname)
    n = 50
    frames = cycle(pool_over(orc, gname, n), nframes)
    peaks = frames[0]
    want, ref = kept(surf, peaks, n)
    assert len(np.unique(bits(ref["strength"]))) == len(ref) > n              # distinct, over the budget
    assert set(np.unique(ref["o"])) == set(range(geo.noct))                   # peaks in every octave
    assert (ref["o"][:n] == 0).all()                                          # KEEP_FIRST at n: octave 0 only
    late = np.setdiff1d(surf.select_strongest(ref, n), np.arange(n))
    assert len(late) >= 8 and set(np.unique(ref["o"][late])) >= set(range(1, geo.noct)), np.bincount(ref["o"][late])
    assert len(np.unique(want["scale"])) > geo.noct                           # and both levels of some octave
    rig = Rig(surf, geo, nframes, max_pts=MID_PTS)
    got = check_strongest(surf, rig, frames, n, "distinct")
    again = check_strongest(surf, rig, frames[::-1], n, "distinct, reversed")  # the same bytes at any position
    assert got == again[::-1]
    rig.close()


# ------------------------------------------------------------ 3: ties across the cut

def tie_frame(geo):
    """Octave 0, level 0: 12 identical isolated 3x3x3 peaks (20 among 2s: the same 27 values, the same
    fit, the same strength bits), 5 single-sample peaks above them and 8 below."""
    def make():
        camp = Campaign(geo, limit=1)
        ny, nx = geo.nblocks(0, 0)
        for t in range(25):
            fi, pl, y, x, s, r, c = camp.site(0, 0, 0, range(3 + (t * 5) % 7, ny - 3), range(3 + (t * 11) % 23, nx - 3))
            if t % 2 == 0 and t < 24:
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        for e in (-1, 0, 1):
                            pl.put(0, s + a, r + b, c + e, F32(2.0))
                pl.put(0, s, r, c, F32(20.0))
            else:
                k = t // 2
                pl.put(0, s, r, c, F32(30.0 + k) if k < 5 else F32(6.0 + k))
        return Frame(geo, camp.frames[0].resp, img=1, name="ties")
    return cached(("ties", geo.name), make)


@pytest.mark.parametrize("nframes", [RANK, BITONIC])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_ties_across_the_cut(surf, orc, gname, nframes):
    geo = geo_of(orc, gname)
    fr = tie_frame(geo)
    ref, cnt = fr.ref()
    u = bits(ref["strength"])
    vals, num = np.unique(u, return_counts=True)
    tie = vals[num.argmax()]
    group = np.nonzero(u == tie)[0]
    above = int((ref["strength"] > ref["strength"][group[0]]).sum())
    assert len(group) == 12 and above == 5 and cnt == 25, (len(group), above, cnt)
    other = pool_over(orc, gname, 16)
    rig = Rig(surf, geo, nframes, max_pts=MID_PTS)
    for n in (above + 1, above + 7, above + 11):                             # the cut inside the tie group
        idx = surf.select_strongest(ref, n)
        inside = np.intersect1d(idx, group)
        assert 0 < len(inside) < len(group) and (inside == group[:len(inside)]).all()   # the earliest win
        frames = cycle([fr] + other[1:3] + [fr], nframes)
        check_strongest(surf, rig, frames, n, "ties")
    rig.close()


# ------------------------------------------------------------ 4: a mixed batch

@pytest.mark.parametrize("nframes", [5, BITONIC])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_mixed_batch(surf, orc, gname, nframes):
    """An empty frame, one below the budget, one exactly at it and frames above it in one batch (of 5:
    k_sort_rank; of 9: k_sort)."""
    geo = geo_of(orc, gname)
    pk, noise = peaks_set(orc, gname)[0], fit_set(orc, gname)[0]
    frames = [sparse_frame(geo, 0), sparse_frame(geo, 3), pk[1], pk[0], noise[1], noise[0], sparse_frame(geo, 0),
              sparse_frame(geo, 1), pk[0]][:nframes]
    n = pk[1].ref()[1]
    cnts = [fr.ref()[1] for fr in frames]
    assert 0 in cnts and n in cnts and any(0 < c < n for c in cnts) and sum(c > n for c in cnts) >= 2, (n, cnts)
    rig = Rig(surf, geo, nframes, max_pts=MID_PTS)
    check_strongest(surf, rig, frames, n, "mixed")
    rig.close()


# ------------------------------------------------------------ 5, 6: budgets and modes on one detector

@pytest.mark.parametrize("nframes", [RANK, BITONIC])
def test_budgets_and_modes_on_one_detector(surf, orc, nframes):
    geo = geo_of(orc, "640x400")
    frames = cycle(pool_over(orc, "640x400", 150), nframes)
    fresh = Rig(surf, geo, nframes, max_pts=MID_PTS)
    assert fresh.det.keep() == (surf.KEEP_FIRST, MID_PTS)                   # a new detector
    all_pts = fresh.run(frames)[0]
    fresh.close()
    for f, fr in enumerate(frames):
        same_points(all_pts[f], fr.ref()[0], f"keep-all frame {f}")
    rig = Rig(surf, geo, nframes, max_pts=MID_PTS)
    for n in (1, 150, 0, 37, MID_PTS, 100):                                  # changed between calls; 0 = max_pts
        check_strongest(surf, rig, frames, n, "budgets")
    # KEEP_FIRST below the frames' counts: the canonical prefix of the keep-all result
    for n in (1, 37, 128):
        rig.det.set_keep(surf.KEEP_FIRST, n)
        assert rig.det.keep() == (surf.KEEP_FIRST, n)
        pts, counts, cand, trunc, total = rig.run(frames)
        for f, fr in enumerate(frames):
            assert counts[f] == n and cand[f] == fr.ref()[1] and not trunc
            assert pts[f].tobytes() == all_pts[f][:n].tobytes(), f"KEEP_FIRST {n} frame {f}"
    # and back to the default: a fresh detector's bytes
    rig.det.set_keep(surf.KEEP_FIRST)
    assert rig.det.keep() == (surf.KEEP_FIRST, MID_PTS)
    back = rig.run(frames)[0]
    assert [p.tobytes() for p in back] == [p.tobytes() for p in all_pts]
    rig.close()


# ------------------------------------------------------------ 7: more slots than the LDS holds

@pytest.mark.parametrize("nframes", [RANK, BITONIC])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_dense_frame_global_path(surf, orc, gname, nframes):
    """More than kSortCap valid candidates (candidate capacity 32,768): k_keep_strongest re-reads keys and
    strengths from global memory, ahead of k_sort_rank's global keys / k_sort's global scratch."""
    geo = geo_of(orc, gname)
    dense = dense_set(orc, gname)[0]
    assert dense.ref()[1] > SORT_CAP
    frames = cycle([dense, sparse_frame(geo, 2), fit_set(orc, gname)[0][1], sparse_frame(geo, 0)], nframes - 1) + [dense]
    rig = Rig(surf, geo, nframes)
    assert rig.det.capacity() == BIG_PTS > SORT_CAP
    got = check_strongest(surf, rig, frames, 1000, "dense")
    assert got[0] == got[-1]
    rig.close()


# ------------------------------------------------------------ 8: the candidate capacity

def test_truncated_frame_selects_among_the_first_survivors(surf, orc):
    geo = geo_of(orc, "640x400")
    f257, flat = spikes_frame(geo, 257), sparse_frame(geo, 0)
    assert f257.ref()[1] == 257
    for nframes in (RANK, BITONIC):
        frames = [flat] * (nframes - 1) + [f257]
        rig = Rig(surf, geo, nframes, max_pts=512, cand_cap=256)
        assert rig.det.capacity() == 256
        pts, counts, cand, trunc, total = rig.run(frames)                   # KEEP_FIRST, n = max_pts
        assert trunc and counts[-1] == 256 and cand[-1] == 257
        first = pts[-1]
        for n in (100, 255, 256, 300):
            for mode in (surf.KEEP_STRONGEST, surf.KEEP_FIRST):
                rig.det.set_keep(mode, n)
                pts, counts, cand, trunc, total = rig.run(frames)
                assert trunc and cand[-1] == 257 and counts[-1] == min(n, 256), (n, mode, counts, cand, trunc)
                want = first[surf.select_strongest(first, n)] if mode == surf.KEEP_STRONGEST else first[:n]
                same_points(pts[-1], want, f"truncated, mode {mode}, n {n}")
        rig.close()


def test_over_budget_is_not_truncation(surf, orc):
    geo = geo_of(orc, "640x400")
    f256 = spikes_frame(geo, 256)
    assert f256.ref()[1] == 256
    rig = Rig(surf, geo, BITONIC, max_pts=512, cand_cap=256)
    for nframes in (RANK, BITONIC):
        got = check_strongest(surf, rig, [f256] * nframes, 100, "over the budget only")   # asserts not truncated,
        assert len(set(got)) == 1                                                          # candidates == 256
    rig.close()


# ------------------------------------------------------------ 9: argument checks

def test_set_keep_argument_checks(surf, orc):
    geo = geo_of(orc, "640x400")
    rig = Rig(surf, geo, 1, max_pts=64)
    lib, h = surf.lib, rig.det.h
    rig.det.set_keep(surf.KEEP_STRONGEST, 7)
    for mode, n in ((surf.KEEP_STRONGEST, -1), (surf.KEEP_STRONGEST, 65), (surf.KEEP_FIRST, 65), (2, 7), (-1, 7), (2, 0)):
        assert lib.surfhip_detector_set_keep(h, mode, n) == -1, (mode, n)     # SURFHIP_ERR_INVALID
        assert rig.det.keep() == (surf.KEEP_STRONGEST, 7)                    # and the setting stays
    with pytest.raises(surf.SurfError, match="invalid argument"):
        rig.det.set_keep(2, 7)
    m, n = C.c_int(), C.c_int()
    assert lib.surfhip_detector_get_keep(h, None, C.byref(n)) == -1 and lib.surfhip_detector_get_keep(h, C.byref(m), None) == -1
    assert lib.surfhip_detector_set_keep(None, 0, 0) == -1
    rig.det.set_keep(surf.KEEP_STRONGEST, 64)
    assert rig.det.keep() == (surf.KEEP_STRONGEST, 64)
    rig.det.set_keep(surf.KEEP_STRONGEST)
    assert rig.det.keep() == (surf.KEEP_STRONGEST, 64)
    rig.close()


# ------------------------------------------------------------ the whole pipeline, descriptors included

def golden_pair(surf):
    z = np.load(os.path.join(GOLDEN, "images.npz"))
    left = z["left_640x480"]
    right = surf.downsample2(z["right_1280x960"], 1280, 960)[:, :640]
    frames = np.zeros((2, 480, 640), np.uint8)
    frames[0], frames[1] = left, right
    return frames, 640, 480


def synth_nine(surf):
    return surf.synth_frames(9, 320, 240, first=200), 320, 240


def oracle_frames(orc, key, frames, w, h, upright):
    def make():
        op = orc.make_param(4, 4.0, upright=upright)
        return [orc.detect(op, frames[f], w, h) for f in range(len(frames))]
    return cached(("keep_oracle", key, upright), make)


class Pipe:
    """A detector with descriptors and its buffers; detect_batch + pack_slab of resident frames."""

    def __init__(self, surf, frames, w, h, upright, max_pts=4096):
        self.surf, self.n, self.w, self.h, self.max_pts = surf, len(frames), w, h, max_pts
        self.param = surf.make_param(4, 4.0, upright=upright)
        self.nf = self.param.nfeatures
        self.pitch = frames.shape[2]
        self.det = surf.Detector(self.param, w, h, max_batch=self.n, max_pts=max_pts)
        self.fb = surf.DeviceBuffer(frames.nbytes)
        self.fb.upload(frames)
        self.pb = surf.DeviceBuffer(48 * self.n * max_pts)
        self.db = surf.DeviceBuffer(4 * self.n * max_pts * self.nf)
        self.cb = surf.DeviceBuffer(4 * self.n)

    def run(self):
        surf, n, mp = self.surf, self.n, self.max_pts
        self.det.detect_batch(self.fb.ptr, n, self.pitch, self.h * self.pitch, self.pb.ptr, self.db.ptr, self.cb.ptr)
        total = self.det.batch_total(n)
        nbytes = self.det.slab_bytes(n, total)
        sb = surf.DeviceBuffer(nbytes)
        self.det.pack_slab(self.pb.ptr, self.db.ptr, self.cb.ptr, n, sb.ptr)
        surf.synchronize()
        counts = self.cb.download(np.int32, n)
        pts = self.pb.download(surf.POINT_DTYPE, n * mp).reshape(n, mp)
        desc = self.db.download(np.float32, n * mp * self.nf).reshape(n, mp, self.nf)
        slab = sb.download(np.uint8, nbytes)
        sb.free()
        return dict(counts=counts, pts=[pts[f, :counts[f]].copy() for f in range(n)],
                    desc=[desc[f, :counts[f]].copy() for f in range(n)], total=total, slab=slab,
                    cand=self.det.candidates(n), trunc=self.det.truncated())

    def close(self):
        self.det.close()
        for b in (self.fb, self.pb, self.db, self.cb):
            b.free()


def check_pipeline(surf, res, refs, n, upright):
    fields = ("x", "y", "scale", "o", "strength", "laplace", "ori")
    for f, (o_pts, o_desc, nc) in enumerate(refs):
        idx = surf.select_strongest(o_pts, n)
        assert res["counts"][f] == n == len(idx) and res["cand"][f] == nc == len(o_pts), (f, res["counts"][f], nc)
        try:
            assert_points_equal(res["pts"][f], o_pts[idx], fields=fields)      # laplace, and ori bit for bit
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from None
        if upright:
            assert (res["pts"][f]["ori"] == 0).all()
        err = desc_l2(res["desc"][f], o_desc[idx])
        assert err.max() <= DESC_TOL, f"frame {f}: descriptor L2 max {err.max():.3g} at {int(err.argmax())}"
    assert not res["trunc"]
    assert res["total"] == int(res["counts"].sum()) == n * len(refs)
    counts, pts, desc = surf.parse_slab(res["slab"])
    assert counts.tolist() == res["counts"].tolist() and len(pts) == res["total"] == len(desc)
    assert pts.tobytes() == np.concatenate(res["pts"]).tobytes()
    assert desc.tobytes() == np.concatenate(res["desc"]).tobytes()


@pytest.mark.parametrize("case", ["golden_pair", "synth_nine", "golden_pair_rotated"])
def test_pipeline_keeps_the_strongest(surf, orc, case):
    upright = not case.endswith("rotated")
    frames, w, h = golden_pair(surf) if case.startswith("golden") else synth_nine(surf)
    refs = oracle_frames(orc, case.replace("_rotated", ""), frames, w, h, upright)
    fewest = min(len(r[0]) for r in refs)
    n = min(200, fewest // 2)
    assert 8 <= n < fewest and all(nc == len(p) for p, _, nc in refs), (n, fewest)        # every frame over n
    for o_pts, _, _ in refs:                                                              # and the cut matters
        assert (np.setdiff1d(surf.select_strongest(o_pts, n), np.arange(n)).size > 0), "the strongest are the first"
    pipe = Pipe(surf, frames, w, h, upright)
    pipe.det.set_keep(surf.KEEP_STRONGEST, n)
    res = pipe.run()
    check_pipeline(surf, res, refs, n, upright)
    again = pipe.run()                                                                     # two identical calls
    assert again["slab"].tobytes() == res["slab"].tobytes()
    assert [p.tobytes() for p in again["pts"]] == [p.tobytes() for p in res["pts"]]
    assert [d.tobytes() for d in again["desc"]] == [d.tobytes() for d in res["desc"]]
    if upright:
        # the ingest ring runs through the detector: the same slab
        ing = surf.Ingest(pipe.det, 2)
        slot = ing.acquire()
        slot[:len(frames), :, :w] = frames[:, :, :w]
        ing.submit(len(frames))
        got = ing.collect()
        assert got.tobytes() == res["slab"].tobytes()
        ing.close()
    pipe.close()
