"""GPU tests of the search phase of surfhip_homography_batch and
surfhip_fundamental_batch, one hypothesis at a time.  A whole RANSAC run
forgives a wrong sampler, rank lookup, minimal solver or tie rule, because
another hypothesis takes over; here the inputs are planted around the
documented sampling hash (ransac_ref.sample) so that exactly one hypothesis,
known in advance, can give the expected mask:

  a. nhyp = 1 and only the K sampled ranks follow the model: the mask reads
     the sampler out;
  b. the same above the LDS capacity: the checkpoint table, its binary search
     and the linear tail past the last checkpoint;
  c. nhyp = k + 1 with hypothesis k the only clean one (ransac_ref.clean_only),
     and nhyp = k against the float64 restatement;
  d. two disjoint consensus sets of equal size: the lower hypothesis index wins;
  e. the degeneracy thresholds of a single sample, from both sides.

Every planting is first run through the float64 restatement on the CPU
(ransac_ref.consensus), which must give the expected status and mask with
every planted inlier below 0.003 px (the data are noise-free; fp32
coordinates carry at most half an ulp of 1920, 6e-5 px), every other candidate
above 2 thr, and no count, threshold or degeneracy ratio close enough to its
limit for rounding to matter; a planting that fails is replaced by the next
planting seed.  On the GPU the mask and ninliers must then be equal exactly,
and every planted inlier within 0.03 px under the returned matrix (10 times
the reference's own bound, 100 times below thr)."""
from __future__ import annotations

import numpy as np
import pytest

import test_gpu_fundamental as tf
import test_gpu_homography as th
from ransac_ref import (AMB, AMB_ABOVE, FUNDAMENTAL, HOMOGRAPHY, THR, candidate_mask, clean_cover, clean_only,
                        consensus, fit_8pt, fit_dlt, octet, sample, sampson, transfer_err, triangle_ratio)

pytestmark = pytest.mark.gpu

FRAME_W, FRAME_H = 1920.0, 1080.0
FAR = 4 * THR                                          # planted outliers: at least this far under the model
TRIES = 64                                             # planting seeds tried before a test gives up


class Homog:
    """surfhip_homography_batch and what its plantings are made of."""
    name, kind, K, field = "homography", HOMOGRAPHY, 4, "h"
    models = th.H_KINDS
    rival = (th.H_PERSPECTIVE, th.H1)                  # the two consensus sets of the tie tests

    @staticmethod
    def cap(surf):
        return surf.HOMOGRAPHY_LDS_CAPACITY

    @staticmethod
    def run(surf, pts, counts, nhyp, seed):
        return th.run(surf, pts, counts, nhyp=nhyp, seed=seed)

    @staticmethod
    def err(model, x, y, u, v):
        return transfer_err(model, x, y, u, v)

    @staticmethod
    def fit(x, y, u, v):
        return fit_dlt(x, y, u, v)

    @staticmethod
    def inliers(rng, model, n):
        x = rng.uniform(20, FRAME_W - 20, n).astype(np.float32)
        y = rng.uniform(20, FRAME_H - 20, n).astype(np.float32)
        return (x, y) + th.f32_project(model, x, y)

    @classmethod
    def minimal(cls, rng, model):
        """A fat quadrilateral in both images."""
        while True:
            x, y, u, v = cls.inliers(rng, model, 4)
            x64, y64, u64, v64 = (a.astype(np.float64) for a in (x, y, u, v))
            if min(triangle_ratio(x64, y64), triangle_ratio(u64, v64)) > 0.1:
                return x, y, u, v

    @staticmethod
    def check_model(surf, res):
        assert res["status"] == surf.HOMOG_OK and res["h"][8] == np.float32(1.0)

    @staticmethod
    def check_failed(surf, res, mask, status):
        th.assert_failed(surf, res, mask, {1: surf.HOMOG_TOO_FEW, 2: surf.HOMOG_DEGENERATE}[status])


class Fund:
    """surfhip_fundamental_batch and what its plantings are made of."""
    name, kind, K, field = "fundamental", FUNDAMENTAL, 8, "f"
    models = tuple(tf.true_f(c) for c in tf.CAM_KINDS)
    cams = {m.tobytes(): c for m, c in zip(models, tf.CAM_KINDS)}
    rival = (models[0], models[2])

    @staticmethod
    def cap(surf):
        return surf.FUNDAMENTAL_LDS_CAPACITY

    @staticmethod
    def run(surf, pts, counts, nhyp, seed):
        return tf.run(surf, pts, counts, nhyp=nhyp, seed=seed)

    @staticmethod
    def err(model, x, y, u, v):
        return np.abs(sampson(model, x, y, u, v))

    @staticmethod
    def fit(x, y, u, v):
        return fit_8pt(x, y, u, v)

    @classmethod
    def inliers(cls, rng, model, n):
        return tf.view_pair(rng, cls.cams[model.tobytes()], n)

    @classmethod
    def minimal(cls, rng, model):
        """8 scene points whose system is far from rank-deficient."""
        while True:
            x, y, u, v = cls.inliers(rng, model, 8)
            if octet(*(a.astype(float) for a in (x, y, u, v)))[1] > 1e-4:
                return x, y, u, v

    @staticmethod
    def check_model(surf, res):
        assert res["status"] == surf.FUND_OK
        tf.assert_model_shape(res["f"])

    @staticmethod
    def check_failed(surf, res, mask, status):
        tf.assert_failed(surf, res, mask, {1: surf.FUND_TOO_FEW, 2: surf.FUND_DEGENERATE}[status])


CALLS = pytest.mark.parametrize("call", (Homog, Fund), ids=lambda c: c.name)


# ---------------------------------------------------------------- planting

def layout(ncand):
    """(count, point index of every candidate rank): every eighth point from
    the third on is no candidate, so a rank is not a point index."""
    idx = np.arange(ncand + ncand // 7 + 9)
    cand = idx[idx % 8 != 2][:ncand]
    return int(cand[-1]) + 1, cand


def blank_pair(rng, dtype, slots, ncand):
    """slots points that all carry decoy correspondences (th.H2): inside the
    count the non-candidates (match = -1, or the ambiguity one fp32 above the
    cut), past it slots that look like candidates.  Returns (points, count,
    point index per rank); the caller fills the candidates in."""
    count, cand = layout(ncand)
    assert count <= slots
    p = np.zeros(slots, dtype)
    p["x"] = rng.uniform(20, FRAME_W - 20, slots).astype(np.float32)
    p["y"] = rng.uniform(20, FRAME_H - 20, slots).astype(np.float32)
    p["scale"], p["strength"], p["laplace"] = 2.0, 100.0, 1
    p["match_x"], p["match_y"] = th.f32_project(th.H2, p["x"], p["y"])
    p["match"] = np.arange(slots) % 7
    p["score"] = 0.9
    p["ambiguity"] = rng.uniform(0.2, 0.9, slots).astype(np.float32)
    non = np.setdiff1d(np.arange(count), cand)
    p["match"][non[0::2]] = -1
    p["ambiguity"][non[1::2]] = AMB_ABOVE
    p["ambiguity"][cand[0]] = AMB                       # `<=` keeps the cut itself
    return p, count, cand


def put(p, at, corr):
    for k, a in zip(("x", "y", "match_x", "match_y"), corr):
        p[k][at] = a


def put_far(call, rng, p, at, models):
    """Random correspondences at the points `at`, at least FAR px from what
    every one of `models` predicts."""
    at = np.asarray(at, int)
    while len(at):
        n = len(at)
        c = (rng.uniform(20, FRAME_W - 20, n).astype(np.float32), rng.uniform(20, FRAME_H - 20, n).astype(np.float32),
             rng.uniform(0, FRAME_W, n).astype(np.float32), rng.uniform(0, FRAME_H, n).astype(np.float32))
        put(p, at, c)
        near = np.zeros(n, bool)
        for m in models:
            near |= ~(call.err(m, *c) >= FAR)
        at = at[near]


def put_inliers(call, rng, p, at, model, avoid=()):
    """Noise-free correspondences of `model` at the points `at`, each at
    least FAR px from what the models in `avoid` predict."""
    at = np.asarray(at, int)
    while len(at):
        c = call.inliers(rng, model, len(at))
        put(p, at, c)
        near = np.zeros(len(at), bool)
        for m in avoid:
            near |= ~(call.err(m, *c) >= FAR)
        at = at[near]


def cpu_check(call, p, count, nhyp, seed, planted, status=0):
    """The conditions of the module docstring on the float64 restatement."""
    st, _, mask, info = consensus(call.kind, p, count, THR, AMB, nhyp, seed)
    if st != status or not info["robust"]:
        return False
    if status != 0:
        return not mask.any()
    others = candidate_mask(p, count) & ~planted
    return bool((mask == planted).all() and (info["err"][planted] < 0.003).all() and
                (info["err"][others] > 2 * THR).all())


def gpu_check(call, surf, res, mask, p, count, planted):
    assert res["ncand"] == candidate_mask(p, count).sum()
    call.check_model(surf, res)
    got = mask.astype(bool)
    assert res["ninliers"] == planted.sum() == got.sum(), (int(res["ninliers"]), int(planted.sum()), int(got.sum()))
    assert (got == planted).all(), (np.nonzero(got & ~planted)[0][:8], np.nonzero(planted & ~got)[0][:8])
    e = call.err(res[call.field], *(p[k][planted] for k in ("x", "y", "match_x", "match_y")))
    assert (e < 0.03).all(), e.max()


def plant_sample_only(call, surf, key, slots, ncand, seed, model):
    """A pair in which only the K ranks of hypothesis 0 follow `model`; every
    other candidate is a random correspondence at least FAR px from the
    float64 fit of those K.  Returns (points, count, planted mask)."""
    ranks = sample(call.K, seed, 0, ncand)
    for s in range(TRIES):
        rng = np.random.default_rng([key, ncand, seed, s])
        p, count, cand = blank_pair(rng, surf.POINT_DTYPE, slots, ncand)
        c = call.minimal(rng, model)
        put(p, cand[ranks], c)
        fit = call.fit(*(a.astype(np.float64) for a in c))
        put_far(call, rng, p, np.setdiff1d(cand, cand[ranks]), [fit])
        planted = np.zeros(slots, bool)
        planted[cand[ranks]] = True
        if cpu_check(call, p, count, 1, seed, planted):
            return p, count, planted
    raise AssertionError(f"no usable planting: {call.name}, ncand {ncand}, seed {seed:#x}")


# ------------------------------------------------- a. the sampler, read out

SAMPLER_SEEDS = (0, 0xFFFFFFFF, 0x80000000, 1, 2, 3, 7, 12345, 0x7FFFFFFF, 0x9E3779B9, 0x61C88647, 0xDEADBEEF,
                 0x00010000, 0xFFFF0000, 0x55555555, 0xAAAAAAAA)
SAMPLER_NCAND = {4: (4, 5, 7), 8: (8, 9, 15)}
SAMPLER_NCAND_BOTH = (63, 64, 65, 255, 256, 257, 1000)


@CALLS
def test_sampler_read_out(surf, call):
    ncands = SAMPLER_NCAND[call.K] + SAMPLER_NCAND_BOTH
    slots = layout(max(ncands))[0] + 8
    assert len(SAMPLER_SEEDS) >= 16 and len(set(SAMPLER_SEEDS)) == len(SAMPLER_SEEDS)
    for seed in SAMPLER_SEEDS:
        pairs = [plant_sample_only(call, surf, 1, slots, n, seed, call.models[i % len(call.models)])
                 for i, n in enumerate(ncands)]
        res, mask = call.run(surf, np.stack([p for p, _, _ in pairs]), [c for _, c, _ in pairs], 1, seed)
        for i, (p, count, planted) in enumerate(pairs):
            assert res[i]["ncand"] == ncands[i]
            gpu_check(call, surf, res[i], mask[i], p, count, planted)


# ------------------------------------ b. rank lookup above the LDS capacity

# Found by trying seed = 0, 1, 2, ... with ransac_ref.sample(K, seed, 0, ncand) (cap = 3072).
# (i) the first seed whose ranks all lie at or above cap
ALL_ABOVE = {4: (3072 + 328, 24244), 8: (2 * 3072, 66)}
# (ii) the first (seed, ncand in cap + 300 .. cap + 400) whose sample holds cap - 1, cap and cap + 1
STRADDLE = {4: (3466, 40221936), 8: (3419, 45385)}
STRADDLE_RANKS = {4: [3072, 3073, 3071, 2416], 8: [2147, 3072, 473, 3071, 275, 1728, 3073, 2994]}
# (iii) the first seed with a rank among the candidates past point 511 * 256, the last checkpoint
PAST_TABLE_POINTS = 512 * 256 + 300
# (ranks 114933 and 114640 of 114950; the first rank behind the table is 114464)
PAST_TABLE = {4: 1169, 8: 202}


@CALLS
def test_rank_lookup_above_the_lds_capacity(surf, call):
    cap = call.cap(surf)
    assert cap == 3072
    ncand, seed = ALL_ABOVE[call.K]
    assert min(sample(call.K, seed, 0, ncand)) >= cap
    ncand2, seed2 = STRADDLE[call.K]
    assert sample(call.K, seed2, 0, ncand2) == STRADDLE_RANKS[call.K]
    assert {cap - 1, cap, cap + 1} <= set(STRADDLE_RANKS[call.K])
    slots = layout(max(ncand, ncand2))[0] + 8
    pairs = [plant_sample_only(call, surf, 2, slots, ncand, seed, call.models[0])]
    res, mask = call.run(surf, pairs[0][0][None], [pairs[0][1]], 1, seed)
    gpu_check(call, surf, res[0], mask[0], *pairs[0])
    pairs = [plant_sample_only(call, surf, 3, slots, ncand2, seed2, call.models[1])]
    res, mask = call.run(surf, pairs[0][0][None], [pairs[0][1]], 1, seed2)
    gpu_check(call, surf, res[0], mask[0], *pairs[0])


@CALLS
def test_rank_lookup_past_the_last_checkpoint(surf, call):
    """One pair of more than 512 * 256 points: the table ends at point
    511 * 256 and the candidates behind it are found by the linear walk."""
    seed = PAST_TABLE[call.K]
    ncand = int((np.arange(PAST_TABLE_POINTS) % 8 != 2).sum())
    count, cand = layout(ncand)
    assert count == PAST_TABLE_POINTS > 512 * 256
    ranks = sample(call.K, seed, 0, ncand)
    assert cand[max(ranks)] >= 511 * 256 and min(ranks) < call.cap(surf)
    p, count, planted = plant_sample_only(call, surf, 4, count + 8, ncand, seed, call.models[2])
    res, mask = call.run(surf, p[None], [count], 1, seed)
    gpu_check(call, surf, res[0], mask[0], p, count, planted)


# ------------------------------------------------ c. one clean hypothesis

def plant_clean(call, surf, key, n, seed, k, nhyp, model):
    """n candidates of which the ranks in clean_only's O are outliers and all
    others follow `model`: hypothesis k is the only clean one below nhyp."""
    got = clean_only(call.K, seed, k, nhyp, n)
    assert got is not None
    _, out = got
    for s in range(TRIES):
        rng = np.random.default_rng([key, n, k, s])
        p, count, cand = blank_pair(rng, surf.POINT_DTYPE, layout(n)[0] + 8, n)
        inl = np.setdiff1d(np.arange(n), out)
        put_inliers(call, rng, p, cand[inl], model)
        put_far(call, rng, p, cand[out], [model])
        planted = np.zeros(len(p), bool)
        planted[cand[inl]] = True
        if not cpu_check(call, p, count, nhyp, seed, planted):
            continue
        st, _, mask, info = consensus(call.kind, p, count, THR, AMB, k, seed)      # without hypothesis k
        if info["robust"] and not (st == 0 and (mask == planted).all()):
            return p, count, planted, st, mask
    raise AssertionError(f"no usable planting: {call.name}, n {n}, k {k}")


CLEAN_CASES = ((63, 64, 160), (64, 65, 160), (255, 256, 160), (256, 257, 160), (299, 300, 160), (4095, 4096, 400))


@CALLS
@pytest.mark.parametrize("k,nhyp,n", CLEAN_CASES)
def test_one_clean_hypothesis(surf, call, k, nhyp, n):
    assert nhyp == k + 1
    seed = 0
    p, count, planted, st, without = plant_clean(call, surf, 5, n, seed, k, nhyp, call.models[k % len(call.models)])
    res, mask = call.run(surf, p[None], [count], nhyp, seed)
    gpu_check(call, surf, res[0], mask[0], p, count, planted)
    # the same data without hypothesis k: what the float64 restatement gives, which is something else
    res, mask = call.run(surf, p[None], [count], k, seed)
    if st != 0:
        call.check_failed(surf, res[0], mask[0], st)
    else:
        call.check_model(surf, res[0])
        assert (mask[0].astype(bool) == without).all() and res[0]["ninliers"] == without.sum()
    assert not (mask[0].astype(bool) == planted).all()


# ----------------------------------------------------------- d. tie rule

def plant_tie(call, surf, key, n, seed, i, j, nhyp, first, second, shrink_first):
    """Two disjoint consensus sets: S1 holds sample i and follows `first`, S2
    holds sample j > i and follows `second`, the ranks of clean_cover's O are
    outliers of both.  Equal sizes, or S1 one smaller.  Returns (points,
    count, S1 mask, S2 mask)."""
    got = clean_cover(call.K, seed, [i, j], nhyp, n)
    assert got is not None and i < j < nhyp
    (si, sj), out = got
    rest = np.setdiff1d(np.arange(n), np.concatenate([si, sj, out]))
    out = list(out)
    if (len(rest) - (1 if shrink_first else 0)) % 2:
        out.append(int(rest[-1]))
        rest = rest[:-1]
    half = (len(rest) + 1) // 2
    s1, s2 = np.concatenate([si, rest[half:]]), np.concatenate([sj, rest[:half]])
    assert len(s2) - len(s1) == (1 if shrink_first else 0)
    for s in range(TRIES):
        rng = np.random.default_rng([key, i, j, s])
        p, count, cand = blank_pair(rng, surf.POINT_DTYPE, layout(n)[0] + 8, n)
        put_inliers(call, rng, p, cand[s1], first, avoid=[second])
        put_inliers(call, rng, p, cand[s2], second, avoid=[first])
        put_far(call, rng, p, cand[out], [first, second])
        m1, m2 = np.zeros(len(p), bool), np.zeros(len(p), bool)
        m1[cand[s1]], m2[cand[s2]] = True, True
        if cpu_check(call, p, count, nhyp, seed, m2 if shrink_first else m1):
            return p, count, m1, m2
    raise AssertionError(f"no usable planting: {call.name}, tie {i} {j}")


# (i, j, nhyp): two waves of one round; the same thread in two rounds
TIE_CASES = ((5, 70, 96), (1, 257, 300))


@CALLS
@pytest.mark.parametrize("i,j,nhyp", TIE_CASES)
def test_lowest_index_wins_a_tie(surf, call, i, j, nhyp):
    a, b = call.rival
    for first, second, shrink in ((a, b, False), (b, a, False), (a, b, True)):
        p, count, m1, m2 = plant_tie(call, surf, 6, 160, 0, i, j, nhyp, first, second, shrink)
        res, mask = call.run(surf, p[None], [count], nhyp, 0)
        gpu_check(call, surf, res[0], mask[0], p, count, m2 if shrink else m1)


# ------------------------------------------------- e. degenerate samples

def thin_quad(ratio, skip):
    """Four points of which the three not at position `skip` form a triangle
    with |cross| / longest^2 = ratio, the third inside the triangle of the
    other three; every other triple is fat."""
    a, b, d = np.array([300.0, 250.0]), np.array([1600.0, 400.0]), np.array([900.0, 950.0])
    ab = b - a
    c = 0.5 * (a + b) + ratio * np.array([-ab[1], ab[0]])           # height ratio * |ab| over the longest side ab
    q = [a, b, c]
    q.insert(skip, d)
    q = np.array(q, np.float32)
    got = triangle_ratio(q[:, 0].astype(float), q[:, 1].astype(float))
    assert abs(got / ratio - 1) < 0.01, got
    return q[:, 0], q[:, 1]


def test_homography_triangle_threshold(surf):
    """|cross| <= 1e-3 longest^2 in either image: at half of it the only
    sample is degenerate, at twice it the pair is solved."""
    pairs, want = [], []
    for ratio in (0.5e-3, 2e-3):
        for image in (1, 2):
            for skip in range(4):
                rng = np.random.default_rng([7, image, skip])
                p, count, cand = blank_pair(rng, surf.POINT_DTYPE, 16, 4)
                x, y = thin_quad(ratio, skip)
                if image == 1:
                    put(p, cand, (x, y) + th.f32_project(th.H_TRANSLATION, x, y))
                    assert abs(triangle_ratio(p["match_x"][cand].astype(float), p["match_y"][cand].astype(float))
                               / ratio - 1) < 0.01
                else:
                    # image 1: the same shape at 20 times the limit, so w > 0 at all four
                    put(p, cand, thin_quad(0.02, skip) + (x, y))
                planted = np.zeros(16, bool)
                planted[cand] = ratio > 1e-3
                st, _, ref, info = consensus(HOMOGRAPHY, p, count, nhyp=1)
                assert st == (0 if ratio > 1e-3 else 2) and (ref == planted).all()
                assert st != 0 or (info["err"][planted] < 0.003).all()
                pairs.append((p, count, planted))
                want.append(st)
    res, mask = Homog.run(surf, np.stack([p for p, _, _ in pairs]), [c for _, c, _ in pairs], 1, 0)
    for i, (p, count, planted) in enumerate(pairs):
        assert res[i]["ncand"] == 4
        if want[i]:
            Homog.check_failed(surf, res[i], mask[i], 2)
        else:
            gpu_check(Homog, surf, res[i], mask[i], p, count, planted)


def test_fundamental_rank_threshold(surf):
    """|last pivot| <= 1e-7 |first pivot|: an octet with s7 / s0 below 1e-9
    is degenerate, a well-spread one (above 1e-5) is solved."""
    pairs, want = [], []
    ki = np.linalg.inv(tf.K)
    for i, cam in enumerate(tf.CAM_KINDS):
        rng = np.random.default_rng([8, i])
        p, count, cand = blank_pair(rng, surf.POINT_DTYPE, 16, 8)
        x = np.float32([100, 300, 500, 700, 900, 1100, 1300, 640])          # 7 of 8 on a line of image 1
        y = np.float32([100, 200, 300, 400, 500, 600, 700, 900])
        q = tf.K @ (cam[0] @ (rng.uniform(4, 20, 8) * (ki @ np.stack([x, y, np.ones(8)]))) + cam[1][:, None])
        put(p, cand, (x, y, (q[0] / q[2]).astype(np.float32), (q[1] / q[2]).astype(np.float32)))
        assert octet(*(p[k][cand].astype(float) for k in ("x", "y", "match_x", "match_y")))[1] < 1e-9
        pairs.append((p, count, np.zeros(16, bool)))
        want.append(2)
        p, count, cand = blank_pair(rng, surf.POINT_DTYPE, 16, 8)
        put(p, cand, Fund.minimal(rng, Fund.models[i]))
        planted = np.zeros(16, bool)
        planted[cand] = True
        assert cpu_check(Fund, p, count, 1, 0, planted)
        pairs.append((p, count, planted))
        want.append(0)
    for (p, count, _), st in zip(pairs, want):
        assert consensus(FUNDAMENTAL, p, count, nhyp=1)[0] == st
    res, mask = Fund.run(surf, np.stack([p for p, _, _ in pairs]), [c for _, c, _ in pairs], 1, 0)
    for i, (p, count, planted) in enumerate(pairs):
        assert res[i]["ncand"] == 8
        if want[i]:
            Fund.check_failed(surf, res[i], mask[i], 2)
        else:
            gpu_check(Fund, surf, res[i], mask[i], p, count, planted)
