"""Float64 numpy reference of the two RANSAC calls (surfhip_homography_batch,
surfhip_fundamental_batch), shared by the GPU tests and the host test of
surfhip_fundamental_math.inc.  Not a test module.

What it holds: the candidate filter, the sampling hash and the K-rank draw,
the two distances, the two least-squares fits, a restatement of each whole
call (the same samples, float64 minimal solvers, two refits), a variant of
the restatement that also says whether its outcome can depend on rounding
(`consensus`), and the planting aid `clean_only` that leaves exactly one
chosen hypothesis free of outliers."""
from __future__ import annotations

import numpy as np

THR = 3.0
AMB = np.float32(0.95)
AMB_ABOVE = np.nextafter(AMB, np.float32(2))          # the first fp32 that fails `ambiguity <= 0.95f`
RANK_TOL = 1e-7                                        # an octet is degenerate below this singular-value ratio
COLLINEAR = 1e-3                                       # a triangle is degenerate when |cross| <= this * longest^2
TINY_H33 = 1e-12                                       # |h33| <= this * ||H||: no usable scale


def candidate_mask(pts, count, amb=AMB):
    n = min(max(int(count), 0), len(pts))
    ok = (pts["match"] >= 0) & (pts["ambiguity"] <= np.float32(amb))
    ok[n:] = False
    return ok


# ------------------------------------------------------------------ sampler

def fmix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample(K, seed, hyp, n):
    """Hypothesis hyp's K distinct candidate ranks below n (K = 4 or 8): draw
    j picks the d(j)-th, in ascending order, of the n - j ranks not taken yet."""
    taken, idx = [], []
    for j in range(K):
        r = fmix32(seed ^ ((0x9E3779B9 * (K * hyp + j + 1)) & 0xFFFFFFFF))
        d = r % (n - j)
        for s in sorted(taken):
            if d >= s:
                d += 1
        taken.append(d)
        idx.append(d)
    return idx


def sample8(seed, hyp, n):
    return sample(8, seed, hyp, n)


def clean_cover(K, seed, keep, nhyp, n):
    """The ranks of the samples in `keep` and a greedy set O of ranks,
    disjoint from them, that holds a rank of every other sample h < nhyp: the
    rank that hits most of the samples not hit yet, the lowest on a tie, until
    none is left.  None when the kept samples overlap or another sample lies
    inside their union (nothing outside could hit it)."""
    idx = np.array([sample(K, seed, h, n) for h in range(nhyp)])
    kept = [list(idx[k]) for k in keep]
    union = np.unique(np.concatenate(kept))
    if len(union) != K * len(keep):
        return None
    inc = np.zeros((nhyp, n), bool)
    inc[np.arange(nhyp)[:, None], idx] = True
    inc[:, union] = False
    todo = np.ones(nhyp, bool)
    todo[list(keep)] = False
    if not inc[todo].any(1).all():
        return None
    out = []
    while todo.any():
        r = int(np.argmax(inc[todo].sum(0)))
        out.append(r)
        todo &= ~inc[:, r]
    return kept, sorted(out)


def clean_only(K, seed, k, nhyp, n):
    """(ranks of sample k, O): with the ranks in O outliers and every other
    candidate an inlier, hypothesis k is the only one of the first nhyp drawn
    from inliers alone.  None if some other sample is a subset of sample k."""
    got = clean_cover(K, seed, [k], nhyp, n)
    return None if got is None else (got[0][0], got[1])


# --------------------------------------------------------------- homography

def project(h, x, y):
    h = np.asarray(h, np.float64).reshape(3, 3)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (h[0, 0] * x + h[0, 1] * y + h[0, 2]) / w, (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / w, w


def transfer_err(h, x, y, u, v):
    """One-way transfer error in image 2, px; w <= 0 is infinitely far."""
    px, py, w = project(h, x, y)
    with np.errstate(invalid="ignore"):
        e = np.hypot(px - np.asarray(u, np.float64), py - np.asarray(v, np.float64))
    return np.where(w > 0, e, np.inf)


def fit_dlt(x, y, u, v):
    """The documented cost, in float64 by QR/SVD least squares instead of
    normal equations: Hartley-normalise both point sets (centroid to the
    origin, mean distance sqrt 2), minimise sum (x h1 + y h2 + h3 - u (x h7 +
    y h8) - u)^2 + (x h4 + y h5 + h6 - v (x h7 + y h8) - v)^2 with h9 = 1,
    de-normalise, scale to h33 = 1."""
    x, y, u, v = (np.asarray(a, np.float64) for a in (x, y, u, v))
    c1, c2 = np.array([x.mean(), y.mean()]), np.array([u.mean(), v.mean()])
    s1 = np.sqrt(2) / np.hypot(x - c1[0], y - c1[1]).mean()
    s2 = np.sqrt(2) / np.hypot(u - c2[0], v - c2[1]).mean()
    xn, yn, un, vn = (x - c1[0]) * s1, (y - c1[1]) * s1, (u - c2[0]) * s2, (v - c2[1]) * s2
    n, z, o = len(x), np.zeros(len(x)), np.ones(len(x))
    a = np.concatenate([np.stack([xn, yn, o, z, z, z, -un * xn, -un * yn], 1),
                        np.stack([z, z, z, xn, yn, o, -vn * xn, -vn * yn], 1)])
    b = np.concatenate([un, vn])
    sol = np.linalg.lstsq(a, b, rcond=None)[0]
    hn = np.append(sol, 1.0).reshape(3, 3)
    t1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]])
    t2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    h = t2i @ hn @ t1
    assert n >= 4
    return h / h[2, 2]


def triangle_ratio(x, y):
    """Smallest |cross| / (longest side)^2 over the four triples of 4 points."""
    best = np.inf
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        cr = abs((x[j] - x[i]) * (y[k] - y[i]) - (y[j] - y[i]) * (x[k] - x[i]))
        l2 = max((x[j] - x[i]) ** 2 + (y[j] - y[i]) ** 2, (x[k] - x[i]) ** 2 + (y[k] - y[i]) ** 2,
                 (x[k] - x[j]) ** 2 + (y[k] - y[j]) ** 2)
        best = min(best, cr / l2 if l2 > 0 else 0.0)
    return best


def four_point(x, y, u, v):
    """The H through 4 correspondences by a float64 8 x 8 solve with h33 = 1;
    None when the system is singular or |h33| <= 1e-12 ||H||."""
    a, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        a[2 * i] = (x[i], y[i], 1, 0, 0, 0, -u[i] * x[i], -u[i] * y[i])
        a[2 * i + 1] = (0, 0, 0, x[i], y[i], 1, -v[i] * x[i], -v[i] * y[i])
        b[2 * i], b[2 * i + 1] = u[i], v[i]
    try:
        h = np.append(np.linalg.solve(a, b), 1.0)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(h).all() or not 1.0 > TINY_H33 * np.linalg.norm(h):
        return None
    return h


def hypotheses_h(x, y, u, v, nhyp, seed):
    """([nhyp][9] 4-point hypotheses, [nhyp] the smaller of the two images'
    triangle ratios).  A hypothesis is computed whenever it can be; the call
    itself uses only those whose ratio exceeds COLLINEAR."""
    n = len(x)
    out, ratio = np.zeros((nhyp, 9)), np.zeros(nhyp)
    for h in range(nhyp):
        i = np.array(sample(4, seed, h, n))
        ratio[h] = min(triangle_ratio(x[i], y[i]), triangle_ratio(u[i], v[i]))
        m = four_point(x[i], y[i], u[i], v[i]) if ratio[h] > 0 else None
        if m is None:
            ratio[h] = 0.0
        else:
            out[h] = m
    return out, ratio


# -------------------------------------------------------------- fundamental

def sampson(f, x, y, u, v):
    """Signed Sampson distance of (x, y) -> (u, v) under row-major f, px:
    r / sqrt(d) of the header's formula, in float64; d == 0 is infinitely far."""
    f = np.asarray(f, np.float64).reshape(3, 3)
    x, y, u, v = (np.asarray(a, np.float64) for a in (x, y, u, v))
    a = f[0, 0] * x + f[0, 1] * y + f[0, 2]
    b = f[1, 0] * x + f[1, 1] * y + f[1, 2]
    c = f[2, 0] * x + f[2, 1] * y + f[2, 2]
    a2 = f[0, 0] * u + f[1, 0] * v + f[2, 0]
    b2 = f[0, 1] * u + f[1, 1] * v + f[2, 1]
    r = u * a + v * b + c
    d = a * a + b * b + a2 * a2 + b2 * b2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, r / np.sqrt(d), np.inf)


def hartley(x, y):
    cx, cy = x.mean(), y.mean()
    s = np.sqrt(2) / np.hypot(x - cx, y - cy).mean()
    return (x - cx) * s, (y - cy) * s, np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])


def epipolar_rows(xn, yn, un, vn):
    return np.stack([un * xn, un * yn, un, vn * xn, vn * yn, vn, xn, yn, np.ones_like(xn)], -1)


def unit_signed(f):
    """Frobenius norm 1; the entry of largest magnitude (the first on a tie) positive."""
    f = f.reshape(9) / np.linalg.norm(f)
    return f if f[np.argmax(np.abs(f))] > 0 else -f


def fit_8pt(x, y, u, v):
    """The documented cost in float64, by SVD of the system itself instead of
    Jacobi on its normal matrix: Hartley-normalise both point sets, the right
    singular vector of the smallest singular value of the n x 9 epipolar
    system, the smallest singular value of that 3 x 3 matrix set to 0,
    de-normalise, Frobenius norm 1, sign."""
    x, y, u, v = (np.asarray(a, np.float64) for a in (x, y, u, v))
    assert len(x) >= 8
    xn, yn, t1 = hartley(x, y)
    un, vn, t2 = hartley(u, v)
    fn = np.linalg.svd(epipolar_rows(xn, yn, un, vn))[2][-1].reshape(3, 3)
    uu, s, vt = np.linalg.svd(fn)
    fn = uu @ np.diag([s[0], s[1], 0.0]) @ vt
    return unit_signed(t2.T @ fn @ t1)


def octet(x, y, u, v):
    """(unprojected unit-norm 8-point f[9] or None, s7 / s0 of the normalised
    8 x 9 system; 0 where the points of an image coincide)."""
    if not (np.hypot(x - x.mean(), y - y.mean()).mean() > 0 and np.hypot(u - u.mean(), v - v.mean()).mean() > 0):
        return None, 0.0
    xn, yn, t1 = hartley(x, y)
    un, vn, t2 = hartley(u, v)
    _, s, vt = np.linalg.svd(epipolar_rows(xn, yn, un, vn))
    f = t2.T @ vt[-1].reshape(3, 3) @ t1
    nf = np.linalg.norm(f)
    if not nf > 0:
        return None, 0.0
    return (f / nf).reshape(9), float(s[7] / s[0])


def hypotheses_f(x, y, u, v, nhyp, seed):
    """([nhyp][9] unprojected 8-point hypotheses, [nhyp] s7 / s0), computed
    whenever they can be; the call uses those whose ratio exceeds RANK_TOL."""
    n = len(x)
    out, ratio = np.zeros((nhyp, 9)), np.zeros(nhyp)
    for h in range(nhyp):
        i = np.array(sample(8, seed, h, n))
        f, ratio[h] = octet(x[i], y[i], u[i], v[i])
        if f is None:
            ratio[h] = 0.0
        else:
            out[h] = f
    return out, ratio


def hypotheses(x, y, u, v, nhyp, seed):
    """[nhyp][9] unprojected 8-point hypotheses (zero where the sample is
    degenerate), in float64."""
    out, ratio = hypotheses_f(x, y, u, v, nhyp, seed)
    out[~(ratio > RANK_TOL)] = 0.0
    return out


def restate(pts, count, thr=THR, amb=AMB, nhyp=256, seed=0):
    """The whole fundamental call in float64: (status, f[9] as fp32, mask over
    the slots); status 0 OK, 1 TOO_FEW, 2 DEGENERATE."""
    cand = np.nonzero(candidate_mask(pts, count, amb))[0]
    zero = (np.zeros(9, np.float32), np.zeros(len(pts), bool))
    if len(cand) < 8:
        return (1,) + zero
    x, y, u, v = (pts[k][cand].astype(np.float64) for k in ("x", "y", "match_x", "match_y"))
    hyp = hypotheses(x, y, u, v, nhyp, seed).astype(np.float32)
    counts = np.array([(np.abs(sampson(h, x, y, u, v)) < thr).sum() if h.any() else 0 for h in hyp])
    best = int(np.argmax(counts))                      # the first of the largest
    if counts[best] < 8:
        return (2,) + zero
    f = hyp[best]
    for _ in range(2):
        inl = np.abs(sampson(f, x, y, u, v)) < thr
        if inl.sum() < 8:
            return (2,) + zero
        f = fit_8pt(x[inl], y[inl], u[inl], v[inl]).astype(np.float32)
    inl = np.abs(sampson(f, x, y, u, v)) < thr
    if inl.sum() < 8:
        return (2,) + zero
    mask = np.zeros(len(pts), bool)
    mask[cand[inl]] = True
    return 0, f, mask


# ------------------------------------- both calls, with the rounding margin

class Kind:
    """What tells the two estimators apart for `consensus`."""

    def __init__(self, name, K, hyps, err, fit, tol, factor, failed):
        self.name, self.K, self.hyps, self.err, self.fit = name, K, hyps, err, fit
        self.tol, self.factor, self.failed = tol, factor, failed


HOMOGRAPHY = Kind("homography", 4, hypotheses_h, transfer_err,
                  lambda x, y, u, v: fit_dlt(x, y, u, v).reshape(9), COLLINEAR, 2.0,
                  np.eye(3, dtype=np.float32).reshape(9))
# the kernel's rule is on the pivot ratio under full pivoting, not on s7 / s0: a factor of 100 between them
FUNDAMENTAL = Kind("fundamental", 8, hypotheses_f, lambda f, x, y, u, v: np.abs(sampson(f, x, y, u, v)),
                   fit_8pt, RANK_TOL, 100.0, np.zeros(9, np.float32))


def consensus(kind, pts, count, thr=THR, amb=AMB, nhyp=256, seed=0, band=0.01):
    """The whole call of `kind` in float64: (status, model[9] as fp32, mask
    over the slots, info).  Hypotheses count from the sample's degeneracy
    ratio up: the winner is the first of the largest count, fewer than K is
    DEGENERATE, then two refits over the current inliers with a recount each.

    info["robust"] says that no rounding can change that outcome: with `lo`
    the count of a hypothesis within thr - band (0 unless its ratio is a
    factor above the threshold) and `hi` the count within thr + band (0 only
    if the ratio is the factor below), the winner's lo exceeds the hi of every
    earlier hypothesis and is not below that of any later one, and no
    candidate lies within `band` px of thr under the winner or either refit.
    info["winner"], info["ratio"] (per hypothesis), info["err"] (per
    candidate slot under the final model, inf elsewhere)."""
    cand = np.nonzero(candidate_mask(pts, count, amb))[0]
    info = {"robust": True, "winner": -1, "ratio": np.zeros(0), "err": np.full(len(pts), np.inf)}
    zero = (kind.failed.copy(), np.zeros(len(pts), bool), info)
    if len(cand) < kind.K:
        return (1,) + zero
    x, y, u, v = (pts[k][cand].astype(np.float64) for k in ("x", "y", "match_x", "match_y"))
    hyp, ratio = kind.hyps(x, y, u, v, nhyp, seed)
    hyp = hyp.astype(np.float32)
    info["ratio"] = ratio
    e = np.stack([kind.err(h, x, y, u, v) for h in hyp])
    cnt = np.where(ratio > kind.tol, (e < thr).sum(1), 0)
    lo = np.where(ratio > kind.tol * kind.factor, (e < thr - band).sum(1), 0)
    hi = np.where(ratio < kind.tol / kind.factor, 0, (e < thr + band).sum(1))
    best = int(np.argmax(cnt))
    info["winner"] = best
    if cnt[best] < kind.K:
        info["robust"] = bool(hi.max() < kind.K)
        return (2,) + zero
    info["robust"] = bool((hi[:best] < lo[best]).all() and (hi[best + 1:] <= lo[best]).all() and lo[best] >= kind.K)
    m = hyp[best]
    for step in range(3):
        err = kind.err(m, x, y, u, v)
        info["robust"] = info["robust"] and not (np.abs(err - thr) <= band).any()
        inl = err < thr
        if inl.sum() < kind.K:
            return (2,) + zero
        if step < 2:
            m = kind.fit(x[inl], y[inl], u[inl], v[inl]).astype(np.float32)
    mask = np.zeros(len(pts), bool)
    mask[cand[inl]] = True
    info["err"][cand] = err
    return 0, m, mask, info


def restate_h(pts, count, thr=THR, amb=AMB, nhyp=256, seed=0):
    """The whole homography call in float64: (status, h[9] as fp32, mask);
    status 0 OK, 1 TOO_FEW, 2 DEGENERATE (h = identity, zero mask)."""
    return consensus(HOMOGRAPHY, pts, count, thr, amb, nhyp, seed)[:3]
