"""surfhip_fundamental_math.inc and the sampler of both RANSAC kernels,
surfhip_ransac_sample.inc, on the CPU: tests/host/fundamental_math_main.cpp
includes the very files the kernels include, built here with g++ and the
address and undefined-behaviour sanitizers, and each of its functions is
compared with a float64 numpy reference (ransac_ref.py, numpy.linalg).  No
GPU is involved.  The bounds are derived in the tests that use them; the
largest values observed are printed (pytest -s) and quoted in DESIGN.md."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from ransac_ref import epipolar_rows, fit_8pt, hartley, octet, sample, sampson

GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ is not installed: the host program cannot be built")

U32 = 2.0 ** -24                                       # unit roundoff of fp32
ANGLE = 2.0 ** -22                                     # see test_eight_point
K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1.0]])
FRAME_W, FRAME_H = 1920.0, 1080.0


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fundamental_math") / "fundamental_math_main")
    # the sanitizer runtimes linked in: the shared ones refuse to start behind any library the
    # environment preloads, and nothing here touches the environment of the child
    cmd = [GXX, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-Wall",
           "-I", os.path.join(REPO, "cuda-surf_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "fundamental_math_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(prog, tmp_path, cases):
    """The program as a child process on the case stream; exit status 0 and
    an empty stderr (the sanitizers report there); the result bytes."""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as f:
        f.write(cases)
    r = subprocess.run([prog, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    with open(dst, "rb") as f:
        return f.read()


def head(op, count):
    return struct.pack("<ii", op, count)


# ------------------------------------------------------------------ scenes

def rot(rx, ry, rz):
    a, b, c = np.radians([rx, ry, rz])
    mx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    my = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    mz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return mz @ my @ mx


# the three camera geometries of tests/test_gpu_fundamental.py: X2 = R X1 + t
CAMS = ((rot(0.5, -3.0, 0.3), np.array([-0.8, 0.02, 0.05])),
        (rot(-1.5, 2.0, -2.5), np.array([0.25, -0.1, -0.75])),
        (rot(2.5, 1.0, 4.0), np.array([0.1, 0.8, 0.1])))


def views(rng, cam, n, sigma=0.0):
    """n fp32 points of image 1 and their fp32 images in camera 2 (depth
    4 .. 20, inside both frames), as float64 arrays."""
    r, t = cam
    ki = np.linalg.inv(K)
    x, y, u, v = (np.zeros(0) for _ in range(4))
    while len(x) < n:
        m = 2 * n + 16
        xi = rng.uniform(20, FRAME_W - 20, m).astype(np.float32).astype(np.float64)
        yi = rng.uniform(20, FRAME_H - 20, m).astype(np.float32).astype(np.float64)
        p = K @ (r @ (rng.uniform(4, 20, m) * (ki @ np.stack([xi, yi, np.ones(m)]))) + t[:, None])
        ui, vi = p[0] / p[2], p[1] / p[2]
        ok = (p[2] > 1) & (ui >= 20) & (ui <= FRAME_W - 20) & (vi >= 20) & (vi <= FRAME_H - 20)
        x, y, u, v = (np.concatenate([a, b[ok]]) for a, b in ((x, xi), (y, yi), (u, ui), (v, vi)))
    x, y, u, v = x[:n], y[:n], u[:n], v[:n]
    if sigma:
        u, v = u + rng.normal(0, sigma, n), v + rng.normal(0, sigma, n)
    return x, y, u.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)


def sine(a, b):
    """Sine of the angle between the lines spanned by two 9-vectors."""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(np.linalg.norm(a - (a @ b) * b))


# ----------------------------------------------------------------- sampler

SAMPLE_SEEDS = (0, 3, 0x80000000, 0xFFFFFFFF)
SAMPLE_TAIL = (255, 256, 257, 3071, 3072, 3073, 65535, 1 << 20)


def test_sample_is_the_documented_draw(prog, tmp_path):
    for K in (4, 8):
        items = [(s, h, n) for n in tuple(range(K, 41)) + SAMPLE_TAIL for s in SAMPLE_SEEDS for h in range(64)]
        cases = head(1, len(items)) + b"".join(struct.pack("<IIii", *it, K) for it in items)
        got = np.frombuffer(run(prog, tmp_path, cases), np.int32).reshape(len(items), K)
        want = np.array([sample(K, s, h, n) for s, h, n in items])
        assert (got == want).all(), (K, items[int(np.nonzero((got != want).any(1))[0][0])])
    assert sample(8, 0, 3, 160) == [52, 44, 61, 71, 17, 45, 57, 132]


def test_sample_is_distinct_and_uniform(prog, tmp_path):
    """Over N = 20,000 hypotheses an index of n lies in a sample of K with
    probability p = K / n, so its hits are binomial(N, p): within 5 sigma =
    5 sqrt(N p (1 - p)) of N p (for n = K that is exactly N)."""
    nhyp = 20000
    for K in (4, 8):
        for seed in (0, 0xFFFFFFFF):
            ns = range(K, K + 5)
            cases = b"".join(head(6, 1) + struct.pack("<Iiii", seed, n, nhyp, K) for n in ns)
            out, at = run(prog, tmp_path, cases), 0
            for n in ns:
                hits = np.frombuffer(out, np.int64, n, at)
                bad = struct.unpack_from("<i", out, at + 8 * n)[0]
                at += 8 * n + 4
                p = float(K) / n
                dev = np.abs(hits - nhyp * p).max()
                print(f"fd_sample<{K}> n {n} seed {seed:#x}: largest deviation {dev:.0f} hits, "
                      f"5 sigma {5 * np.sqrt(nhyp * p * (1 - p)):.0f}")
                assert bad == 0 and hits.sum() == K * nhyp
                assert dev <= 5 * np.sqrt(nhyp * p * (1 - p))
            assert at == len(out)


# ----------------------------------------------------------------- sampson

class Bounded:
    """A float64 value together with a bound on how far the fp32 evaluation
    of the same expression can lie from it: every written operation rounds
    once, relative error at most 2^-24, on top of what its operands carry."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    def __mul__(self, o):
        p = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        v = self.v * o.v
        return Bounded(v, p + U32 * (np.abs(v) + p))

    def __add__(self, o):
        p = self.e + o.e
        v = self.v + o.v
        return Bounded(v, p + U32 * (np.abs(v) + p))

    def __truediv__(self, o):
        v = self.v / o.v
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(np.abs(o.v) > o.e, (self.e + np.abs(v) * o.e) / (np.abs(o.v) - o.e), np.inf)
        return Bounded(v, p + U32 * (np.abs(v) + p))


def test_sampson2_within_its_rounding_bound(prog, tmp_path):
    rng = np.random.default_rng(101)
    n = 10000
    f = np.zeros((n, 9), np.float32)
    for i in range(n):                                  # F of a random camera pair, or any unit matrix
        if i % 2:
            r, t = rot(*rng.uniform(-5, 5, 3)), rng.normal(0, 1, 3)
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            m = np.linalg.inv(K).T @ tx @ r @ np.linalg.inv(K)
        else:
            m = rng.normal(0, 1, (3, 3))
        f[i] = (m / np.linalg.norm(m)).reshape(9)
    pt = np.stack([rng.uniform(0, FRAME_W, n), rng.uniform(0, FRAME_H, n), rng.uniform(0, FRAME_W, n),
                   rng.uniform(0, FRAME_H, n)], 1).astype(np.float32)
    got = np.frombuffer(run(prog, tmp_path, head(2, n) + np.hstack([f, pt]).tobytes()), np.float32)
    F = [Bounded(f[:, i]) for i in range(9)]
    x, y, u, v = (Bounded(pt[:, i]) for i in range(4))
    a = (F[0] * x + F[1] * y) + F[2]
    b = (F[3] * x + F[4] * y) + F[5]
    c = (F[6] * x + F[7] * y) + F[8]
    a2 = (F[0] * u + F[3] * v) + F[6]
    b2 = (F[1] * u + F[4] * v) + F[7]
    r = (u * a + v * b) + c
    d = (a * a + b * b) + (a2 * a2 + b2 * b2)
    e2 = (r * r) / d
    assert np.isfinite(e2.e).all()
    err = np.abs(got.astype(np.float64) - e2.v)
    worst = int(np.argmax(err / e2.e))
    print(f"fd_sampson2: largest error / bound {err[worst] / e2.e[worst]:.3f}, "
          f"largest relative error {np.max(err / e2.v):.3e}")
    assert (err <= e2.e).all(), (worst, err[worst], e2.e[worst])
    # ... and the float64 expression is the Sampson distance the reference uses
    ref = np.array([sampson(f[i], *pt[i]) for i in range(0, n, 50)])
    assert np.allclose(ref ** 2, e2.v[::50], rtol=1e-9)


# ------------------------------------------------------------- eight_point

def degenerate_octets():
    """Octets whose 8 x 9 system has a null space of more than one dimension."""
    rng = np.random.default_rng(5)
    ki = np.linalg.inv(K)
    out = []
    for cam in CAMS:
        x = np.array([100, 300, 500, 700, 900, 1100, 1300, 640], np.float64)      # 7 of 8 on a line of image 1
        y = np.array([100, 200, 300, 400, 500, 600, 700, 900], np.float64)
        p = K @ (cam[0] @ (rng.uniform(4, 20, 8) * (ki @ np.stack([x, y, np.ones(8)]))) + cam[1][:, None])
        out.append((x, y, p[0] / p[2], p[1] / p[2]))
        a, b, c, d = views(rng, cam, 8)                  # one correspondence three times
        a[5:], b[5:], c[5:], d[5:] = a[4], b[4], c[4], d[4]
        out.append((a, b, c, d))
        a, b, c, d = views(rng, cam, 8)                  # image 2 on a line
        out.append((a, b, c, 0.5 * c + 100.0))
    return out


def test_eight_point_against_the_svd_null_vector(prog, tmp_path):
    """The output is the unit null vector rounded to fp32 per entry: each of
    the 9 entries moves by at most 2^-24 of the unit norm, the vector by at
    most 3 * 2^-24 (sqrt 9), which bounds the sine of the angle; the fp64
    elimination adds about eps * s0 / s7 <= 1e-12 where s7 / s0 >= 1e-4."""
    rng = np.random.default_rng(77)
    octs = [views(rng, CAMS[i % 3], 8) for i in range(2000)] + degenerate_octets()
    cases = head(3, len(octs)) + b"".join(np.concatenate(o).astype(np.float64).tobytes() for o in octs)
    out = np.frombuffer(run(prog, tmp_path, cases), np.dtype([("ok", "<i4"), ("f", "<f4", 9)]))
    worst, tested, low, high = 0.0, 0, 0, 0
    for o, r in zip(octs, out):
        ref, ratio = octet(*o)
        if ratio < 1e-9:
            low += 1
            assert r["ok"] == 0, ratio
        if ratio > 1e-5:
            high += 1
            assert r["ok"] == 1, ratio
        if r["ok"]:
            assert abs(np.linalg.norm(r["f"].astype(np.float64)) - 1.0) <= 1e-6
        else:
            assert not r["f"].any()
        if ratio >= 1e-4:
            tested += 1
            s = sine(r["f"].astype(np.float64), ref)
            worst = max(worst, s)
            assert s <= ANGLE, (s, ratio)
    print(f"fd_eight_point: largest sine {worst:.3e} over {tested} octets with s7/s0 >= 1e-4; "
          f"{high} above 1e-5 accepted, {low} below 1e-9 refused")
    assert tested >= 1500 and low >= 9


# ------------------------------------------------------------------ jacobi

def gram9(x, y, u, v):
    xn, yn, _ = hartley(x, y)
    un, vn, _ = hartley(u, v)
    a = epipolar_rows(xn, yn, un, vn)
    return a.T @ a


def jacobi_matrices():
    """(class, symmetric matrix) for the Jacobi test."""
    rng = np.random.default_rng(909)
    out = []
    for i in range(1000):                               # Gram matrices of normalised point sets, 9 x 9
        n = int(rng.integers(8, 201))
        out.append(("gram9", gram9(*views(rng, CAMS[i % 3], n, sigma=0.5 if i % 4 == 0 else 0.0))))
    for i in range(200):                                # F^T F of a 3 x 3 matrix: what the rank-2 step sees
        m = rng.normal(0, 1, (3, 3))
        out.append(("gram3", m.T @ m))
    for n in (3, 9):
        out.append(("diagonal", np.diag(rng.uniform(0.1, 5, n))))
        out.append(("diagonal", np.diag(np.arange(n, 0, -1.0))))
        out.append(("zero", np.zeros((n, n))))
        for _ in range(5):
            w = rng.normal(0, 1, n)
            out.append(("rank1", np.outer(w, w)))
            q = np.linalg.qr(rng.normal(0, 1, (n, n)))[0]
            lam = np.repeat(rng.uniform(0.5, 2, (n + 2) // 3), 3)[:n]       # every eigenvalue three times
            m = (q * lam) @ q.T
            out.append(("repeated", 0.5 * (m + m.T)))
            out.append(("identity", 2.5 * np.eye(n)))
    return out


def test_jacobi_against_eigh(prog, tmp_path):
    """Bounds of about 1e4 eps: eigenvalues and the residual A V - V diag
    within 1e-12 lmax, V^T V - I within 1e-13."""
    mats = jacobi_matrices()
    cases = head(4, len(mats)) + b"".join(struct.pack("<i", len(m)) + m.astype(np.float64).tobytes()
                                          for _, m in mats)
    out, at = run(prog, tmp_path, cases), 0
    worst = {}
    for kind, m in mats:
        n = len(m)
        d = np.frombuffer(out, np.float64, n * n, at).reshape(n, n)
        v = np.frombuffer(out, np.float64, n * n, at + 8 * n * n).reshape(n, n)
        at += 16 * n * n
        lam = np.diag(d)
        lmax = max(np.abs(np.linalg.eigvalsh(m)).max(), 1e-300)
        e_val = np.abs(np.sort(lam) - np.linalg.eigvalsh(m)).max() / lmax
        e_res = np.abs(m @ v - v * lam).max() / lmax
        e_orth = np.abs(v.T @ v - np.eye(n)).max()
        e_off = np.abs(d - np.diag(lam)).max() / lmax
        w = worst.setdefault(kind, [0.0, 0.0, 0.0, 0.0])
        worst[kind] = [max(a, b) for a, b in zip(w, (e_val, e_res, e_orth, e_off))]
    assert at == len(out)
    for kind, w in worst.items():
        print(f"fd_jacobi {kind}: eigenvalues {w[0]:.2e} lmax, residual {w[1]:.2e} lmax, "
              f"orthogonality {w[2]:.2e}, off-diagonal left {w[3]:.2e} lmax")
    for kind, w in worst.items():
        assert w[0] <= 1e-12 and w[1] <= 1e-12 and w[2] <= 1e-13, (kind, w)


# ------------------------------------------------------------- refit_solve

def moments(x, y, u, v):
    """fd_refit_solve's arguments, in float64: the 36 sums and the two similarities."""
    cx, cy, cu, cv = x.mean(), y.mean(), u.mean(), v.mean()
    s1 = np.sqrt(2) / np.hypot(x - cx, y - cy).mean()
    s2 = np.sqrt(2) / np.hypot(u - cu, v - cv).mean()
    xn, yn, un, vn = (x - cx) * s1, (y - cy) * s1, (u - cu) * s2, (v - cv) * s2
    pp = np.stack([xn * xn, xn * yn, xn, yn * yn, yn, np.ones_like(xn)])
    qq = np.stack([un * un, un * vn, un, vn * vn, vn, np.ones_like(xn)])
    return np.concatenate([(qq @ pp.T).reshape(36), [cx, cy, s1, cu, cv, s2]])


def test_refit_solve_against_the_svd_fit(prog, tmp_path):
    """Same angle bound as the 8-point solver (fp32 rounding of a unit
    vector), both signed by the rule; rank 2 and unit norm as the GPU tests
    ask of the returned f."""
    rng = np.random.default_rng(4242)
    sets = []
    for i in range(300):
        n = 8 if i % 10 == 0 else int(rng.integers(8, 201))
        sets.append(views(rng, CAMS[i % 3], n, sigma=0.5 if i % 3 == 0 and n > 8 else 0.0))
    t = np.linspace(0, 1, 40)
    line = (100 + 1500 * t, 200 + 700 * t) + views(rng, CAMS[0], 40)[2:]          # image 1 on one line
    cases = head(5, len(sets) + 1) + b"".join(moments(*s).tobytes() for s in sets + [line])
    out = np.frombuffer(run(prog, tmp_path, cases), np.dtype([("ok", "<i4"), ("f", "<f4", 9)]))
    worst = worst_rank = 0.0
    for s, r in zip(sets, out):
        assert r["ok"] == 1
        f = r["f"].astype(np.float64)
        ref = fit_8pt(*s)
        assert f @ ref > 0 and r["f"][np.argmax(np.abs(r["f"]))] > 0
        sv = np.linalg.svd(f.reshape(3, 3), compute_uv=False)
        worst, worst_rank = max(worst, sine(f, ref)), max(worst_rank, sv[2] / sv[0])
        assert sine(f, ref) <= ANGLE, (sine(f, ref), len(s[0]))
        assert sv[2] <= 1e-6 * sv[0] and abs(np.linalg.norm(f) - 1.0) <= 1e-6
    print(f"fd_refit_solve: largest sine {worst:.3e}, largest s3/s1 {worst_rank:.3e} over {len(sets)} sets")
    assert out[-1]["ok"] == 0
