"""The NMS stage (k_nms_scan, the prefix scan, k_nms_fit, k_sort / k_sort_rank, k_offsets) on planted
response planes, case by case.

`surfhip_run_nms` runs the stage on whatever the detector's response planes hold, so these tests write
the planes themselves: one flat float32 array per frame in the reference layout (octave o plane s at
ooff[o] + s osize[o], row pitch swhp[o].z).  Only the real planes are planted (all five of octave 0,
planes 2-4 of later octaves); for the oracle planes 0 / 1 of an octave > 0 are filled as halfImage
fills them (dst[r, c] = src[2r, 2c] of the previous octave's planes 2 / 4, `fill_views`), in the GPU
copy those stored planes and every pad column [sw, sp) hold +inf (`gpu_copy`): the kernels must read
the views, never the storage.  Reference: `or_find_points` on the same planes and the integral of the
same noise frame; every field of every point bit for bit, counts and candidates equal, nothing dropped.

Every class a test names is decided on the reference side only -- `level_blocks` (numpy restatement of
the 2x2x2 argmax and the 3x3x3 test, surfd.cu:678-792), `simulate_fit` (the interpolation loop,
surfd.cu:795-819, around `or_test_fit`) and the oracle's points -- and asserted populated before the
GPU result is looked at.

Geometries: 640 x 400, 4 octaves, sampling step 2, and 333 x 211, 3 octaves, step 1 (`geometry_facts`).
A scan workgroup is 4 waves x 64 block columns x 16 block rows of one (octave, level); wave w takes the
rows y = 16 R + w + 4 u, u < 4, as one pass, so a scan item is (R, w, x // 64), a block's candidate
order within its item is (u, lane) and kItemCap = 256.
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from conftest import assert_points_equal
from test_gpu_parity import took

pytestmark = pytest.mark.gpu

F32 = np.float32
THRESH = 4.0
ITEM_CAP, CUBE_CAP, SCAN_ROWS, SCAN_CHUNK = 256, 8, 16, 2048      # surfhip_internal.h, surfhip_nms.inc
RANK_LDS, SORT_CAP = 16384, 16384                                   # k_sort_rank's / k_sort's LDS key capacity
POISON = 0xA7
TAIL = 4096
BIG_PTS = 32768
GEOMS = {"640x400": (640, 400, 4, 2), "333x211": (333, 211, 3, 1)}
FIELDS = ("x", "y", "scale", "o", "strength", "laplace", "ori", "score", "match", "match_x", "match_y", "ambiguity")


# ------------------------------------------------------------ geometry

class Geo:
    def __init__(self, orc, name):
        self.name = name
        self.w, self.h, self.noct, self.step = GEOMS[name]
        self.orc = orc
        self.p = orc.make_param(self.noct, THRESH, sampling_step=self.step, upright=True)
        self.g, self.octs = orc.geometry(self.p, self.w, self.h)
        self.tot = int(self.g.tot_osize)
        self.sw = [self.g.swhp[o].x for o in range(self.noct)]
        self.sh = [self.g.swhp[o].y for o in range(self.noct)]
        self.sp = [self.g.swhp[o].z for o in range(self.noct)]
        self.osize = [self.g.osize[o] for o in range(self.noct)]
        self.ooff = [int(self.g.ooff[o]) for o in range(self.noct)]
        self.mb = [list(self.octs[o].mborders)[:2] for o in range(self.noct)]
        self.borders = [list(self.octs[o].borders)[:5] for o in range(self.noct)]
        self.gx = [self.octs[o].nms_gx for o in range(self.noct)]
        self.gy = [self.octs[o].nms_gy for o in range(self.noct)]
        self.nlev = (self.p.max_scale - 1) // 2
        self.pitch = (self.w + 15) // 16 * 16
        self.imgs, self.iis = [], []
        for seed in (5, 11):
            im = np.zeros((self.h, self.pitch), np.uint8)
            im[:, :self.w] = np.random.default_rng(seed).integers(0, 256, (self.h, self.w), dtype=np.uint8)
            self.imgs.append(im)
            self.iis.append(orc.integral(im, self.w, self.h))

    def nblocks(self, o, z):
        """In-range block rows / columns of level z: i = mb + 2y < sh - mb inside the launch extent."""
        mb = self.mb[o][z]
        ny = min(self.gy[o], max(0, (self.sh[o] - 2 * mb + 1) // 2))
        nx = min(self.gx[o], max(0, (self.sw[o] - 2 * mb + 1) // 2))
        return ny, nx

    def scan_wgs(self):
        return sum(self.nlev * ((self.gx[o] + 63) // 64) * ((self.gy[o] + SCAN_ROWS - 1) // SCAN_ROWS)
                   for o in range(self.noct))

    def planes(self, resp, o):
        return resp[self.ooff[o]:self.ooff[o] + 5 * self.osize[o]].reshape(5, self.sh[o], self.sp[o])

    def fill_views(self, resp):
        for o in range(1, self.noct):
            cur, prev = self.planes(resp, o), self.planes(resp, o - 1)
            sh, sw = self.sh[o], self.sw[o]
            cur[0, :, :sw] = prev[2, 0:2 * sh:2, 0:2 * sw:2]
            cur[1, :, :sw] = prev[4, 0:2 * sh:2, 0:2 * sw:2]
        return resp

    def gpu_copy(self, resp):
        out = resp.copy()
        for o in range(self.noct):
            pl = self.planes(out, o)
            pl[:, :, self.sw[o]:] = np.inf
            if o > 0:
                pl[0:2] = np.inf
        return out


_GEO = {}


def geo_of(orc, name):
    if name not in _GEO:
        _GEO[name] = Geo(orc, name)
    return _GEO[name]


def geometry_facts(geo):
    """The facts the classes below rely on, from or_octave_params: a changed constant fails here."""
    if geo.name == "640x400":
        assert [(geo.sw[o], geo.sh[o]) for o in range(4)] == [(320, 200), (160, 100), (80, 50), (40, 25)]
        assert geo.gx == [160, 80, 32, 16] and geo.tot == 560000
        assert geo.scan_wgs() == 52 and geo.scan_wgs() * 4 == 208
        assert [(geo.gx[o] + 63) // 64 for o in range(4)] == [3, 2, 1, 1]
    else:
        assert (geo.sw[0], geo.sh[0]) == (333, 211) and geo.noct == 3
        assert (geo.gx[0] + 63) // 64 == 3
        assert geo.sw[0] % 2 == 1 and geo.sh[0] % 2 == 1
    for o in range(geo.noct):
        for z in range(geo.nlev):
            ny, nx = geo.nblocks(o, z)
            assert ny > 0 and nx > 0, (o, z)                       # every octave has NMS rows
    assert geo.p.max_scale == 5 and geo.nlev == 2 and float(geo.p.thresh) == THRESH


# ------------------------------------------------------------ reference-side classification

def level_blocks(geo, resp, o, z):
    """The 2x2x2 argmax in the reference's order with strict '>', the threshold and top-scale tests and
    the 19 outside neighbours (ties survive) of every in-range block of level z (surfd.cu:678-792), on
    oracle-layout planes.  Arrays [ny, nx]."""
    A = geo.planes(resp, o)
    k, mb = 2 * z + 1, geo.mb[o][z]
    ny, nx = geo.nblocks(o, z)
    i, j = (mb + 2 * np.arange(ny))[:, None], (mb + 2 * np.arange(nx))[None, :]
    with np.errstate(invalid="ignore"):
        best = A[k, i, j].copy()
        cas = np.zeros((ny, nx), np.int64)
        for t in range(1, 8):
            v = A[k + (t >> 2), i + ((t >> 1) & 1), j + (t & 1)]
            m = v > best
            best, cas = np.where(m, v, best), np.where(m, t, cas)
        cand = ~(best < F32(THRESH) * F32(0.8)) & ~((k + 1 == geo.p.max_scale - 1) & (cas > 3))
        s, r, c = k + (cas >> 2), i + ((cas >> 1) & 1), j + (cas & 1)
        surv = cand.copy()
        for a, b, e in itertools.product((-1, 0, 1), repeat=3):
            if (a, b, e) != (0, 0, 0):
                surv &= ~(best < A[np.clip(s + a, 0, 4), r + b, c + e])
        # the lane-neighbour columns of the same block row (k_nms_scan's early test)
        lmax = np.fmax(np.fmax(A[k, i, j], A[k, i + 1, j]), np.fmax(A[k + 1, i, j], A[k + 1, i + 1, j]))
        rmax = np.fmax(np.fmax(A[k, i, j + 1], A[k, i + 1, j + 1]), np.fmax(A[k + 1, i, j + 1], A[k + 1, i + 1, j + 1]))
    return dict(best=best, cas=cas, cand=cand, surv=surv, s=s, r=r + 0 * c, c=c + 0 * r, lmax=lmax, rmax=rmax,
                ny=ny, nx=nx)


def survivors(geo, resp):
    """Every NMS survivor of a frame in canonical order: structured (o, z, y, x, cas, s, r, c)."""
    out = []
    for o in range(geo.noct):
        for z in range(geo.nlev):
            L = level_blocks(geo, resp, o, z)
            ys, xs = np.nonzero(L["surv"])
            rec = np.zeros(len(ys), [(n, "i4") for n in ("o", "z", "y", "x", "cas", "s", "r", "c")])
            rec["o"], rec["z"], rec["y"], rec["x"] = o, z, ys, xs
            for n in ("cas", "s", "r", "c"):
                rec[n] = L[n][ys, xs]
            out.append(rec)
    return np.concatenate(out)


def item_slots(sv):
    """Per survivor (of one frame): its scan item's survivor count and its slot in the item (scan order:
    u = (y % 16) // 4, then lane)."""
    item = (((sv["o"].astype(np.int64) * 2 + sv["z"]) * 1024 + sv["y"] // SCAN_ROWS) * 4 + sv["y"] % 4) * 16 + sv["x"] // 64
    order = np.lexsort((sv["x"] % 64, (sv["y"] % SCAN_ROWS) // 4, item))
    slot, count = np.zeros(len(sv), np.int64), np.zeros(len(sv), np.int64)
    it = item[order]
    start = np.r_[0, np.nonzero(np.diff(it))[0] + 1, len(it)]
    for a, b in zip(start[:-1], start[1:]):
        slot[order[a:b]] = np.arange(b - a)
        count[order[a:b]] = b - a
    return slot, count


def simulate_fit(geo, resp, o, s, r, c):
    """The interpolation loop of surfd.cu:795-819 around or_test_fit: moves, whether a move was stopped by
    a borders[s] clamp (and which), and the outcome."""
    src = resp[geo.ooff[o]:geo.ooff[o] + 5 * geo.osize[o]]
    sw, sh, bs = geo.sw[o], geo.sh[o], geo.borders[o][s]
    newr, newc, moves, clamp = r, c, 0, set()
    lim, thr = F32(0.6), F32(THRESH)
    for mv in range(5):
        r, c = newr, newc
        with np.errstate(all="ignore"):
            st, off = geo.orc.fit_quadrat(src, s, r, c, geo.osize[o], geo.sp[o])
        if off[1] > lim:
            if r < sh - bs: newr += 1
            else: clamp.add("bottom")
        if off[1] < -lim:
            if r > bs: newr -= 1
            else: clamp.add("top")
        if off[2] > lim:
            if c < sw - bs: newc += 1
            else: clamp.add("right")
        if off[2] < -lim:
            if c > bs: newc -= 1
            else: clamp.add("left")
        if newr == r and newc == c:
            break
        moves += 1
    if np.isnan(off).any():
        why = "nan"
    elif (np.abs(off) > F32(1.5)).any():
        why = "off"
    elif st < thr:
        why = "weak"
    else:
        why = "ok"
    return dict(moves=moves, clamp=clamp, why=why, off=off, strength=st)


def trace_sides(geo, pts):
    """Sides on which makePoint's getTrace box (surfd.cu:1010-1020) leaves the integral image."""
    ns = pts["scale"].astype(F32) / F32(1.2)
    temp = (F32(3) * ns + F32(0.5)).astype(np.int64)
    v0 = (pts["x"].astype(F32) / F32(geo.p.divisor) + F32(0.5)).astype(np.int64)
    v1 = (pts["y"].astype(F32) / F32(geo.p.divisor) + F32(0.5)).astype(np.int64)
    reach = temp + temp // 2
    return dict(left=v0 - reach < 0, right=v0 + reach + 1 > geo.w, top=v1 - reach < 0, bottom=v1 + reach + 1 > geo.h)


# ------------------------------------------------------------ frames

class Frame:
    """Planted planes of one frame: the oracle's copy (views filled), the GPU's (+inf storage) and the
    oracle's points."""

    def __init__(self, geo, resp, img=0, name=""):
        self.geo, self.name, self.img = geo, name, img
        self.resp = geo.fill_views(resp)
        self.gpu = geo.gpu_copy(self.resp)
        self._ref = self._sv = None

    def ref(self):
        if self._ref is None:
            g = self.geo
            with np.errstate(all="ignore"):
                self._ref = g.orc.find_points(g.p, g.g, g.octs, g.iis[self.img], self.resp, 65536)
        return self._ref

    def surv(self):
        if self._sv is None:
            self._sv = survivors(self.geo, self.resp)
        return self._sv


class Planter:
    """Places sites (a peak and the cells within one sample of it) on a frame so that no two interact:
    a site claims the samples within 2 of its peak (`occ`), and marks the samples its cells are seen at
    in the neighbouring octaves (through the halfImage views) so that no site is placed on those; what
    the marks of two sites do to each other in a third place is left to the oracle."""

    def __init__(self, geo):
        self.geo = geo
        self.resp = np.zeros(geo.tot, F32)
        self.occ = [np.zeros((geo.sh[o], geo.sw[o]), bool) for o in range(geo.noct)]
        self.sites = [np.zeros((geo.sh[o], geo.sw[o]), bool) for o in range(geo.noct)]

    def put(self, o, s, r, c, v):
        if o > 0 and s < 2:                     # a halfImage view: plant the sample it shows
            self.put(o - 1, 2 if s == 0 else 4, 2 * r, 2 * c, v)
        else:
            self.geo.planes(self.resp, o)[s, r, c] = v

    def _regions(self, o, r, c):
        reg = [(o, r, c, 2)]
        if o > 0:
            reg.append((o - 1, 2 * r, 2 * c, 2))
        if o + 1 < self.geo.noct:
            reg.append((o + 1, r // 2, c // 2, 1))
        return reg

    def claim(self, o, r, c):
        reg = self._regions(o, r, c)
        for (oo, rr, cc, rad) in reg:
            taken = self.occ if oo == o else self.sites
            if taken[oo][max(rr - rad, 0):rr + rad + 1, max(cc - rad, 0):cc + rad + 1].any():
                return False
        for (oo, rr, cc, rad) in reg:
            self.occ[oo][max(rr - rad, 0):rr + rad + 1, max(cc - rad, 0):cc + rad + 1] = True
            if oo == o:
                self.sites[oo][max(rr - rad, 0):rr + rad + 1, max(cc - rad, 0):cc + rad + 1] = True
        return True


class Campaign:
    """Sites over as many frames as they need."""

    def __init__(self, geo, limit=16):
        self.geo, self.frames, self.limit = geo, [], limit

    def site(self, o, z, cas, ys, xs):
        """Claim the first free block (y, x) of the given rows / columns on the first frame with room;
        returns (frame index, planter, y, x, s, r, c)."""
        mb, k = self.geo.mb[o][z], 2 * z + 1
        for fi in range(self.limit):
            if fi == len(self.frames):
                self.frames.append(Planter(self.geo))
            pl = self.frames[fi]
            for y in ys:
                for x in xs:
                    r, c = mb + 2 * y + ((cas >> 1) & 1), mb + 2 * x + (cas & 1)
                    if not pl.occ[o][r, c] and pl.claim(o, r, c):
                        return fi, pl, y, x, k + (cas >> 2), r, c
        raise AssertionError("no room for a site")

    def finish(self, tag):
        return [Frame(self.geo, pl.resp, img=i % 2, name=f"{tag}{i}") for i, pl in enumerate(self.frames)]


def sign(cas):
    return (1 if cas >> 2 else -1), (1 if (cas >> 1) & 1 else -1), (1 if cas & 1 else -1)


# ------------------------------------------------------------ GPU side

class Rig:
    """A detector, its planes written by the test, run_nms into poisoned buffers."""

    def __init__(self, surf, geo, max_batch, max_pts=BIG_PTS, cand_cap=0):
        self.surf, self.geo, self.max_pts = surf, geo, max_pts
        par = surf.make_param(geo.noct, THRESH, sampling_step=geo.step, upright=True)
        self.det = surf.Detector(par, geo.w, geo.h, max_batch=max_batch, max_pts=max_pts, cand_cap=cand_cap)
        _, _, self.resp_ptr, self.stride = self.det.workspace()
        assert self.stride >= geo.tot
        gi, gs, go, gz = self.det.geometry()
        assert [x[:3] for x in gs[:geo.noct]] == [(geo.sw[o], geo.sh[o], geo.sp[o]) for o in range(geo.noct)]
        assert go[:geo.noct] == geo.ooff and gz[:geo.noct] == geo.osize
        self.fb = surf.DeviceBuffer(max_batch * geo.h * geo.pitch)

    def switches(self):
        return {"switches": self.det.switches()}

    def run(self, frames):
        """run_nms of `frames`: per-frame point arrays, counts, candidates, truncated, batch_total."""
        surf, geo, n, mp = self.surf, self.geo, len(frames), self.max_pts
        self.fb.upload(np.stack([geo.imgs[fr.img] for fr in frames]))
        self.det.run_integral(self.fb.ptr, n, geo.pitch, geo.h * geo.pitch)
        surf.synchronize()
        for f, fr in enumerate(frames):
            surf.upload_ptr(self.resp_ptr + 4 * f * self.stride, fr.gpu)
        pb, cb = surf.DeviceBuffer(48 * n * mp + TAIL), surf.DeviceBuffer(4 * n + TAIL)
        pb.upload(np.full(pb.nbytes, POISON, np.uint8))
        cb.upload(np.full(cb.nbytes, POISON, np.uint8))
        self.det.run_nms(n, pb.ptr, cb.ptr)
        surf.synchronize()
        raw, rawc = pb.download(np.uint8, pb.nbytes), cb.download(np.uint8, cb.nbytes)
        cand, trunc, total = self.det.candidates(n), self.det.truncated(), self.det.batch_total(n)
        pb.free()
        cb.free()
        assert (raw[-TAIL:] == POISON).all() and (rawc[-TAIL:] == POISON).all(), "written past the buffers' ends"
        counts = rawc[:4 * n].view(np.int32).copy()
        assert ((counts >= 0) & (counts <= mp)).all(), counts
        slots = raw[:48 * n * mp].reshape(n, mp, 48)
        pts = []
        for f in range(n):
            assert (slots[f, counts[f]:] == POISON).all(), f"frame {f}: slots at or past the count written"
            pts.append(slots[f, :counts[f]].copy().view(surf.POINT_DTYPE).reshape(-1))
        assert total == int(counts.sum()), (total, counts)
        return pts, counts, cand, trunc, total

    def close(self):
        self.det.close()
        self.fb.free()


def same_points(got, ref, what):
    try:
        assert_points_equal(got, ref, fields=FIELDS)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def check_frames(rig, frames, what):
    """One run_nms of `frames`, every frame against the oracle; returns the points' bytes per frame."""
    pts, counts, cand, trunc, total = rig.run(frames)
    out = []
    for f, fr in enumerate(frames):
        ref, n = fr.ref()
        assert n <= rig.max_pts
        tag = f"{what} frame {f} ({fr.name})"
        assert counts[f] == len(ref) and cand[f] == n, f"{tag}: count {counts[f]} / candidates {cand[f]}, oracle {n}"
        same_points(pts[f], ref, tag)
        out.append(pts[f].tobytes())
    assert not trunc, what
    return out


def with_env(monkeypatch, env):
    for name in ("SURFHIP_FIT_CUBE", "SURFHIP_SORT_BITONIC", "SURFHIP_FIT_GRID"):
        monkeypatch.delenv(name, raising=False)
    for kv in filter(None, env.split(",")):
        name, _, val = kv.partition("=")
        monkeypatch.setenv(name, val)


_SETS = {}


def cached(key, make):
    if key not in _SETS:
        _SETS[key] = make()
    return _SETS[key]


# ------------------------------------------------------------ (a) isolated peaks

def peak_frames(geo):
    """Single-sample peaks (fit: offset 0, strength = the value): each cas x level x octave, block columns
    0, 1, 62, 63 (mod 64), every row residue mod 16, the first and last in-range block row and column."""
    camp = Campaign(geo)
    rng = np.random.default_rng(21)
    planted = []                                                    # (frame, o, z, y, x, cas)

    def add(o, z, cas, ys, xs):
        fi, pl, y, x, s, r, c = camp.site(o, z, cas, ys, xs)
        pl.put(o, s, r, c, F32(rng.uniform(6.0, 40.0)))
        planted.append((fi, o, z, y, x, cas))

    for o in reversed(range(geo.noct)):                             # the small octaves first: they have least room
        for z in range(geo.nlev):
            ny, nx = geo.nblocks(o, z)
            inner_y, inner_x = list(range(1, ny - 1)), [x for x in range(2, nx - 1) if 2 <= x % 64 <= 61]
            for cas in range(8):
                add(o, z, cas, inner_y, inner_x)
            for t, xm in enumerate((0, 1, 62, 63, 0, 1, 62, 63)):
                xs = [x for x in range(64, nx) if x % 64 == xm] or [x for x in range(nx) if x % 64 == xm]
                if xs and nx > 64:
                    add(o, z, (2 * t + (xm & 1) + (t >= 4)) % 8 if z == 0 else t % 4, inner_y or [0], xs)
            for res in range(min(16, ny)):
                add(o, z, (res * 3) % (8 if z == 0 else 4), [y for y in range(ny) if y % 16 == res], inner_x)
            for cas in range(4):                                    # the outermost samples of the level
                add(o, z, cas, [0] if not (cas >> 1) & 1 else [ny - 1], inner_x)
                add(o, z, cas, inner_y or [0], [0] if not cas & 1 else [nx - 1])
    return camp.finish("peaks"), planted


def peaks_set(orc, gname):
    return cached(("peaks", gname), lambda: peak_frames(geo_of(orc, gname)))


@pytest.mark.parametrize("gname", list(GEOMS))
def test_isolated_peaks(surf, orc, gname):
    geo = geo_of(orc, gname)
    geometry_facts(geo)
    frames, planted = peaks_set(orc, gname)
    seen, accepted = set(), 0
    for fi, fr in enumerate(frames):
        lev = {(o, z): level_blocks(geo, fr.resp, o, z) for o in range(geo.noct) for z in range(geo.nlev)}
        for (pf, o, z, y, x, cas) in planted:
            if pf != fi:
                continue
            L = lev[(o, z)]
            ny, nx = L["ny"], L["nx"]
            assert L["cas"][y, x] == cas, (fi, o, z, y, x, cas)
            if z == 1 and cas > 3:                                  # top-scale rejection: nothing
                assert not L["cand"][y, x]
                seen.add(("rejected", o, cas))
                continue
            assert L["surv"][y, x], (fi, o, z, y, x, cas)
            accepted += 1
            seen.update({("cas", o, z, cas), ("xmod", x % 64 if x % 64 in (0, 1, 62, 63) else "in"),
                         ("ymod", o, z, y % 16), ("row", o, z, "first" if y == 0 else "last" if y == ny - 1 else "in"),
                         ("col", o, z, "first" if x == 0 else "last" if x == nx - 1 else "in")})
        assert sum(int(L["surv"].sum()) for L in lev.values()) == fr.ref()[1]
    # (a peak planted in plane 4 at even coordinates is also a level-0 peak of the next octave's view)
    total = sum(fr.ref()[1] for fr in frames)
    assert accepted <= total <= accepted + len(planted)
    for o in range(geo.noct):
        for z in range(geo.nlev):
            ny, nx = geo.nblocks(o, z)
            for cas in range(8 if z == 0 else 4):
                assert ("cas", o, z, cas) in seen, (o, z, cas)
            for res in range(min(16, ny)):
                assert ("ymod", o, z, res) in seen, (o, z, res)
            for side in ("first", "last", "in"):
                assert ("row", o, z, side) in seen and ("col", o, z, side) in seen, (o, z, side)
        for cas in range(4, 8):
            assert ("rejected", o, cas) in seen, (o, cas)
    for xm in (0, 1, 62, 63, "in"):
        assert ("xmod", xm) in seen, xm
    print(f"(a) {gname}: {len(frames)} frames, {accepted} accepted peaks, {len(planted) - accepted} rejected on level 1, "
          f"{total} oracle points")
    rig = Rig(surf, geo, len(frames))
    check_frames(rig, frames, "peaks")
    rig.close()


# ------------------------------------------------------------ (b) neighbour matrix

def matrix_frames(geo, o, z):
    """For each cas and each of the 19 outside neighbours: a peak whose neighbour equals it (survives)
    and one whose neighbour is one ulp above (vanishes); in the interior, across the lane 63 / 64
    boundary, and with the neighbour in the border strip outside the first / last block row / column."""
    camp = Campaign(geo)
    rng = np.random.default_rng(31 + o)
    ny, nx = geo.nblocks(o, z)
    inner_y = list(range(1, ny - 1))
    inner_x = [x for x in range(1, nx - 1) if 1 <= x % 64 <= 62]
    sites = []                                                      # (frame, y, x, cas, (a, b, e), kind, equal)
    for cas in range(8 if z == 0 else 4):
        ds, dr, dc = sign(cas)
        for a, b, e in itertools.product((-1, 0, 1), repeat=3):
            if a in (0, -ds) and b in (0, -dr) and e in (0, -dc):
                continue                                            # inside the block
            kinds = [("interior", inner_y, inner_x)]
            if e == dc:
                kinds.append(("lane", inner_y, [63] if dc > 0 else [64]))
                kinds.append(("coledge", inner_y, [0] if dc < 0 else [nx - 1]))
            if b == dr:
                kinds.append(("rowedge", [0] if dr < 0 else [ny - 1], inner_x))
            for kind, ys, xs in kinds:
                for equal in (True, False):
                    fi, pl, y, x, s, r, c = camp.site(o, z, cas, ys, xs)
                    P = F32(rng.uniform(8.0, 30.0))
                    pl.put(o, s, r, c, P)
                    pl.put(o, s + a, r + b, c + e, P if equal else np.nextafter(P, F32(np.inf)))
                    sites.append((fi, y, x, cas, (a, b, e), kind, equal))
    return camp.finish(f"matrix_o{o}_"), sites


@pytest.mark.parametrize("o", [0, 1])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_neighbour_matrix(surf, orc, gname, o):
    geo = geo_of(orc, gname)
    geometry_facts(geo)
    frames, sites = cached(("matrix", gname, o), lambda: matrix_frames(geo, o, 0))
    lev = [level_blocks(geo, fr.resp, o, 0) for fr in frames]
    seen = set()
    for (fi, y, x, cas, pos, kind, equal) in sites:
        L = lev[fi]
        assert L["cas"][y, x] == cas and L["cand"][y, x], (fi, y, x, cas, pos)
        assert bool(L["surv"][y, x]) == equal, (fi, y, x, cas, pos, kind, equal)
        if equal:                                                   # and the survivor is a point
            fit = simulate_fit(geo, frames[fi].resp, o, int(L["s"][y, x]), int(L["r"][y, x]), int(L["c"][y, x]))
            assert fit["why"] == "ok", (cas, pos, fit)
        seen.add((cas, pos, kind, equal))
    n_view = sum(1 for (_, _, _, cas, pos, _, _) in sites if o > 0 and 1 + (cas >> 2) + pos[0] < 2)
    assert len(seen) == len(sites) and len({(c, p) for (c, p, _, _) in seen}) == 8 * 19
    for kind in ("interior", "lane", "coledge", "rowedge"):
        assert sum(1 for s in seen if s[2] == kind) >= 8 * 9 * 2, kind
    assert o == 0 or n_view >= 8 * 3 * 2                            # neighbours planted through a view
    print(f"(b) {gname} octave {o}: {len(frames)} frames, {len(sites)} peaks, {n_view} neighbours on view planes")
    rig = Rig(surf, geo, len(frames))
    check_frames(rig, frames, "matrix")
    rig.close()


# ------------------------------------------------------------ (c) dense lattice

def dense_frame(geo, levels=(0, 1), seed=41):
    """Octave 0: every block of the given levels holds a peak (10 .. 20) at its first sample among
    samples of 1 .. 3: an isolated bump two samples from the next, fitted with small offsets."""
    rng = np.random.default_rng(seed)
    resp = np.zeros(geo.tot, F32)
    A = geo.planes(resp, 0)
    A[:, :, :geo.sw[0]] = rng.uniform(1.0, 3.0, (5, geo.sh[0], geo.sw[0])).astype(F32)
    n = 0
    for z in levels:
        ny, nx = geo.nblocks(0, z)
        mb = geo.mb[0][z]
        A[2 * z + 1, mb:mb + 2 * ny:2, mb:mb + 2 * nx:2] = rng.uniform(10.0, 20.0, (ny, nx)).astype(F32)
        n += ny * nx
    # octaves > 0 see planes 2 / 4 of octave 0 (1 .. 3 < 0.8 thresh) and zeros: no candidates there
    return Frame(geo, resp, img=0, name="dense"), n


def dense_set(orc, gname):
    return cached(("dense", gname), lambda: dense_frame(geo_of(orc, gname)))


def assert_dense_classes(fr, planted):
    ref, n = fr.ref()
    assert n == planted == len(ref) and n > RANK_LDS, (n, planted)
    sv = fr.surv()
    assert len(sv) == n
    slot, count = item_slots(sv)
    assert (count == ITEM_CAP).sum() >= ITEM_CAP * 8 and count.max() == ITEM_CAP      # full items
    assert (slot < CUBE_CAP).sum() >= 8 and (slot >= CUBE_CAP).sum() >= 8
    return n


@pytest.mark.parametrize("gname", list(GEOMS))
def test_dense_lattice(surf, orc, monkeypatch, gname):
    """More than 16,384 survivors in one frame: full scan items, record slots on both sides of kCubeCap,
    k_sort_rank's global-key path (1 frame); under SURFHIP_SORT_BITONIC=1 and at 9 frames k_sort's
    global-scratch path (candidate capacity 32,768)."""
    geo = geo_of(orc, gname)
    geometry_facts(geo)
    fr, planted = dense_set(orc, gname)
    n = assert_dense_classes(fr, planted)
    print(f"(c) {gname}: {n} accepted peaks of {planted} planted")
    with_env(monkeypatch, "")
    rig = Rig(surf, geo, 9)
    assert rig.det.capacity() == BIG_PTS > SORT_CAP
    one = check_frames(rig, [fr], "dense x1")
    sparse = sparse_frame(geo, 0)
    nine = check_frames(rig, [fr, sparse, fr] + [sparse] * 5 + [fr], "dense x9")
    assert nine[0] == nine[2] == nine[8] == one[0]
    rig.close()
    with_env(monkeypatch, "SURFHIP_SORT_BITONIC=1")
    rig = Rig(surf, geo, 1)
    assert took(rig.switches(), "SURFHIP_SORT_BITONIC=1"), rig.switches()
    assert check_frames(rig, [fr], "dense bitonic") == one
    rig.close()


# ------------------------------------------------------------ (d) late candidates

def late_frame(geo):
    """Octave 0 level 0, wave 1 of scan row 2, block columns 64 .. 127: the pass's first block row
    (u = 0, y = 33) holds 64 candidates that pass the argmax, threshold and lane tests and are all
    suppressed from plane s - 1 (even lanes) or s + 1 (odd lanes); three survivors follow in rows 37, 41,
    45 of the same wave, so their candidate index is >= 64 and their record slot < 8."""
    pl = Planter(geo)
    mb, y0 = geo.mb[0][0], 2 * SCAN_ROWS + 1
    rng = np.random.default_rng(51)
    for x in range(64, 128):
        P = F32(rng.uniform(8.0, 30.0))
        r, c = mb + 2 * y0, mb + 2 * x
        pl.put(0, 1, r, c, P)
        if x % 2 == 0:
            pl.put(0, 0, r, c, P + F32(1))                          # plane s - 1
        else:
            pl.put(0, 2, r - 1, c, P + F32(1))                      # plane s + 1, row r - 1 (outside the block)
    late = [(y0 + 4, 70, 0), (y0 + 8, 90, 3), (y0 + 12, 110, 5)]
    for (y, x, cas) in late:
        pl.put(0, 1 + (cas >> 2), mb + 2 * y + ((cas >> 1) & 1), mb + 2 * x + (cas & 1), F32(rng.uniform(8.0, 30.0)))
    return Frame(geo, pl.resp, img=1, name="late"), y0, late


@pytest.mark.parametrize("env", ["", "SURFHIP_FIT_CUBE=0"])
def test_late_candidates(surf, orc, monkeypatch, env):
    geo = geo_of(orc, "640x400")
    geometry_facts(geo)
    fr, y0, late = cached(("late",), lambda: late_frame(geo))
    L = level_blocks(geo, fr.resp, 0, 0)
    row = slice(64, 128)
    assert L["cand"][y0, row].all() and (L["cas"][y0, row] == 0).all() and not L["surv"][y0, row].any()
    # cas 0: the lane test compares with lane - 1's right column, -inf for lane 0
    assert not (L["best"][y0, 65:128] < L["rmax"][y0, 64:127]).any()
    sv = fr.surv()
    mine = sv[(sv["o"] == 0) & (sv["z"] == 0) & (sv["y"] % SCAN_ROWS % 4 == 1) & (sv["y"] // SCAN_ROWS == 2) & (sv["x"] // 64 == 1)]
    assert sorted((int(a), int(b), int(c)) for a, b, c in zip(mine["y"], mine["x"], mine["cas"])) == sorted(late)
    assert 0 < len(mine) < CUBE_CAP
    print(f"(d) 64 suppressed candidates in row {y0}, {len(mine)} late survivors, {fr.ref()[1]} points in the frame")
    with_env(monkeypatch, env)
    rig = Rig(surf, geo, 1)
    assert took(rig.switches(), env) and ("SURFHIP_FIT_CUBE" in rig.switches()["switches"]) == bool(env)
    check_frames(rig, [fr], "late")
    rig.close()


# ------------------------------------------------------------ (e) fit outcomes

def noise_frames(geo):
    """White and 3x3x3-smoothed noise on all real planes, at an amplitude around thresh (0 .. 2 thresh)
    and squeezed into [0.75, 1.25] thresh."""
    out = []
    for i, (smooth, lo, hi) in enumerate(((False, 0.0, 2.0), (True, 0.0, 2.0), (False, 0.75, 1.25), (True, 0.75, 1.25))):
        rng = np.random.default_rng(61 + i)
        resp = np.zeros(geo.tot, F32)
        for o in range(geo.noct):
            A = geo.planes(resp, o)
            v = rng.uniform(0.0, 1.0, (5, geo.sh[o], geo.sw[o]))
            if smooth:
                pad = np.pad(v, 1, mode="edge")
                v = sum(pad[1 + a:1 + a + 5, 1 + b:1 + b + geo.sh[o], 1 + e:1 + e + geo.sw[o]]
                        for a, b, e in itertools.product((-1, 0, 1), repeat=3)) / 27.0
                v = (v - v.min()) / (v.max() - v.min())
            first = 0 if o == 0 else 2
            A[first:, :, :geo.sw[o]] = (THRESH * (lo + (hi - lo) * v[first:])).astype(F32)
        out.append(Frame(geo, resp, img=i % 2, name=("smooth" if smooth else "white") + f"_{lo:g}"))
    return out


def special_frame(geo):
    """Planted fit cases: 3x3x3 plateaus (0 / 0 -> NaN), a NaN response as a block's first value, and
    peaks whose interpolated scale makes the getTrace box leave the frame on each side."""
    camp = Campaign(geo, limit=1)
    cases = []
    o = 0
    ny, nx = geo.nblocks(o, 0)
    for z in (0, 1, 0, 1):                                          # plateaus around a block's first sample
        fi, pl, y, x, s, r, c = camp.site(o, z, 0, range(3, ny - 3), range(3, nx - 3))
        for a, b, e in itertools.product((-1, 0, 1), repeat=3):
            pl.put(o, s + a, r + b, c + e, F32(9.0))
        cases.append(("plateau", o, s, r, c))
    for z in (0, 1):                                                # NaN as the block's first value
        fi, pl, y, x, s, r, c = camp.site(o, z, 0, range(3, ny - 3), range(3, nx - 3))
        pl.put(o, s, r, c, F32(np.nan))
        cases.append(("nanfirst", o, s, r, c))
    # getTrace: the last octave's level 1 (s = 3) with a scale offset of about +1.4 from the coupling of the
    # scale with the axis along the border (H01 = 37 against H00 = -20.5, H11 = -100, g0 = 9.75): the box
    # reaches 1.5 temp, temp = 3 ns, from the centre
    o = geo.noct - 1
    ny, nx = geo.nblocks(o, 1)
    for side, ys, xs in (("top", [0], [nx // 2]), ("bottom", [ny - 1], [nx // 2]), ("left", [ny // 2], [0]),
                         ("right", [ny // 2], [nx - 1])):
        cas = {"top": 0, "bottom": 2, "left": 0, "right": 1}[side]
        fi, pl, y, x, s, r, c = camp.site(o, 1, cas, ys, xs)
        along = (1, 0) if side in ("left", "right") else (0, 1)    # couple the scale with the axis along the border
        b, e = along
        pl.put(o, s, r, c, F32(10.0))
        pl.put(o, s + 1, r, c, F32(9.5))
        pl.put(o, s - 1, r, c, F32(-10.0))
        pl.put(o, s, r + b, c + e, F32(-40.0))
        pl.put(o, s, r - b, c - e, F32(-40.0))
        pl.put(o, s + 1, r + b, c + e, F32(9.0))
        pl.put(o, s - 1, r - b, c - e, F32(9.0))
        pl.put(o, s + 1, r - b, c - e, F32(-65.0))
        pl.put(o, s - 1, r + b, c + e, F32(-65.0))
        cases.append(("trace_" + side, o, s, r, c))
    # borders[s] clamps: a level-0 peak of octave 0 on the outermost sample of the first / last block row /
    # column, m = 1 or 2 samples from the line r == borders[s] (r == sh - borders[s], ...).  Along t (samples
    # towards the border) plane s holds 10, -10, -15, -17, -18 and planes s + 1 / s - 1 the values below: the
    # first fit's scale-row coupling gives an offset of 0.66 towards the border, every later one's negative
    # slope on positive curvature 0.83 and 1.17, so the survivor moves m times and is then held by the clamp
    o, z, s = 0, 0, 1
    ny, nx = geo.nblocks(o, z)
    mb, bs = geo.mb[o][z], geo.borders[o][s]
    f_t = {-1: -10.0, 0: 10.0, 1: -10.0, 2: -15.0, 3: -17.0, 4: -18.0}
    n_t = {-1: -134.0, 0: 9.5, 1: -30.0, 2: 0.0, 3: 0.0, 4: 0.0}
    p_t = {-1: 10.0, 0: -89.5, 1: -30.0, 2: -99.0, 3: 0.0, 4: 0.0}
    for side, ys, xs, cas, (b, e) in (("top", [0], [nx // 2 + 7], 0, (-1, 0)), ("bottom", [ny - 1], [nx // 2 + 7], 2, (1, 0)),
                                      ("left", [ny // 2 + 5], [0], 0, (0, -1)), ("right", [ny // 2 + 5], [nx - 1], 1, (0, 1))):
        fi, pl, y, x, s_, r, c = camp.site(o, z, cas, ys, xs)
        m = {"top": r - bs, "bottom": geo.sh[o] - bs - r, "left": c - bs, "right": geo.sw[o] - bs - c}[side]
        assert s_ == s and m in (1, 2), (side, m)
        for t in range(-1, m + 2):
            pl.put(o, s, r + t * b, c + t * e, F32(f_t[t]))
            pl.put(o, s + 1, r + t * b, c + t * e, F32(n_t[t]))
            pl.put(o, s - 1, r + t * b, c + t * e, F32(p_t[t]))
        cases.append((f"clamp_{side}_{m}", o, s, r, c))
    return Frame(geo, camp.frames[0].resp, img=1, name="special"), cases


def fit_set(orc, gname):
    def make():
        geo = geo_of(orc, gname)
        sp, cases = special_frame(geo)
        return noise_frames(geo) + [sp], cases
    return cached(("fit", gname), make)


FIT_CLASSES = ("not_moved", "moved_1", "moved_ge2", "off_gt_1.5", "weak")


def classify_fits(geo, frames):
    """Every survivor of the noise frames through simulate_fit: class -> count; also the clamp sides."""
    tally = {k: 0 for k in FIT_CLASSES + ("moved_5", "nan", "clamp_top", "clamp_bottom", "clamp_left", "clamp_right",
                                          "survivors", "accepted")}
    for fr in frames:
        sv = fr.surv()
        tally["survivors"] += len(sv)
        for q in sv:
            fit = simulate_fit(geo, fr.resp, int(q["o"]), int(q["s"]), int(q["r"]), int(q["c"]))
            m = fit["moves"]
            tally["not_moved" if m == 0 else "moved_1" if m == 1 else "moved_ge2"] += 1
            tally["moved_5"] += m == 5
            tally["nan"] += fit["why"] == "nan"
            tally["off_gt_1.5"] += fit["why"] == "off"
            tally["weak"] += fit["why"] == "weak"
            tally["accepted"] += fit["why"] == "ok"
            for side in fit["clamp"]:
                tally["clamp_" + side] += 1
    return tally


@pytest.mark.parametrize("gname", list(GEOMS))
def test_fit_outcomes(surf, orc, gname):
    geo = geo_of(orc, gname)
    geometry_facts(geo)
    frames, cases = fit_set(orc, gname)
    noise, special = frames[:-1], frames[-1]
    tally = cached(("tally", gname), lambda: classify_fits(geo, noise))
    print(f"(e) {gname}: noise survivors per frame {[len(fr.surv()) for fr in noise]}, points "
          f"{[fr.ref()[1] for fr in noise]}; classes {tally}")
    assert tally["accepted"] == sum(fr.ref()[1] for fr in noise)
    for k in FIT_CLASSES:
        assert tally[k] >= 8, (k, tally[k])
    sides = trace_sides(geo, special.ref()[0])
    for name, o, s, r, c in cases:
        fit = simulate_fit(geo, special.resp, o, s, r, c)
        if name in ("plateau", "nanfirst"):
            assert fit["why"] == "nan", (name, fit)
        elif name.startswith("clamp"):
            _, side, m = name.split("_")
            assert fit["clamp"] == {side} and fit["moves"] == int(m), (name, fit)
        else:
            assert fit["why"] == "ok" and fit["moves"] == 0 and fit["off"][0] > 1.0, (name, fit)
            assert sides[name[6:]].any(), name
    sv = special.surv()
    for name, o, s, r, c in cases:
        assert ((sv["o"] == o) & (sv["s"] == s) & (sv["r"] == r) & (sv["c"] == c)).any(), (name, o, s, r, c)
    rig = Rig(surf, geo, len(frames))
    check_frames(rig, frames, "fit")
    rig.close()


# ------------------------------------------------------------ (f) sparse batches

def sparse_frame(geo, kind):
    """kind 0: flat; 1 .. 3: one or two peaks in different places."""
    def make():
        pl = Planter(geo)
        ny, nx = geo.nblocks(0, 0)
        spots = {1: [(0, 0, 3, 5, 5)], 2: [(0, 1, 2, ny - 2, nx - 3), (geo.noct - 1, 0, 1, 1, 2)],
                 3: [(1, 0, 6, 7, 66), (0, 0, 0, 40, 127)]}.get(kind, [])
        for (o, z, cas, y, x) in spots:
            mb = geo.mb[o][z]
            pl.put(o, 2 * z + 1 + (cas >> 2), mb + 2 * y + ((cas >> 1) & 1), mb + 2 * x + (cas & 1), F32(11.0 + kind))
        return Frame(geo, pl.resp, img=kind % 2, name=f"sparse{kind}")
    return cached(("sparse", geo.name, kind), make)


def test_sparse_batches(surf, orc):
    """17 frames, survivors in frames 0, 8 and 16 only: two prefix chunks (k_scan_top + k_scan_add), a
    fit wave whose survivors are more than 64 scan items apart (k_nms_fit's per-lane search), empty
    frames between; then an all-flat batch."""
    geo = geo_of(orc, "640x400")
    geometry_facts(geo)
    items = geo.scan_wgs() * 4
    assert 17 * items == 3536 > SCAN_CHUNK and 8 * items > 64
    flat = sparse_frame(geo, 0)
    frames = [flat] * 17
    frames[0], frames[8], frames[16] = sparse_frame(geo, 1), sparse_frame(geo, 2), sparse_frame(geo, 3)
    total = 0
    for f, fr in enumerate(frames):
        n = fr.ref()[1]
        assert n == len(fr.surv()) == ({0: 1, 8: 2, 16: 2}.get(f, 0)), (f, n)
        total += n
    assert total <= 64                                               # one fit wave holds them all
    rig = Rig(surf, geo, 17, max_pts=64)
    check_frames(rig, frames, "sparse")
    pts, counts, cand, trunc, tot = rig.run([flat] * 17)
    assert not counts.any() and not cand.any() and tot == 0 and not trunc
    check_frames(rig, frames, "sparse again")
    rig.close()


# ------------------------------------------------------------ (g) batch shapes

def pool(orc, gname):
    return peaks_set(orc, gname)[0] + [dense_set(orc, gname)[0]] + fit_set(orc, gname)[0]


@pytest.mark.parametrize("gname", list(GEOMS))
def test_batch_shapes(surf, orc, monkeypatch, gname):
    """The frames of (a), (c) and (e) as batches of 1, 3, 8, 9 and 17: k_sort_rank (<= 8 frames), k_sort
    (more), the XCD frame mapping (>= 8); a frame gives the same bytes at every position of every batch."""
    geo = geo_of(orc, gname)
    geometry_facts(geo)
    frames = pool(orc, gname)
    L = len(frames)
    assert_dense_classes(*dense_set(orc, gname))
    with_env(monkeypatch, "")
    rig = Rig(surf, geo, 17)
    assert rig.switches()["switches"].count("SURFHIP_FIT_CUBE") == 0
    want = {}
    for n in (17, 9, 8, 3, 1):
        positions = set()
        for b, start in enumerate(range(0, L, n)):
            idx = [(start + i + b) % L for i in range(n)]
            got = check_frames(rig, [frames[i] for i in idx], f"batch of {n}")
            for pos, (i, raw) in enumerate(zip(idx, got)):
                assert want.setdefault(i, raw) == raw, f"frame {i} differs at position {pos} of a batch of {n}"
                positions.add(pos)
        assert positions == set(range(n)) and (n > 1 or len(want) == L)
    rig.close()
    for env in ("SURFHIP_FIT_CUBE=0", "SURFHIP_SORT_BITONIC=1"):
        with_env(monkeypatch, env)
        rig = Rig(surf, geo, 1)
        assert took(rig.switches(), env), rig.switches()
        for i, fr in enumerate(frames):
            assert check_frames(rig, [fr], env)[0] == want[i], (env, i)
        rig.close()


# ------------------------------------------------------------ (h) caps

def spikes_frame(geo, n):
    def make():
        camp = Campaign(geo, limit=1)
        ny, nx = geo.nblocks(0, 0)
        rng = np.random.default_rng(71)
        for t in range(n):
            fi, pl, y, x, s, r, c = camp.site(0, 0, t % 8, range(ny), range((t * 7) % 5, nx))
            pl.put(0, s, r, c, F32(rng.uniform(6.0, 40.0)))
        return Frame(geo, camp.frames[0].resp, img=0, name=f"spikes{n}")
    return cached(("spikes", geo.name, n), make)


def test_max_pts_cut(surf, orc):
    geo = geo_of(orc, "640x400")
    frames = [peaks_set(orc, "640x400")[0][0], fit_set(orc, "640x400")[0][0], dense_set(orc, "640x400")[0]]
    rig = Rig(surf, geo, 3, max_pts=20, cand_cap=BIG_PTS)
    pts, counts, cand, trunc, total = rig.run(frames)
    for f, fr in enumerate(frames):
        ref, n = fr.ref()
        assert n > 20 and counts[f] == 20 and cand[f] == n
        same_points(pts[f], ref[:20], f"max_pts frame {f}")       # the oracle's canonical prefix
    assert not trunc
    rig.close()


def test_candidate_cap(surf, orc):
    """cand_cap = 256 with 256 and 257 accepted peaks: the first fits; the second is truncated to exactly
    256, a canonically ordered subset of the full result (which survivor is dropped is not pinned), the
    same bytes run to run and at position 8 of a 17-frame batch."""
    geo = geo_of(orc, "640x400")
    f256, f257 = spikes_frame(geo, 256), spikes_frame(geo, 257)
    assert f256.ref()[1] == 256 == len(f256.surv()) and f257.ref()[1] == 257 == len(f257.surv())
    rig = Rig(surf, geo, 17, max_pts=512, cand_cap=256)
    assert rig.det.capacity() == 256
    check_frames(rig, [f256], "cap 256")
    runs = []
    flat = sparse_frame(geo, 0)
    for batch, at in (([f257], 0), ([f257], 0), ([flat] * 8 + [f257] + [flat] * 8, 8)):
        pts, counts, cand, trunc, total = rig.run(batch)
        assert trunc and counts[at] == 256 and cand[at] == 257, (counts, cand, trunc)
        assert counts.sum() == 256
        got, full = pts[at], f257.ref()[0]
        key = lambda p: [(a.tobytes()) for a in p]
        fk = key(full)
        where = [fk.index(k) for k in key(got)]                     # every point is one of the full result's
        assert where == sorted(where) and len(set(where)) == 256     # in canonical order, each once
        runs.append(got.tobytes())
    assert runs[0] == runs[1] == runs[2]
    check_frames(rig, [f256], "cap 256 after a truncated batch")   # the flag is reset
    rig.close()


# ------------------------------------------------------------ (i) stale state

def test_stale_state(surf, orc):
    """Dense, sparse, flat, then dense with another frame count on one detector: item_count,
    cand_count, status, scan_cube and keys of the previous batch must not show."""
    geo = geo_of(orc, "640x400")
    dense, sp, flat = dense_set(orc, "640x400")[0], sparse_frame(geo, 2), sparse_frame(geo, 0)
    noise = fit_set(orc, "640x400")[0][0]
    rig = Rig(surf, geo, 9)
    a = check_frames(rig, [dense, noise, dense], "dense")
    b = check_frames(rig, [sp, sp, flat, sp], "sparse after dense")
    pts, counts, cand, trunc, tot = rig.run([flat] * 3)
    assert not counts.any() and not cand.any() and tot == 0
    c = check_frames(rig, [noise, dense] + [flat] * 6 + [dense], "dense after flat")
    rig.close()
    fresh = Rig(surf, geo, 9)
    assert check_frames(fresh, [sp, sp, flat, sp], "sparse, fresh") == b
    assert check_frames(fresh, [noise, dense] + [flat] * 6 + [dense], "dense, fresh") == c
    fresh.close()
    assert a[0] == a[2] == c[1] == c[8] and a[1] == c[0]


# ------------------------------------------------------------ (j) argument checks

def test_run_nms_argument_checks(surf, orc):
    geo = geo_of(orc, "640x400")
    rig = Rig(surf, geo, 2, max_pts=64)
    pb, cb = surf.DeviceBuffer(48 * 2 * 64), surf.DeviceBuffer(8)
    with pytest.raises(surf.SurfError, match="invalid argument"):          # no integral resident yet
        rig.det.run_nms(1, pb.ptr, cb.ptr)
    rig.fb.upload(np.stack([geo.imgs[0]]))
    rig.det.run_integral(rig.fb.ptr, 1, geo.pitch, geo.h * geo.pitch)
    surf.synchronize()
    for args in ((0, pb.ptr, cb.ptr), (3, pb.ptr, cb.ptr), (-1, pb.ptr, cb.ptr), (1, None, cb.ptr), (1, pb.ptr, None)):
        with pytest.raises(surf.SurfError, match="invalid argument"):
            rig.det.run_nms(*args)
    with pytest.raises(surf.SurfError, match="invalid argument"):
        surf.check(surf.lib.surfhip_run_nms(None, 1, pb.ptr, cb.ptr), "run_nms")
    rig.det.run_nms(1, pb.ptr, cb.ptr)                                      # and a valid call goes through
    surf.synchronize()
    assert cb.download(np.int32, 1)[0] == 0                                 # the planes are still zero
    rig.close()
