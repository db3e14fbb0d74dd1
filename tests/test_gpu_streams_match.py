"""The stateless calls on a caller's non-blocking stream: surfhip_match,
surfhip_match_batch, _cross, _window, _guided, surfhip_homography_batch and
surfhip_fundamental_batch, each through the late-upload protocol of
stream_ref.late ("Caller streams"): the inputs reach the live
buffers on the stream, behind a delay, and the snapshot taken on the stream
after the call equals, byte for byte, the null-stream run of the same chain.

Two positive controls first: the same chain with the call itself on another
stream must NOT give the reference, or the protocol proves nothing here.
"""
from __future__ import annotations

import numpy as np
import pytest

from match_ref import FULL_TAIL, SAME_LAPLACE, make_points, small_batch, with_canary
from stream_ref import Streams, copy_async, late
from test_gpu_fundamental import CAM_VERTICAL
from test_gpu_fundamental import COUNTS as F_COUNTS
from test_gpu_fundamental import plant_pair as f_plant_pair
from test_gpu_fundamental import ragged_data as f_ragged_data
from test_gpu_homography import COUNTS as H_COUNTS
from test_gpu_homography import H_PERSPECTIVE
from test_gpu_homography import plant_pair as h_plant_pair
from test_gpu_homography import ragged_data as h_ragged_data

pytestmark = pytest.mark.gpu

MUTUAL = 4
S1, S2 = 160, 96                                   # two 128-point blocks of set 1, three tiles of set 2
C1, C2 = (160, 0, 97), (96, 50, 33)                # ragged, a pair with no set-1 point; 50, 33: partial tiles
WINDOW = (-32.0, 32.0, -32.0, 32.0)


def batch_sets(surf, p1, f1, c1, p2, f2, c2):
    """Live buffers of one batched call: (buffers, inputs for late(), the eight leading arguments)."""
    arrs = [p1, f1, np.asarray(c1, np.int32), p2, f2, np.asarray(c2, np.int32)]
    live = [surf.DeviceBuffer(max(a.nbytes, 4)) for a in arrs]
    args = (live[0].ptr, live[1].ptr, live[2].ptr, p1.shape[1], live[3].ptr, live[4].ptr, live[5].ptr, p2.shape[1])
    return live, list(zip(live, arrs)), args


def ragged(surf, nf, seed=77):
    _, p1, f1, p2, f2 = small_batch(surf, seed + nf, len(C1), S1, S2, nf)
    return p1, f1, p2, f2


def free(*bufs):
    for b in bufs:
        b.free()


# ---------------------------------------------------------------- controls

def poison_points(surf, got, p1):
    """The set-1 points as a match call leaves them that ran on the poison (counts 0: nothing
    written) before the points arrived: the uploaded bytes, canaries and all."""
    return got == np.ascontiguousarray(p1).tobytes()


@pytest.mark.parametrize("where", ["other", "null"])
def test_control_match_batch_on_another_stream_is_seen(surf, where):
    """surfhip_match_batch issued on a second non-blocking stream / on the null stream while spin,
    uploads and snapshot stay on S: it runs at once, finds counts 0 and writes nothing."""
    p1, f1, p2, f2 = ragged(surf, 64)
    live, inputs, args = batch_sets(surf, p1, f1, C1, p2, f2, C2)
    with Streams(surf, 2) as (s, t):
        r = late(surf, s, inputs, [live[0]], lambda st: surf.match_batch(*args, len(C1), 64, FULL_TAIL, st),
                 call_stream=t if where == "other" else None, poison=True, label=f"control match_batch {where}")
    free(*live)
    assert r.ref[0] != r.poison[0] and poison_points(surf, r.poison[0], p1)
    assert r.got[0] != r.ref[0], "protocol cannot see a call on another stream"
    assert r.got[0] == r.poison[0]


@pytest.mark.parametrize("where", ["other", "null"])
def test_control_homography_batch_on_another_stream_is_seen(surf, where):
    """surfhip_homography_batch likewise: on counts 0 every record is TOO_FEW with the identity."""
    pts, _ = h_ragged_data(surf)
    n, slots = pts.shape
    pb, cb = surf.DeviceBuffer(pts.nbytes), surf.DeviceBuffer(4 * n)
    ob, mb = surf.DeviceBuffer(64 * n), surf.DeviceBuffer(n * slots)
    with Streams(surf, 2) as (s, t):
        r = late(surf, s, [(pb, pts), (cb, np.asarray(H_COUNTS, np.int32))], [ob, mb],
                 lambda st: surf.homography_batch(pb.ptr, cb.ptr, slots, n, ob.ptr, mb.ptr, stream=st),
                 call_stream=t if where == "other" else None, poison=True, label=f"control homography {where}")
    free(pb, cb, ob, mb)
    early = np.frombuffer(r.poison[0], surf.HOMOGRAPHY_DTYPE)
    assert (early["status"] == surf.HOMOG_TOO_FEW).all() and (early["ncand"] == 0).all()
    assert not np.frombuffer(r.poison[1], np.uint8).any()
    assert (np.frombuffer(r.ref[0], surf.HOMOGRAPHY_DTYPE)["status"] == surf.HOMOG_OK).sum() >= 8
    assert r.got[0] != r.ref[0], "protocol cannot see a call on another stream"
    assert r.got[0] == r.poison[0] and r.got[1] == r.poison[1]


# ------------------------------------------------------------ surfhip_match

@pytest.mark.parametrize("own_scratch", [False, True], ids=["library-scratch", "caller-scratch"])
@pytest.mark.parametrize("n1,n2,nf", [(70, 90, 64), (129, 333, 36)])
def test_match(surf, n1, n2, nf, own_scratch):
    """One pair; (129, 333, 36): k_match_part<0>, more than one chunk of set 2 and the merge.  With the
    library's scratch the call synchronises inside: it is the chain's last call."""
    rng = np.random.default_rng(5 + n1)
    f1 = rng.standard_normal((n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((n2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 1, n1, surf.POINT_DTYPE))[0]
    p2 = make_points(rng, 1, n2, surf.POINT_DTYPE)[0]
    arrs = [p1, p2, f1, f2]
    live = [surf.DeviceBuffer(a.nbytes) for a in arrs]
    scratch = [surf.DeviceBuffer(surf.match_scratch_bytes(n1, n2, FULL_TAIL))] if own_scratch else []

    def call(st):
        surf.match_points(live[0].ptr, live[1].ptr, live[2].ptr, live[3].ptr, n1, n2, nf, FULL_TAIL,
                          scratch[0].ptr if own_scratch else None, st)

    with Streams(surf) as s:
        r = late(surf, s, list(zip(live, arrs)), [live[0]], call if own_scratch else (lambda st: None),
                 scratch=scratch, last=None if own_scratch else call, label=f"match {n1}x{n2}x{nf}")
    free(*live, *scratch)
    r.assert_equal(["set-1 points"])
    got = np.frombuffer(r.got[0], surf.POINT_DTYPE)
    assert (got["match"] >= 0).sum() >= n1 // 2


# ------------------------------------------------------- the batched matches

@pytest.mark.parametrize("flags", [0, SAME_LAPLACE | FULL_TAIL])
@pytest.mark.parametrize("nf", [64, 36])
def test_match_batch(surf, nf, flags):
    p1, f1, p2, f2 = ragged(surf, nf)
    live, inputs, args = batch_sets(surf, p1, f1, C1, p2, f2, C2)
    with Streams(surf) as s:
        r = late(surf, s, inputs, [live[0]], lambda st: surf.match_batch(*args, len(C1), nf, flags, st),
                 label=f"match_batch nf {nf} flags {flags}")
    free(*live)
    r.assert_equal(["set-1 points"])
    got = np.frombuffer(r.got[0], surf.POINT_DTYPE).reshape(len(C1), S1)
    assert (got["match"][0] >= 0).sum() >= 32 and (got["match"][1] == p1["match"][1]).all()


@pytest.mark.parametrize("flags", [0, SAME_LAPLACE | FULL_TAIL])
@pytest.mark.parametrize("nf", [64, 36])
def test_match_batch_cross(surf, nf, flags):
    """The memset of the back-direction words, the main kernel and k_match_cross_filter."""
    p1, f1, p2, f2 = ragged(surf, nf)
    live, inputs, args = batch_sets(surf, p1, f1, C1, p2, f2, C2)
    sb = surf.DeviceBuffer(surf.match_batch_cross_scratch_bytes(len(C1), S1, S2))
    with Streams(surf) as s:
        r = late(surf, s, inputs, [live[0]],
                 lambda st: surf.match_batch_cross(*args, len(C1), nf, sb.ptr, flags, st), scratch=[sb],
                 label=f"match_batch_cross nf {nf} flags {flags}")
    free(*live, sb)
    r.assert_equal(["set-1 points"])
    got = np.frombuffer(r.got[0], surf.POINT_DTYPE).reshape(len(C1), S1)
    assert (got["match"][0] >= 0).sum() >= 8


@pytest.mark.parametrize("counts", ["late-counts", "resident-counts"])
@pytest.mark.parametrize("flags", [0, MUTUAL])
def test_match_batch_window(surf, flags, counts):
    """k_match_tile_boxes, the memset of the keys, the kernel and the filter, in a +-32 px window.

    late-counts is the protocol as everywhere.  It cannot see k_match_tile_boxes running too early:
    with n2 = 0 that kernel writes no box, and the 0xFF it leaves in the scratch are NaN boxes, which
    keep every tile -- the result is right.  resident-counts closes that: both count arrays are in
    place from the start, only points and descriptors are late and the scratch is not filled again
    on the stream, so boxes made too early are the boxes of zero points, (0, 0, 0, 0), and the waves
    whose points lie more than the window from the origin skip every tile."""
    p1, f1, p2, f2 = ragged(surf, 64)
    live, inputs, args = batch_sets(surf, p1, f1, C1, p2, f2, C2)
    resident = []
    if counts == "resident-counts":
        resident = [inputs[2], inputs[5]]
        inputs = [inputs[k] for k in (0, 1, 3, 4)]
    sb = surf.DeviceBuffer(surf.match_batch_window_scratch_bytes(len(C1), S1, S2, flags))
    with Streams(surf) as s:
        r = late(surf, s, inputs, [live[0]],
                 lambda st: surf.match_batch_window(*args, len(C1), 64, flags, WINDOW, sb.ptr, st), scratch=[sb],
                 resident=resident, refill=not resident, label=f"match_batch_window flags {flags} {counts}")
    free(*live, sb)
    r.assert_equal(["set-1 points"])
    got = np.frombuffer(r.got[0], surf.POINT_DTYPE).reshape(len(C1), S1)
    assert (got["match"][0] >= 0).sum() >= 8 and (got["match"][0] == -1).any()


def test_match_batch_window_more_tiles_than_one_list_chunk(surf):
    """The shape of test_gpu_match_window.test_more_tiles_than_one_list_chunk: n2 = 8300, 260 tiles,
    the kept-tile list built in two chunks."""
    nf, n1, n2, flags = 64, 64, 8300, FULL_TAIL | MUTUAL
    rng = np.random.default_rng(123)
    f1 = rng.standard_normal((3, n1, nf)).astype(np.float32)
    f2 = rng.standard_normal((3, n2, nf)).astype(np.float32)
    p1 = with_canary(make_points(rng, 3, n1, surf.POINT_DTYPE))
    p2 = make_points(rng, 3, n2, surf.POINT_DTYPE)
    p2["x"] = rng.uniform(0, 100, (3, n2))
    p2["y"] = np.arange(n2, dtype=np.float32)[None, :]
    p1["x"] = rng.uniform(0, 100, (3, n1))
    top, bottom = rng.uniform(0, 150, (3, 32)), rng.uniform(8250, 8299, (3, 32))
    p1["y"][0] = np.concatenate([top[0], bottom[0]])
    p1["y"][1] = np.concatenate([bottom[1], bottom[2]])
    p1["y"][2] = np.concatenate([top[1], top[2]])
    live, inputs, args = batch_sets(surf, p1, f1, [n1] * 3, p2, f2, [n2] * 3)
    sb = surf.DeviceBuffer(surf.match_batch_window_scratch_bytes(3, n1, n2, flags))
    with Streams(surf) as s:
        r = late(surf, s, inputs, [live[0]],
                 lambda st: surf.match_batch_window(*args, 3, nf, flags, (-40.0, 40.0, -40.0, 40.0), sb.ptr, st),
                 scratch=[sb], label="match_batch_window 260 tiles")
    free(*live, sb)
    r.assert_equal(["set-1 points"])
    got = np.frombuffer(r.got[0], surf.POINT_DTYPE).reshape(3, n1)
    assert all((got["match"][i] >= 0).sum() >= 16 for i in range(3))


# ------------------------------------------------- homography, fundamental

def model_case(surf, which, big):
    if which == "homography":
        if not big:
            return h_ragged_data(surf)[0], H_COUNTS
        n = surf.HOMOGRAPHY_LDS_CAPACITY + 33
        p, _ = h_plant_pair(np.random.default_rng(55), surf.POINT_DTYPE, n + 40, n, H_PERSPECTIVE, out_frac=0.3,
                            sprinkle=False)
    else:
        if not big:
            return f_ragged_data(surf)[0], F_COUNTS
        n = surf.FUNDAMENTAL_LDS_CAPACITY + 33
        p, _ = f_plant_pair(np.random.default_rng(55), surf.POINT_DTYPE, n + 40, n, CAM_VERTICAL, out_frac=0.3,
                            sprinkle=False)
    return p[None], (n,)


@pytest.mark.parametrize("big", [False, True], ids=["ragged", "above-lds-capacity"])
@pytest.mark.parametrize("which", ["homography", "fundamental"])
def test_model_batch(surf, which, big):
    pts, counts = model_case(surf, which, big)
    n, slots = pts.shape
    fn, ok = ((surf.homography_batch, surf.HOMOG_OK) if which == "homography"
              else (surf.fundamental_batch, surf.FUND_OK))
    pb, cb = surf.DeviceBuffer(pts.nbytes), surf.DeviceBuffer(4 * n)
    ob, mb = surf.DeviceBuffer(64 * n), surf.DeviceBuffer(n * slots)
    with Streams(surf) as s:
        r = late(surf, s, [(pb, pts), (cb, np.asarray(counts, np.int32))], [ob, mb],
                 lambda st: fn(pb.ptr, cb.ptr, slots, n, ob.ptr, mb.ptr, nhyp=256, stream=st),
                 label=f"{which} {'big' if big else 'ragged'}")
    free(pb, cb, ob, mb)
    r.assert_equal(["records", "inlier mask"])
    res = np.frombuffer(r.got[0], surf.HOMOGRAPHY_DTYPE)
    assert (res["status"] == ok).sum() >= (1 if big else 7) and np.frombuffer(r.got[1], np.uint8).any()


# ---------------------------------------------------------------- the chain

def test_chain_match_homography_guided_homography(surf):
    """match_batch -> homography_batch -> match_batch_guided reading the records where they lie, at
    stride 16 -> homography_batch, on S with no host call between; every input late, every
    intermediate buffer poisoned (the records 0xA5: a NaN-free but wild matrix; the scratch 0xFF)."""
    npairs, s1, s2, nf, flags = 3, 160, 192, 64, FULL_TAIL | MUTUAL
    rng = np.random.default_rng(2024)
    p2 = make_points(rng, npairs, s2, surf.POINT_DTYPE)
    f2 = rng.standard_normal((npairs, s2, nf)).astype(np.float32)
    f2 /= np.linalg.norm(f2, axis=2, keepdims=True)
    # set 1: set-2 points moved back by a small similarity, their descriptors with a little noise
    p1 = with_canary(make_points(rng, npairs, s1, surf.POINT_DTYPE))
    f1 = np.zeros((npairs, s1, nf), np.float32)
    for i in range(npairs):
        ang, tx, ty = np.radians(1.0 + i), 9.0 + i, -6.0 - i
        src = rng.permutation(s2)[:s1]
        x, y = p2["x"][i][src] - tx, p2["y"][i][src] - ty
        p1["x"][i] = (np.cos(ang) * x + np.sin(ang) * y).astype(np.float32)
        p1["y"][i] = (-np.sin(ang) * x + np.cos(ang) * y).astype(np.float32)
        p1["laplace"][i] = p2["laplace"][i][src]
        f1[i] = f2[i][src] + 0.02 * rng.standard_normal((s1, nf)).astype(np.float32)
    c1, c2 = (160, 140, 0), (192, 180, 64)
    live, inputs, args = batch_sets(surf, p1, f1, c1, p2, f2, c2)
    ob1, ob2 = surf.DeviceBuffer(64 * npairs), surf.DeviceBuffer(64 * npairs)
    mb = surf.DeviceBuffer(npairs * s1)
    snap1 = surf.DeviceBuffer(live[0].nbytes)             # the points as the first match left them
    sb = surf.DeviceBuffer(surf.match_batch_guided_scratch_bytes(npairs, s1, s2, flags))

    def chain(st):
        surf.match_batch(*args, npairs, nf, FULL_TAIL, st)
        copy_async(surf, snap1.ptr, live[0].ptr, snap1.nbytes, st)
        surf.homography_batch(live[0].ptr, live[2].ptr, s1, npairs, ob1.ptr, None, stream=st)
        surf.match_batch_guided(*args, npairs, nf, flags, ob1.ptr, 16, (-8.0, 8.0, -8.0, 8.0), sb.ptr, st)
        surf.homography_batch(live[0].ptr, live[2].ptr, s1, npairs, ob2.ptr, mb.ptr, stream=st)

    with Streams(surf) as s:
        r = late(surf, s, inputs, [snap1, ob1, live[0], ob2, mb], chain, scratch=[sb], label="chain")
    free(*live, ob1, ob2, mb, snap1, sb)
    r.assert_equal(["first match", "first homographies", "guided match", "second homographies", "inlier mask"])
    first = np.frombuffer(r.got[1], surf.HOMOGRAPHY_DTYPE)
    second = np.frombuffer(r.got[3], surf.HOMOGRAPHY_DTYPE)
    guided = np.frombuffer(r.got[2], surf.POINT_DTYPE).reshape(npairs, s1)
    print("chain: first", first["status"], first["ninliers"], "second", second["status"], second["ninliers"])
    assert list(first["status"]) == [surf.HOMOG_OK, surf.HOMOG_OK, surf.HOMOG_TOO_FEW]
    assert list(second["status"]) == [surf.HOMOG_OK, surf.HOMOG_OK, surf.HOMOG_TOO_FEW]
    assert (guided["match"][0] >= 0).sum() >= 100 and second["ninliers"][0] >= 100
