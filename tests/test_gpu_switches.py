"""The SURFHIP_* switches belong to the detector: it reads them once, when it
is created, and a variable changed afterwards does not reach it.

Two detectors of one process, created under different environments, each
report their own switches and run their own kernels; the three switches used
(fit records from the scan or the planes, the bitonic or the rank sort,
getTrace in the fit or the describe) are documented as bit-identical, so the
outputs are compared byte for byte, with no tolerance.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_schedule import H, N, W, frames_on_gpu

pytestmark = pytest.mark.gpu

MAX_PTS = 4096
CONFTEST = "SURFHIP_HESS_GATHER=0 SURFHIP_DESC_UR=0"        # tests/conftest.py: streaming plan, k_describe_u2
THREE = {"SURFHIP_FIT_CUBE": "0", "SURFHIP_SORT_BITONIC": "1", "SURFHIP_TRACE_DESC": "0"}
OPPOSITE = {"SURFHIP_FIT_CUBE": "1", "SURFHIP_SORT_BITONIC": None, "SURFHIP_TRACE_DESC": "1"}


def run(surf, det, n):
    """detect_batch of the first n of the N frames: (counts, points, descriptors) as bytes."""
    buf, pitch = frames_on_gpu(surf, W, H)[0]
    pb = surf.DeviceBuffer(48 * n * MAX_PTS)
    db = surf.DeviceBuffer(4 * n * MAX_PTS * 64)
    cb = surf.DeviceBuffer(4 * n)
    det.detect_batch(buf.ptr, n, pitch, H * pitch, pb.ptr, db.ptr, cb.ptr)
    surf.synchronize()
    c = cb.download(np.int32, n)
    assert (c >= 50).all() and (c < MAX_PTS).all(), c
    p = pb.download(surf.POINT_DTYPE, n * MAX_PTS).reshape(n, MAX_PTS)
    d = db.download(np.float32, n * MAX_PTS * 64).reshape(n, MAX_PTS, 64)
    return (c.tobytes(), b"".join(p[f, :c[f]].tobytes() for f in range(n)),
            b"".join(d[f, :c[f]].tobytes() for f in range(n)))


def test_switches_belong_to_the_detector(surf, monkeypatch):
    """Detector A is created with SURFHIP_FIT_CUBE=0, SURFHIP_SORT_BITONIC=1 and
    SURFHIP_TRACE_DESC=0 set, detector B after they are removed.  Each names
    its own switches; the 9-frame batch (past the 8-frame XCD grouping and
    kGatherBatch, two k_hess_w strips) and a 1-frame batch (where the rank and
    the bitonic sort differ) give the same bytes through both; A, run again
    with the three variables set the other way, repeats its first run."""
    for name, value in [kv.split("=") for kv in CONFTEST.split()] + list(THREE.items()):
        monkeypatch.setenv(name, value)
    gp = surf.make_param(4, 4.0, upright=True)
    a = surf.Detector(gp, W, H, max_batch=N, max_pts=MAX_PTS)
    for name in THREE:
        monkeypatch.delenv(name)
    b = surf.Detector(gp, W, H, max_batch=N, max_pts=MAX_PTS)
    a_text = f"{CONFTEST} SURFHIP_TRACE_DESC=0 SURFHIP_SORT_BITONIC=1 SURFHIP_FIT_CUBE=0"
    assert a.switches() == a_text
    assert b.switches() == CONFTEST == surf.switches_from_env()
    first = {n: run(surf, a, n) for n in (N, 1)}
    for n in (N, 1):
        got = run(surf, b, n)
        for what, x, y in zip(("counts", "points", "descriptors"), first[n], got):
            assert x == y, f"{n} frames: {what} of the two detectors differ"
    for name, value in OPPOSITE.items():
        if value is not None:
            monkeypatch.setenv(name, value)
    assert a.switches() == a_text
    assert surf.switches_from_env() == f"{CONFTEST} SURFHIP_TRACE_DESC=1 SURFHIP_FIT_CUBE=1"
    for n in (N, 1):
        assert run(surf, a, n) == first[n], f"{n} frames: detector A changed with the environment"
    a.close()
    b.close()
