"""bench.py's host logic on the CPU (no GPU calls): the rank launcher's
argument checks and failure propagation, the config labels and the CPU
baseline's core accounting."""
from __future__ import annotations

import importlib.util
import os
import subprocess
import sys
import time

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(kw)
    return env


def test_world_size_mismatch_fails():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--batch", "1", "--steps", "1"],
                       capture_output=True, text=True, timeout=120, cwd=REPO,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and "disagrees" in r.stderr


def test_spawned_rank_failure_ends_the_job():
    """Without a GPU every spawned rank refuses the RCCL exchange (one GPU per
    rank); the launcher must return that failure, not hang or print a line."""
    t0 = time.time()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--batch", "1", "--steps", "1", "--no-cpu"],
                       capture_output=True, text=True, timeout=240, cwd=REPO, env=_env())
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "one GPU per rank" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert time.time() - t0 < 200


def test_full_only_options_need_full():
    """--exchange-proxy is a --full measurement and --dump-outputs has nothing
    to write in a --hessian-only run: both are refused before any GPU work."""
    for extra, word in ((["--exchange-proxy", "8"], "--full"), (["--hessian-only", "--dump-outputs", "x"], "--hessian-only")):
        r = subprocess.run([sys.executable, BENCH, "--batch", "1", "--steps", "1"] + extra,
                           capture_output=True, text=True, timeout=120, cwd=REPO, env=_env())
        assert r.returncode == 2 and word in r.stderr, (extra, r.returncode, r.stderr[-500:])


def test_dump_outputs_layout(tmp_path):
    """dump_outputs on host tensors laid out like detect_batch's buffers: every
    frame's count, a seeded sample of frames, and exactly their first
    `count` SurfPoints and descriptors, float32 / float64, within 64 MB."""
    import numpy as np
    import pytest
    torch = pytest.importorskip("torch")
    from conftest import load_surf_amd
    surf = load_surf_amd()
    b = _bench()
    B, max_pts, nf = 5, 7, 4
    rng = np.random.default_rng(3)
    counts = np.array([3, 0, 7, 1, 5], np.int32)
    pts = np.zeros((B, max_pts), surf.POINT_DTYPE)
    for k in b.DUMP_FIELDS:
        pts[k] = rng.integers(-50, 50, (B, max_pts)).astype(pts[k].dtype)
    desc = rng.standard_normal((B, max_pts, nf)).astype(np.float32)
    d_pts = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy())
    d_desc = torch.from_numpy(desc.reshape(-1).copy())

    def dump(name):
        out = tmp_path / name
        b.dump_outputs(str(out), surf, d_pts, d_desc, counts, max_pts, nf, 0, 1)
        return {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}

    d = dump("a")
    assert sorted(d) == ["counts", "descriptors", "points", "sample_frames"]
    assert d["counts"].dtype == np.float64 and d["sample_frames"].dtype == np.float64
    assert d["points"].dtype == np.float32 and d["descriptors"].dtype == np.float32
    assert np.array_equal(d["counts"], counts)
    picked = d["sample_frames"].astype(int)
    assert sorted(picked) == list(range(B))                   # the budget holds this whole batch
    want_p = np.concatenate([np.stack([pts[f, :counts[f]][k].astype(np.float32) for k in b.DUMP_FIELDS], 1)
                             for f in picked])
    want_d = np.concatenate([desc[f, :counts[f]] for f in picked])
    assert np.array_equal(d["points"], want_p) and np.array_equal(d["descriptors"], want_d)
    again = dump("b")
    assert all(np.array_equal(d[k], again[k]) for k in d)      # the sample is fixed
    assert sum(a.nbytes for a in d.values()) <= 64 << 20


def test_dump_outputs_budget(tmp_path, monkeypatch):
    """A batch beyond the byte budget is cut: frames in the seeded order until
    the rows run out, the last one truncated at the budget."""
    import numpy as np
    import pytest
    torch = pytest.importorskip("torch")
    from conftest import load_surf_amd
    surf = load_surf_amd()
    b = _bench()
    B, max_pts, nf = 6, 10, 2
    row = 4 * (len(b.DUMP_FIELDS) + nf)
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 25 * row)
    counts = np.full(B, 10, np.int32)
    d_pts = torch.zeros(B * max_pts * 48, dtype=torch.uint8)
    d_desc = torch.arange(B * max_pts * nf, dtype=torch.float32)
    b.dump_outputs(str(tmp_path), surf, d_pts, d_desc, counts, max_pts, nf, 0, 1)
    picked = np.load(tmp_path / "sample_frames.npy").astype(int)
    desc = np.load(tmp_path / "descriptors.npy")
    assert len(picked) == 3 and len(desc) == 25 and len(np.load(tmp_path / "points.npy")) == 25
    full = d_desc.numpy().reshape(B, max_pts, nf)
    assert np.array_equal(desc, np.concatenate([full[picked[0]], full[picked[1]], full[picked[2], :5]]))


def test_config_labels():
    b = _bench()

    class A:
        width, height, octaves, upright, extend, batch = 1920, 1080, 4, 1, 0, 256
    assert b.config_name(A, 1) == "config#3"
    assert b.config_name(A, 8) == "config#4"
    A.batch = 1
    assert b.config_name(A, 1) == "config#2"
    A.width, A.height, A.octaves, A.upright, A.extend, A.batch = 3840, 2160, 5, 0, 1, 64
    assert b.config_name(A, 8) == "config#5"
    assert b.config_name(A, 1).startswith("config#5 per-rank")
    A.octaves = 4
    assert b.config_name(A, 1) == "custom"


def test_cpu_share_reports_host():
    b = _bench()
    share, host = b.cpu_share()
    assert 1 <= share <= host["host_cpus"]
    assert share <= host["affinity_cpus"]
    assert host["cpu_model"]


def test_committed_hessian_profiles_consistent():
    """profiles/hessian_profile.json (bench.py's frac_profile / bound source,
    written by tools/hessian_profile.py) holds one entry per single-GPU config
    whose stage time is the sum of its kernels' rocprof averages, a bound
    the rule allows, and utilisations that justify it; bench.py finds the
    entry for its config only when the kernel names match."""
    import json
    b = _bench()
    d = json.load(open(os.path.join(REPO, "profiles", "hessian_profile.json")))
    assert {"256x1920x1080x4u", "1x1920x1080x4u", "64x3840x2160x5rx"} <= set(d)
    for key, e in d.items():
        assert abs(e["stage_ms"] - sum(e["kernels_avg_ns"].values()) * 1e-6) < 1e-9, key
        ev = e["bound_evidence"]
        units = {"hbm": ev.get("hbm_util", 0), "valu-issue": ev.get("valu_util", 0), "lds": ev.get("lds_util", 0)}
        top = max(units, key=units.get)
        assert e["bound"] == (top if units[top] >= 0.6 else "latency"), key
        assert os.path.exists(os.path.join(REPO, "profiles", f"{e['tag']}_kernel_stats.csv")), key

    class A:
        width, height, octaves, upright, extend, batch = 1920, 1080, 4, 1, 0, 256
    e = b.hessian_profile(A, "k_hess_p0 (octave 0) + k_hess_w (octaves 1-3)")
    assert e is not None and set(e["kernels_avg_ns"]) == {"k_hess_p0", "k_hess_w"}
    assert b.hessian_profile(A, "k_hess_q0 (octave 0) + k_hess_w (octaves 1-3)") is None
    A.batch = 1
    e = b.hessian_profile(A, "k_hessian_t0 (octave 0) + k_hessian (octaves 1-3)")
    assert e is not None and set(e["kernels_avg_ns"]) == {"k_hessian_t0", "k_hessian"}
