#!/usr/bin/env python3
"""Time surfhip_match (Surfor::match) on one GPU: n x n points, nf-D
descriptors, caller-provided scratch, HIP events via torch on the null
stream.  Prints one JSON line per case.

    python tools/match_bench.py [--n 3000] [--iters 50]

--batch NPAIRS instead times NPAIRS pairs of n x n points (flags 0, nf 64
then 128) two ways on the same data, alternating in one run: a loop of NPAIRS
surfhip_match calls with caller scratch, and one surfhip_match_batch call.
It checks that both write the same bits and prints, per nf, one JSON line
with both times in ms (median and range over --reps), their ratio and the
batch call's fp32 TFLOP/s.

    python tools/match_bench.py --batch 255 [--n 3000] [--reps 7]

--batch NPAIRS --cross times one surfhip_match_batch call against one
surfhip_match_batch_cross call (the same match with the mutual-best test) on
the same data, alternating in one run, and prints both medians with their
ranges and the ratio cross / batch.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_surf():
    pkg = os.path.join(REPO, "cuda-surf_amd")
    spec = importlib.util.spec_from_file_location("surf_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["surf_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def bench_batch(surf, torch, npairs, n, reps, inner):
    for nf in (64, 128):
        torch.manual_seed(nf)
        ft = torch.randn((2, npairs, n, nf), device="cuda")
        ft /= ft.norm(dim=3, keepdim=True)
        pts = torch.zeros((2, npairs, n, 48), dtype=torch.uint8, device="cuda")
        pts_b = torch.zeros((npairs, n, 48), dtype=torch.uint8, device="cuda")
        counts = torch.full((2, npairs), n, dtype=torch.int32, device="cuda")
        scratch = torch.empty(max(surf.match_scratch_bytes(n, n, 0), 4), dtype=torch.uint8, device="cuda")

        def loop():
            for i in range(npairs):
                surf.match_points(pts[0, i].data_ptr(), pts[1, i].data_ptr(), ft[0, i].data_ptr(),
                                  ft[1, i].data_ptr(), n, n, nf, 0, scratch.data_ptr())

        def batch():
            surf.match_batch(pts_b.data_ptr(), ft[0].data_ptr(), counts[0].data_ptr(), n, pts[1].data_ptr(),
                             ft[1].data_ptr(), counts[1].data_ptr(), n, npairs, nf, 0)

        loop()
        batch()
        torch.cuda.synchronize()
        same = bool(torch.equal(pts[0], pts_b))
        t_loop, t_batch = [], []
        for _ in range(reps):                       # alternate the two in the same run
            for fn, k, out in ((loop, 1, t_loop), (batch, inner, t_batch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / k)
        lm, bm = float(np.median(t_loop)), float(np.median(t_batch))
        fma = npairs * n * (32 * (n // 32)) * nf
        print(json.dumps({"case": f"match {npairs} pairs of {n}x{n} nf={nf} flags=0",
                          "loop_ms": round(lm, 4), "loop_ms_range": [round(min(t_loop), 4), round(max(t_loop), 4)],
                          "batch_ms": round(bm, 4),
                          "batch_ms_range": [round(min(t_batch), 4), round(max(t_batch), 4)],
                          "ratio": round(lm / bm, 3), "batch_fp32_tflops": round(2 * fma / bm / 1e9, 2),
                          "loop_fp32_tflops": round(2 * fma / lm / 1e9, 2), "reps": reps,
                          "bit_identical": same}), flush=True)
        if not same:
            raise SystemExit("surfhip_match_batch and the surfhip_match loop disagree")
        del ft, pts, pts_b, scratch


def bench_cross(surf, torch, npairs, n, reps, inner):
    """surfhip_match_batch against surfhip_match_batch_cross on the same
    data, alternating in one run.  The cost of composing the mutual test by
    hand is two match_batch calls (before the caller's own filter kernel and
    slab copy), so cross_over_batch below 2 is the library doing better."""
    for nf in (64, 128):
        torch.manual_seed(nf)
        ft = torch.randn((2, npairs, n, nf), device="cuda")
        ft /= ft.norm(dim=3, keepdim=True)
        pts = torch.zeros((2, npairs, n, 48), dtype=torch.uint8, device="cuda")
        pts_c = torch.zeros((npairs, n, 48), dtype=torch.uint8, device="cuda")
        counts = torch.full((2, npairs), n, dtype=torch.int32, device="cuda")
        nbytes = surf.match_batch_cross_scratch_bytes(npairs, n, n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        tail = (counts[0].data_ptr(), n, pts[1].data_ptr(), ft[1].data_ptr(), counts[1].data_ptr(), n, npairs, nf)

        def batch():
            surf.match_batch(pts[0].data_ptr(), ft[0].data_ptr(), *tail, 0)

        def cross():
            surf.match_batch_cross(pts_c.data_ptr(), ft[0].data_ptr(), *tail, scratch.data_ptr(), 0)

        batch()
        cross()
        torch.cuda.synchronize()
        a = pts[0].cpu().numpy().reshape(-1).view(surf.POINT_DTYPE)
        c = pts_c.cpu().numpy().reshape(-1).view(surf.POINT_DTYPE)
        kept = c["match"] >= 0
        ok = bool((a["score"] == c["score"]).all() and (a["ambiguity"] == c["ambiguity"]).all()
                  and (a["match"][kept] == c["match"][kept]).all())
        partners = c["match"].reshape(npairs, n)
        injective = all(len(np.unique(r[r >= 0])) == int((r >= 0).sum()) for r in partners)
        t_batch, t_cross = [], []
        for _ in range(reps):                       # alternate the two in the same run
            for fn, out in ((batch, t_batch), (cross, t_cross)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / inner)
        bm, cm = float(np.median(t_batch)), float(np.median(t_cross))
        nscan = 32 * (n // 32)
        atomic_bytes = 8 * npairs * nscan * ((n + 127) // 128)     # one key per (128-point block, scanned p2)
        print(json.dumps({"case": f"cross match {npairs} pairs of {n}x{n} nf={nf} flags=0",
                          "batch_ms": round(bm, 4),
                          "batch_ms_range": [round(min(t_batch), 4), round(max(t_batch), 4)],
                          "cross_ms": round(cm, 4),
                          "cross_ms_range": [round(min(t_cross), 4), round(max(t_cross), 4)],
                          "cross_over_batch": round(cm / bm, 3), "reps": reps,
                          "forward_matches": int((a["match"] >= 0).sum()), "kept": int(kept.sum()),
                          "atomic_mbytes": round(atomic_bytes / 1e6, 2), "scratch_mbytes": round(nbytes / 1e6, 2),
                          "consistent": ok and injective}), flush=True)
        if not (ok and injective):
            raise SystemExit("surfhip_match_batch_cross disagrees with surfhip_match_batch")
        del ft, pts, pts_c, scratch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=0, metavar="NPAIRS",
                    help="time NPAIRS surfhip_match calls against one surfhip_match_batch call")
    ap.add_argument("--reps", type=int, default=7, help="--batch: timed repeats of each side")
    ap.add_argument("--inner", type=int, default=4, help="--batch: batch calls per timed window")
    ap.add_argument("--cross", action="store_true",
                    help="--batch: time surfhip_match_batch against surfhip_match_batch_cross instead")
    args = ap.parse_args()
    import torch
    surf = load_surf()
    if args.batch > 0 and args.cross:
        bench_cross(surf, torch, args.batch, args.n, args.reps, args.inner)
        return
    if args.batch > 0:
        bench_batch(surf, torch, args.batch, args.n, args.reps, args.inner)
        return
    for nf in (64, 128):
        for flags in (0, 1):
            n = args.n
            rng = np.random.default_rng(nf)
            f = rng.standard_normal((2, n, nf)).astype(np.float32)
            f /= np.linalg.norm(f, axis=2, keepdims=True)
            ft = torch.from_numpy(f).cuda()
            pts = torch.zeros((2, n, 48), dtype=torch.uint8, device="cuda")
            scratch = torch.empty(max(surf.match_scratch_bytes(n, n, flags), 4), dtype=torch.uint8, device="cuda")
            args_ = (pts[0].data_ptr(), pts[1].data_ptr(), ft[0].data_ptr(), ft[1].data_ptr(), n, n, nf, flags,
                     scratch.data_ptr())
            for _ in range(3):
                surf.match_points(*args_)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                surf.match_points(*args_)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            fma = n * (n if flags else 32 * (n // 32)) * nf
            print(json.dumps({"case": f"match {n}x{n} nf={nf} full_tail={flags}", "ms": round(ms, 4),
                              "pairs_per_s": round(n * n / ms * 1e3, 1),
                              "fp32_tflops": round(2 * fma / ms / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
