#!/usr/bin/env python3
"""Time surfhip_fundamental_batch on one GPU, beside surfhip_homography_batch
on the same matches and the surfhip_match_batch call that feeds both: one
resident batch of synthetic frames is detected and described, consecutive
frames are matched (set 2 = set 1 advanced one frame) and one fundamental
matrix and one homography per pair are estimated, all on the detector's own
buffers.  HIP events via torch on the current stream, warm-up first, the
stages alternating inside every repeat.  Synthetic frames share no content,
so few matches pass the ambiguity filter; the stage is therefore also timed
with the filter wide open (every matched point a candidate), its heaviest
load.  Prints one JSON line with the times in ms (median and range over
--reps); exits non-zero if two calls on the same input gave different bits.

    python tools/fundamental_bench.py [--batch 256] [--width 1920] [--height 1080] [--nhyp 1024] [--reps 7]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256, help="frames (pairs = frames - 1)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--thresh", type=float, default=4.0)
    ap.add_argument("--max-pts", type=int, default=8192, help="keypoint slots per frame")
    ap.add_argument("--nhyp", type=int, default=1024, help="hypotheses per pair, for both estimators")
    ap.add_argument("--max-ambiguity", type=float, default=0.95)
    ap.add_argument("--inlier-thresh", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=7, help="timed repeats of each stage")
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    args = ap.parse_args()
    import torch                      # first: its HIP runtime is the one copy in this process
    surf = load_surf()
    dev = torch.device("cuda", 0)
    surf.set_device(0)
    B, W, H, slots = args.batch, args.width, args.height, args.max_pts
    npairs = B - 1
    pitch = surf.align_up(W, 128)
    frames = surf.synth_frames(B, W, H, pitch)
    d_frames = torch.from_numpy(frames).to(dev)
    param = surf.make_param(4, args.thresh, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    stream = torch.cuda.current_stream(dev).cuda_stream
    det = surf.Detector(param, W, H, max_batch=B, max_pts=slots, stream=stream)
    d_pts = torch.zeros(B * slots * 48, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(B * slots * nf, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_out = torch.zeros(npairs * 64, dtype=torch.uint8, device=dev)
    d_out_all = torch.zeros(npairs * 64, dtype=torch.uint8, device=dev)
    d_out_h = torch.zeros(npairs * 64, dtype=torch.uint8, device=dev)
    d_mask = torch.zeros(npairs * slots, dtype=torch.uint8, device=dev)
    d_mask_all = torch.zeros(npairs * slots, dtype=torch.uint8, device=dev)

    def detect():
        det.detect_batch(d_frames.data_ptr(), B, pitch, H * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                         d_cnt.data_ptr())

    def match():
        surf.match_batch(d_pts.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), slots,
                         d_pts.data_ptr() + 48 * slots, d_desc.data_ptr() + 4 * slots * nf, d_cnt.data_ptr() + 4,
                         slots, npairs, nf, 0, stream)

    def fundamental():
        surf.fundamental_batch(d_pts.data_ptr(), d_cnt.data_ptr(), slots, npairs, d_out.data_ptr(),
                               d_mask.data_ptr(), args.max_ambiguity, args.inlier_thresh, args.nhyp, 0, stream)

    def fundamental_all():            # the heaviest filter setting: every matched point is a candidate
        surf.fundamental_batch(d_pts.data_ptr(), d_cnt.data_ptr(), slots, npairs, d_out_all.data_ptr(),
                               d_mask_all.data_ptr(), 3.0e38, args.inlier_thresh, args.nhyp, 0, stream)

    def homography():
        surf.homography_batch(d_pts.data_ptr(), d_cnt.data_ptr(), slots, npairs, d_out_h.data_ptr(),
                              None, args.max_ambiguity, args.inlier_thresh, args.nhyp, 0, stream)

    stages = (("detect", detect), ("match", match), ("fundamental", fundamental),
              ("fundamental_all_candidates", fundamental_all), ("homography", homography))
    for _ in range(2):                # warm-up: code objects, the detector's first batch
        for _, fn in stages:
            fn()
    torch.cuda.synchronize()
    first = [t.cpu().numpy().copy() for t in (d_out, d_mask, d_out_all, d_mask_all)]
    times = {name: [] for name, _ in stages}
    for _ in range(args.reps):        # the stages alternate inside one run
        for name, fn in stages:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.inner)
    last = [t.cpu().numpy() for t in (d_out, d_mask, d_out_all, d_mask_all)]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(first, last))
    res = last[0].view(surf.FUNDAMENTAL_DTYPE)
    res_all = last[2].view(surf.FUNDAMENTAL_DTYPE)
    res_h = d_out_h.cpu().numpy().view(surf.HOMOGRAPHY_DTYPE)
    counts = d_cnt.cpu().numpy()
    out = {"case": f"{npairs} consecutive pairs of {B} {W}x{H} frames, nhyp {args.nhyp}, "
                   f"ambiguity <= {args.max_ambiguity}, {args.inlier_thresh} px",
           "reps": args.reps, "inner": args.inner, "run_to_run_identical": same,
           "keypoints_mean": round(float(counts.mean()), 1), "keypoints_max": int(counts.max()),
           "ncand_mean": round(float(res["ncand"].mean()), 1), "ncand_max": int(res["ncand"].max()),
           "inliers_mean": round(float(res["ninliers"].mean()), 1),
           "status_counts": [int((res["status"] == s).sum()) for s in (0, 1, 2)],
           "homography_status_counts": [int((res_h["status"] == s).sum()) for s in (0, 1, 2)],
           "all_candidates_ncand_mean": round(float(res_all["ncand"].mean()), 1),
           "all_candidates_status_counts": [int((res_all["status"] == s).sum()) for s in (0, 1, 2)],
           "lds_capacity": surf.FUNDAMENTAL_LDS_CAPACITY}
    for name, t in times.items():
        out[f"{name}_ms"] = round(float(np.median(t)), 4)
        out[f"{name}_ms_range"] = [round(min(t), 4), round(max(t), 4)]
    out["fundamental_over_match"] = round(out["fundamental_ms"] / out["match_ms"], 4)
    out["fundamental_over_homography"] = round(out["fundamental_ms"] / out["homography_ms"], 4)
    print(json.dumps(out), flush=True)
    det.close()
    if not same:
        raise SystemExit("surfhip_fundamental_batch gave different bits on the same input")


if __name__ == "__main__":
    main()
