#!/usr/bin/env python3
"""Time the per-frame keypoint budget (Detector.set_keep) on one GPU, on the bench configuration: one
resident batch of synthetic frames (256 x 1920x1080, 4 octaves, 64-D upright, thresh 4, max_pts 65536)
is detected and described keeping every keypoint and under KEEP_STRONGEST at n = 2048, 512 and 128.
Per setting: the pipelined step as bench.py runs it (detect_batch_next, the next batch's integral beside
describe) and the `sort` and `describe` stage times of a profiled serial call (the selection kernel runs
in the sort stage).  HIP events via torch on the current stream, warm-up first, the settings alternating
inside every repeat.  Every frame's count must equal min(candidates, n).  Prints one JSON line with the
times in ms (median and range over --reps).

    python tools/keep_bench.py [--batch 256] [--width 1920] [--height 1080] [--reps 7]
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--thresh", type=float, default=4.0)
    ap.add_argument("--max-pts", type=int, default=65536, help="keypoint slots per frame")
    ap.add_argument("--budgets", type=int, nargs="+", default=[2048, 512, 128], help="KEEP_STRONGEST budgets")
    ap.add_argument("--reps", type=int, default=7, help="timed repeats of each setting")
    ap.add_argument("--inner", type=int, default=4, help="steps per timed window")
    args = ap.parse_args()
    import torch                      # first: its HIP runtime is the one copy in this process
    surf = load_surf()
    dev = torch.device("cuda", 0)
    surf.set_device(0)
    B, W, H, slots = args.batch, args.width, args.height, args.max_pts
    pitch = surf.align_up(W, 128)
    frames = surf.synth_frames(B, W, H, pitch)
    d_frames = torch.from_numpy(frames).to(dev)
    param = surf.make_param(4, args.thresh, False, 9, 2, True, False, 4)
    nf = param.nfeatures
    stream = torch.cuda.current_stream(dev).cuda_stream
    det = surf.Detector(param, W, H, max_batch=B, max_pts=slots, stream=stream)
    d_pts = torch.empty(B * slots * 48, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(B * slots * nf, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    settings = [("keep_all", surf.KEEP_FIRST, 0)] + [(f"strongest_{n}", surf.KEEP_STRONGEST, n) for n in args.budgets]

    def step():                       # bench.py's step: the next batch (the same frames) prefetched
        det.detect_batch_next(d_frames.data_ptr(), B, pitch, H * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                              d_cnt.data_ptr(), d_frames.data_ptr(), B, pitch, H * pitch)

    def serial():
        det.detect_batch(d_frames.data_ptr(), B, pitch, H * pitch, d_pts.data_ptr(), d_desc.data_ptr(),
                         d_cnt.data_ptr())

    def check(name, n):
        torch.cuda.synchronize()
        counts, cand = d_cnt.cpu().numpy(), det.candidates(B)
        want = np.minimum(cand, n if n else slots)
        if det.truncated() or (counts != want).any():
            raise SystemExit(f"{name}: counts differ from min(candidates, n) in {int((counts != want).sum())} frames")
        return counts, cand

    for name, mode, n in settings:    # warm-up: code objects, the detector's first batches
        det.set_keep(mode, n)
        step()
        step()
        check(name, n)
    times = {name: {"step": [], "sort": [], "describe": []} for name, _, _ in settings}
    kept = {}
    for _ in range(args.reps):        # the settings alternate inside one run
        for name, mode, n in settings:
            det.set_keep(mode, n)
            step()                    # the pipeline's first step of a setting is not timed
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[name]["step"].append(e0.elapsed_time(e1) / args.inner)
            det.set_profiling(True)
            serial()
            st = det.stage_times()
            det.set_profiling(False)
            times[name]["sort"].append(st["sort"])
            times[name]["describe"].append(st["describe"])
            counts, cand = check(name, n)
            kept[name] = (round(float(counts.mean()), 1), round(float(cand.mean()), 1))
    out = {"case": f"{B} {W}x{H} frames, 4 octaves, 64-D upright, thresh {args.thresh:g}, max_pts {slots}",
           "reps": args.reps, "inner": args.inner, "candidates_mean": kept["keep_all"][1]}
    for name, t in times.items():
        row = {"keypoints_mean": kept[name][0]}
        for k, v in t.items():
            row[f"{k}_ms"] = round(float(np.median(v)), 4)
            row[f"{k}_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        out[name] = row
    base = out["keep_all"]
    for name, _, _ in settings[1:]:
        row = out[name]
        row["step_saved_ms"] = round(base["step_ms"] - row["step_ms"], 4)
        row["sort_added_ms"] = round(row["sort_ms"] - base["sort_ms"], 4)
        row["describe_saved_ms"] = round(base["describe_ms"] - row["describe_ms"], 4)
    print(json.dumps(out), flush=True)
    det.close()


if __name__ == "__main__":
    main()
