"""Measure FEARMultiTracker against K FEARTrackers and against fear_track alone, on 1080p frames.

Frames: the demo-geometry clip (tests/clipgen.demo_clip) tiled to 1920 x 1080, as bench.py's latency_batch1 builds them.
Targets: K boxes spread over the frame on a deterministic lattice, the first ones on the four frame edges and corners.
For each K it reports ms per frame and target-updates/s of
  update      FEARMultiTracker.update per frame (submit + wait)
  submit      a pipelined loop: frame t + 1 submitted before frame t's result is read
  singles     K independent FEARTrackers, one update each per frame (K <= 64 only)
  track_only  fear_track of the same K search crops and templates, back to back: the floor the tracker is measured against
Usage: python tools/multi_track_bench.py [--ks 1,16,64,256,1024] [--frames 40] [--out profiles/....json] [--no-singles]
       [--submit-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from clipgen import demo_clip  # noqa: E402
from feartracker_amd import DEFAULT_TRACKING_CONFIG, DEFAULT_WEIGHTS, FEARMultiTracker, FEARNetHIP, FEARTracker  # noqa: E402


def hd_frames(n):
    frames, _ = demo_clip(min(n, 220))
    reps = (-(-1080 // frames.shape[1]), -(-1920 // frames.shape[2]))
    return np.ascontiguousarray(np.tile(frames, (1, reps[0], reps[1], 1))[:, :1080, :1920])


def target_boxes(k, h=1080, w=1920):
    edges = [(-10, 400, 60, 80), (w - 40, 500, 70, 90), (800, -15, 50, 60), (900, h - 30, 60, 70), (-5, -5, 40, 40),
             (w - 30, h - 30, 50, 50)]
    out = []
    for j in range(k):
        if j < len(edges):
            out.append(edges[j])
            continue
        bw, bh = 30 + (j * 7) % 90, 40 + (j * 11) % 120
        out.append(((j * 97) % (w - bw), (j * 53) % (h - bh), bw, bh))
    return np.array(out)


def timed(fn, n, sync):
    sync()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    sync()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,64,256,1024")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--no-singles", action="store_true")
    ap.add_argument("--submit-only", action="store_true", help="time only the pipelined submit loop (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sync = torch.cuda.synchronize
    frames = hd_frames(args.frames + 4)
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=0, max_batch=args.max_batch)
    cfg = DEFAULT_TRACKING_CONFIG
    res = {"frame_shape": list(frames[0].shape), "frames_timed": args.frames, "max_batch": args.max_batch,
           "device": torch.cuda.get_device_name(0), "per_k": []}
    for k in (int(v) for v in args.ks.split(",")):
        boxes = target_boxes(k)
        row = {"k": k}
        if not args.submit_only:
            mt = FEARMultiTracker(net, cuda_id=0, **cfg)
            mt.add(frames[0], boxes)
            for f in frames[1:4]:
                mt.update(f)
            row["update_ms"] = timed(lambda i: mt.update(frames[4 + i]), args.frames, sync)
        mt = FEARMultiTracker(net, cuda_id=0, **cfg)
        mt.add(frames[0], boxes)
        for f in frames[1:4]:
            mt.update(f)
        state = {"p": None}

        def pipelined(i):
            nxt = mt.submit(frames[4 + i])
            if state["p"] is not None:
                state["p"].result()
            state["p"] = nxt

        row["submit_ms"] = timed(pipelined, args.frames, sync)
        state["p"].result()
        if args.submit_only:
            res["per_k"].append(row)
            print(json.dumps(row), flush=True)
            continue
        if k <= 64 and not args.no_singles:
            trks = []
            for b in boxes:
                t = FEARTracker(net, cuda_id=0, **cfg)
                t.initialize(frames[0], b.copy())
                trks.append(t)
            for f in frames[1:4]:
                for t in trks:
                    t.update(f)
            row["singles_ms"] = timed(lambda i: [t.update(frames[4 + i]) for t in trks], args.frames, sync)
        search = torch.randn(k, 3, 256, 256, device="cuda")
        z = net.get_features(torch.randn(k, 3, 128, 128, device="cuda"))
        for _ in range(3):
            net.track_maps(search, z)
        row["track_only_ms"] = timed(lambda i: net.track_maps(search, z), args.frames, sync)
        for key in ("update", "submit", "singles"):
            if f"{key}_ms" in row:
                row[f"{key}_targets_per_s"] = 1e3 * k / row[f"{key}_ms"]
        row["submit_over_track"] = row["submit_ms"] / row["track_only_ms"]
        res["per_k"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
