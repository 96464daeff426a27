#!/usr/bin/env python3
"""The two measurements of DESIGN.md section 12 (needs the MI355X; prints one JSON line per measurement).

  python tools/metrics_bench.py step [--batch 128] [--steps 20] [--runs 7]
      ms per training step (FEARNetTrainHIP.step, the configuration bench.py times) alone and followed by TrainMetrics.update,
      alternating the two in every run: median and spread of each, and the operator's own time from device events.
  python tools/metrics_bench.py validate [--sequences 32] [--frames 200] [--runs 5]
      wall time of SequenceValidator.run over `sequences` sequences of `frames` 1080p frames — device tensors, and the same
      frames as host arrays — against the same sequences through one FEARTracker loop after the other (host arrays: the frames
      FEARTracker's device crop reads).  Both produce the same IoUs, which is checked.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def bench_step(args) -> None:
    from feartracker_amd.metrics import TrainMetrics
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(31)
    tmpl, srch = torch.randn(B, 3, 128, 128, generator=g).to(dev), torch.randn(B, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(B, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.9).float().to(dev)
    boxes = torch.randint(40, 140, (B, 4), generator=g, dtype=torch.int32).to(dev)
    vis = (torch.rand(B, generator=g) < 0.9).to(torch.int32).to(dev)
    ds = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)
    net = FEARNetTrainHIP(random_init_state(3), device=0)
    metrics = TrainMetrics(0, ["got10k", "lasot", "coco"])

    def window(with_metrics: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
            if with_metrics:
                metrics.update(out, boxes, vis, ds)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    for w in (False, True):                     # warm both shapes of the loop
        window(w)
    plain, with_m = [], []
    for _ in range(args.runs):                  # alternate: the two share whatever else the machine is doing
        plain.append(window(False))
        with_m.append(window(True))
    out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    own = []
    for _ in range(50):
        torch.cuda.synchronize()
        e0.record()
        metrics.update(out, boxes, vis, ds)
        e1.record()
        e1.synchronize()
        own.append(e0.elapsed_time(e1) * 1e3)
    print(json.dumps(dict(measurement="step_metrics", batch=B, steps_per_run=args.steps, step_ms=_spread(plain),
                          step_with_metrics_ms=_spread(with_m),
                          difference_of_medians_ms=round(statistics.median(with_m) - statistics.median(plain), 4),
                          update_alone_us=_spread(own))))


def _clip(n_frames: int, h: int = 1080, w: int = 1920, seed: int = 0):
    """A pool of 1080p frames: seeded texture, a bright 120 x 260 object moving right; and its boxes."""
    rng = np.random.RandomState(seed)
    bg = rng.randint(40, 120, size=(h // 8, w // 8, 3)).astype(np.uint8).repeat(8, axis=0).repeat(8, axis=1)
    frames, boxes = [], []
    for t in range(n_frames):
        f = bg.copy()
        x, y = 300 + 5 * t, 400 + (t % 7)
        f[y:y + 260, x:x + 120] = (220, 60, 150)
        f[y + 20:y + 60, x + 30:x + 90] = (70, 20, 50)
        frames.append(f)
        boxes.append((x, y, 120, 260))
    return frames, np.array(boxes)


def bench_validate(args) -> None:
    from feartracker_amd import DEFAULT_TRACKING_CONFIG, DEFAULT_WEIGHTS, FEARNetHIP, FEARTracker
    from feartracker_amd.metrics import get_iou
    from feartracker_amd.validate import SequenceValidator
    S, T = args.sequences, args.frames
    pool, boxes = _clip(args.pool)
    dev_pool = [torch.from_numpy(f).cuda() for f in pool]
    # sequence s walks the pool back and forth from its own starting frame: T frames each, no two sequences in step
    order = list(range(args.pool)) + list(range(args.pool - 2, 0, -1))
    index = [[order[(3 * s + t) % len(order)] for t in range(T)] for s in range(S)]
    host = [([pool[i] for i in idx], boxes[idx], f"set{s % 3}") for s, idx in enumerate(index)]
    device = [([dev_pool[i] for i in idx], boxes[idx], f"set{s % 3}") for s, idx in enumerate(index)]
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=0, max_batch=64)
    val = SequenceValidator(net, max_samples=T, **DEFAULT_TRACKING_CONFIG)

    def sequential():
        means = []
        for frames, ann, _ in host:
            trk = FEARTracker(net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
            trk.initialize(frames[0], list(map(int, ann[0])))
            ious = [get_iou(np.array(trk.update(frames[i])["bbox"]), np.array(list(map(int, ann[i])))) for i in range(1, T)]
            means.append(np.mean(ious))
        return np.mean(means)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, value

    small = SequenceValidator(net, max_samples=8, **DEFAULT_TRACKING_CONFIG)
    small.run(device[:S])                       # warm up: the S-target plan, the uploads, the pinned buffers
    small.run(host[:S])
    t_dev, t_host, t_seq = [], [], []
    v_dev = v_host = v_seq = None
    for _ in range(args.runs):
        dt, v_dev = timed(lambda: val.run(device)["valid/metrics/box_iou"])
        t_dev.append(dt)
        dt, v_host = timed(lambda: val.run(host)["valid/metrics/box_iou"])
        t_host.append(dt)
        if len(t_seq) < args.baseline_runs:
            dt, v_seq = timed(sequential)
            t_seq.append(dt)
    print(json.dumps(dict(measurement="validation", sequences=S, frames=T, frame="1080p", box_iou=float(v_dev),
                          same_value_on_all_three=bool(v_dev == v_host == v_seq),
                          validator_device_frames_s=_spread(t_dev), validator_host_frames_s=_spread(t_host),
                          sequential_trackers_host_frames_s=_spread(t_seq),
                          speedup_device=round(statistics.median(t_seq) / statistics.median(t_dev), 2),
                          speedup_host=round(statistics.median(t_seq) / statistics.median(t_host), 2))))


def main() -> None:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    s = sub.add_parser("step")
    s.add_argument("--batch", type=int, default=128)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--runs", type=int, default=7)
    v = sub.add_parser("validate")
    v.add_argument("--sequences", type=int, default=32)
    v.add_argument("--frames", type=int, default=200)
    v.add_argument("--runs", type=int, default=5)
    v.add_argument("--baseline-runs", type=int, default=5)
    v.add_argument("--pool", type=int, default=24, help="distinct 1080p frames the sequences are cut from")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py measures on the GPU; none is visible")
    (bench_step if args.what == "step" else bench_validate)(args)


if __name__ == "__main__":
    main()
