#!/usr/bin/env python3
"""The measurements of DESIGN.md section 15 (needs the MI355X): writes profiles/visuals_bench.json and prints it as one JSON line.

  python tools/visuals_bench.py [--batch 128] [--steps 20] [--runs 5] [--out profiles/visuals_bench.json]

  step            ms per 128-pair training step (FEARNetTrainHIP.step, the configuration bench.py times), alone
  step + miner    the same step followed by BestWorstMiner.update, in a steady state where nothing is taken (the same score every
                  step); the loop never reads the miner's state
  step + taken    the same with every update taken by one side (min_delta very negative, two alternating scores)
  draw            fear_draw_boxes_u8 for 1, 64 and 256 boxes of 40 to 300 pixels on one 1080p frame, thickness 5, from device events
The three loops alternate within every run, so they share whatever else the machine is doing; medians of `--runs` runs.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


class _Batch:
    pass


def bench_miner(args) -> dict:
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    from feartracker_amd.visuals import BestWorstMiner
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(31)
    batch = _Batch()
    batch.template, batch.search = torch.randn(B, 3, 128, 128, generator=g).to(dev), torch.randn(B, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(B, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.9).float().to(dev)
    batch.search_bbox = torch.randint(40, 140, (B, 4), generator=g, dtype=torch.int32).to(dev)
    vis = (torch.rand(B, generator=g) < 0.9).to(torch.int32).to(dev)
    net = FEARNetTrainHIP(random_init_state(3), device=0)
    steady = BestWorstMiner(0, max_images=16, metric_mode="min", min_delta=1e-4)
    taken = BestWorstMiner(0, max_images=16, metric_mode="min", min_delta=-1e30)
    same = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    alternating = [torch.full((1,), v, dtype=torch.float32, device=dev) for v in (0.25, 0.75)]

    def window(kind: str) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out = net.step(batch.template, batch.search, gt_reg, gt_cls, gt_w)
            if kind == "steady":
                steady.update(out, batch, vis, score=same)
            elif kind == "taken":
                taken.update(out, batch, vis, score=alternating[i & 1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    kinds = ("plain", "steady", "taken")
    for k in kinds:                                 # warm every shape of the loop; the steady miner takes its first step here
        window(k)
    times = {k: [] for k in kinds}
    for _ in range(args.runs):
        for k in kinds:
            times[k].append(window(k))
    assert steady.state()["step"].tolist() == [0, 0], "the steady-state miner took a later step"
    assert taken.state()["take"].sum() >= 1, "the always-taken miner took nothing"
    out = net.step(batch.template, batch.search, gt_reg, gt_cls, gt_w)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    own = {"steady": [], "taken": []}
    for i in range(50):
        for kind, miner, score in (("steady", steady, same), ("taken", taken, alternating[i & 1])):
            torch.cuda.synchronize()
            e0.record()
            miner.update(out, batch, vis, score=score)
            e1.record()
            e1.synchronize()
            own[kind].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(batch=B, steps_per_run=args.steps, max_images=16, step_ms=_spread(times["plain"]),
                step_with_miner_steady_ms=_spread(times["steady"]), step_with_miner_taken_ms=_spread(times["taken"]),
                steady_minus_step_ms=round(med["steady"] - med["plain"], 4), taken_minus_step_ms=round(med["taken"] - med["plain"], 4),
                update_alone_steady_us=_spread(own["steady"]), update_alone_taken_us=_spread(own["taken"]))


def bench_draw(args) -> dict:
    from feartracker_amd.visuals import draw_boxes
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(7)
    frame = torch.from_numpy(rng.randint(0, 256, size=(1080, 1920, 3)).astype(np.uint8)).to(dev)
    out = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for K in (1, 64, 256):
        wh = rng.randint(40, 301, size=(K, 2))
        xy = np.stack([rng.randint(0, 1920 - wh[:, 0]), rng.randint(0, 1080 - wh[:, 1])], axis=1)
        boxes = torch.from_numpy(np.concatenate([xy, wh], axis=1).astype(np.int32)).to(dev)
        frame_of = torch.zeros(K, dtype=torch.int32, device=dev)
        cols = torch.from_numpy(rng.randint(0, 256, size=(K, 3)).astype(np.uint8)).to(dev)
        for _ in range(10):
            draw_boxes(frame, boxes, frame_of, cols, 5)
        us = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(100):
                draw_boxes(frame, boxes, frame_of, cols, 5)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / 100)
        out[f"draw_{K}_boxes_us"] = _spread(us)
    return dict(frame="1080p", thickness=5, box_sides="40..300", calls_per_run=100, **out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visuals_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/visuals_bench.py measures on the GPU; none is visible")
    result = dict(measurement="visuals", device=torch.cuda.get_device_name(0), miner=bench_miner(args), draw=bench_draw(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
