#!/usr/bin/env python3
"""Cost of the training-pair builder (feartracker_amd/train_data.py) on one GPU.

Reports, for 128 pairs out of 1080p device frames (two frames of their own per pair: 256 distinct frames, the most the frame means
can cost):
  device_ms          fear_frame_border_u8 + fear_train_pairs, HIP events over `--iters` back-to-back calls
  host_ms            TrainPairBuilder.draw + .tables (the per-pair host work and the FearPairGeom / lookup-table records), median
  step_ms            FEARNetTrainHIP.step on fixed inputs, wall time per step over `--steps` steps
  step_with_build_ms builder.build + step per iteration, the same way
Prints one JSON object; with --out also writes it there.

Usage: python tools/train_pairs_bench.py [--pairs 128] [--frames 256] [--steps 20] [--iters 50] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from feartracker_amd.train_data import FRAME_DTYPE, TrainPairBuilder
    from feartracker_amd.train_head import load_train_library
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state

    dev = torch.device("cuda", 0)
    B, F = args.pairs, args.frames
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(0, 256, (1080, 1920, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(F)]
    rng = np.random.default_rng(0)
    pairs = np.zeros((B, 11))
    w, h = rng.integers(40, 400, B), rng.integers(40, 400, B)
    pairs[:, 0], pairs[:, 5] = (2 * np.arange(B)) % F, (2 * np.arange(B) + 1) % F
    pairs[:, 1], pairs[:, 2], pairs[:, 3], pairs[:, 4] = rng.integers(0, 1920 - w), rng.integers(0, 1080 - h), w, h
    w2, h2 = rng.integers(40, 400, B), rng.integers(40, 400, B)
    pairs[:, 6], pairs[:, 7], pairs[:, 8], pairs[:, 9] = rng.integers(0, 1920 - w2), rng.integers(0, 1080 - h2), w2, h2
    pairs[:, 10] = 1
    shapes = [tuple(f.shape) for f in frames]
    builder = TrainPairBuilder(device=0, seed=0)

    # ---- host: draw + tables
    times = []
    for _ in range(50):
        t0 = time.perf_counter()
        params = builder.draw(pairs, shapes)
        tab = builder.tables(pairs, params)
        times.append(time.perf_counter() - t0)
    host_ms = 1e3 * float(np.median(times))

    # ---- device: the two kernels on staged tables
    lib = load_train_library()
    ftab = np.zeros(F, dtype=FRAME_DTYPE)
    for i, f in enumerate(frames):
        ftab[i] = (f.data_ptr(), 1080, 1920)
    d_ftab = torch.from_numpy(ftab.view(np.uint8).copy()).to(dev)
    d_geom = torch.from_numpy(tab["geom"].view(np.uint8).copy()).to(dev)
    d_lut = torch.from_numpy(tab["lut"].copy()).to(dev)
    border = torch.empty((F, 3), dtype=torch.uint8, device=dev)
    outs = [torch.empty(s, device=dev) for s in ((B, 3, 128, 128), (B, 3, 256, 256), (B, 4, 16, 16), (B, 1, 16, 16), (B, 16, 16))]
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)

    def kernels(which=3):
        if which & 1:
            assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), F, P(border.data_ptr()), st) == 0
        if which & 2:
            assert lib.fear_train_pairs(P(d_ftab.data_ptr()), F, P(border.data_ptr()), P(d_geom.data_ptr()), P(d_lut.data_ptr()), B,
                                        *[P(o.data_ptr()) for o in outs], st) == 0

    res = {}
    for name, which in (("device_ms", 3), ("border_ms", 1), ("pairs_ms", 2)):
        for _ in range(5):
            kernels(which)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            kernels(which)
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / args.iters

    # ---- the step without and with the builder in the loop
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    batch = builder.build(frames, pairs)
    fixed = [t.clone() for t in batch[:5]]

    def run(with_build):
        for _ in range(3):
            b = builder.build(frames, pairs) if with_build else fixed
            net.step(*b[:5])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            b = builder.build(frames, pairs) if with_build else fixed
            out = net.step(*b[:5])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, out

    step_ms, _ = run(False)
    step_build_ms, out = run(True)
    step_ms_2, _ = run(False)                      # the plain step again: the spread between the two plain runs is the noise
    loss = (float(out["loss_cls"]), float(out["loss_reg"]))
    report = {
        "pairs": B, "frames": F, "frame_hw": [1080, 1920],
        "device_ms": round(res["device_ms"], 4), "border_ms": round(res["border_ms"], 4), "pairs_ms": round(res["pairs_ms"], 4),
        "host_ms": round(host_ms, 4),
        "step_ms": round(min(step_ms, step_ms_2), 3), "step_ms_runs": [round(step_ms, 3), round(step_ms_2, 3)],
        "step_with_build_ms": round(step_build_ms, 3),
        "build_overhead_pct": round(100.0 * (step_build_ms - min(step_ms, step_ms_2)) / min(step_ms, step_ms_2), 2),
        "device_pct_of_step": round(100.0 * res["device_ms"] / min(step_ms, step_ms_2), 2),
        "losses_finite": bool(np.all(np.isfinite(loss))),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(report)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
