#!/usr/bin/env python3
"""Cost of the training-pair builder (feartracker_amd/train_data/) on one GPU.

Reports, for 128 pairs out of 1080p device frames (two frames of their own per pair: 256 distinct frames, the most the frame means
can cost):
  device_ms          fear_frame_border_u8 + fear_train_pairs, HIP events over `--iters` back-to-back calls
  host_ms            TrainPairBuilder.draw + .tables (the per-pair host work and the FearPairGeom / lookup-table records), median
  step_ms            FEARNetTrainHIP.step on fixed inputs, wall time per step over `--steps` steps
  step_with_build_ms builder.build + step per iteration, the same way
Prints one JSON object; with --out also writes it there.

With --photometric it reports the photometric stage instead (same pairs and frames):
  build_off_ms       TrainPairBuilder.build with the stage off, wall time per call (synchronised at the end of `--iters` calls), one
                     figure per fresh process (`--repeats`); with --parent-root DIR the same for the checkout at DIR, the processes
                     of the two trees taking turns, so that both see the same box in the same minutes
  build_on_ms        the same with photometric=True at the reference's probabilities, fresh draws per call
  median7_ms         fear_photometric_u8 alone on the batch's 128 templates and 128 searches (two calls), every crop forced to the
                     7 x 7 median, HIP events
  step_ms            FEARNetTrainHIP.step on fixed inputs, for the shares
With --colour all it reports the colour members behind `colour_members` (same pairs and frames):
  build_default_ms   `build` with the default members, one figure per fresh process; with --parent-root DIR against that checkout's
                     `build` in alternating processes, as above: the same code path, so a difference beyond the spread is a finding
  build_all_ms       `build` with colour_members="all" at the reference's probabilities, fresh draws per call
  colour_u8_ms       fear_colour_u8 alone on the batch's 128 templates and 128 searches (two calls), every crop forced to one member,
                     per member, HIP events; worst_member names the slowest
  step_ms            FEARNetTrainHIP.step on fixed inputs, for the shares
With --noise all it reports ImageCompression, the member behind `noise_members` (same pairs and frames, the photometric stage on):
  build_default_ms   `build` with photometric=True and the default members, one figure per fresh process; with --parent-root DIR against
                     that checkout's `build` in alternating processes, as above: the same launches, so a difference beyond the spread
                     is a finding
  build_all_ms       `build` with noise_members="all" at the reference's probabilities, fresh draws per call
  jpeg_u8_ms         fear_jpeg_u8 alone on the batch's 128 templates and 128 searches (two calls), every crop at quality 50, HIP events
  step_ms            FEARNetTrainHIP.step on fixed inputs, for the shares
With --iso and / or --weather all it reports ISONoise and the weather group, the members behind `iso_noise` and `weather_members` (same
pairs and frames, the photometric stage on), in ONE run on one commit:
  build_default_ms   `build` with photometric=True alone, one figure per fresh process
  build_on_ms        `build` with the keys on at the reference's probabilities, fresh draws per call, the processes of the two arms
                     taking turns.  The figure to report is this one against build_default_ms; no target is set
  hls_u8_ms          fear_hls_u8 alone on the batch's 128 templates and 128 searches (two calls), every crop forced to one member, per
                     member (ISONoise, rain with its H W // 600 drops, a shadow of two polygons), HIP events
  step_ms            FEARNetTrainHIP.step on fixed inputs, for the shares
With --glass it reports GlassBlur, the member behind `glass_blur` (same pairs and frames, the photometric stage on):
  build_default_ms   `build` with photometric=True and the default members, one figure per fresh process; with --parent-root DIR against
                     that checkout's `build` in alternating processes, as above: the same launches, so a difference beyond the spread
                     is a finding
  build_on_ms        `build` with glass_blur=True at the reference's probabilities, fresh draws per call
  glass_u8_ms        fear_glass_u8 alone on the batch's 128 templates and 128 searches (two calls), every crop forced to the member, HIP
                     events
  step_ms            FEARNetTrainHIP.step on fixed inputs, for the shares
With --store DIR it reports the resident JPEG store in front of the builder (DIR holds the files of tools/jpeg_decode_bench.py --make,
256 synthetic 1280 x 720 files; 128 pairs, two frames of their own per pair), in ONE run, medians of `--repeats` + 2 runs with minimum and
maximum, a host clock around work that ends in a synchronise:
  decode_build_ms        store.decode(ids) + builder.build(frames, pairs, params)
  rows_build_ms          store.decode_rows(ids, builder.frame_rows(...)) + builder.build(frames, pairs, params, borders=store.borders(ids))
  decode_ms, decode_rows_ms, build_ms, build_borders_ms     the parts alone
  boxes                  the seeded boxes: sides uniform in [lo, hi) pixels; rows_per_frame is the mean of what frame_rows asks for
The two builds are compared with torch.equal before anything is timed (`batches_equal`).  It sets no gate: the gain depends on the boxes.
--build-only is the child mode of the above: it times `build` of the package under --root and prints {"build_ms": ...}.

Usage: python tools/train_pairs_bench.py [--pairs 128] [--frames 256] [--steps 20] [--iters 50] [--out FILE]
       python tools/train_pairs_bench.py --photometric [--parent-root DIR] [--repeats 3] [--out FILE]
       python tools/train_pairs_bench.py --colour all [--parent-root DIR] [--repeats 3] [--out profiles/train_pairs_colour_bench.json]
       python tools/train_pairs_bench.py --noise all [--parent-root DIR] [--repeats 3] [--out profiles/train_pairs_jpeg_bench.json]
       python tools/train_pairs_bench.py --iso --weather all [--repeats 3] [--out profiles/train_pairs_hls_bench.json]
       python tools/train_pairs_bench.py --glass [--parent-root DIR] [--repeats 3] [--out profiles/train_pairs_glass_bench.json]
       python tools/train_pairs_bench.py --store DIR [--repeats 3] [--out profiles/train_pairs_store_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, F, dev):
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
    return frames, pairs


def _time_build(builder, frames, pairs, iters):
    for _ in range(5):
        builder.build(frames, pairs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        builder.build(frames, pairs)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def build_only(args):
    """Child mode: `build` of the package under args.root (a checkout with its library built), stage off or on."""
    sys.path.insert(0, os.path.abspath(args.root))
    from feartracker_amd.train_data import TrainPairBuilder
    frames, pairs = _inputs(args.pairs, args.frames, torch.device("cuda", 0))
    config = dict(photometric=True) if args.stage_on else {}
    if args.colour:                                    # (only ever passed for a tree that knows the key)
        config["colour_members"] = args.colour
    if args.noise:
        config["noise_members"] = args.noise
    if args.iso:
        config["iso_noise"] = True
    if args.weather:
        config["weather_members"] = args.weather
    if args.glass:
        config["glass_blur"] = True
    builder = TrainPairBuilder(config or None, device=0, seed=0)
    print(json.dumps({"build_ms": round(_time_build(builder, frames, pairs, args.iters), 4)}))


def _child(root, args, stage_on=False, colour=None, noise=None, iso=False, weather=None, glass=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--build-only", "--root", root, "--pairs", str(args.pairs), "--frames",
           str(args.frames), "--iters", str(args.iters)] + (["--stage-on"] if stage_on else []) + (["--colour", colour] if colour else [])
    cmd += ["--noise", noise] if noise else []
    cmd += (["--iso"] if iso else []) + (["--weather", weather] if weather else []) + (["--glass"] if glass else [])
    res = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return json.loads(res.stdout.strip().splitlines()[-1])["build_ms"]


def photometric(args):
    # the fresh processes first, one at a time, before this process opens the GPU
    off, parent, on = [], [], []
    for _ in range(args.repeats):
        off.append(_child(ROOT, args))
        if args.parent_root:
            parent.append(_child(args.parent_root, args))
        on.append(_child(ROOT, args, stage_on=True))
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_abi import load_train_library
    from feartracker_amd.train_data import BLUR_MEDIAN, PHOTO_DTYPE, TrainPairBuilder, normal_quantiles
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    dev = torch.device("cuda", 0)
    B = args.pairs
    lib = load_train_library()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    ops = np.zeros(B, dtype=PHOTO_DTYPE)
    ops["blur"], ops["ksize"], ops["tap_row"] = BLUR_MEDIAN, 7, -1
    d_ops = torch.from_numpy(ops.view(np.uint8).copy()).to(dev)
    q = torch.from_numpy(normal_quantiles().copy()).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    crops = [torch.randint(0, 256, (B, s, s, 3), generator=g, device=dev, dtype=torch.uint8) for s in (128, 256)]
    outs = [torch.empty((B, 3, s, s), device=dev) for s in (128, 256)]

    def median7():
        for c, o, s in zip(crops, outs, (128, 256)):
            assert lib.fear_photometric_u8(P(c.data_ptr()), B, s, s, P(d_ops.data_ptr()), None, P(q.data_ptr()), P(o.data_ptr()), st) == 0

    for _ in range(5):
        median7()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        median7()
    e1.record()
    torch.cuda.synchronize()
    median7_ms = e0.elapsed_time(e1) / args.iters

    frames, pairs = _inputs(B, args.frames, dev)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    fixed = [t.clone() for t in TrainPairBuilder(device=0, seed=0).build(frames, pairs)[:5]]
    steps = []
    for _ in range(2):
        for _ in range(3):
            net.step(*fixed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            net.step(*fixed)
        torch.cuda.synchronize()
        steps.append(1e3 * (time.perf_counter() - t0) / args.steps)
    step_ms = min(steps)
    med = lambda v: round(float(np.median(v)), 4) if v else None
    report = {
        "pairs": B, "frames": args.frames, "frame_hw": [1080, 1920], "iters": args.iters,
        "build_off_ms": med(off), "build_off_runs": off,
        "parent_build_ms": med(parent), "parent_build_runs": parent,
        "build_on_ms": med(on), "build_on_runs": on,
        "median7_ms": round(median7_ms, 4),
        "step_ms": round(step_ms, 3), "step_ms_runs": [round(v, 3) for v in steps],
        "stage_ms": round(med(on) - med(off), 4),
        "stage_pct_of_step": round(100.0 * (med(on) - med(off)) / step_ms, 2),
        "median7_pct_of_step": round(100.0 * median7_ms / step_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }
    return report


def _step_ms(args, frames, pairs):
    """FEARNetTrainHIP.step on fixed inputs, wall time per step: (the smaller of two runs, both runs)."""
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    fixed = [t.clone() for t in TrainPairBuilder(device=0, seed=0).build(frames, pairs)[:5]]
    steps = []
    for _ in range(2):
        for _ in range(3):
            net.step(*fixed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            net.step(*fixed)
        torch.cuda.synchronize()
        steps.append(1e3 * (time.perf_counter() - t0) / args.steps)
    return min(steps), steps


def colour(args):
    # the fresh processes first, one at a time, before this process opens the GPU
    default, parent, wide = [], [], []
    for _ in range(args.repeats):
        default.append(_child(ROOT, args))
        if args.parent_root:
            parent.append(_child(args.parent_root, args))
        wide.append(_child(ROOT, args, colour=args.colour))
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_abi import load_train_library
    from feartracker_amd.train_data import (COLOUR_EMBOSS, COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_JITTER, TrainPairParams, colour_tables)
    dev = torch.device("cuda", 0)
    B = args.pairs
    lib = load_train_library()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    crops = [torch.randint(0, 256, (B, s, s, 3), generator=g, device=dev, dtype=torch.uint8) for s in (128, 256)]
    outs = [torch.empty_like(c) for c in crops]
    rng = np.random.default_rng(2)
    member_ms = {}
    for name, kind in (("equalize", COLOUR_EQUALIZE), ("hsv", COLOUR_HSV), ("colour_jitter", COLOUR_JITTER), ("emboss", COLOUR_EMBOSS)):
        params = TrainPairParams(context=np.zeros(B), jitter=np.zeros((B, 4)), tone=np.zeros(B, np.int32), colour=np.full(B, kind, np.int32),
                                 alpha=np.ones(B), beta=np.zeros(B), gamma=np.ones(B), shift=np.zeros((B, 3)), frame_shapes=(),
                                 hsv=rng.uniform(-20, 20, (B, 3)),
                                 colour_jitter=np.concatenate([rng.uniform(0.8, 1.2, (B, 3)), rng.uniform(-0.2, 0.2, (B, 1))], axis=1),
                                 colour_jitter_order=rng.permuted(np.tile(np.arange(4, dtype=np.int32), (B, 1)), axis=1),
                                 emboss=np.stack([rng.uniform(0.2, 0.5, B), rng.uniform(0.2, 0.7, B)], axis=1))
        ops, aux = colour_tables(params)
        d_ops, d_aux = torch.from_numpy(ops.view(np.uint8).copy()).to(dev), torch.from_numpy(aux).to(dev)

        def both():
            for c, o, s in zip(crops, outs, (128, 256)):
                assert lib.fear_colour_u8(P(c.data_ptr()), B, s, s, P(d_ops.data_ptr()), P(d_aux.data_ptr()), P(o.data_ptr()), st) == 0

        for _ in range(5):
            both()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            both()
        e1.record()
        torch.cuda.synchronize()
        member_ms[name] = round(e0.elapsed_time(e1) / args.iters, 4)
    frames, pairs = _inputs(B, args.frames, dev)
    step_ms, steps = _step_ms(args, frames, pairs)
    med = lambda v: round(float(np.median(v)), 4) if v else None
    worst = max(member_ms, key=member_ms.get)
    return {
        "pairs": B, "frames": args.frames, "frame_hw": [1080, 1920], "iters": args.iters, "colour_members": args.colour,
        "build_default_ms": med(default), "build_default_runs": default,
        "parent_build_ms": med(parent), "parent_build_runs": parent,
        "build_all_ms": med(wide), "build_all_runs": wide,
        "colour_u8_ms": member_ms, "worst_member": worst,
        "step_ms": round(step_ms, 3), "step_ms_runs": [round(v, 3) for v in steps],
        "members_ms": round(med(wide) - med(default), 4),
        "members_pct_of_step": round(100.0 * (med(wide) - med(default)) / step_ms, 2),
        "worst_member_pct_of_step": round(100.0 * member_ms[worst] / step_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }


def noise(args):
    # the fresh processes first, one at a time, before this process opens the GPU
    default, parent, wide = [], [], []
    for _ in range(args.repeats):
        default.append(_child(ROOT, args, stage_on=True))
        if args.parent_root:
            parent.append(_child(args.parent_root, args, stage_on=True))
        wide.append(_child(ROOT, args, stage_on=True, noise=args.noise))
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_abi import load_train_library
    dev = torch.device("cuda", 0)
    B = args.pairs
    lib = load_train_library()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    crops = [torch.randint(0, 256, (B, s, s, 3), generator=g, device=dev, dtype=torch.uint8) for s in (128, 256)]
    outs = [torch.empty_like(c) for c in crops]
    quality = torch.full((B,), 50, dtype=torch.int32, device=dev)
    ws_bytes = lib.fear_jpeg_workspace_bytes(B, 256, 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def both():
        for c, o, s in zip(crops, outs, (128, 256)):
            assert lib.fear_jpeg_u8(P(c.data_ptr()), B, s, s, P(quality.data_ptr()), P(ws.data_ptr()), ws_bytes, P(o.data_ptr()), st) == 0

    for _ in range(5):
        both()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        both()
    e1.record()
    torch.cuda.synchronize()
    jpeg_ms = e0.elapsed_time(e1) / args.iters
    frames, pairs = _inputs(B, args.frames, dev)
    step_ms, steps = _step_ms(args, frames, pairs)
    med = lambda v: round(float(np.median(v)), 4) if v else None
    return {
        "pairs": B, "frames": args.frames, "frame_hw": [1080, 1920], "iters": args.iters, "noise_members": args.noise,
        "build_default_ms": med(default), "build_default_runs": default,
        "parent_build_ms": med(parent), "parent_build_runs": parent,
        "build_all_ms": med(wide), "build_all_runs": wide,
        "jpeg_u8_ms": round(jpeg_ms, 4),
        "step_ms": round(step_ms, 3), "step_ms_runs": [round(v, 3) for v in steps],
        "member_ms": round(med(wide) - med(default), 4),
        "member_pct_of_step": round(100.0 * (med(wide) - med(default)) / step_ms, 2),
        "jpeg_u8_pct_of_step": round(100.0 * jpeg_ms / step_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }


def hls(args):
    # the fresh processes first, one at a time, before this process opens the GPU
    default, on = [], []
    for _ in range(args.repeats):
        default.append(_child(ROOT, args, stage_on=True))
        on.append(_child(ROOT, args, stage_on=True, iso=args.iso, weather=args.weather))
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_abi import load_train_library
    from feartracker_amd.train_data import (HLS_DTYPE, HLS_ISO, HLS_RAIN, HLS_SHADOW, iso_exp_table, normal_quantiles, rain_drop_count,
                                            rain_segments, shadow_segments)
    dev = torch.device("cuda", 0)
    B = args.pairs
    lib = load_train_library()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    sides = (128, 256)
    crops = [torch.randint(0, 256, (B, s, s, 3), generator=g, device=dev, dtype=torch.uint8) for s in sides]
    outs = [torch.empty_like(c) for c in crops]
    q, table = torch.from_numpy(normal_quantiles().copy()).to(dev), torch.from_numpy(iso_exp_table().copy()).to(dev)
    rng = np.random.default_rng(2)
    member_ms = {}
    for name, kind in (("iso_noise", HLS_ISO), ("rain", HLS_RAIN), ("shadow", HLS_SHADOW)):
        d_ops, d_seg = [], []
        for s in sides:                                    # a record and segments per crop, drawn as the builder draws them
            ops = np.zeros(B, dtype=HLS_DTYPE)
            ops["kind"], ops["intensity"], ops["key"] = kind, rng.uniform(0.1, 0.5, B), rng.integers(0, 2 ** 32, (B, 2))
            ops["hue_scale"] = rng.uniform(0.01, 0.05, B) * 360.0 * ops["intensity"]
            rows, n_rows = [np.zeros((1, 4), np.int16)], 1
            for b in range(B):
                if kind == HLS_RAIN:
                    slant, n = int(rng.integers(-10, 11)), rain_drop_count(s)
                    seg = rain_segments(slant, np.stack([rng.integers(min(slant, 0), s - max(slant, 0) + 1, n),
                                                         rng.integers(0, s - 19, n)], axis=1))
                else:
                    seg = shadow_segments([np.stack([rng.integers(0, s + 1, 5), rng.integers(s // 2, s + 1, 5)], axis=1) for _ in range(2)])
                ops["seg_offset"][b], ops["seg_count"][b] = n_rows, len(seg)
                rows.append(seg)
                n_rows += len(seg)
            d_ops.append(torch.from_numpy(ops.view(np.uint8).copy()).to(dev))
            d_seg.append(torch.from_numpy(np.concatenate(rows)).to(dev))

        def both():
            for c, o, s, r, sg in zip(crops, outs, sides, d_ops, d_seg):
                assert lib.fear_hls_u8(P(c.data_ptr()), B, s, s, P(r.data_ptr()), P(sg.data_ptr()), P(q.data_ptr()), P(table.data_ptr()),
                                       P(o.data_ptr()), st) == 0

        for _ in range(5):
            both()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            both()
        e1.record()
        torch.cuda.synchronize()
        member_ms[name] = round(e0.elapsed_time(e1) / args.iters, 4)
    frames, pairs = _inputs(B, args.frames, dev)
    step_ms, steps = _step_ms(args, frames, pairs)
    med = lambda v: round(float(np.median(v)), 4) if v else None
    worst = max(member_ms, key=member_ms.get)
    return {
        "pairs": B, "frames": args.frames, "frame_hw": [1080, 1920], "iters": args.iters, "iso_noise": bool(args.iso),
        "weather_members": args.weather or "",
        "build_default_ms": med(default), "build_default_runs": default,
        "build_on_ms": med(on), "build_on_runs": on,
        "hls_u8_ms": member_ms, "worst_member": worst,
        "step_ms": round(step_ms, 3), "step_ms_runs": [round(v, 3) for v in steps],
        "members_ms": round(med(on) - med(default), 4),
        "members_pct_of_step": round(100.0 * (med(on) - med(default)) / step_ms, 2),
        "worst_member_pct_of_step": round(100.0 * member_ms[worst] / step_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }


def glass(args):
    # the fresh processes first, one at a time, before this process opens the GPU
    default, parent, on = [], [], []
    for _ in range(args.repeats):
        default.append(_child(ROOT, args, stage_on=True))
        if args.parent_root:
            parent.append(_child(args.parent_root, args, stage_on=True))
        on.append(_child(ROOT, args, stage_on=True, glass=True))
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_abi import load_train_library
    from feartracker_amd.train_data import BLUR_GLASS, PHOTO_DTYPE
    dev = torch.device("cuda", 0)
    B = args.pairs
    lib = load_train_library()
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    crops = [torch.randint(0, 256, (B, s, s, 3), generator=g, device=dev, dtype=torch.uint8) for s in (128, 256)]
    outs = [torch.empty_like(c) for c in crops]
    ops = np.zeros(B, dtype=PHOTO_DTYPE)
    ops["blur"], ops["tap_row"], ops["key"] = BLUR_GLASS, -1, np.random.default_rng(2).integers(0, 2 ** 32, (B, 2))
    d_ops = torch.from_numpy(ops.view(np.uint8).copy()).to(dev)

    def both():
        for c, o, s in zip(crops, outs, (128, 256)):
            assert lib.fear_glass_u8(P(c.data_ptr()), B, s, s, P(d_ops.data_ptr()), P(o.data_ptr()), st) == 0

    for _ in range(5):
        both()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        both()
    e1.record()
    torch.cuda.synchronize()
    glass_ms = e0.elapsed_time(e1) / args.iters
    frames, pairs = _inputs(B, args.frames, dev)
    step_ms, steps = _step_ms(args, frames, pairs)
    med = lambda v: round(float(np.median(v)), 4) if v else None
    return {
        "pairs": B, "frames": args.frames, "frame_hw": [1080, 1920], "iters": args.iters, "glass_blur": True,
        "build_default_ms": med(default), "build_default_runs": default,
        "parent_build_ms": med(parent), "parent_build_runs": parent,
        "build_on_ms": med(on), "build_on_runs": on,
        "glass_u8_ms": round(glass_ms, 4),
        "step_ms": round(step_ms, 3), "step_ms_runs": [round(v, 3) for v in steps],
        "member_ms": round(med(on) - med(default), 4),
        "member_pct_of_step": round(100.0 * (med(on) - med(default)) / step_ms, 2),
        "glass_u8_pct_of_step": round(100.0 * glass_ms / step_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }


def store_mode(args):
    """decode + build against decode_rows + build(borders=) out of a resident store."""
    import glob
    sys.path.insert(0, ROOT)
    from feartracker_amd import JpegStore
    from feartracker_amd.train_data import TrainPairBuilder
    blobs = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.store, "*.jpg")))]
    B = args.pairs
    assert len(blobs) >= 2 * B, "the store mode takes two frames of their own per pair: run tools/jpeg_decode_bench.py --make first"
    store = JpegStore(device=0, threads=16)
    ids = store.add(blobs[:2 * B])
    shapes = store.shape(ids)
    Hf, Wf = int(shapes[0, 0]), int(shapes[0, 1])
    lo, hi = 40, 300
    rng = np.random.default_rng(0)
    pairs = np.zeros((B, 11))
    pairs[:, 0], pairs[:, 5], pairs[:, 10] = 2 * np.arange(B), 2 * np.arange(B) + 1, 1
    for col in (1, 6):
        w, h = rng.integers(lo, hi, B), rng.integers(lo, hi, B)
        pairs[:, col], pairs[:, col + 1], pairs[:, col + 2], pairs[:, col + 3] = rng.integers(0, Wf - w), rng.integers(0, Hf - h), w, h
    builder = TrainPairBuilder(device=0, seed=0)
    params = builder.draw(pairs, shapes, np.random.default_rng(1))
    rows = builder.frame_rows(pairs, params, shapes)

    def whole():
        return builder.build(store.decode(ids), pairs, params)

    def bands():
        return builder.build(store.decode_rows(ids, builder.frame_rows(pairs, params, shapes)), pairs, params, borders=store.borders(ids))

    frames = store.decode(ids)
    parts = {"decode_ms": lambda: store.decode(ids), "decode_rows_ms": lambda: store.decode_rows(ids, rows),
             "build_ms": lambda: builder.build(frames, pairs, params),
             "build_borders_ms": lambda: builder.build(frames, pairs, params, borders=store.borders(ids))}
    x, y = whole(), bands()
    store.check()
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for a, b in zip(x, y))
    assert equal, "build on band frames differs from build on whole frames"

    def runs(fn):
        out = []
        for k in range(args.repeats + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
            del keep
        out = out[1:]                                   # the first run warms
        return {"median": round(float(np.median(out)), 4), "min": round(min(out), 4), "max": round(max(out), 4)}

    report = {"pairs": B, "frames": 2 * B, "frame_hw": [Hf, Wf], "repeats": args.repeats + 2, "batches_equal": equal,
              "boxes": {"side_lo": lo, "side_hi": hi, "distribution": "uniform integers, template and search boxes alike, seed 0",
                        "context": "the builder's defaults, drawn with seed 1",
                        "rows_per_frame": round(float((rows[:, 1] - rows[:, 0]).mean()), 1)},
              "decode_build_ms": runs(whole), "rows_build_ms": runs(bands)}
    for name, fn in parts.items():
        report[name] = runs(fn)
    store.check()
    report["device"] = torch.cuda.get_device_name(0)
    store.close()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--photometric", action="store_true")
    ap.add_argument("--colour", default=None, help='"all": report the members behind colour_members')
    ap.add_argument("--noise", default=None, help='"all": report ImageCompression, the member behind noise_members')
    ap.add_argument("--iso", action="store_true", help="report ISONoise, the member behind iso_noise")
    ap.add_argument("--weather", default=None, help='"all": report RandomRain and RandomShadow, the members behind weather_members')
    ap.add_argument("--glass", action="store_true", help="report GlassBlur, the member behind glass_blur")
    ap.add_argument("--store", default=None, help="DIR of the synthetic 720p files: the resident store in front of the builder")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--stage-on", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.build_only:
        return build_only(args)
    if args.store:
        args.out = args.out or os.path.join(ROOT, "profiles", "train_pairs_store_bench.json")
        return emit(store_mode(args), args)
    if args.glass:
        args.out = args.out or os.path.join(ROOT, "profiles", "train_pairs_glass_bench.json")
        return emit(glass(args), args)
    if args.iso or args.weather:
        args.out = args.out or os.path.join(ROOT, "profiles", "train_pairs_hls_bench.json")
        return emit(hls(args), args)
    if args.photometric:
        return emit(photometric(args), args)
    if args.colour:
        return emit(colour(args), args)
    if args.noise:
        args.out = args.out or os.path.join(ROOT, "profiles", "train_pairs_jpeg_bench.json")
        return emit(noise(args), args)
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_data import FRAME_DTYPE, TrainPairBuilder
    from feartracker_amd.train_head import load_train_library
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state

    dev = torch.device("cuda", 0)
    B, F = args.pairs, args.frames
    frames, pairs = _inputs(B, F, dev)
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
    emit(report, args)


def emit(report, args):
    line = json.dumps(report)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
