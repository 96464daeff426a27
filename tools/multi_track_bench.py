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

Video frames: `--format rgb,nv12,i420` times the pipelined submit loop on the same frames as packed RGB,
NV12 and I420 (`YUVFrame`; the YUV frames are the RGB frames through tests/yuvgen.rgb_to_yuv420), host frames, and with
`--device-frames` device frames as well; on device YUV frames also what a caller without the planar crop does: fear_yuv_to_rgb
per frame, then the RGB path.  It then times the crop launches alone at each K with device events: fear_crop_normalize_frames on
the RGB frame, fear_crop_normalize_planar on the NV12 and I420 frames, fear_yuv_to_rgb of one frame.  Default output
profiles/multi_track_yuv_bench.json (with --out: that file).
       python tools/multi_track_bench.py --format rgb,nv12,i420 --device-frames [--ks 1,16,64,256] [--frames 40]

Frames kept in a JpegStore ("Rows from the device"): `--store DIR` takes the JPEG files of DIR (the 256 files
of tools/jpeg_decode_bench.py --make) and tracks S streams with one target each, S = 1, 16, 64, stream s reading every S-th file.  In ONE
run, medians of 5 with minimum and maximum, it reports frames per second (streams x steps / time, pipelined: a step's boxes are read
behind the next step's submit) of
  decode_submit     store.decode(ids) + submit: whole frames, the baseline
  rows_submit       search_rows + store.decode_rows(ids, rows) + submit: only the rows the tracker is about to read
and `band_rows_mean`, the mean number of frame rows per stream and step that search_rows asks for (clipped to the frame).  The boxes of
both loops are compared before anything is timed.  Default output profiles/multi_track_store_bench.json.
       python tools/multi_track_bench.py --store DIR [--ks 1,16,64] [--frames 40]
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
from feartracker_amd import DEFAULT_TRACKING_CONFIG, DEFAULT_WEIGHTS, FEARMultiTracker, FEARNetHIP, FEARTracker, YUVFrame  # noqa: E402
from yuvgen import rgb_to_yuv420  # noqa: E402


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


def event_ms(fn, n):
    """Device time per call of `fn` over n back-to-back calls, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def yuv_frames(planes, fmt):
    return [YUVFrame.nv12(y, np.stack([u, v], -1).reshape(u.shape[0], -1)) if fmt == "nv12" else YUVFrame.i420(y, u, v)
            for y, u, v in planes]


def pipelined_ms(net, cfg, first, frames, boxes, n, prep=None):
    """ms per frame of the pipelined submit loop over frames[4:4 + n] (frames[1:4] warm up)."""
    prep = prep or (lambda f: f)
    mt = FEARMultiTracker(net, cuda_id=0, **cfg)
    mt.add(first, boxes)
    for f in frames[1:4]:
        mt.update(prep(f))
    state = {"p": None}

    def step(i):
        nxt = mt.submit(prep(frames[4 + i]))
        if state["p"] is not None:
            state["p"].result()
        state["p"] = nxt

    ms = timed(step, n, torch.cuda.synchronize)
    state["p"].result()
    return ms


def yuv_main(args):
    """--format: pipelined submit on RGB / NV12 / I420 frames, host and device, and the crop launches alone."""
    fmts = [f.strip().lower() for f in args.format.split(",")]
    rgb = hd_frames(args.frames + 4)
    planes = [rgb_to_yuv420(f, seed=t) for t, f in enumerate(rgb)] if set(fmts) - {"rgb"} else []
    frames = {f: (list(rgb) if f == "rgb" else yuv_frames(planes, f)) for f in fmts}
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=0, max_batch=args.max_batch)
    cfg = DEFAULT_TRACKING_CONFIG
    dev = torch.device("cuda:0")
    on_dev = {f: ([torch.from_numpy(x).to(dev) for x in v] if f == "rgb" else [x.to(dev) for x in v]) for f, v in frames.items()}
    res = {"frame_shape": list(rgb[0].shape), "frames_timed": args.frames, "max_batch": args.max_batch,
           "device": torch.cuda.get_device_name(0), "formats": fmts, "per_k": []}
    for k in (int(v) for v in args.ks.split(",")):
        boxes = target_boxes(k)
        row = {"k": k}
        for f in fmts:
            row[f"submit_host_{f}_ms"] = pipelined_ms(net, cfg, frames[f][0], frames[f], boxes, args.frames)
            if args.device_frames:
                row[f"submit_device_{f}_ms"] = pipelined_ms(net, cfg, on_dev[f][0], on_dev[f], boxes, args.frames)
                if f != "rgb":
                    row[f"submit_device_{f}_via_yuv_to_rgb_ms"] = pipelined_ms(net, cfg, on_dev[f][0], on_dev[f], boxes,
                                                                               args.frames, prep=net.yuv_to_rgb)
        # the crop launches alone, on one device frame per format: the search crops of the K targets' first frame
        mt = FEARMultiTracker(net, cuda_id=0, **cfg)
        mt.add(rgb[0], boxes)
        fidx, ctx, pad = mt._fidx, mt._ctx, mt._pad
        S = cfg["instance_size"]
        out = torch.empty((k, 3, S, S), dtype=torch.float32, device=dev)
        if "rgb" in fmts:
            tab = net.frame_table([on_dev["rgb"][0]])
            row["crop_rgb_us"] = 1e3 * event_ms(lambda: net.crop_normalize_frames(tab, fidx, ctx, pad, S, out=out), 50)
        for f in fmts:
            if f == "rgb":
                continue
            tab_p = net.frame_table_planar([on_dev[f][0]])
            rgb_buf = torch.empty(rgb[0].shape, dtype=torch.uint8, device=dev)
            tab_c = net.frame_table([rgb_buf])
            row[f"crop_planar_{f}_us"] = 1e3 * event_ms(lambda: net.crop_normalize_planar(tab_p, fidx, ctx, pad, S, out=out), 50)
            row[f"yuv_to_rgb_{f}_us"] = 1e3 * event_ms(lambda: net.yuv_to_rgb(on_dev[f][0], out=rgb_buf), 50)
            row[f"yuv_to_rgb_then_crop_{f}_us"] = 1e3 * event_ms(
                lambda: (net.yuv_to_rgb(on_dev[f][0], out=rgb_buf), net.crop_normalize_frames(tab_c, fidx, ctx, pad, S, out=out)),
                50)
        res["per_k"].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "multi_track_yuv_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)


def store_main(args):
    """--store: decode + submit against search_rows + decode_rows + submit on frames kept in a JpegStore."""
    import glob
    import statistics
    from feartracker_amd import JpegStore
    blobs = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.store, "*.jpg")))]
    assert blobs, "no .jpg files in --store DIR"
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=0, max_batch=args.max_batch)
    cfg, repeats, steps = DEFAULT_TRACKING_CONFIG, 5, args.frames
    store = JpegStore(device=0, threads=16)
    all_ids = store.add(blobs)
    (h, w), n = store.shape(all_ids[:1])[0].tolist(), len(all_ids)
    res = {"files": n, "frame_shape": [h, w, 3], "steps_timed": steps, "repeats": repeats, "max_batch": args.max_batch,
           "device": torch.cuda.get_device_name(0), "subsequence_bytes": store.subsequence_bytes, "per_streams": []}

    def spread(values, digits=1):
        return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}

    for S in (int(v) for v in args.ks.split(",")):
        ids_at = lambda t: all_ids[(np.arange(S) + S * t) % n]               # stream s reads file s, s + S, s + 2 S, ...
        boxes = target_boxes(S + 6, h, w)[6:]                                # one target per stream, inside the frame

        def fresh():
            mt = FEARMultiTracker(net, cuda_id=0, **cfg)
            first = store.decode(ids_at(0))
            for s in range(S):
                mt.add(first[s], boxes[s], stream=s)
            return mt

        def loop(mt, rows_form, keep_rows=None, keep_boxes=None):
            """`steps` pipelined steps; seconds."""
            pending = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(1, steps + 1):
                if rows_form:
                    rows = mt.search_rows(S)
                    frames = store.decode_rows(ids_at(t), rows)
                    if keep_rows is not None:
                        keep_rows.append(rows)
                else:
                    frames = store.decode(ids_at(t))
                nxt = mt.submit(frames)
                if pending is not None:
                    got = pending.result()
                    if keep_boxes is not None:
                        keep_boxes.append(got)
                pending = nxt
            got = pending.result()
            if keep_boxes is not None:
                keep_boxes.append(got)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        # warm, and the same boxes from both loops before anything is timed
        rows_seen, boxes_a, boxes_b = [], [], []
        loop(fresh(), False, keep_boxes=boxes_a)
        loop(fresh(), True, keep_rows=rows_seen, keep_boxes=boxes_b)
        store.check()
        assert all(np.array_equal(x[i], y[i]) for x, y in zip(boxes_a, boxes_b) for i in x), "the two loops track differently"
        band = torch.stack(rows_seen).clamp(0, h).cpu().numpy()
        row = {"streams": S, "boxes_equal": True, "band_rows_mean": round(float((band[..., 1] - band[..., 0]).clip(min=0).mean()), 1)}
        a = [loop(fresh(), False) for _ in range(repeats)]
        b = [loop(fresh(), True) for _ in range(repeats)]
        row["decode_submit_fps"] = spread([S * steps / t for t in a])
        row["rows_submit_fps"] = spread([S * steps / t for t in b])
        row["decode_submit_ms_per_step"] = spread([1e3 * t / steps for t in a], 4)
        row["rows_submit_ms_per_step"] = spread([1e3 * t / steps for t in b], 4)
        row["rows_faster"] = bool(max(b) < min(a))
        res["per_streams"].append(row)
        print(json.dumps(row), flush=True)
    store.close()
    out = args.out or os.path.join(ROOT, "profiles", "multi_track_store_bench.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--no-singles", action="store_true")
    ap.add_argument("--submit-only", action="store_true", help="time only the pipelined submit loop (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    ap.add_argument("--format", default="", help="rgb,nv12,i420: time video frames (see the module docstring)")
    ap.add_argument("--device-frames", action="store_true", help="with --format: device frames too")
    ap.add_argument("--store", default="", help="a directory of JPEG files: track on frames kept in a JpegStore (see the module docstring)")
    args = ap.parse_args()
    args.ks = args.ks or ("1,16,64" if args.store else "1,16,64,256,1024")
    if args.store:
        return store_main(args)
    if args.format:
        return yuv_main(args)
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
