"""Measures the JPEG encoder (jpeg_encode.JpegEncoder, DESIGN.md section 14 "Writing JPEG files") on the 256 synthetic 1280 x 720 frames of
tools/jpeg_decode_bench.py at quality 90 and writes profiles/jpeg_encode_bench.json.  Needs the GPU; Pillow only for the baseline.

    python tools/jpeg_encode_bench.py [--frames 256] [--repeats 5] [--subsampling MODE]

Without --subsampling the run and its output file are those of the first encoder (4:2:0).  With it the same frames are written in that
layout ("gray": the luma of the RGB frames, Pillow's convert("L")) and the result goes under the layout's name into
profiles/jpeg_encode_modes_bench.json, beside what other runs have put there.

  encode_fps              JpegEncoder.encode + PendingJpegs.result() end to end: frames on the device -> files' bytes on the host
  kernels_ms              fear_jpeg_encode_u8 alone between HIP events (the memset and the eight launches of the 256 frames); the split
                          by pass comes from a kernel trace of this same script run with --kernels-only
  download_bytes_per_frame    the files' bytes, against 3 H W raw
  pillow_fps              what a user does without the encoder: copy the raw frames to the host and Image.save them on 16 threads, timed
                          in the same run on the same machine
Every timing is the median of --repeats runs after one warm-up run, with the minimum and maximum of the runs."""
import argparse
import importlib.util
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUALITY = 90


def decode_bench():
    spec = importlib.util.spec_from_file_location("jpeg_decode_bench", os.path.join(ROOT, "tools", "jpeg_decode_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="three encode calls and nothing else: the run to put under a kernel trace")
    ap.add_argument("--subsampling", default=None, choices=("4:2:0", "4:2:2", "4:4:4", "gray"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mode = args.subsampling
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_encode_bench.json" if mode is None else "jpeg_encode_modes_bench.json")
    import torch
    from feartracker_amd import JpegEncoder
    from feartracker_amd import train_abi as abi
    db = decode_bench()
    host = [img for img, _ in zip(db.images(), range(args.frames))]
    n = len(host)
    frames = [torch.from_numpy(f).cuda() for f in host]
    enc = JpegEncoder(0, quality=QUALITY) if mode is None else JpegEncoder(0, quality=QUALITY, subsampling=mode)
    if args.kernels_only:
        for _ in range(3):
            enc.encode(frames).result()
        return
    files = enc.encode(frames).result()
    res = {"frames": n, "width": db.W, "height": db.H, "quality": QUALITY, "repeats": args.repeats,
           "cpus_available": len(os.sched_getaffinity(0)),
           "download_bytes_per_frame": {"files": round(sum(map(len, files)) / n, 1), "raw": 3 * db.H * db.W,
                                        "ratio": round(sum(map(len, files)) / n / (3 * db.H * db.W), 4)}}

    def end_to_end():
        return enc.encode(frames).result()
    res["encode_fps"] = db.spread([n / t for t in db.run_seconds(end_to_end, args.repeats)], digits=1)
    captured, real = {}, abi.launch

    def spy(lib, name, *a):
        captured[name] = a
        return real(lib, name, *a)
    abi.launch = spy
    try:
        pending = enc.encode(frames)                                       # (jpeg_encode imports launch inside encode: the spy is seen)
    finally:
        abi.launch = real
    call = captured["fear_jpeg_encode_u8"]                                 # (`pending` keeps the call's buffers alive for the replays)
    res["kernels_ms"] = db.spread(db.event_ms(torch, lambda: enc._lib.fear_jpeg_encode_u8(*call), args.repeats))
    assert pending.result() == files
    res["kernels_fps"] = round(n / (res["kernels_ms"]["median"] * 1e-3), 1)
    try:
        from PIL import Image
    except ImportError:
        res["pillow_fps"] = None
    else:
        def save(f):
            buf = io.BytesIO()
            if mode is None:
                Image.fromarray(f).save(buf, "JPEG", quality=QUALITY)
            elif mode == "gray":
                Image.fromarray(f).convert("L").save(buf, "JPEG", quality=QUALITY)
            else:
                Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, subsampling={"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}[mode])
            return buf.getvalue()

        with ThreadPoolExecutor(max_workers=16) as pool:
            def baseline():
                stack = torch.stack(frames).cpu().numpy()                  # the raw pixels come down first
                return list(pool.map(save, stack))
            assert baseline() == files, "the encoder's files differ from Pillow's"
            res["pillow_fps"] = db.spread([n / t for t in db.run_seconds(baseline, args.repeats)], digits=1)
        res["files_equal_pillow"] = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    whole = res
    if mode is not None:                                                   # one entry per layout in a file other runs add to
        whole = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                whole = json.load(fh)
        whole.setdefault("modes", {})[mode] = res
    with open(args.out, "w") as fh:
        json.dump(whole, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
