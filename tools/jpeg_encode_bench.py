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
Every timing is the median of --repeats runs after one warm-up run, with the minimum and maximum of the runs.

    python tools/jpeg_encode_bench.py --optimize [--parent-lib LIB] [--passes-from STATS.csv]

measures per-file Huffman tables (JpegEncoder(optimize=True)) beside the default path in one run, 4:2:0, and writes
profiles/jpeg_encode_optimize_bench.json: per path encode_fps, kernels_ms and bytes_per_frame, and their size_ratio; the optimised files
are compared with Pillow's optimize=True files.  --parent-lib times the default path of the parent commit's library on the same call,
beside this build's: `not_slower_than_parents_slowest` is this build's median against the slowest of the parent's runs.  --passes-from
takes the kernel statistics of a trace of `--optimize --kernels-only` (three calls) and adds the kernel time per pass."""
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


PASSES = {"jpeg_enc_transform_kernel": "transform", "jpeg_enc_stats_kernel": "stats", "jpeg_enc_tables_kernel": "tables",
          "jpeg_enc_code_kernel<false>": "sizes", "jpeg_enc_segments_kernel": "segments", "jpeg_enc_image_scan_kernel<false>": "offsets",
          "jpeg_enc_code_kernel<true>": "write", "jpeg_enc_stuff_kernel<false>": "count", "jpeg_enc_image_scan_kernel<true>": "lengths",
          "jpeg_enc_stuff_kernel<true>": "assemble"}


def passes_ms(stats_csv, calls):
    """Kernel time per pass and encode call, in ms, from the kernel statistics (csv) of a trace of `--optimize --kernels-only`."""
    import csv
    out = {}
    with open(stats_csv) as fh:
        for row in csv.DictReader(fh):
            for key, name in PASSES.items():
                if key in row["Name"]:                                     # (demangled: the template argument is part of the name)
                    out[name] = round(int(row["TotalDurationNs"]) / calls / 1e6, 4)
    return out


def optimize_bench(args, torch, db, frames, host):
    """--optimize: the optimised path beside the default path, and the default path of this build beside the parent commit's build."""
    import ctypes
    from feartracker_amd import JpegEncoder
    from feartracker_amd import train_abi as abi
    n = len(frames)
    res = {"frames": n, "width": db.W, "height": db.H, "quality": QUALITY, "repeats": args.repeats}
    captured, real = {}, abi.launch

    def spy(lib, name, *a):
        captured[name] = a
        return real(lib, name, *a)
    keep = []
    for on in (False, True, False, True):                                  # both paths warm (allocator, pinned memory) before either is timed
        JpegEncoder(0, quality=QUALITY, optimize=on).encode(frames).result()
    for name, on in (("plain", False), ("optimize", True), ("plain_again", False)):
        enc = JpegEncoder(0, quality=QUALITY, optimize=on)
        files = enc.encode(frames).result()
        if name == "plain_again":                                          # the order of the two paths must not decide the comparison
            res["plain"]["encode_fps_after_optimize"] = db.spread([n / t for t in db.run_seconds(lambda: enc.encode(frames).result(), args.repeats)],
                                                                  digits=1)
            break
        one = {"bytes_per_frame": round(sum(map(len, files)) / n, 1)}
        one["encode_fps"] = db.spread([n / t for t in db.run_seconds(lambda: enc.encode(frames).result(), args.repeats)], digits=1)
        abi.launch = spy
        try:
            pending = enc.encode(frames)
        finally:
            abi.launch = real
        call = captured["fear_jpeg_encode_u8"]
        keep.append(pending)                                               # (keeps the call's buffers alive for the replays)
        one["kernels_ms"] = db.spread(db.event_ms(torch, lambda: enc._lib.fear_jpeg_encode_u8(*call), args.repeats))
        assert pending.result() == files
        res[name] = one
        if on:
            try:
                from PIL import Image
            except ImportError:
                res["files_equal_pillow"] = None
            else:
                def save(f):
                    buf = io.BytesIO()
                    Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, optimize=True)
                    return buf.getvalue()
                with ThreadPoolExecutor(max_workers=16) as pool:
                    res["files_equal_pillow"] = list(pool.map(save, host)) == files
        elif args.parent_lib:
            # the default path of both builds on the same call: a plain record is the same 96 bytes in both
            parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
            parent.fear_jpeg_encode_u8.argtypes, parent.fear_jpeg_encode_u8.restype = abi.TRAIN_SYMBOLS["fear_jpeg_encode_u8"]
            theirs = db.spread(db.event_ms(torch, lambda: parent.fear_jpeg_encode_u8(*call), args.repeats))
            ours = db.spread(db.event_ms(torch, lambda: enc._lib.fear_jpeg_encode_u8(*call), args.repeats))
            res["default_path"] = {"parent_kernels_ms": theirs, "kernels_ms": ours, "not_slower_than_parents_slowest": ours["median"] <= theirs["max"]}
    res["size_ratio"] = round(res["optimize"]["bytes_per_frame"] / res["plain"]["bytes_per_frame"], 4)
    if args.passes_from:
        res["optimize"]["passes_ms"] = passes_ms(args.passes_from, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimize", action="store_true", help="per-file Huffman tables beside the default path: profiles/jpeg_encode_optimize_bench.json")
    ap.add_argument("--parent-lib", default=None, help="with --optimize: the parent commit's library, whose default path is timed on the same call")
    ap.add_argument("--passes-from", default=None, help="with --optimize: the kernel statistics (csv) of a trace of --optimize --kernels-only")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="three encode calls and nothing else: the run to put under a kernel trace")
    ap.add_argument("--subsampling", default=None, choices=("4:2:0", "4:2:2", "4:4:4", "gray"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mode = args.subsampling
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_encode_optimize_bench.json" if args.optimize else
                                "jpeg_encode_bench.json" if mode is None else "jpeg_encode_modes_bench.json")
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
            enc.encode(frames, optimize=args.optimize).result()
        return
    if args.optimize:
        res = optimize_bench(args, torch, db, frames, host)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res))
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
