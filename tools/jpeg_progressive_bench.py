"""Measures progressive files in the JPEG frame path ("Progressive files") on the 256 synthetic 1280 x 720,
quality 90, 4:2:0 images of tools/jpeg_decode_bench.py, saved both ways, and writes profiles/jpeg_progressive_bench.json.

    python tools/jpeg_progressive_bench.py --make --dir DIR     # needs Pillow: writes DIR/baseline and DIR/progressive (any machine)
    python tools/jpeg_progressive_bench.py --dir DIR            # needs the GPU: measures

Everything in ONE run, every shape warmed first, medians of 5 with minimum and maximum:
  add_files_per_s          JpegStore(progressive=True).add of the 256 progressive files into a fresh store (the transcode on 16 threads
                           included) against JpegStore().add of their baseline twins
  transcode_ms_per_file    fear_jpeg_progressive_parse + fear_jpeg_progressive_to_baseline, one thread, mean over the files
  bytes_per_file           the progressive file, its baseline twin, its transcode, and what the store keeps resident for it and for the twin
  decode_ms_per_call       store.decode of the 256 ids in a seeded permutation with check(), a host clock around work that ends in a
                           synchronise: the transcodes against the baseline twins
  decode_rows_ms_per_call  the same for decode_rows at a quarter of the height, seeded positions
  decoder_fps              JpegDecoder(progressive=True).decode of the progressive files end to end (every scan on 16 host threads),
                           against JpegDecoder().decode of the twins
Before anything is timed the frames of the two stores and of the decoder are compared: the same coefficients, so the same bytes
(`frames_equal_twins`)."""
import argparse
import glob
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_decode_bench import H, QUALITY, W, images, run_seconds, spread  # noqa: E402


def make(directory):
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = 1 << 24          # a progressive save needs the whole file in one buffer
    for kind in ("baseline", "progressive"):
        os.makedirs(os.path.join(directory, kind), exist_ok=True)
    count = 0
    for i, img in enumerate(images()):
        for kind in ("baseline", "progressive"):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=QUALITY, subsampling=2, progressive=kind == "progressive")
            with open(os.path.join(directory, kind, f"frame{i:03d}.jpg"), "wb") as fh:
                fh.write(buf.getvalue())
        count += 1
    print("wrote", count, "files each to", os.path.join(directory, "baseline"), "and", os.path.join(directory, "progressive"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--make", action="store_true")
    ap.add_argument("--files", type=int, default=0, help="use the first N files only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_progressive_bench.json"))
    args = ap.parse_args()
    if args.make:
        return make(args.dir)
    base = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.dir, "baseline", "*.jpg")))]
    prog = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.dir, "progressive", "*.jpg")))]
    assert base and len(base) == len(prog), "no files: run with --make first"
    if args.files:
        base, prog = base[:args.files], prog[:args.files]
    import torch
    from feartracker_amd import JpegDecoder, JpegStore
    n, repeats = len(prog), 5
    res = {"files": n, "width": W, "height": H, "quality": QUALITY, "cpus_available": len(os.sched_getaffinity(0)), "repeats": repeats}

    probe = JpegDecoder(device=0, threads=16, progressive=True)
    transcodes = [probe.to_baseline(b) for b in prog]
    assert all(isinstance(t, bytes) for t in transcodes)
    res["transcode_ms_per_file"] = spread([t / n for t in run_seconds(lambda: [probe.to_baseline(b) for b in prog], repeats)], 1e3)

    stores = {"progressive": JpegStore(device=0, threads=16, progressive=True), "baseline": JpegStore(device=0, threads=16)}
    ids = {"progressive": stores["progressive"].add(prog), "baseline": stores["baseline"].add(base)}
    assert set(stores["progressive"].kinds) == {"scan"}
    res["subsequence_bytes"] = stores["baseline"].subsequence_bytes
    res["bytes_per_file"] = {
        "progressive_file": round(sum(map(len, prog)) / n, 1), "baseline_file": round(sum(map(len, base)) / n, 1),
        "transcode": round(sum(map(len, transcodes)) / n, 1),
        "resident_progressive": dict({k: round(v / n, 1) for k, v in stores["progressive"].resident.items()}, total=round(stores["progressive"].nbytes / n, 1)),
        "resident_baseline": dict({k: round(v / n, 1) for k, v in stores["baseline"].resident.items()}, total=round(stores["baseline"].nbytes / n, 1)),
        "decoded": 3 * H * W}
    perm = np.random.default_rng(17).permutation(n)
    heights = stores["baseline"].shape(ids["baseline"][perm])[:, 0].astype(np.int64)
    y0 = np.random.default_rng(29).integers(0, heights - heights // 4 + 1)
    rows = np.stack([y0, y0 + heights // 4], axis=1)
    plain = JpegDecoder(device=0, threads=16)

    def whole(kind):
        frames = stores[kind].decode(ids[kind][perm], check=True)
        torch.cuda.synchronize()
        return frames

    def bands(kind):
        frames = stores[kind].decode_rows(ids[kind][perm], rows, check=True)
        torch.cuda.synchronize()
        return frames

    def decoder(dec, blobs):
        frames = dec.decode(blobs)
        torch.cuda.synchronize()
        return frames

    # the same coefficients, so the same bytes: checked before anything is timed, which also warms every shape
    want = whole("baseline")
    assert all(torch.equal(x, y) for x, y in zip(whole("progressive"), want)), "the transcodes decode differently from the baseline twins"
    for x, y, z, (a, b) in zip(bands("progressive"), bands("baseline"), want, rows.tolist()):
        assert torch.equal(x[a:b], z[a:b]) and torch.equal(y[a:b], z[a:b]), "decode_rows differs from decode"
    del want
    straight = decoder(plain, base)
    assert all(torch.equal(x, y) for x, y in zip(decoder(probe, prog), straight)), "JpegDecoder(progressive=True) differs from the twins' frames"
    del straight
    res["frames_equal_twins"] = True

    res["decode_ms_per_call"], res["decode_rows_ms_per_call"] = {}, {}
    for kind in ("baseline", "progressive"):
        res["decode_ms_per_call"][kind] = spread(run_seconds(lambda: whole(kind), repeats), 1e3)
        res["decode_rows_ms_per_call"][kind] = dict(spread(run_seconds(lambda: bands(kind), repeats), 1e3), rows_asked=H // 4)
    res["decoder_fps"] = {"progressive": spread([n / t for t in run_seconds(lambda: decoder(probe, prog), repeats)], digits=1),
                          "baseline": spread([n / t for t in run_seconds(lambda: decoder(plain, base), repeats)], digits=1)}

    def add_once(kind):
        fresh = JpegStore(device=0, threads=16, progressive=kind == "progressive")
        t0 = time.perf_counter()
        fresh.add(prog if kind == "progressive" else base)
        t = time.perf_counter() - t0
        fresh.close()
        return t
    res["add_files_per_s"] = {}
    for kind in ("baseline", "progressive"):
        add_once(kind)
        res["add_files_per_s"][kind] = spread([n / add_once(kind) for _ in range(repeats)], digits=1)
    res["add_files_per_s"]["ratio"] = round(res["add_files_per_s"]["progressive"]["median"] / res["add_files_per_s"]["baseline"]["median"], 3)
    for s in stores.values():
        s.close()
    probe.close()
    plain.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
