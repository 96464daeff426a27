"""The demo loop on the device: JPEG frames in, one target tracked, its box drawn, JPEG frames (or one Motion-JPEG AVI) out.

    python tools/track_demo.py FRAMES_DIR X Y W H --out OUT_DIR            # numbered .jpg files
    python tools/track_demo.py FRAMES_DIR X Y W H --out clip.avi --fps 25  # one .avi
    python tools/track_demo.py FRAMES_DIR X Y W H --out OUT_DIR --subsampling 4:4:4

FRAMES_DIR holds baseline JPEG files, read in sorted order; X Y W H is the target's box in the first frame.  Every stage runs on the GPU:
`JpegDecoder` -> `FEARMultiTracker.submit` -> `FEARMultiTracker.draw` -> `JpegEncoder`; only the files' bytes come back to the host.  The
counterpart of the reference's demo_video.py without cv2, Pillow or a codec."""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("frames_dir")
    ap.add_argument("box", type=int, nargs=4, metavar=("X", "Y", "W", "H"))
    ap.add_argument("--out", required=True, help="a directory for numbered .jpg files, or a path ending in .avi")
    ap.add_argument("--fps", type=float, default=25.0)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", default="4:2:0", choices=("4:2:0", "4:2:2", "4:4:4", "gray"),
                    help="the files' layout: 4:4:4 keeps the outline's colour, 4:2:0 (the default) halves its chroma both ways")
    ap.add_argument("--optimize", action="store_true", help="per-file Huffman tables, built on the device: smaller files, equal pixels")
    ap.add_argument("--thickness", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="frames decoded and encoded per call")
    ap.add_argument("--weights", default=None)
    args = ap.parse_args()
    from feartracker_amd import (DEFAULT_TRACKING_CONFIG, DEFAULT_WEIGHTS, FEARMultiTracker, FEARNetHIP, JpegDecoder, JpegEncoder,
                                 draw_boxes, write_mjpeg_avi)
    paths = sorted(glob.glob(os.path.join(args.frames_dir, "*.jpg")) + glob.glob(os.path.join(args.frames_dir, "*.jpeg")))
    if len(paths) < 2:
        raise SystemExit("the directory needs at least two .jpg frames")
    net = FEARNetHIP(args.weights or DEFAULT_WEIGHTS, device=0, max_batch=8)
    tracker = FEARMultiTracker(net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    decoder, encoder = JpegDecoder(device=0), JpegEncoder(0, quality=args.quality, subsampling=args.subsampling, optimize=args.optimize)
    files, started = [], False
    for at in range(0, len(paths), args.batch):
        frames = decoder.decode(paths[at:at + args.batch])
        for frame in frames:
            if not started:
                tracker.add(frame, np.array([args.box]), stream=0)
                started = True
                draw_boxes(frame, np.array([args.box], dtype=np.int32), thickness=args.thickness)       # the box it was given
            else:
                tracker.submit([frame])
                tracker.draw([frame], thickness=args.thickness)
        files += encoder.encode(frames).result()
    decoder.close()
    if args.out.lower().endswith(".avi"):
        write_mjpeg_avi(args.out, files, args.fps)
    else:
        os.makedirs(args.out, exist_ok=True)
        for k, data in enumerate(files):
            with open(os.path.join(args.out, f"frame{k:05d}.jpg"), "wb") as fh:
                fh.write(data)
    print(f"{len(files)} frames, {sum(map(len, files))} bytes -> {args.out}")


if __name__ == "__main__":
    main()
