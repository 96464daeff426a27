"""Writes tests/golden/jpeg_encode_optimize.npz: frames, their parameters and the files Pillow (libjpeg-turbo) writes for them with
`optimize=True` — the fixture `jpeg_encode.jpeg_encode_host(..., optimize=True)` and `JpegEncoder(optimize=True)` are held to (DESIGN.md
section 14, "Per-file Huffman tables").  Needs Pillow.

    python tools/make_jpeg_encode_optimize_golden.py

The file's form is that of jpeg_encode_modes.npz: `names`, `modes`, `quality`, `restart_rows`, `frames` (the name of its frame) and
`plane` per case, `in_<frame>` per frame, and the cases' files one behind the other in `files`, case k's at `file_at[k]:file_at[k + 1]`.
A gray case with `plane` -1 and an (H, W, 3) frame goes through `convert("L")`; the `limit` frame is (H, W) itself.

The general cases cross the four layouts with eight frames.  The `limit` case forces Adjust_BITS: a 1024 x 2056 gray picture whose
blocks are flat but for 20 kinds of block `128 + amplitude x (one DCT basis function)`, each of which quantises to a single AC
coefficient and so to one (run, size) symbol; the kinds' block counts grow so that each exceeds the sum of all before it, which makes the
unlimited Huffman tree a chain of depth 21."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feartracker_amd.jpeg_frames import ZIGZAG  # noqa: E402

MODES = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0, "gray": None}               # the name -> Pillow's subsampling=
LIMIT_COUNTS = (1, 3, 3, 6, 9, 15, 24, 39, 63, 102, 165, 267, 432, 699, 1131, 1830, 2961, 4791, 7752, 12543)
LIMIT_SHAPE = (2056, 1024)                                                # (H, W): 257 x 128 blocks
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_encode_optimize.npz")


def general_cases(rng):
    """(name, (H, W, 3) frame, quality, restart_rows)"""
    def noise(h, w):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:96, 0:128]
    picture = np.stack([xx * 2, yy * 2 + 30, (xx + yy)], axis=-1) + rng.integers(-12, 13, (96, 128, 3))    # gradients plus noise
    big = noise(50, 70)
    return [("1x1", noise(1, 1), 75, 0), ("8x8", noise(8, 8), 75, 0), ("13x17", noise(13, 17), 85, 0),
            ("flat16", np.full((16, 16, 3), 77, dtype=np.uint8), 75, 0),                  # one DC symbol and EOB only
            ("restart1_31x33", noise(31, 33), 75, 1), ("noise_q100", big, 100, 0), ("noise_q1", big, 1, 0),
            ("picture_q90", np.clip(picture, 0, 255).astype(np.uint8), 90, 0)]


def limit_frame():
    """The (H, W) uint8 picture described above and the 20 (zigzag position, amplitude) kinds in the order of LIMIT_COUNTS."""
    kinds = [(k, amp) for amp in (30, 60) for k in range(1, 17)][:len(LIMIT_COUNTS)]
    H, W = LIMIT_SHAPE
    x = (2 * np.arange(8) + 1) * np.pi / 16
    frame = np.full((H // 8, W // 8, 8, 8), 128, dtype=np.uint8)
    flat = frame.reshape(-1, 8, 8)
    at = 0
    for (k, amp), count in zip(kinds, LIMIT_COUNTS):
        v, u = divmod(int(ZIGZAG[k]), 8)
        flat[at:at + count] = np.rint(128 + amp * np.cos(v * x)[:, None] * np.cos(u * x)[None, :]).astype(np.uint8)
        at += count
    return np.ascontiguousarray(frame.transpose(0, 2, 1, 3).reshape(H, W)), kinds


def pillow_file(frame, quality, restart_rows, mode):
    buf = io.BytesIO()
    extra = dict(restart_marker_rows=int(restart_rows)) if restart_rows else {}
    if MODES[mode] is not None:
        extra["subsampling"] = MODES[mode]
    image = Image.fromarray(np.ascontiguousarray(frame))
    if mode == "gray" and frame.ndim == 3:
        image = image.convert("L")
    image.save(buf, "JPEG", quality=int(quality), optimize=True, **extra)
    return buf.getvalue()


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    made = []                                                              # (name, mode, frame, quality, restart_rows, frame's name)
    for mode in MODES:
        for name, frame, quality, rows in general_cases(np.random.default_rng(20261020)):
            made.append((f"{mode.replace(':', '')}_{name}", mode, frame, quality, rows, name))
    made.append(("gray_limit", "gray", limit_frame()[0], 75, 0, "limit"))
    arrays = dict(names=np.array([c[0] for c in made]), modes=np.array([c[1] for c in made]),
                  quality=np.array([c[3] for c in made], dtype=np.int32), restart_rows=np.array([c[4] for c in made], dtype=np.int32),
                  frames=np.array([c[5] for c in made]), plane=np.full(len(made), -1, dtype=np.int32))
    files = []
    for name, mode, frame, quality, rows, frame_name in made:
        arrays[f"in_{frame_name}"] = frame
        files.append(np.frombuffer(pillow_file(frame, quality, rows, mode), dtype=np.uint8))
    arrays["files"] = np.concatenate(files)
    arrays["file_at"] = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
