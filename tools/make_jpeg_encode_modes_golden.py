"""Writes tests/golden/jpeg_encode_modes.npz: frames, their parameters and the files Pillow (libjpeg-turbo) writes for them in each of
the four layouts `JpegEncoder(subsampling=...)` knows — the fixture `jpeg_encode.jpeg_encode_host(..., subsampling=m)` and
`fear_jpeg_encode_u8` are held to ("Writing JPEG files").  Needs Pillow.  tools/make_jpeg_encode_golden.py and
its jpeg_encode.npz are the 4:2:0 fixture of the first encoder and stay as they are.

    python tools/make_jpeg_encode_modes_golden.py

The file holds `names`, `modes`, `quality`, `restart_rows`, `frames` (the name of its frame) and `plane` per case, `in_<frame>` (H, W, 3)
uint8 per frame, and the cases' files one behind the other in `files` (uint8), case k's at `file_at[k]:file_at[k + 1]` (one array, not
one per case: a member of the archive costs more than a small file).  A case's input is its frame, or, where `plane` is not -1, that channel of it as an
(H, W) frame: the gray cases, except `gray_rgb_*`, whose (H, W, 3) frames go through `convert("L")`."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

SIZES = ((1, 1), (5, 7), (8, 8), (16, 16), (9, 17), (40, 23), (23, 40), (31, 33), (70, 50))          # (H, W)
QUALITIES = (1, 50, 90, 100)
MODES = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0, "gray": None}               # the name -> Pillow's subsampling=
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_encode_modes.npz")


def colour_cases(rng):
    """(name, frame, quality, restart_rows, name of the frame): make_jpeg_encode_golden.py's cases at four qualities.  Every third size
    is a smooth frame, the others noise."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(xx * 9 + yy * 3) % 256, (xx * 2 + yy * 11 + 40) % 256, (255 - xx * 5 - yy * 7) % 256], axis=-1).astype(np.uint8)
        frame = smooth if k % 3 == 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for q in QUALITIES:
            out.append((f"{h}x{w}_q{q}", frame, q, 0, f"{h}x{w}"))
    noise = rng.integers(0, 256, (56, 40, 3), dtype=np.uint8)
    out.append(("noise_q100", noise, 100, 0, "noise"))                    # stuffed FF 00 bytes, blocks without an EOB
    out.append(("noise_q10", noise, 10, 0, "noise"))                      # ZRL symbols
    yy, xx = np.mgrid[0:16, 0:64]
    gray = lambda p: np.repeat(p.astype(np.uint8)[..., None], 3, axis=-1)
    out.append(("columns_q100", gray(((xx // 8) & 1) * 255), 100, 0, "columns"))   # a DC difference of 2040: the 11th category
    yy, xx = np.mgrid[0:16, 0:16]
    out.append(("checker_q100", gray(((yy + xx) & 1) * 255), 100, 0, "checker"))   # a file larger than the raw pixels
    out.append(("restart1_31x33", rng.integers(0, 256, (31, 33, 3), dtype=np.uint8), 75, 1, "restart1"))
    out.append(("restart2_70x50", rng.integers(0, 256, (70, 50, 3), dtype=np.uint8), 90, 2, "restart2"))
    return out


def pillow_file(frame, quality, restart_rows, mode):
    buf = io.BytesIO()
    extra = dict(restart_marker_rows=int(restart_rows)) if restart_rows else {}
    if MODES[mode] is not None:
        extra["subsampling"] = MODES[mode]
    image = Image.fromarray(np.ascontiguousarray(frame))
    if mode == "gray" and frame.ndim == 3:
        image = image.convert("L")
    image.save(buf, "JPEG", quality=int(quality), **extra)
    return buf.getvalue()


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    colour = colour_cases(np.random.default_rng(20241020))
    made = []                                                              # (name, mode, frame, quality, restart_rows, frame's name, plane)
    for mode in MODES:
        tag = mode.replace(":", "")
        for name, frame, quality, rows, frame_name in colour:
            if mode == "gray":                                             # one plane: the green channel of the colour case's frame
                made.append((f"gray_{name}", mode, frame, quality, rows, frame_name, 1))
            else:
                made.append((f"{tag}_{name}", mode, frame, quality, rows, frame_name, -1))
    by_name = {c[0]: c for c in colour}
    for name in ("40x23_q90", "restart1_31x33"):                           # gray from RGB frames, through convert("L")
        _, frame, quality, rows, frame_name = by_name[name]
        made.append((f"gray_rgb_{name}", "gray", frame, quality, rows, frame_name, -1))
    arrays = dict(names=np.array([c[0] for c in made]), modes=np.array([c[1] for c in made]),
                  quality=np.array([c[3] for c in made], dtype=np.int32), restart_rows=np.array([c[4] for c in made], dtype=np.int32),
                  frames=np.array([c[5] for c in made]), plane=np.array([c[6] for c in made], dtype=np.int32))
    files = []
    for name, mode, frame, quality, rows, frame_name, plane in made:
        arrays[f"in_{frame_name}"] = frame
        source = frame if plane < 0 else np.ascontiguousarray(frame[..., plane])
        files.append(np.frombuffer(pillow_file(source, quality, rows, mode), dtype=np.uint8))
    arrays["files"] = np.concatenate(files)
    arrays["file_at"] = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
