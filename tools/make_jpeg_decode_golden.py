"""Writes tests/golden/jpeg_decode.npz: small JPEG files and what Pillow (libjpeg-turbo) decodes them to — the fixture
`jpeg_frames.jpeg_decode_host` and `fear_jpeg_decode_u8` are held to.  Needs Pillow.

    python tools/make_jpeg_decode_golden.py

Main grid: ten sizes (W, H) by four modes, each pair once; content (random | smooth), quality (30 | 75 | 95 | 100) and option (plain |
restart_marker_blocks=3 | optimize) cycle across the cases (16 x 16 4:2:0 is a plain file: the malformed-data tests cut and flip it).
Extra cases: 4:2:0 with restart_marker_rows=1, a file with COM and APP1 segments, 64 x 48 4:4:4 random at quality 100, and one
progressive file (unsupported: its pixels are Pillow's all the same, for the fallback).  The file holds `names`, and per case i `jpg_i` (the file's bytes) and `px_i` (Pillow's convert("RGB"), (H, W, 3) uint8)."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

SIZES = ((1, 1), (7, 5), (8, 8), (16, 16), (17, 23), (33, 31), (40, 24), (15, 50), (64, 48), (80, 72))
MODES = ("444", "422", "420", "gray")
QUALITIES = (30, 75, 95, 100)
OPTIONS = ({}, {"restart_marker_blocks": 3}, {"optimize": True})
OPTION_NAMES = ("plain", "rst3", "opt")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_decode.npz")


def content(kind, w, h, rng):
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + 2 * yy) * 5) % 256], axis=-1).astype(np.uint8)


def encode(rgb, mode, quality, **options):
    buf = io.BytesIO()
    if mode == "gray":
        Image.fromarray(rgb).convert("L").save(buf, format="JPEG", quality=quality, **options)
    else:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[mode], **options)
    return buf.getvalue()


def pillow_pixels(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def cases():
    rng = np.random.default_rng(20240925)
    out, i = [], 0
    for w, h in SIZES:
        for mode in MODES:
            kind, quality, opt = ("random", "smooth")[i % 2], QUALITIES[(i // 2) % 4], (i + 1) % 3
            out.append((f"{w}x{h}_{mode}_{kind}_q{quality}_{OPTION_NAMES[opt]}", encode(content(kind, w, h, rng), mode, quality, **OPTIONS[opt])))
            i += 1
    out.append(("40x24_420_random_q75_rstrows1", encode(content("random", 40, 24, rng), "420", 75, restart_marker_rows=1)))
    out.append(("33x31_422_smooth_q75_com_app1", encode(content("smooth", 33, 31, rng), "422", 75, comment=b"a comment segment",
                                                          exif=b"Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08\x00\x00\x00\x00\x00\x00")))
    out.append(("64x48_444_random_q100_plain2", encode(content("random", 64, 48, rng), "444", 100)))
    out.append(("33x31_420_smooth_q75_progressive", encode(content("smooth", 33, 31, rng), "420", 75, progressive=True)))
    return out


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    made = cases()
    arrays = dict(names=np.array([name for name, _ in made]))
    for i, (_, data) in enumerate(made):
        arrays[f"jpg_{i}"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"px_{i}"] = pillow_pixels(data)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
