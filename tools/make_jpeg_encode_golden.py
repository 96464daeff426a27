"""Writes tests/golden/jpeg_encode.npz: RGB frames, their parameters and the files Pillow (libjpeg-turbo) writes for them — the fixture
`jpeg_encode.jpeg_encode_host` and `fear_jpeg_encode_u8` are held to ("Writing JPEG files").  Needs Pillow.

    python tools/make_jpeg_encode_golden.py

The file holds `names`, `quality`, `restart_rows` and `frames` (the name of its frame) per case, `in_<frame>` (H, W, 3) uint8 per frame,
`file_<name>` uint8 per case, and the four
standard Huffman tables as every one of those files carries them: `dht_<class><id>_counts` (16,) and `dht_<class><id>_values`."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

SIZES = ((1, 1), (5, 7), (8, 8), (16, 16), (9, 17), (40, 23), (23, 40), (31, 33), (70, 50))          # (H, W)
QUALITIES = (1, 10, 50, 75, 90, 100)
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_encode.npz")


def cases(rng):
    """(name, frame, quality, restart_rows, name of the frame).  Every size at every quality; every third size is a smooth frame, the others noise."""
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


def pillow_file(frame, quality, restart_rows):
    buf = io.BytesIO()
    extra = dict(restart_marker_rows=int(restart_rows)) if restart_rows else {}
    Image.fromarray(np.ascontiguousarray(frame)).save(buf, "JPEG", quality=int(quality), **extra)
    return buf.getvalue()


def huffman_tables(data):
    tables, p = {}, 2
    while data[p + 1] != 0xDA:
        length = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xC4:
            seg = data[p + 4:p + 2 + length]
            tables[f"dht_{seg[0] >> 4}{seg[0] & 15}_counts"] = np.frombuffer(seg[1:17], dtype=np.uint8)
            tables[f"dht_{seg[0] >> 4}{seg[0] & 15}_values"] = np.frombuffer(seg[17:], dtype=np.uint8)
        p += 2 + length
    return tables


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    made = cases(np.random.default_rng(20241019))
    arrays = dict(names=np.array([c[0] for c in made]), quality=np.array([c[2] for c in made], dtype=np.int32),
                  restart_rows=np.array([c[3] for c in made], dtype=np.int32), frames=np.array([c[4] for c in made]))
    for name, frame, quality, restart_rows, frame_name in made:
        data = pillow_file(frame, quality, restart_rows)
        arrays[f"in_{frame_name}"] = frame
        arrays[f"file_{name}"] = np.frombuffer(data, dtype=np.uint8)
    arrays.update(huffman_tables(data))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
