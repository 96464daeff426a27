"""Writes tests/golden/jpeg_entropy.npz: seven 256 x 192 JPEG files, one of 128 x 96, and what Pillow (libjpeg-turbo) decodes them to — files long enough
for the device's Huffman stage (fear_jpeg_huffman) to walk several sequences of 256 subsequences, in every sampling
mode, with standard and optimised tables, with and without restart markers.  Needs Pillow; the tests do not.

    python tools/make_jpeg_entropy_golden.py

The file has the layout of jpeg_decode.npz: `names`, and per case i `jpg_i` (the file's bytes) and `px_i` (Pillow's convert("RGB"))."""
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_jpeg_decode_golden import encode, pillow_pixels          # noqa: E402

W, H = 256, 192
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_entropy.npz")


def cases():
    rng = np.random.default_rng(20241018)
    yy, xx = np.mgrid[0:H, 0:W]
    gradient = np.stack([xx, yy * 255 // (H - 1), (xx + 2 * yy) // 3 % 256], axis=-1)
    noisy = np.clip(gradient + rng.integers(-12, 13, gradient.shape), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, (H // 2, W // 2, 3), dtype=np.uint8)   # at full size this one file would be a fifth of a megabyte
    gray = np.clip(96 + rng.normal(0, 40, (H, W, 1)), 0, 255).astype(np.uint8).repeat(3, axis=2)
    flat = np.broadcast_to(np.array([201, 17, 94], dtype=np.uint8), (H, W, 3)).copy()
    return [("256x192_420_noisygradient_q90", encode(noisy, "420", 90)),
            ("256x192_420_noisygradient_q50_opt", encode(noisy, "420", 50, optimize=True)),
            ("256x192_444_noisygradient_q95", encode(noisy, "444", 95)),
            ("256x192_422_noisygradient_q75_opt", encode(noisy, "422", 75, optimize=True)),
            ("256x192_gray_noise_q90", encode(gray, "gray", 90)),
            ("256x192_gray_noise_q90_rst8", encode(gray, "gray", 90, restart_marker_blocks=8)),
            ("256x192_420_flat_q90", encode(flat, "420", 90)),
            ("128x96_444_random_q100", encode(noise, "444", 100))]


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    made = cases()
    arrays = dict(names=np.array([name for name, _ in made]))
    for i, (name, data) in enumerate(made):
        arrays[f"jpg_{i}"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"px_{i}"] = pillow_pixels(data)
        print(name, len(data), "bytes")
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
