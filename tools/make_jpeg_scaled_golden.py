"""Writes tests/golden/jpeg_scaled.npz: what Pillow (libjpeg-turbo) decodes at 1/2, 1/4 and 1/8 size through `Image.draft` — the fixture
`jpeg_frames.jpeg_decode_host(scale=)` and `fear_jpeg_decode_scaled_u8` are held to ("Reduced-size decoding").
Needs Pillow only.

    python tools/make_jpeg_scaled_golden.py

Files: the supported files of tests/golden/jpeg_decode.npz (read, not copied: the fixture names them) and a few new ones stored with
their bytes — 4:2:2 files whose scaled chroma width is exactly 3 and exactly 2 (the threshold between fancy upsampling and replication),
a 4:2:2 file wider than 32 pixels (libjpeg turns fancy upsampling off at 1/8, which only such a file shows) and its progressive twin.
`draft` cannot force a scale above a file's smaller side, so a file x scale pair is recorded only where min(W, H) >= scale; after
`load()` the size must be (ceil(W / s), ceil(H / s)), which shows that the scale was really taken.
The file holds `names` (the new files), `jpg_i` (their bytes), `keys` ("<name>@<scale>") and per key k `px_k` (Pillow's convert("RGB"))."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_jpeg_decode_golden import content, encode          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
OUT = os.path.join(GOLDEN, "jpeg_scaled.npz")
SCALES = (2, 4, 8)


def new_files():
    rng = np.random.default_rng(20261020)
    wide = content("random", 48, 16, rng)
    return [("12x9_422_random_q90_cw3_cw2", encode(content("random", 12, 9, rng), "422", 90)),       # chroma width 3 at 1/2, 2 at 1/4
            ("24x10_422_smooth_q75_cw3", encode(content("smooth", 24, 10, rng), "422", 75)),         # chroma width 3 at 1/4, 2 at 1/8
            ("48x16_422_random_q90_wide", encode(wide, "422", 90)),                                  # chroma width 3 at 1/8: no fancy there
            ("64x40_422_smooth_q95_wide", encode(content("smooth", 64, 40, rng), "422", 95)),
            ("48x16_422_random_q90_wide_progressive", encode(wide, "422", 90, progressive=True))]


def draft_pixels(data, scale):
    """Pillow's decode at 1 / scale, or None where `draft` cannot take the scale."""
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if min(w, h) < scale:
        return None
    im.draft(im.mode, (max(1, w // scale), max(1, h // scale)))
    im.load()
    assert im.size == (-(-w // scale), -(-h // scale)), (im.size, w, h, scale)
    return np.ascontiguousarray(np.asarray(im.convert("RGB")))


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    files = []
    with np.load(os.path.join(GOLDEN, "jpeg_decode.npz")) as d:
        for i, name in enumerate(d["names"]):
            if "progressive" not in str(name):
                files.append((str(name), d[f"jpg_{i}"].tobytes()))
    made = new_files()
    arrays = dict(names=np.array([name for name, _ in made]))
    for i, (_, data) in enumerate(made):
        arrays[f"jpg_{i}"] = np.frombuffer(data, dtype=np.uint8)
    keys = []
    for name, data in files + made:
        for s in SCALES:
            px = draft_pixels(data, s)
            if px is not None:
                arrays[f"px_{len(keys)}"] = px
                keys.append(f"{name}@{s}")
    arrays["keys"] = np.array(keys)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(files), "+", len(made), "files;", len(keys), "file x scale pairs; Pillow", Image.__version__,
          "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
