"""Writes tests/golden/jpeg_roundtrip.npz: crops, qualities and what Pillow (libjpeg-turbo) returns for them after a JPEG round trip —
the fixture `train_data.jpeg_roundtrip_u8_host` and `fear_jpeg_u8` are held to.  Needs Pillow.

    python tools/make_jpeg_golden.py

The operator's libjpeg sees channel 2 as R (cv2 reads albumentations' RGB crop as BGR), so Pillow is fed the channel-reversed crop and
its result is reversed back.  Per size (H, W) the file holds `in_HxW` (contents, H, W, 3) and `out_HxW` (contents, qualities, H, W, 3),
with `contents` (names) and `qualities` beside them."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

SIZES = ((16, 16), (16, 32), (48, 32))
QUALITIES = (50, 51, 75, 90, 99, 100)
CONTENTS = ("random", "constant", "ramp_h", "ramp_v", "checker", "saturated")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_roundtrip.npz")


def contents(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    gray = lambda p: np.repeat(p.astype(np.uint8)[..., None], 3, axis=-1)
    ramp_h = np.stack([xx * 255 // (w - 1), 255 - xx * 255 // (w - 1), xx * 128 // (w - 1) + 64], axis=-1).astype(np.uint8)
    ramp_v = np.stack([yy * 255 // (h - 1), yy * 128 // (h - 1), 255 - yy * 255 // (h - 1)], axis=-1).astype(np.uint8)
    # 8 x 8 blocks at 0 and 255 side by side, one channel inverted: the inverse DCT overshoots on both sides of every edge
    sat = gray((((yy // 8) + (xx // 8)) & 1) * 255)
    sat[..., 1] = 255 - sat[..., 1]
    sat[4:12, 4:12] = (255, 0, 255)                      # and an edge inside a block
    return dict(random=rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
                constant=np.broadcast_to(np.array([201, 17, 94], dtype=np.uint8), (h, w, 3)).copy(),
                ramp_h=ramp_h, ramp_v=ramp_v, checker=gray(((yy + xx) & 1) * 255), saturated=sat)


def pillow_roundtrip(crop, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(crop[..., ::-1])).save(buf, format="JPEG", quality=int(quality), subsampling=2)
    buf.seek(0)
    return np.ascontiguousarray(np.asarray(Image.open(buf).convert("RGB"))[..., ::-1])


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    rng = np.random.default_rng(20240611)
    arrays = dict(contents=np.array(CONTENTS), qualities=np.array(QUALITIES, dtype=np.int32))
    for h, w in SIZES:
        made = contents(h, w, rng)
        crops = np.stack([made[name] for name in CONTENTS])
        arrays[f"in_{h}x{w}"] = crops
        arrays[f"out_{h}x{w}"] = np.stack([np.stack([pillow_roundtrip(c, q) for q in QUALITIES]) for c in crops])
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
