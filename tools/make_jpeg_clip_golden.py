"""Writes tests/golden/jpeg_clip.npz: two short clips as JPEG files, for the tests that track on frames kept in a `JpegStore`
(tests/test_multi_tracker_store_gpu.py; DESIGN.md section 14, "Rows from the device").  Needs Pillow; the tests read the fixture only.

    python tools/make_jpeg_clip_golden.py

Both clips come from tests/clipgen.py's generator (`demo_clip`: the geometry of the reference demo, a tall object that moves towards
and partly out of the right frame edge).
    clip 0   12 frames of 480 x 256, every 20th frame of the demo clip, so that the object reaches the edge; 4:2:0 with a restart
             interval of one MCU row
    clip 1   12 frames of 247 x 197 (odd sizes: partial MCUs on both axes), a window of every 6th frame; 4:4:4 without restarts
The file holds per clip c `n_c` (the frame count), `jpg_c_t` (frame t's file) and `boxes_c` ((n, 4) xywh, the generator's boxes in the
clip's coordinates: the annotations of a validation sequence)."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clipgen import demo_clip  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_clip.npz")
WINDOW = (100, 30, 247, 197)               # clip 1: x, y, w, h inside the demo frame
QUALITY = 60


def encode(rgb, subsampling, **options):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=QUALITY, subsampling=subsampling, **options)
    return buf.getvalue()


def main():
    frames, boxes = demo_clip(221)
    x, y, w, h = WINDOW
    clips = [
        ([encode(frames[t], 2, restart_marker_rows=1) for t in range(0, 221, 20)], boxes[0:221:20]),
        ([encode(np.ascontiguousarray(frames[t][y:y + h, x:x + w]), 0) for t in range(0, 72, 6)], boxes[0:72:6] - np.array([x, y, 0, 0])),
    ]
    arrays = {}
    for c, (files, ann) in enumerate(clips):
        assert len(files) == 12 == len(ann)
        arrays[f"n_{c}"] = np.int64(len(files))
        arrays[f"boxes_{c}"] = ann.astype(np.int64)
        for t, data in enumerate(files):
            arrays[f"jpg_{c}_{t}"] = np.frombuffer(data, dtype=np.uint8)
    np.savez(OUT, **arrays)                  # (JPEG bytes do not compress)
    print(OUT, os.path.getsize(OUT), "bytes; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
