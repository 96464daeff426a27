"""Plumbing shared by the tests of the store's bands of rows (test_jpeg_rows_host, test_jpeg_rows_gpu): the bands and windows of an
image that the tests walk, and the frames and pairs of the builder tests.  A plain module, imported by name as jpegdec is."""
import numpy as np

import jpeghuff


def all_bands(mcus_y):
    return [(a, b) for a in range(mcus_y) for b in range(a + 1, mcus_y + 1)]


def slices(hd, ref, a, b):
    """The rows of an image's coefficients that belong to the MCU rows a .. b)."""
    return [ref[c][a * (hd.v[0] if c == 0 else 1):b * (hd.v[0] if c == 0 else 1)] for c in range(len(ref))]


def windows(H, mcu_h):
    """Every MCU-aligned window of an image, each moved by one row at either end, the first row alone, the last alone, the whole."""
    edges = sorted(set(range(0, H, mcu_h)) | {H})
    out = {(0, 1), (H - 1, H), (0, H)}
    for i, y0 in enumerate(edges[:-1]):
        for y1 in edges[i + 1:]:
            for d0, d1 in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= y0 + d0 < y1 + d1 <= H:
                    out.add((y0 + d0, y1 + d1))
    return sorted(out)


def frames_and_pairs():
    """Five frames of three sizes and eight pairs: context boxes inside, partly outside and wholly outside their frames, a pair without
    presence, frame 2 shared by several pairs, frame 4 used by none."""
    names = ("80x72_420", "64x48_444_random_q100_plain2", "256x192_420_noisygradient_q90", "80x72_422", "64x48_gray")
    frames = [np.ascontiguousarray(next(c for c in jpeghuff.supported() if c[0].startswith(n))[2]) for n in names]
    pairs = np.array([
        # t_frame, box xywh,         s_frame, box xywh,          presence
        [0, 30, 28, 16, 12,          1, 20, 16, 18, 14,          1],
        [2, 100, 80, 40, 30,         2, 110, 90, 10, 8,          1],
        [0, 10, 60, 20, 20,          3, 60, 2, 14, 10,           1],     # partly outside at the bottom | at the top
        [1, 5, 5, 10, 10,            2, 120, 92, 8, 6,           0],     # presence == 0
        [3, 30, 300, 12, 12,         0, 30, -200, 12, 12,        1],     # wholly outside: below | above
        [2, 128, 96, 20, 20,         2, 60, 94, 8, 6,            1],
        [0, 1, 1, 6, 6,              1, 50, 40, 10, 6,           1],
        [3, 70, 60, 8, 9,            3, 2, 50, 16, 20,           1],
    ], dtype=np.float64)
    return frames, pairs
