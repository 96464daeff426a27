"""GlassBlur on the host: the numpy restatement of fear_glass_u8 (include/fear_train.h), in the gather form the
kernel uses.  albumentations' defaults: sigma 0.7, max_delta 4, two iterations, mode "fast"."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .colour import _even_sides, _windows
from .photometric import philox4x32_10
from .records import GLASS_ITERATIONS, GLASS_MAX_DELTA, GLASS_WEIGHTS

__all__ = ["glass_gauss_u8", "glass_offsets", "glass_swap_u8", "glass_u8_host"]


def glass_gauss_u8(img: np.ndarray) -> np.ndarray:
    """cv2.GaussianBlur(img, ksize=(0, 0), sigmaX=0.7) on uint8 (H, W, 3): the 8-bit kernel GLASS_WEIGHTS on both axes, one rounding,
    BORDER_REFLECT_101 — BLUR_GAUSSIAN's form with other weights."""
    w = np.asarray(GLASS_WEIGHTS, dtype=np.int64)
    s = (_windows(img, len(w) // 2, "reflect").astype(np.int64) * (w[:, None] * w[None, :])).sum(axis=(-1, -2))
    return ((s + 32768) >> 16).astype(np.uint8)


def glass_offsets(H: int, W: int, key, iteration: int) -> Tuple[np.ndarray, np.ndarray]:
    """(dy, dx), each (H, W) int64 in [-4, 3]: the offsets of iteration `iteration` at every pixel (the swaps read the interior's), from
    word 0 of Philox4x32-10 at counter (w, h, 1 + iteration, 0) with the crop's key."""
    yy, xx = np.mgrid[0:H, 0:W]
    counter = np.stack([xx, yy, np.full_like(xx, 1 + iteration), np.zeros_like(xx)], axis=-1)
    word = philox4x32_10(counter, np.asarray(key))[..., 0].astype(np.int64)
    return (word & 7) - GLASS_MAX_DELTA, ((word >> 3) & 7) - GLASS_MAX_DELTA


def glass_swap_u8(x0: np.ndarray, dy: np.ndarray, dx: np.ndarray) -> np.ndarray:
    """One iteration of the swaps on (H, W, 3), as a gather.  Over the interior h in [D + 1, H - D], w in [D + 1, W - D] (D = 4), element
    n = (H - D - h) + (H - 2 D) (W - D - w), the statement is x[h, w], x[h + dy, w + dx] = x[h + dy, w + dx], x[h, w] with both right-hand
    sides read from x0.  A pixel q the second assignment reaches takes x0 of the source with the largest n that points at it — the
    smallest w, then the smallest h, among the 8 x 8 sources q - d, d in [-4, 3]; any other pixel keeps the first assignment's
    x0[q + d(q)] inside the interior and x0[q] outside."""
    H, W = x0.shape[:2]
    D = GLASS_MAX_DELTA
    yy, xx = np.mgrid[0:H, 0:W]
    interior = (yy > D) & (yy <= H - D) & (xx > D) & (xx <= W - D)
    sy, sx = np.where(interior, yy + dy, yy), np.where(interior, xx + dx, xx)
    # the interior's offsets as the kernel keeps them, dy + D in bits 0-2 and dx + D in bits 3-5, with a margin of D of "no source"
    code = np.full((H + 2 * D, W + 2 * D), 255, dtype=np.uint8)
    code[D:D + H, D:D + W] = np.where(interior, (dy + D) | ((dx + D) << 3), 255)
    found = np.zeros((H, W), dtype=bool)
    for ix in range(2 * D):                                   # sources by falling n: the first that points at q wins
        for iy in range(2 * D):
            # the source (y - (D - 1) + iy, x - (D - 1) + ix) reaches (y, x) with dy = D - 1 - iy and dx = D - 1 - ix
            hit = ~found & (code[iy + 1:iy + 1 + H, ix + 1:ix + 1 + W] == ((2 * D - 1 - iy) | ((2 * D - 1 - ix) << 3)))
            sy, sx = np.where(hit, yy - (D - 1) + iy, sy), np.where(hit, xx - (D - 1) + ix, sx)
            found |= hit
    return x0[sy, sx]


def glass_u8_host(crop_u8: np.ndarray, op) -> np.ndarray:
    """fear_glass_u8's result for one (H, W, 3) uint8 crop whose FearPhotoOp record `op` (a PHOTO_DTYPE scalar; its key is read)
    carries BLUR_GLASS: the Gaussian, two iterations of swaps, the Gaussian again."""
    v = np.asarray(crop_u8)
    _even_sides(v, "glass")
    H, W = v.shape[:2]
    v = glass_gauss_u8(v)
    for i in range(GLASS_ITERATIONS):
        v = glass_swap_u8(v, *glass_offsets(H, W, op["key"], i))
    return np.ascontiguousarray(glass_gauss_u8(v))
