"""Crop and warp geometry over rows, the 8-bit crop and warpAffine restatements, and the targets."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ..geometry import _linear_taps
from .records import CONTEXT_SIZE, SCORE_SIZE, SEARCH_SIZE, TOTAL_STRIDE


def _extend(box: np.ndarray, offset) -> np.ndarray:
    """extend_bbox over rows: [x - w o, y - h o, w (1 + o + o), h (1 + o + o)] truncated to int32 (utils.py:29-57)."""
    x, y, w, h = box.T
    o = np.asarray(offset, dtype=np.float64)
    grow = (1.0 + o) + o
    return np.stack([x - w * o, y - h * o, w * grow, h * grow], axis=1).astype(np.int32)


def _ensure(box: np.ndarray, h, w) -> np.ndarray:
    """ensure_bbox_boundaries over rows (utils.py:60-71)."""
    x, y, bw, bh = box.T
    x_lo = np.minimum(np.maximum(0, x), w)
    y_lo = np.minimum(np.maximum(0, y), h)
    x_hi = np.minimum(np.maximum(0, x_lo + bw), w)
    y_hi = np.minimum(np.maximum(0, y_lo + bh), h)
    return np.stack([x_lo, y_lo, x_hi - x_lo, y_hi - y_lo], axis=1).astype(np.int32)


def _box_in_crop(box: np.ndarray, ctx: np.ndarray, size: int) -> np.ndarray:
    """get_extended_crop's box output over rows: the box in the padded context, then albumentations' coco Resize (float64)."""
    rel = np.stack([box[:, 0] - ctx[:, 0], box[:, 1] - ctx[:, 1], box[:, 2], box[:, 3]], axis=1)
    cw, ch = ctx[:, 2].astype(np.float64), ctx[:, 3].astype(np.float64)
    b = _ensure(rel, ctx[:, 3], ctx[:, 2])
    x_min, y_min = np.clip(b[:, 0] / cw, 0.0, 1.0), np.clip(b[:, 1] / ch, 0.0, 1.0)
    x_max, y_max = np.clip((b[:, 0] + b[:, 2]) / cw, 0.0, 1.0), np.clip((b[:, 1] + b[:, 3]) / ch, 0.0, 1.0)
    x_min, x_max, y_min, y_max = x_min * size, x_max * size, y_min * size, y_max * size
    return np.stack([x_min, y_min, x_max - x_min, y_max - y_min], axis=1)


def jittered_crop(jitter: np.ndarray, scale_shift_box=(128, 128, 256, 256), img: int = CONTEXT_SIZE) -> np.ndarray:
    """BBoxCropWithOffsets.get_params_dependent_on_targets (aug.py:88-107) over rows: the modified crop box, float64 xywh."""
    x, y, w, h = scale_shift_box
    sx, sy, tx, ty = jitter.T
    nx = np.maximum(0, x - sx * w / 2 + tx)
    ny = np.maximum(0, y - sy * h / 2 + ty)
    nw = np.minimum(img, nx + w + sx * w) - nx
    nh = np.minimum(img, ny + h + sy * h) - ny
    return np.stack([nx, ny, nw, nh], axis=1)


def apply_to_bbox(box: np.ndarray, crop: np.ndarray, size: int = SEARCH_SIZE) -> np.ndarray:
    """BBoxCropWithOffsets.apply_to_bbox (aug.py:109-129) over rows, int truncation at the end: int64 xywh."""
    nx = (box[:, 0] - crop[:, 0]) * size / crop[:, 2]
    ny = (box[:, 1] - crop[:, 1]) * size / crop[:, 3]
    nw = box[:, 2] * size / crop[:, 2]
    nh = box[:, 3] * size / crop[:, 3]
    nw = np.where(nx < 0, nw + nx, nw)
    nx = np.where(nx < 0, 0.0, nx)
    nh = np.where(ny < 0, nh + ny, nh)
    ny = np.where(ny < 0, 0.0, ny)
    nw = np.minimum(size, nx + nw) - nx
    nh = np.minimum(size, ny + nh) - ny
    return np.trunc(np.stack([nx, ny, nw, nh], axis=1)).astype(np.int64)


def warp_matrix(crop: np.ndarray, out_size: int = SEARCH_SIZE) -> np.ndarray:
    """affine_crop's forward matrices (aug.py:131-143) over rows: (B, 2, 3) [[a, 0, c], [0, b, d]], a = (out - 1) / w, c = -a x."""
    a = (out_size - 1) / crop[:, 2]
    b = (out_size - 1) / crop[:, 3]
    c = -a * crop[:, 0]
    d = -b * crop[:, 1]
    z = np.zeros_like(a)
    return np.stack([np.stack([a, z, c], axis=1), np.stack([z, b, d], axis=1)], axis=1)


def invert_affine(M: np.ndarray) -> np.ndarray:
    """cv2.warpAffine's inversion of a forward matrix (imgwarp.cpp, no WARP_INVERSE_MAP), in its float64 order of operations.
    M (..., 2, 3) -> (..., 2, 3)."""
    M = np.asarray(M, dtype=np.float64)
    m0, m1, m2, m3, m4, m5 = (M[..., i // 3, i % 3] for i in range(6))
    D = m0 * m4 - m1 * m3
    with np.errstate(divide="ignore"):
        D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
    a11, a22 = m4 * D, m0 * D
    i0, i1, i3, i4 = a11, m1 * -D, m3 * -D, a22
    b1 = -i0 * m2 - i1 * m5
    b2 = -i3 * m2 - i4 * m5
    return np.stack([np.stack([i0, i1, b1], axis=-1), np.stack([i3, i4, b2], axis=-1)], axis=-2)


def _bilinear_tab() -> np.ndarray:
    """initInterTab2D(INTER_LINEAR, fixed point) -> (1024, 4) int64 weights (w00, w01, w10, w11) of entry fy * 32 + fx: the
    products (1 - fy/32 | fy/32) (1 - fx/32 | fx/32) * 32768 are exact; entry 0's 32768 saturates to 32767 and the table's sum
    correction puts the missing 1 on its (1, 1) weight."""
    f = np.arange(32, dtype=np.int64)
    fy, fx = np.meshgrid(f, f, indexing="ij")
    tab = np.stack([(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx], axis=-1).reshape(1024, 4) * 32
    tab[0] = (32767, 0, 0, 1)
    return tab


_TAB = _bilinear_tab()


def remap_affine_u8(src: np.ndarray, Minv: np.ndarray, dsize: Tuple[int, int]) -> np.ndarray:
    """cv2.warpAffine(src, M, dsize, INTER_LINEAR, BORDER_CONSTANT, 0) for uint8 (H, W, C), given the INVERTED matrix: OpenCV
    4.x's fixed point (AB_BITS 10, INTER_BITS 5, round_delta 16, row term and column delta rounded separately, half to even), the
    15-bit weight table, `(sum + (1 << 14)) >> 15`; taps outside the source read 0."""
    out_w, out_h = dsize
    m0, m1, m2, m3, m4, m5 = (float(Minv[i // 3][i % 3]) for i in range(6))
    ys = np.arange(out_h, dtype=np.float64)
    xs = np.arange(out_w, dtype=np.float64)
    X0 = np.rint((m1 * ys + m2) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m4 * ys + m5) * 1024).astype(np.int64) + 16
    adelta = np.rint(m0 * xs * 1024).astype(np.int64)
    bdelta = np.rint(m3 * xs * 1024).astype(np.int64)
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy = X >> 5, Y >> 5
    w = _TAB[(Y & 31) * 32 + (X & 31)]                                     # (out_h, out_w, 4)
    h, wd = src.shape[:2]
    img = src.reshape(h, wd, -1).astype(np.int64)
    acc = np.zeros((out_h, out_w, img.shape[2]), dtype=np.int64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + oy, sx + ox
        inside = (xx >= 0) & (xx < wd) & (yy >= 0) & (yy < h)
        v = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, wd - 1)] * inside[..., None]
        acc += v * w[..., k:k + 1]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8).reshape((out_h, out_w) + src.shape[2:])


def warp_affine_u8(src: np.ndarray, M: np.ndarray, dsize: Tuple[int, int]) -> np.ndarray:
    """cv2.warpAffine(src, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0) on uint8 (forward M)."""
    return remap_affine_u8(src, invert_affine(M), dsize)


def crop_u8(frame: Optional[np.ndarray], pad: Sequence[int], ctx: Sequence[int], size: int) -> np.ndarray:
    """resize_bilinear_u8(copy_make_border(frame's part of ctx, pad), size, size) (geometry.get_extended_crop's pixels) computed
    per tap, without the padded context: what the device kernels compute.  `frame` None: a frame with no pixels."""
    cx, cy, cw, ch = (int(v) for v in ctx)
    fh, fw = (frame.shape[0], frame.shape[1]) if frame is not None else (0, 0)
    padv = np.asarray(pad, dtype=np.int64).reshape(3)

    def sample(ys, xs):            # (len(ys), len(xs), 3) int64 context pixels
        fy, fx = cy + ys[:, None], cx + xs[None, :]
        inside = (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)
        out = np.broadcast_to(padv, inside.shape + (3,)).copy()
        if frame is not None and inside.any():
            out[inside] = frame[np.clip(fy, 0, fh - 1), np.clip(fx, 0, fw - 1)][inside]
        return out

    if cw == size and ch == size:
        return sample(np.arange(size), np.arange(size)).astype(np.uint8)
    if cw == 2 * size and ch == 2 * size:
        e, o = np.arange(0, 2 * size, 2), np.arange(1, 2 * size, 2)
        return ((sample(e, e) + sample(e, o) + sample(o, e) + sample(o, o) + 2) >> 2).astype(np.uint8)
    ix, ax0, ax1 = _linear_taps(size, cw, clamp=True)
    iy, ay0, ay1 = _linear_taps(size, ch, clamp=False)
    ix1 = np.minimum(ix + 1, cw - 1)
    iy0, iy1 = np.clip(iy, 0, ch - 1), np.clip(iy + 1, 0, ch - 1)
    r0 = sample(iy0, ix) * ax0[None, :, None] + sample(iy0, ix1) * ax1[None, :, None]
    r1 = sample(iy1, ix) * ax0[None, :, None] + sample(iy1, ix1) * ax1[None, :, None]
    out = (((ay0[:, None, None] * (r0 >> 4)) >> 16) + ((ay1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def encode_targets(search_bbox: np.ndarray, presence: np.ndarray, r_pos: int = 2):
    """FEARBoxCoder.encode + get_regression_weight_label(bbox, 256, 16) over rows, zeros where presence == 0:
    gt_reg (B, 4, 16, 16), gt_cls (B, 1, 16, 16), gt_weight (B, 16, 16), fp32."""
    ticks = (np.arange(SCORE_SIZE) - np.floor(float(SCORE_SIZE // 2))) * TOTAL_STRIDE + SEARCH_SIZE // 2
    gx, gy = np.meshgrid(ticks, ticks)
    b = search_bbox.astype(np.float64)[:, :, None, None]
    x0, y0 = b[:, 0], b[:, 1]
    reg = np.stack([gx - x0, gy - y0, (x0 + b[:, 2]) - gx, (y0 + b[:, 3]) - gy], axis=1).astype(np.float32)
    cls = (reg.min(axis=1, keepdims=True) > 0).astype(np.float32)
    c_x = search_bbox[:, 0] + search_bbox[:, 2] // 2
    c_y = search_bbox[:, 1] + search_bbox[:, 3] // 2
    sz_x = np.floor(c_x / SEARCH_SIZE * SCORE_SIZE)
    sz_y = np.floor(c_y / SEARCH_SIZE * SCORE_SIZE)
    jj, ii = np.meshgrid(np.arange(SCORE_SIZE), np.arange(SCORE_SIZE))
    dist = np.abs(jj[None] - sz_x[:, None, None]) + np.abs(ii[None] - sz_y[:, None, None])
    wgt = (dist <= r_pos).astype(np.float32)
    keep = (np.asarray(presence) != 0).astype(np.float32)
    return reg * keep[:, None, None, None], cls * keep[:, None, None, None], wgt * keep[:, None, None]
