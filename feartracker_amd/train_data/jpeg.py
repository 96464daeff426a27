"""ImageCompression on the host: the lossy part of a baseline JPEG round trip (libjpeg: 4:2:0, jpeg_set_quality(q, force_baseline),
islow DCT both ways, fancy upsampling), in integers.  The entropy coding is lossless and is left out.  DESIGN.md section 11 states
the contract; tests/test_jpeg_host.py holds it to Pillow's libjpeg-turbo byte for byte."""
from __future__ import annotations

from typing import Tuple

import numpy as np

JPEG_LUMA_BASE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
JPEG_CHROMA_BASE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)
# jfdctint / jidctint's constants: FIX(x) = rint(x * 2 ** 13)
_F0_298, _F0_390, _F0_541, _F0_765, _F0_899, _F1_175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1_501, _F1_847, _F1_961, _F2_053, _F2_562, _F3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def jpeg_quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_set_quality(quality, force_baseline)'s luminance and chrominance tables, (64,) int64 each in natural (row-major) order:
    scale = 5000 / quality below 50, else 200 - 2 quality; q = clamp((base scale + 50) / 100, 1, 255), integer divisions."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("a JPEG quality lies in 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (JPEG_LUMA_BASE, JPEG_CHROMA_BASE))


def _descale(x, n: int):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One pass of jfdctint over eight int64 arrays (a row's or a column's samples): rows first (scaled up by 2 ** PASS1_BITS), then
    columns (PASS1_BITS removed, the factor 8 of the DCT kept)."""
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15                       # CONST_BITS - PASS1_BITS | CONST_BITS + PASS1_BITS
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _F0_541
    out[2] = _descale(z1 + t13 * _F0_765, n)
    out[6] = _descale(z1 - t12 * _F1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F1_175
    t4, t5, t6, t7 = t4 * _F0_298, t5 * _F2_053, t6 * _F3_072, t7 * _F1_501
    z1, z2, z3, z4 = -z1 * _F0_899, -z2 * _F2_562, -z3 * _F1_961 + z5, -z4 * _F0_390 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return out


def _idct_pass(d, first: bool):
    """One pass of jidctint (islow) over eight int64 arrays: columns first, then rows with the final DESCALE by CONST_BITS +
    PASS1_BITS + 3."""
    z1 = (d[2] + d[6]) * _F0_541
    t2, t3 = z1 - d[6] * _F1_847, z1 + d[2] * _F0_765
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _F1_175
    t0, t1, t2, t3 = t0 * _F0_298, t1 * _F2_053, t2 * _F3_072, t3 * _F1_501
    z1, z2, z3, z4 = -z1 * _F0_899, -z2 * _F2_562, -z3 * _F1_961 + z5, -z4 * _F0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return [_descale(v, n) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)]


def jpeg_fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """jfdctint on level-shifted samples (..., 8, 8) -> int64 coefficients (..., 8, 8), 8 times the orthonormal DCT."""
    b = np.asarray(blocks).astype(np.int64)
    b = np.stack(_fdct_pass([b[..., i] for i in range(8)], True), axis=-1)                 # rows
    return np.stack(_fdct_pass([b[..., i, :] for i in range(8)], False), axis=-2)          # columns


def jpeg_idct_islow(coef: np.ndarray) -> np.ndarray:
    """jidctint on dequantised coefficients (..., 8, 8) -> int64 samples (..., 8, 8) before the level shift and the clamp."""
    c = np.asarray(coef).astype(np.int64)
    c = np.stack(_idct_pass([c[..., i, :] for i in range(8)], True), axis=-2)              # columns
    return np.stack(_idct_pass([c[..., i] for i in range(8)], False), axis=-1)             # rows


def _jpeg_ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """jdcolor's YCbCr -> RGB on int64 planes (h, w), `cb` and `cr` less 128: uint8 (h, w, 3), clamped."""
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _jpeg_plane(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """One component through FDCT, quantiser, dequantiser and IDCT: int64 (h, w) in 0..255 -> int64 (h, w) in 0..255."""
    h, w = plane.shape
    blocks = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    v = jpeg_fdct_islow(blocks)
    div = (q << 3).reshape(8, 8)
    coef = np.sign(v) * ((np.abs(v) + (div >> 1)) // div)
    out = np.clip(jpeg_idct_islow(coef * q.reshape(8, 8)) + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(h, w)


def _jpeg_upsample(c: np.ndarray) -> np.ndarray:
    """h2v2 fancy upsampling of a chroma plane (h, w) -> (2 h, 2 w): 3 near + far vertically (the first and last rows are their own
    far rows), then (3 this + neighbour + 8 | 7) >> 4 horizontally (the first and last columns are their own neighbours)."""
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    v = np.stack([3 * c + up, 3 * c + down], axis=1).reshape(2 * c.shape[0], c.shape[1])
    left, right = np.concatenate([v[:, :1], v[:, :-1]], axis=1), np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    return np.stack([(3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4], axis=2).reshape(v.shape[0], 2 * v.shape[1])


def jpeg_roundtrip_u8_host(crop_u8: np.ndarray, quality: int) -> np.ndarray:
    """ImageCompression at one quality on a uint8 (H, W, 3) crop, H and W multiples of 16: what cv2.imdecode(cv2.imencode(".jpg", crop,
    quality)) returns, computed without the entropy coding.  cv2 reads the crop as BGR, so libjpeg's R is channel 2 and its B is
    channel 0 (albumentations hands over its RGB crop unconverted)."""
    v = np.asarray(crop_u8)
    if v.ndim != 3 or v.shape[2] != 3 or v.dtype != np.uint8:
        raise ValueError("the crop must be uint8 (H, W, 3)")
    H, W = v.shape[:2]
    if H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError("the JPEG round trip takes sides that are positive multiples of 16 (whole MCUs)")
    q_luma, q_chroma = jpeg_quant_tables(quality)
    p = v.astype(np.int64)
    r, g, b = p[..., 2], p[..., 1], p[..., 0]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2], dtype=np.int64), W // 4)              # alternates along a row of the downsampled plane

    def down(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2

    y = _jpeg_plane(y, q_luma)
    cb = _jpeg_upsample(_jpeg_plane(down(cb), q_chroma)) - 128
    cr = _jpeg_upsample(_jpeg_plane(down(cr), q_chroma)) - 128
    return np.ascontiguousarray(_jpeg_ycc_to_rgb(y, cb, cr)[..., ::-1])                 # libjpeg's R, G, B back into cv2's B, G, R
