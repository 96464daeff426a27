"""The photometric stage on the host: Philox, GaussNoise's quantile table, MotionBlur's kernels, the FearPhotoOp records and the
restatement of fear_photometric_u8."""
from __future__ import annotations

import statistics
from typing import Optional, Tuple

import numpy as np

from .colour import _even_sides, _normalise_u8, _windows, filter2d_u8
from .jpeg import jpeg_roundtrip_u8_host
from .records import (BLUR_BOX, BLUR_GAUSSIAN, BLUR_GLASS, BLUR_MEDIAN, BLUR_MOTION, BLUR_NONE, GAUSS_WEIGHTS, N_QUANTILES, NOISE_GAUSS, NOISE_ISO,
                      NOISE_JPEG, NOISE_MULTIPLICATIVE, NOISE_NONE, PHOTO_DTYPE, PhotoParams)

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter: np.ndarray, key: np.ndarray) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., Random123) over rows: counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32."""
    c = np.asarray(counter).astype(np.uint64)
    k = np.asarray(key).astype(np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(_PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(_PHILOX_W1)) & mask
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


_QUANTILES = None


def normal_quantiles() -> np.ndarray:
    """GaussNoise's normal variates: (4096,) fp32, entry i = the standard normal's quantile at (i + 0.5) / 4096.  A table lookup has
    the same bits on the host and on the device, which logf / cosf do not.  Tails end at +-3.67, the variance is 0.9997."""
    global _QUANTILES
    if _QUANTILES is None:
        nd = statistics.NormalDist()
        _QUANTILES = np.array([nd.inv_cdf((i + 0.5) / N_QUANTILES) for i in range(N_QUANTILES)], dtype=np.float32)
    return _QUANTILES


def line_u8(k: int, xs: int, ys: int, xe: int, ye: int) -> np.ndarray:
    """cv2.line(zeros((k, k), uint8), (xs, ys), (xe, ye), 1, thickness=1): OpenCV's 8-connected LineIterator, left to right (the end
    points swap when xe < xs), one pixel per step of the longer axis, the error term deciding the steps of the shorter one."""
    img = np.zeros((k, k), dtype=np.uint8)
    x, y, dx, dy = int(xs), int(ys), int(xe) - int(xs), int(ye) - int(ys)
    if dx < 0:
        x, y, dx, dy = int(xe), int(ye), -dx, -dy
    step_y = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err = major - 2 * minor
    for _ in range(major + 1):
        img[y, x] = 1
        diag = err < 0
        err += -2 * minor + (2 * major if diag else 0)
        if steep:
            y += step_y
            x += 1 if diag else 0
        else:
            x += 1
            y += step_y if diag else 0
    return img


def motion_kernel(k: int, xs: int, ys: int, xe: int, ye: int) -> np.ndarray:
    """MotionBlur.get_params' kernel for drawn end points: the line divided by its sum, (k, k) fp32."""
    line = line_u8(k, xs, ys, xe, ye)
    return line.astype(np.float32) / np.float32(line.sum())


def motion_taps(kernel: np.ndarray) -> np.ndarray:
    """A (k, k) kernel as one row of the device's tap table: centred in 7 x 7, row-major, (49,) fp32."""
    k = kernel.shape[0]
    full = np.zeros((7, 7), dtype=np.float32)
    o = (7 - k) // 2
    full[o:o + k, o:o + k] = kernel
    return full.reshape(49)


def photo_tables(photo: PhotoParams) -> Tuple[np.ndarray, np.ndarray]:
    """FearPhotoOp records (B, 2) and the tap table (m, 49) fp32 of the drawn MotionBlurs (m may be 0), in record order."""
    B = photo.blur.shape[0]
    ops = np.zeros((B, 2), dtype=PHOTO_DTYPE)
    ops["blur"], ops["ksize"], ops["noise"] = photo.blur, photo.ksize, photo.noise
    sigma = np.sqrt(np.asarray(photo.var, dtype=np.float64)).astype(np.float32)
    ops["scale"] = np.where(photo.noise == NOISE_GAUSS, sigma, np.asarray(photo.mult).astype(np.float32))
    ops["key"] = photo.key
    ops["downscale"] = (np.asarray(photo.downscale) != 0).astype(np.int32)
    ops["tap_row"] = -1
    taps = []
    for b, j in np.argwhere(photo.blur == BLUR_MOTION):
        ops["tap_row"][b, j] = len(taps)
        taps.append(motion_taps(motion_kernel(int(photo.ksize[b, j]), *(int(v) for v in photo.line[b, j]))))
    return ops, np.stack(taps) if taps else np.zeros((0, 49), dtype=np.float32)


def split_jpeg_records(ops: np.ndarray, quality: Optional[np.ndarray], later: Optional[np.ndarray] = None
                       ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The records of the path with launches between fear_photometric_stage_u8 and fear_photometric_u8, for a batch in which crops drew
    ImageCompression, ISONoise or a weather member, from the FearPhotoOp records `ops` and the drawn qualities, both (B, 2) (`quality`
    None without ImageCompression): (first, tail, quality).  `later`, (B, 2) bool, marks the crops fear_hls_u8 works on.  `first` is
    fear_photometric_stage_u8's: `ops` with the noise of the JPEG and the ISONoise crops and the Downscale of every crop with a launch
    of its own behind taken off.  `quality` is fear_jpeg_u8's: int32, 0 (a copy) for the other crops.  `tail` is fear_photometric_u8's
    behind them: those crops' Downscale, "none" otherwise, and everybody's normalisation.  `ops` is left as it is."""
    drew = ops["noise"] == NOISE_JPEG
    moved = drew if later is None else drew | np.asarray(later, dtype=bool)
    first, tail = ops.copy(), np.zeros(ops.shape, dtype=PHOTO_DTYPE)
    first["noise"][drew | (ops["noise"] == NOISE_ISO)] = NOISE_NONE
    first["downscale"][moved] = 0
    tail["downscale"], tail["tap_row"] = np.where(moved, ops["downscale"], 0), -1
    return first, tail, np.where(drew, 0 if quality is None else quality, 0).astype(np.int32)


def photometric_u8_host(crop_u8: np.ndarray, op, taps: Optional[np.ndarray], q: np.ndarray, quality: int = 0, hls=None,
                        glass: bool = False) -> np.ndarray:
    """fear_photometric_u8's uint8 result for one (H, W, 3) crop and its FearPhotoOp record `op` (a PHOTO_DTYPE scalar), before the
    normalisation: blur, then noise, then Downscale(0.5).  Records the device treats as "none" are "none" here too.  A record whose
    noise is NOISE_JPEG takes `jpeg_roundtrip_u8_host` at `quality` in the noise's place (the builder's three-launch path); with a
    quality outside 1..100 — the default — that noise is "none", as it is to fear_photometric_u8 and fear_jpeg_u8.
    `hls` = (iso, weather, segments, exp_table) brings in fear_hls_u8's members (hls.hls_u8_host): the FearHlsOp record `iso` in the
    noise's place when the noise is NOISE_ISO, the record `weather` between the noise and the Downscale; either may be None.  Without
    `hls` a NOISE_ISO is "none", as it is to fear_photometric_u8.
    `glass` brings in fear_glass_u8's member (glass.glass_u8_host) in the blur's place when the blur is BLUR_GLASS; without it a
    BLUR_GLASS is "none", as it is to fear_photometric_u8."""
    v = np.asarray(crop_u8)
    H, W = v.shape[:2]
    _even_sides(v, "photometric")
    blur, k, noise, row = int(op["blur"]), int(op["ksize"]), int(op["noise"]), int(op["tap_row"])
    if k not in (3, 5, 7) or (blur == BLUR_MOTION and (taps is None or row < 0)):
        blur = BLUR_NONE
    r = k // 2
    if int(op["blur"]) == BLUR_GLASS:                      # (whatever the record's ksize)
        blur = BLUR_NONE
        if glass:
            from .glass import glass_u8_host
            v = glass_u8_host(v, op)
    if blur == BLUR_BOX:
        s = _windows(v, r, "reflect").astype(np.int64).sum(axis=(-1, -2))
        v = ((s + k * k // 2) // (k * k)).astype(np.uint8)
    elif blur == BLUR_GAUSSIAN:
        w = np.asarray(GAUSS_WEIGHTS[k], dtype=np.int64)
        s = (_windows(v, r, "reflect").astype(np.int64) * (w[:, None] * w[None, :])).sum(axis=(-1, -2))
        v = ((s + 32768) >> 16).astype(np.uint8)
    elif blur == BLUR_MEDIAN:
        win = _windows(v, r, "edge").reshape(H, W, 3, k * k)
        v = np.sort(win, axis=-1)[..., k * k // 2]
    elif blur == BLUR_MOTION:
        v = filter2d_u8(v, taps[row], 7)
    if noise == NOISE_MULTIPLICATIVE:
        v = np.clip(v.astype(np.float32) * np.float32(op["scale"]), 0, 255).astype(np.uint8)
    elif noise == NOISE_GAUSS:
        yy, xx = np.mgrid[0:H, 0:W]
        counter = np.stack([xx, yy, np.zeros_like(xx), np.zeros_like(xx)], axis=-1)
        idx = philox4x32_10(counter, np.asarray(op["key"]))[..., :3] >> np.uint32(20)
        f = np.float32(op["scale"]) * np.asarray(q, dtype=np.float32)[idx]
        f = v.astype(np.float32) + f
        v = np.clip(f, 0, 255).astype(np.uint8)
    elif noise == NOISE_JPEG and 1 <= int(quality) <= 100:
        v = jpeg_roundtrip_u8_host(np.ascontiguousarray(v), int(quality))
    if hls is not None:
        from .hls import hls_u8_host
        iso, weather, segments, exp_table = hls
        if noise == NOISE_ISO and iso is not None:
            v = hls_u8_host(np.ascontiguousarray(v), iso, segments, q, exp_table)
        if weather is not None:
            v = hls_u8_host(np.ascontiguousarray(v), weather, segments, q, exp_table)
    if int(op["downscale"]) != 0:
        v = np.repeat(np.repeat(v[::2, ::2], 2, axis=0), 2, axis=1)
    return np.ascontiguousarray(v)


def photometric_host(crop_u8: np.ndarray, op, taps: Optional[np.ndarray], q: np.ndarray, quality: int = 0, hls=None,
                     glass: bool = False) -> np.ndarray:
    """numpy restatement of fear_photometric_u8 for one crop: (H, W, 3) uint8 -> normalised fp32 (3, H, W)."""
    return _normalise_u8(photometric_u8_host(crop_u8, op, taps, q, quality, hls, glass))
