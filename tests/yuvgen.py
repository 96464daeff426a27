"""Deterministic RGB -> 4:2:0 YUV for the YUV tests (test infrastructure).

The tests compare tracking on a YUV clip with tracking on that clip's RGB conversion, so the encoder only has to be
deterministic: BT.601 limited-range coefficients in float64, a seeded dither of less than one code value on luma, chroma from
the 2 x 2 mean.  Its inverse is NOT the package's conversion; nothing here is compared with it.
"""
import numpy as np


def rgb_to_yuv420(rgb: np.ndarray, seed: int = 0):
    """(H, W, 3) uint8, H and W even -> (Y (H, W), U (H/2, W/2), V (H/2, W/2)) uint8."""
    rng = np.random.RandomState(seed)
    x = rgb.astype(np.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = 16.0 + 0.257 * r + 0.504 * g + 0.098 * b + rng.uniform(-0.45, 0.45, r.shape)
    h, w = rgb.shape[:2]
    m = x.reshape(h // 2, 2, w // 2, 2, 3).mean(axis=(1, 3))
    u = 128.0 - 0.148 * m[..., 0] - 0.291 * m[..., 1] + 0.439 * m[..., 2]
    v = 128.0 + 0.439 * m[..., 0] - 0.368 * m[..., 1] - 0.071 * m[..., 2]
    q = [np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, u, v)]
    return q[0], q[1], q[2]


def nv12_packed(y, u, v) -> np.ndarray:
    """The (H*3/2, W) NV12 buffer of cv2 / ffmpeg rawvideo: Y rows, then the interleaved UV rows."""
    h, w = y.shape
    uv = np.stack([u, v], axis=-1).reshape(h // 2, w)
    return np.concatenate([y, uv], axis=0)


def i420_packed(y, u, v) -> np.ndarray:
    """The (H*3/2, W) I420 buffer: Y rows, then the U plane, then the V plane (each (H/2, W/2), packed row after row)."""
    h, w = y.shape
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(h * 3 // 2, w)


def full_chroma_frame(seed: int = 3):
    """A 512 x 512 frame whose 256 x 256 chroma samples are every (U, V) pair: U = the chroma column, V = the chroma row; seeded
    luma.  Returns (y, u, v)."""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, 256, (512, 512)).astype(np.uint8)
    v, u = np.mgrid[0:256, 0:256].astype(np.uint8)
    return y, u, v
