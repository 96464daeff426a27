"""`YUVFrame`: a 4:2:0 video frame (NV12 or I420) as decoders deliver it, for the trackers and the crop entry points.

A hardware decoder hands out NV12 surfaces in device memory, a software decoder (ffmpeg `yuv420p`) I420 planes on the host.
Both carry 1.5 bytes per pixel against packed RGB's 3.  A `YUVFrame` wraps the planes without converting them: numpy arrays or
CUDA tensors, row-strided tensors (a decoder surface with a pitch) included, no copy.  `shape` is `(H, W, 3)`, the shape of the RGB
frame it stands for, so the trackers' geometry (`clamp_bbox(rect, image.shape)`) reads it unchanged.

The colour conversion is OpenCV 4.x's `cv2.cvtColor(frame, COLOR_YUV2RGB_NV12 / COLOR_YUV2RGB_I420)`, BT.601 limited range in
20-bit integer arithmetic with nearest chroma (`yuv_to_rgb_numpy`; csrc/fear_yuv.h runs the same integers on the device).  The
crop kernel `fear_crop_normalize_planar` reads the planes directly and produces, bit for bit, the crops of the converted frame.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

FMT_RGB, FMT_NV12, FMT_I420 = 0, 1, 2            # FEAR_FMT_* of include/fear_hip.h
_FORMATS = {"nv12": FMT_NV12, "i420": FMT_I420, "yuv420p": FMT_I420}

# OpenCV's ITUR_BT_601_* constants (color_yuv.simd.hpp), shift 20
_CY, _CVR, _CVG, _CUG, _CUB, _SHIFT = 1220542, 1673527, -852492, -409993, 2116026, 20


def yuv_to_rgb_numpy(y: np.ndarray, u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Y (H, W), U and V (H/2, W/2) uint8 -> (H, W, 3) uint8 RGB, cv2's integer BT.601 limited-range conversion with nearest
    chroma: pixel (x, y) takes chroma sample (x >> 1, y >> 1)."""
    uu = np.repeat(np.repeat(u.astype(np.int64) - 128, 2, axis=0), 2, axis=1)
    vv = np.repeat(np.repeat(v.astype(np.int64) - 128, 2, axis=0), 2, axis=1)
    yv = np.maximum(y.astype(np.int64) - 16, 0) * _CY + (1 << (_SHIFT - 1))
    out = np.empty(y.shape + (3,), dtype=np.uint8)
    out[..., 0] = np.clip((yv + _CVR * vv) >> _SHIFT, 0, 255)
    out[..., 1] = np.clip((yv + _CVG * vv + _CUG * uu) >> _SHIFT, 0, 255)
    out[..., 2] = np.clip((yv + _CUB * uu) >> _SHIFT, 0, 255)
    return out


def _is_array(p) -> bool:
    return isinstance(p, (np.ndarray, torch.Tensor))


def _check_plane(p, name: str, shape: Tuple[int, ...]) -> None:
    if not _is_array(p):
        raise TypeError(f"{name} must be a numpy array or a torch tensor")
    if (p.dtype != np.uint8) if isinstance(p, np.ndarray) else (p.dtype != torch.uint8):
        raise TypeError(f"{name} must be uint8, got {p.dtype}")
    if tuple(p.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}, got {tuple(p.shape)}")
    # the kernels read rows through a byte pitch (uint8: numpy's and torch's strides are both in bytes): the bytes of a row must
    # be contiguous, in order, and rows must not overlap
    strides = tuple(p.strides) if isinstance(p, np.ndarray) else tuple(p.stride())
    inner, row = ((2, 1), 2 * shape[1]) if len(shape) == 3 else ((1,), shape[1])
    if strides[1:] != inner or strides[0] < row:
        raise ValueError(f"{name}: the bytes of a row must be contiguous and rows must not overlap (strides {strides})")


class YUVFrame:
    """One NV12 or I420 frame: Y (H, W) and the chroma planes, numpy arrays or CUDA tensors, all on the same side.

    NV12: `uv` is the interleaved chroma plane, (H/2, W) or (H/2, W/2, 2).  I420: `u` and `v` are (H/2, W/2).  H and W are even.
    Rows may be strided (a pitched surface: `buf[:, :W]` of a wider buffer); the bytes inside a row must be contiguous."""

    __slots__ = ("format", "planes", "height", "width")

    def __init__(self, fmt: int, planes: tuple, height: int, width: int) -> None:
        self.format, self.planes, self.height, self.width = int(fmt), tuple(planes), int(height), int(width)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def nv12(cls, y, uv) -> "YUVFrame":
        h, w = cls._luma(y)
        if _is_array(uv) and uv.ndim == 3:
            _check_plane(uv, "uv", (h // 2, w // 2, 2))
        else:
            _check_plane(uv, "uv", (h // 2, w))
        cls._same_side((y, uv))
        return cls(FMT_NV12, (y, uv), h, w)

    @classmethod
    def i420(cls, y, u, v) -> "YUVFrame":
        h, w = cls._luma(y)
        _check_plane(u, "u", (h // 2, w // 2))
        _check_plane(v, "v", (h // 2, w // 2))
        cls._same_side((y, u, v))
        return cls(FMT_I420, (y, u, v), h, w)

    @classmethod
    def from_packed(cls, buf, height: int, width: int, fmt: str = "nv12") -> "YUVFrame":
        """The (H*3/2, W) layout of cv2 and ffmpeg rawvideo (or the same H*W*3/2 bytes flat): Y rows, then the interleaved UV rows
        (NV12) or the U plane then the V plane (I420).  The planes are views of `buf`."""
        h, w = int(height), int(width)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"NV12 / I420 frames have even sizes >= 2, got {h} x {w}")
        key = str(fmt).lower()
        if key not in _FORMATS:
            raise ValueError(f"unknown format {fmt!r}: 'nv12' or 'i420'")
        if not _is_array(buf):
            raise TypeError("buf must be a numpy array or a torch tensor")
        n = h * w * 3 // 2
        if tuple(buf.shape) not in ((h * 3 // 2, w), (n,)):
            raise ValueError(f"buf must be ({h * 3 // 2}, {w}) or ({n},), got {tuple(buf.shape)}")
        flat = buf.reshape(-1)
        y = flat[: h * w].reshape(h, w)
        if _FORMATS[key] == FMT_NV12:
            return cls.nv12(y, flat[h * w:].reshape(h // 2, w))
        q = (h // 2) * (w // 2)
        return cls.i420(y, flat[h * w: h * w + q].reshape(h // 2, w // 2), flat[h * w + q:].reshape(h // 2, w // 2))

    @staticmethod
    def _luma(y) -> Tuple[int, int]:
        if not _is_array(y) or y.ndim != 2:
            raise ValueError("y must be a 2-D (H, W) uint8 plane")
        h, w = int(y.shape[0]), int(y.shape[1])
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"NV12 / I420 frames have even sizes >= 2, got {h} x {w}")
        _check_plane(y, "y", (h, w))
        return h, w

    @staticmethod
    def _same_side(planes) -> None:
        dev = {p.device if isinstance(p, torch.Tensor) else None for p in planes}
        if len(dev) != 1:
            raise ValueError("all planes must be numpy arrays, or tensors on one device")
        (d,) = dev
        if d is not None and d.type != "cuda":
            raise ValueError("tensor planes must be CUDA tensors (host planes are numpy arrays)")

    # ------------------------------------------------------------------ properties
    @property
    def shape(self) -> Tuple[int, int, int]:
        """(H, W, 3): the shape of the RGB frame this frame converts to."""
        return (self.height, self.width, 3)

    @property
    def is_cuda(self) -> bool:
        return isinstance(self.planes[0], torch.Tensor)

    @property
    def device(self) -> Optional[torch.device]:
        return self.planes[0].device if self.is_cuda else None

    def chroma(self):
        """(U, V) planes, (H/2, W/2) each (views of the NV12 plane for NV12)."""
        if self.format == FMT_I420:
            return self.planes[1], self.planes[2]
        uv = self.planes[1]
        if uv.ndim == 2:
            uv = uv.reshape(self.height // 2, self.width // 2, 2) if isinstance(uv, np.ndarray) else \
                uv.view(self.height // 2, self.width // 2, 2)
        return uv[..., 0], uv[..., 1]

    def pitches(self) -> Tuple[int, int, int]:
        """Byte pitch of each plane (0 for a plane the format does not have)."""
        out = [int(p.strides[0] if isinstance(p, np.ndarray) else p.stride(0)) for p in self.planes]
        return tuple(out + [0] * (3 - len(out)))

    # ------------------------------------------------------------------ conversion and transfer
    def to_rgb(self, net=None):
        """The (H, W, 3) uint8 RGB frame: numpy (`yuv_to_rgb_numpy`) for host planes; for device planes `fear_yuv_to_rgb` through
        `net` (a FEARNetHIP on the planes' device; one is created when none is given), a device tensor."""
        if not self.is_cuda:
            y = np.asarray(self.planes[0])
            u, v = self.chroma()
            return yuv_to_rgb_numpy(y, np.asarray(u), np.asarray(v))
        if net is None:
            net = _conversion_net(self.device)
        return net.yuv_to_rgb(self)

    def to(self, device, non_blocking: bool = False) -> "YUVFrame":
        """The frame with its planes copied to `device` (contiguous planes, a pitch of one row)."""
        planes = tuple(torch.as_tensor(np.ascontiguousarray(p)) if isinstance(p, np.ndarray) else p for p in self.planes)
        planes = tuple(p.to(device, non_blocking=non_blocking).contiguous() for p in planes)
        if self.format == FMT_NV12 and planes[1].dim() == 3:
            planes = (planes[0], planes[1].reshape(self.height // 2, self.width))
        return YUVFrame(self.format, planes, self.height, self.width)


def host_rgb(frame: YUVFrame, net=None) -> np.ndarray:
    """The frame's RGB conversion as a numpy array (the trackers' host path); `net` converts device planes when it can."""
    rgb = frame.to_rgb(net if hasattr(net, "yuv_to_rgb") else None)
    return rgb.cpu().numpy() if isinstance(rgb, torch.Tensor) else rgb


def mean_color(frame: YUVFrame, net=None) -> np.ndarray:
    """np.mean(frame.to_rgb(), axis=(0, 1)), the float64 mean colour of the converted frame.  For device planes the RGB frame stays
    on the device and only its channel sums come back: integer sums are exact, so the quotient is numpy's number."""
    if not frame.is_cuda:
        return np.mean(frame.to_rgb(), axis=(0, 1))
    rgb = frame.to_rgb(net if hasattr(net, "yuv_to_rgb") else None)
    sums = rgb.to(torch.int64).sum(dim=(0, 1)).cpu().numpy()
    return sums.astype(np.float64) / float(frame.height * frame.width)


_CONVERSION_NETS = {}


def _conversion_net(device: torch.device):
    """An engine handle per device for `YUVFrame.to_rgb` called without one."""
    from .hip_backend import DEFAULT_WEIGHTS, FEARNetHIP
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _CONVERSION_NETS:
        _CONVERSION_NETS[idx] = FEARNetHIP(DEFAULT_WEIGHTS, device=idx, max_batch=1)
    return _CONVERSION_NETS[idx]
