"""Training pairs from frames on the GPU: the data stage in front of `FEARNetTrainHIP.step`.

`TrainPairBuilder` turns (frames, template box, search box) into exactly the five tensors the step takes, the way the reference's
`SiameseTrackingDataset._transform` does per pair on the CPU (model_training/dataset/siam_dataset.py:33-61):

* template  `get_extended_crop(frame, box, 128, offset=0.2)`, padded with the frame's mean colour   (tracking_dataset.py:139-156)
* search    `get_extended_crop(frame, box, 512, offset=u)`, u = random() * 3 + 2.5, then `BBoxCropWithOffsets` (scale 0.35,
            shift 48): a jittered square of the 512 crop warped to 256 x 256 by `cv2.warpAffine` (tracking_dataset.py:107-137,
            aug.py:52-143); the box follows through `apply_to_bbox`, `ensure_bbox_boundaries`, `handle_empty_bbox`
* colour    `OneOf([ToGray, ToSepia], p=0.05)` and, at p = 0.5, one of RandomBrightnessContrast / RandomGamma / RGBShift — drawn once
            per pair and applied to both crops (siam_dataset.py:64-67; the subset is DESIGN.md section 11's).  `colour_members`
            widens the group to RandomToneCurve (one more lookup table), Equalize, HueSaturationValue, ColorJitter and Emboss, which
            the device's `fear_colour_u8` applies per crop behind the tables; `colour_u8_host` restates it
* photometric  (`photometric=True`, off by default) `PHOTOMETRIC_AUGMENTATIONS` on each crop on its own, between the colour stage and
            the normalisation: a blur group, a noise group and Downscale(0.5), each at p = 0.2 (aug.py:8-25, tracking_dataset.py:
            158-175; the members built are DESIGN.md section 11's); `photometric_host` restates the device's `fear_photometric_u8`.
            `noise_members` widens the noise group to ImageCompression: a JPEG round trip without its entropy coding
            (`fear_jpeg_u8`), which `jpeg_roundtrip_u8_host` restates and the tests hold to Pillow's libjpeg-turbo byte for byte
* targets   `FEARBoxCoder.encode(search_bbox)` and `get_regression_weight_label(search_bbox, 256, 16)`, zeros without presence

Every scalar per-pair step runs here on the host, vectorised over the batch: the draws (`draw`), the context boxes (`extend_bbox`,
`crop_geometry` of geometry.py), the jittered box, `apply_to_bbox` with its truncations, the inverse warp matrix (cv2's order of
operations, float64) and the colour lookup tables.  The device (include/fear_train.h: `fear_frame_border_u8`, `fear_train_pairs`)
does the per-pixel and per-cell work.  `build_host` restates the device arithmetic in numpy; `build` equals it bit for bit.

The reference calls cv2 (`copyMakeBorder`, `resize`, `warpAffine`, `cvtColor`) and albumentations, neither of which is installed
here: the restatements follow OpenCV 4.x's 8u code paths and albumentations' uint8 lookup-table forms, but parity with the real
libraries is unpinned (as for the crop).  What pins the geometry and the targets is the reference's own
Python run on recorded draws (tests/golden/train_pairs_geometry.npz, tools/make_train_pairs_golden.py).
"""
from __future__ import annotations

import ctypes
import statistics
from collections import namedtuple
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .geometry import _INV_STD, _MEAN, _linear_taps, border_color_u8, extend_bbox  # noqa: F401  (extend_bbox: the scalar form)

TEMPLATE_SIZE, CONTEXT_SIZE, SEARCH_SIZE, SCORE_SIZE, TOTAL_STRIDE = 128, 512, 256, 16, 16

# (the values of config/dataset/got10k_train.yaml and config/tracker/siam_tracker.yaml)
DEFAULT_TRAIN_DATA_CONFIG: Dict[str, Any] = dict(
    template_bbox_offset=0.2,
    search_context=2,            # the dataset doubles it: offsets u in [2 * 2 - 3 / 2, 2 * 2 + 3 / 2)
    context_range=3,
    search_image_scale=0.35,
    search_image_shift=48,
    r_pos=2,
    tone_p=0.05,                 # OneOf([ToGray, ToSepia])
    colour_p=0.5,                # OneOf([RandomBrightnessContrast, RandomGamma, RGBShift]), or the members named below
    # the members of the colour OneOf, a subset of COLOUR_MEMBERS in its order; "all" = every one of COLOUR_MEMBERS (8 of the
    # reference's 9: CLAHE is not built)
    colour_members=("brightness_contrast", "gamma", "rgb_shift"),
    brightness_limit=0.2, contrast_limit=0.2, gamma_limit=(0.8, 1.2), rgb_shift_limit=20.0,
    # PHOTOMETRIC_AUGMENTATIONS (dataset/aug.py:8-25), per crop, off unless asked for
    photometric=False,
    blur_p=0.2,                  # OneOf([Blur, GaussianBlur, MedianBlur, MotionBlur])
    noise_p=0.2,                 # OneOf([MultiplicativeNoise, GaussNoise]), or the members named below
    # the members of the noise OneOf, a subset of NOISE_MEMBERS in its order; "all" adds ImageCompression (3 of the reference's 4:
    # ISONoise is not built)
    noise_members=("multiplicative", "gauss"),
    jpeg_quality=(50, 100),      # ImageCompression(quality_lower=50): the quality is uniform over these, both ends included
    downscale_p=0.2,             # Downscale(0.5, 0.5)
    blur_limit=7, gauss_var_limit=(10, 35), multiplier=(0.9, 1.1),
)

TONE_NONE, TONE_GRAY, TONE_SEPIA = 0, 1, 2
COLOUR_NONE, COLOUR_BRIGHTNESS_CONTRAST, COLOUR_GAMMA, COLOUR_RGB_SHIFT = 0, 1, 2, 3
COLOUR_TONE_CURVE, COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_JITTER, COLOUR_EMBOSS = 4, 5, 6, 7, 8
COLOUR_MEMBERS = {"brightness_contrast": COLOUR_BRIGHTNESS_CONTRAST, "gamma": COLOUR_GAMMA, "rgb_shift": COLOUR_RGB_SHIFT,
                  "tone_curve": COLOUR_TONE_CURVE, "equalize": COLOUR_EQUALIZE, "hsv": COLOUR_HSV, "colour_jitter": COLOUR_JITTER,
                  "emboss": COLOUR_EMBOSS}                                      # (in the order `colour_members` keeps)
DEVICE_COLOUR_KINDS = (COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_JITTER, COLOUR_EMBOSS)   # fear_colour_u8's; the others are lookup tables
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3       # ColorJitter's operations, as `order` names them

BLUR_NONE, BLUR_BOX, BLUR_GAUSSIAN, BLUR_MEDIAN, BLUR_MOTION = 0, 1, 2, 3, 4
NOISE_NONE, NOISE_MULTIPLICATIVE, NOISE_GAUSS, NOISE_JPEG = 0, 1, 2, 3
NOISE_MEMBERS = {"multiplicative": NOISE_MULTIPLICATIVE, "gauss": NOISE_GAUSS, "jpeg": NOISE_JPEG}   # (in the order `noise_members` keeps)
N_QUANTILES = 4096
GAUSS_WEIGHTS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}

# columns of the pairs table
PAIR_COLUMNS = ("template_frame", "tx", "ty", "tw", "th", "search_frame", "sx", "sy", "sw", "sh", "presence")

TrainBatch = namedtuple("TrainBatch", ["template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox"])

_SEPIA = np.array([[0.393, 0.769, 0.189], [0.349, 0.686, 0.168], [0.272, 0.534, 0.131]], dtype=np.float32)

GEOM_DTYPE = np.dtype([("t_frame", "<i4"), ("s_frame", "<i4"), ("t_ctx", "<i4", 4), ("s_ctx", "<i4", 4), ("box", "<i4", 4),
                       ("presence", "<i4"), ("tone", "<i4"), ("inv", "<f8", 4)])
assert GEOM_DTYPE.itemsize == 96
FRAME_DTYPE = np.dtype([("data", "<u8"), ("h", "<i4"), ("w", "<i4")])        # fear_frame
PHOTO_DTYPE = np.dtype([("blur", "<i4"), ("ksize", "<i4"), ("noise", "<i4"), ("scale", "<f4"), ("key", "<u4", 2),
                        ("downscale", "<i4"), ("tap_row", "<i4")])             # FearPhotoOp
assert PHOTO_DTYPE.itemsize == 32
COLOUR_DTYPE = np.dtype([("kind", "<i4"), ("order", "u1", 4), ("contrast", "<f8"), ("alpha", "<f4"), ("beta", "<f4"),
                         ("taps", "<f4", 9), ("reserved", "<i4")])             # FearColourOp
assert COLOUR_DTYPE.itemsize == 64


@dataclass
class PhotoParams:
    """The photometric draws of one batch, every array shaped (B, 2, ...): [:, 0] the template crop, [:, 1] the search crop.  The
    values of all members are drawn; only the drawn member's are used."""
    blur: np.ndarray             # int32, BLUR_*
    ksize: np.ndarray            # int32, 3 / 5 / 7
    line: np.ndarray             # (B, 2, 4) int32: MotionBlur's end points xs, ys, xe, ye
    noise: np.ndarray            # int32, NOISE_*
    var: np.ndarray              # float64, GaussNoise's variance
    mult: np.ndarray             # float64, MultiplicativeNoise's multiplier
    key: np.ndarray              # (B, 2, 2) uint32, the Philox key of GaussNoise
    downscale: np.ndarray        # int32, 0 / 1


@dataclass
class TrainPairParams:
    """Every random parameter of one batch (a replayable host record).  Per pair: the search context offset, the jitter
    (scale_x, scale_y, shift_x, shift_y), the tone branch, the colour branch and the values of all three colour members (only the
    drawn branch's are used)."""
    context: np.ndarray          # (B,) float64
    jitter: np.ndarray           # (B, 4) float64
    tone: np.ndarray             # (B,) int32, TONE_*
    colour: np.ndarray           # (B,) int32, COLOUR_*
    alpha: np.ndarray            # (B,) contrast
    beta: np.ndarray             # (B,) brightness
    gamma: np.ndarray            # (B,)
    shift: np.ndarray            # (B, 3) RGB shift
    frame_shapes: Tuple[Tuple[int, int], ...]
    photo: Optional[PhotoParams] = None      # the photometric draws, None with the stage off
    # the values of the members `colour_members` adds, each None unless its member is configured
    tone_curve: Optional[np.ndarray] = None      # (B, 2) low_y, high_y
    hsv: Optional[np.ndarray] = None             # (B, 3) hue, saturation and value shifts
    colour_jitter: Optional[np.ndarray] = None   # (B, 4) ColorJitter's brightness, contrast, saturation factors and hue shift
    colour_jitter_order: Optional[np.ndarray] = None   # (B, 4) int32, a permutation of JITTER_* per pair
    emboss: Optional[np.ndarray] = None          # (B, 2) alpha, strength
    # ImageCompression's quality per crop, (B, 2) int32 like the arrays of `photo`; None unless "jpeg" is a configured noise member and
    # the photometric stage is on
    jpeg_quality: Optional[np.ndarray] = None


def _pairs_array(pairs) -> np.ndarray:
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    p = np.asarray(p, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != len(PAIR_COLUMNS):
        raise ValueError(f"pairs must be (B, {len(PAIR_COLUMNS)}): {', '.join(PAIR_COLUMNS)}")
    return p


# --------------------------------------------------------------------------------------------------------------------- geometry
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


# ------------------------------------------------------------------------------------------------------------------------ colour
def colour_luts(params: TrainPairParams) -> np.ndarray:
    """(B, 3, 256) uint8 lookup tables of the drawn colour members, albumentations' uint8 forms:
    brightness / contrast  trunc(clip(fp32(v) * fp32(alpha) + fp32(beta * 255), 0, 255))
    gamma                  trunc((v / 255) ** gamma * 255), float64
    RGB shift              trunc(clip(fp32(v) + fp32(shift_c), 0, 255))
    tone curve             rint(bezier(v / 255) * 255), float64 (`tone_curve_lut`), the same table for the three channels
    and the identity where no member was drawn or the drawn one is fear_colour_u8's."""
    B = len(params.colour)
    v32 = np.arange(256, dtype=np.float32)
    lut = np.broadcast_to(np.arange(256, dtype=np.uint8), (B, 3, 256)).copy()
    kind = np.asarray(params.colour)
    sel = kind == COLOUR_BRIGHTNESS_CONTRAST
    if sel.any():
        t = v32[None, :] * params.alpha[sel].astype(np.float32)[:, None]
        t = t + (params.beta[sel] * 255.0).astype(np.float32)[:, None]
        lut[sel] = np.clip(t, 0, 255).astype(np.uint8)[:, None, :]
    sel = kind == COLOUR_GAMMA
    if sel.any():
        t = (np.arange(256, dtype=np.float64)[None, :] / 255.0) ** params.gamma[sel][:, None] * 255.0
        lut[sel] = t.astype(np.uint8)[:, None, :]
    sel = kind == COLOUR_RGB_SHIFT
    if sel.any():
        t = v32[None, None, :] + params.shift[sel].astype(np.float32)[:, :, None]
        lut[sel] = np.clip(t, 0, 255).astype(np.uint8)
    for k in np.flatnonzero(kind == COLOUR_TONE_CURVE):
        lut[k] = tone_curve_lut(*_member_values(params, "tone_curve")[k])[None, :]
    return lut


def _member_values(params: TrainPairParams, name: str) -> np.ndarray:
    v = getattr(params, name)
    if v is None:
        raise ValueError(f"a pair drew a colour member whose values ({name}) the params do not carry (drawn without it in colour_members?)")
    return v


def tone_curve_lut(low_y: float, high_y: float) -> np.ndarray:
    """RandomToneCurve's table: the cubic Bezier through (0, 0), (0.25, low_y), (0.75, high_y), (1, 1) evaluated at t = v / 255 in
    float64, rint(... * 255) as uint8 (256,)."""
    t = np.linspace(0.0, 1.0, 256)
    curve = 3 * (1 - t) ** 2 * t * low_y + 3 * (1 - t) * t ** 2 * high_y + t ** 3
    return np.rint(curve * 255).astype(np.uint8)


# cv2's 8-bit RGB -> HSV division tables (hsv_shift 12): rint((255 << 12) / i) and rint((180 << 12) / (6 i)), entry 0 = 0
_SDIV = np.concatenate([[0], np.rint(1044480 / np.arange(1, 256))]).astype(np.int64)
_HDIV = np.concatenate([[0], np.rint(737280 / (6 * np.arange(1, 256)))]).astype(np.int64)
# HSV -> RGB: which of (v, v (1 - s), v (1 - s f), v (1 - s (1 - f))) is b, g, r in each sector
_SECTOR_BGR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def _gray_u8(rgb: np.ndarray) -> np.ndarray:
    """cv2 COLOR_RGB2GRAY on uint8 (..., 3): 14-bit fixed point, int64 (...)."""
    v = rgb.astype(np.int64)
    return (4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14


def _round_u8(x: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def rgb_to_hsv_u8(rgb: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_RGB2HSV) on uint8 (..., 3), H in [0, 180): v = max, s = (d sdiv[v] + 2048) >> 12, h from the channel that is
    the maximum (r first, then g), (h' hdiv[d] + 2048) >> 12, + 180 when negative."""
    c = rgb.astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = (d * _SDIV[v] + 2048) >> 12
    hp = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (hp * _HDIV[d] + 2048) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv_to_rgb_u8(hsv: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_HSV2RGB) on uint8 (..., 3) with H in [0, 180): through fp32, every product and sum rounded on its own;
    a sector outside 0..5 becomes 0 with f = 0; s == 0 is gray."""
    one = np.float32(1.0)
    hf = hsv[..., 0].astype(np.float32) * np.float32(6.0 / 180.0)
    sf = hsv[..., 1].astype(np.float32) * np.float32(1.0 / 255.0)
    vf = hsv[..., 2].astype(np.float32) * np.float32(1.0 / 255.0)
    sector = np.floor(hf)
    f = hf - sector
    outside = (sector < 0) | (sector > 5)
    f = np.where(outside, np.float32(0.0), f)
    k = np.where(outside, 0, sector).astype(np.int64)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], axis=-1)
    bgr = np.take_along_axis(tab, _SECTOR_BGR[k], axis=-1)
    rgb = np.where((hsv[..., 1] == 0)[..., None], vf[..., None], bgr[..., ::-1])
    assert rgb.dtype == np.float32
    return _round_u8(rgb * np.float32(255.0))


def equalize_u8(img: np.ndarray) -> np.ndarray:
    """cv2.equalizeHist on each channel of a uint8 (H, W, C) crop: i0 the first non-empty bin; a channel of one value keeps it;
    otherwise lut[i] = saturate(rint(fp32(sum of hist(i0, i]) * (fp32(255) / fp32(H W - hist[i0]))))."""
    out = np.empty_like(img)
    total = img.shape[0] * img.shape[1]
    for c in range(img.shape[2]):
        hist = np.bincount(img[..., c].reshape(-1), minlength=256)
        i0 = int(np.flatnonzero(hist)[0])
        if hist[i0] == total:
            out[..., c] = img[..., c]
            continue
        scale = np.float32(255.0) / np.float32(total - hist[i0])
        sums = np.cumsum(np.where(np.arange(256) > i0, hist, 0))
        lut = _round_u8(sums.astype(np.float32) * scale)
        out[..., c] = lut[img[..., c]]
    return out


def jitter_brightness_lut(factor: float) -> np.ndarray:
    return np.clip(np.arange(256, dtype=np.float64) * float(factor), 0, 255).astype(np.uint8)


def jitter_hue_lut(hue: float) -> np.ndarray:
    return np.mod(np.arange(256, dtype=np.float64) + 180.0 * float(hue), 180.0).astype(np.uint8)


def jitter_brightness_u8(img: np.ndarray, factor: float) -> np.ndarray:
    """ColorJitter's brightness on uint8: trunc(clip(v * factor, 0, 255)), float64."""
    return jitter_brightness_lut(factor)[img]


def jitter_contrast_u8(img: np.ndarray, factor: float) -> np.ndarray:
    """ColorJitter's contrast on a uint8 (H, W, 3) crop: trunc(clip(v * factor + mean * (1 - factor), 0, 255)) in float64, mean = the
    crop's gray plane's (an exact integer sum over H W)."""
    factor = float(factor)
    mean = float(int(_gray_u8(img).sum())) / float(img.shape[0] * img.shape[1])
    lut = np.clip(np.arange(256, dtype=np.float64) * factor + mean * (1.0 - factor), 0, 255).astype(np.uint8)
    return lut[img]


def jitter_saturation_u8(img: np.ndarray, alpha, beta) -> np.ndarray:
    """ColorJitter's saturation on uint8 (..., 3): rint(fp32(c) * alpha + fp32(gray) * beta), alpha = fp32(factor), beta = fp32(1 -
    factor), the products and the sum rounded on their own."""
    g = _gray_u8(img).astype(np.float32) * np.float32(beta)
    return _round_u8(img.astype(np.float32) * np.float32(alpha) + g[..., None])


def jitter_hue_u8(img: np.ndarray, lh: np.ndarray) -> np.ndarray:
    """ColorJitter's hue on uint8 (..., 3): RGB -> HSV, the table `lh` on H, HSV -> RGB."""
    hsv = rgb_to_hsv_u8(img)
    hsv[..., 0] = lh[hsv[..., 0]]
    return hsv_to_rgb_u8(hsv)


def emboss_taps(alpha: float, strength: float) -> np.ndarray:
    """Emboss's kernel (1 - alpha) [centre] + alpha [[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]] in float64, as nine fp32 taps."""
    a, s = float(alpha), float(strength)
    nochange = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    effect = np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]], dtype=np.float64)
    return ((1 - a) * nochange + a * effect).astype(np.float32).reshape(9)


def emboss_u8(img: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """cv2.filter2D(img, -1, taps) on a uint8 (H, W, 3) crop as MotionBlur's is defined: correlation, BORDER_REFLECT_101, the non-zero
    taps in row-major order accumulated in fp32, rint half to even, saturate."""
    win = _windows(img, 1, "reflect")
    acc = np.zeros(img.shape, dtype=np.float32)
    for t, wt in enumerate(np.asarray(taps, dtype=np.float32).reshape(9)):
        if wt != 0:
            acc = acc + wt * win[..., t // 3, t % 3].astype(np.float32)
    return _round_u8(acc)


def colour_tables(params: TrainPairParams) -> Tuple[np.ndarray, np.ndarray]:
    """FearColourOp records (B,) and the tables `aux_lut` (B, 3, 256) uint8 of the pairs that drew one of fear_colour_u8's members
    (kind 0 and zeros for the others).  HueSaturationValue: lh = trunc(mod(i + hue, 180)), ls = trunc(clip(i + sat, 0, 255)), lv the same
    with val.  ColorJitter: row 0 the brightness table, row 1 lh = trunc(mod(i + 180 hue, 180))."""
    kind = np.asarray(params.colour)
    B = len(kind)
    ops = np.zeros(B, dtype=COLOUR_DTYPE)
    aux = np.zeros((B, 3, 256), dtype=np.uint8)
    ramp = np.arange(256, dtype=np.float64)
    ops["kind"] = np.where(np.isin(kind, DEVICE_COLOUR_KINDS), kind, 0)
    for k in np.flatnonzero(kind == COLOUR_HSV):
        hue, sat, val = (float(v) for v in _member_values(params, "hsv")[k])
        aux[k, 0] = np.mod(ramp + hue, 180.0).astype(np.uint8)
        aux[k, 1] = np.clip(ramp + sat, 0, 255).astype(np.uint8)
        aux[k, 2] = np.clip(ramp + val, 0, 255).astype(np.uint8)
    for k in np.flatnonzero(kind == COLOUR_JITTER):
        brightness, contrast, saturation, hue = (float(v) for v in _member_values(params, "colour_jitter")[k])
        ops["order"][k] = _member_values(params, "colour_jitter_order")[k]
        ops["contrast"][k] = contrast
        ops["alpha"][k], ops["beta"][k] = np.float32(saturation), np.float32(1.0 - saturation)
        aux[k, 0], aux[k, 1] = jitter_brightness_lut(brightness), jitter_hue_lut(hue)
    for k in np.flatnonzero(kind == COLOUR_EMBOSS):
        ops["taps"][k] = emboss_taps(*_member_values(params, "emboss")[k])
    return ops, aux


def colour_u8_host(crop_u8: np.ndarray, op, aux: np.ndarray) -> np.ndarray:
    """fear_colour_u8's result for one (H, W, 3) uint8 crop, its FearColourOp record `op` (a COLOUR_DTYPE scalar) and its tables `aux`
    (3, 256).  A record the device copies the crop for (an unknown kind, a ColorJitter order that is no permutation) copies it here."""
    v = np.ascontiguousarray(crop_u8)
    H, W = v.shape[:2]
    if H < 4 or W < 4 or H % 2 or W % 2:
        raise ValueError("the colour stage takes even sides of at least 4")
    kind = int(op["kind"])
    if kind == COLOUR_EQUALIZE:
        return equalize_u8(v)
    if kind == COLOUR_HSV:
        hsv = rgb_to_hsv_u8(v)
        return hsv_to_rgb_u8(np.stack([aux[c][hsv[..., c]] for c in range(3)], axis=-1))
    if kind == COLOUR_JITTER:
        order = [int(o) for o in op["order"]]
        if sorted(order) != [0, 1, 2, 3]:
            return v.copy()
        for o in order:
            if o == JITTER_BRIGHTNESS:
                v = aux[0][v]
            elif o == JITTER_CONTRAST:
                v = jitter_contrast_u8(v, float(op["contrast"]))
            elif o == JITTER_SATURATION:
                v = jitter_saturation_u8(v, op["alpha"], op["beta"])
            else:
                v = jitter_hue_u8(v, aux[1])
        return np.ascontiguousarray(v)
    if kind == COLOUR_EMBOSS:
        return emboss_u8(v, op["taps"])
    return v.copy()


def apply_tone(rgb: np.ndarray, tone: int) -> np.ndarray:
    """The tone stage on uint8 (..., 3): cv2 RGB2GRAY (14-bit fixed point) to all channels, or albumentations' sepia matrix
    accumulated in fp32 (j = 0, 1, 2), rounded half to even and saturated."""
    if tone == TONE_GRAY:
        v = rgb.astype(np.int64)
        g = (4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14
        return np.repeat(g[..., None], 3, axis=-1).astype(np.uint8)
    if tone == TONE_SEPIA:
        v = rgb.astype(np.float32)
        out = []
        for i in range(3):
            acc = _SEPIA[i, 0] * v[..., 0]
            acc = acc + _SEPIA[i, 1] * v[..., 1]
            acc = acc + _SEPIA[i, 2] * v[..., 2]
            out.append(np.clip(np.rint(acc), 0, 255))
        return np.stack(out, axis=-1).astype(np.uint8)
    return rgb


def _colour_u8(rgb: np.ndarray, tone: int, lut: np.ndarray) -> np.ndarray:
    """(H, W, 3) uint8 -> tone -> lut -> (H, W, 3) uint8: fear_train_pairs_u8's crop."""
    v = apply_tone(rgb, tone)
    return np.stack([lut[c][v[..., c]] for c in range(3)], axis=-1)


def _normalise_u8(rgb: np.ndarray) -> np.ndarray:
    """(H, W, 3) uint8 -> normalised fp32 (3, H, W)."""
    v = rgb.astype(np.float32)
    v -= _MEAN
    v *= _INV_STD
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def _colour_normalise(rgb: np.ndarray, tone: int, lut: np.ndarray) -> np.ndarray:
    """(H, W, 3) uint8 -> tone -> lut -> normalised fp32 (3, H, W)."""
    return _normalise_u8(_colour_u8(rgb, tone, lut))


# ------------------------------------------------------------------------------------------------------------------- photometric
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


def _windows(img: np.ndarray, r: int, mode: str) -> np.ndarray:
    """(H, W, 3) -> (H, W, 3, k, k) windows of the image padded by r (`reflect` = BORDER_REFLECT_101, `edge` = BORDER_REPLICATE)."""
    padded = np.pad(img, ((r, r), (r, r), (0, 0)), mode=mode)
    return np.lib.stride_tricks.sliding_window_view(padded, (2 * r + 1, 2 * r + 1), axis=(0, 1))


def photometric_u8_host(crop_u8: np.ndarray, op, taps: Optional[np.ndarray], q: np.ndarray, quality: int = 0) -> np.ndarray:
    """fear_photometric_u8's uint8 result for one (H, W, 3) crop and its FearPhotoOp record `op` (a PHOTO_DTYPE scalar), before the
    normalisation: blur, then noise, then Downscale(0.5).  Records the device treats as "none" are "none" here too.  A record whose
    noise is NOISE_JPEG takes `jpeg_roundtrip_u8_host` at `quality` in the noise's place (the builder's three-launch path); with a
    quality outside 1..100 — the default — that noise is "none", as it is to fear_photometric_u8 and fear_jpeg_u8."""
    v = np.asarray(crop_u8)
    H, W = v.shape[:2]
    if H < 4 or W < 4 or H % 2 or W % 2:
        raise ValueError("the photometric stage takes even sides of at least 4")
    blur, k, noise, row = int(op["blur"]), int(op["ksize"]), int(op["noise"]), int(op["tap_row"])
    if k not in (3, 5, 7) or (blur == BLUR_MOTION and (taps is None or row < 0)):
        blur = BLUR_NONE
    r = k // 2
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
        win = _windows(v, 3, "reflect")
        acc = np.zeros((H, W, 3), dtype=np.float32)
        for t, wt in enumerate(np.asarray(taps[row], dtype=np.float32)):
            if wt != 0:
                acc = acc + wt * win[..., t // 7, t % 7].astype(np.float32)
        v = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
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
    if int(op["downscale"]) != 0:
        v = np.repeat(np.repeat(v[::2, ::2], 2, axis=0), 2, axis=1)
    return np.ascontiguousarray(v)


def photometric_host(crop_u8: np.ndarray, op, taps: Optional[np.ndarray], q: np.ndarray, quality: int = 0) -> np.ndarray:
    """numpy restatement of fear_photometric_u8 for one crop: (H, W, 3) uint8 -> normalised fp32 (3, H, W)."""
    v = photometric_u8_host(crop_u8, op, taps, q, quality).astype(np.float32)
    v -= _MEAN
    v *= _INV_STD
    return np.ascontiguousarray(v.transpose(2, 0, 1))



# -------------------------------------------------------------------------------------------------------------------------- JPEG
# ImageCompression: the lossy part of a baseline JPEG round trip (libjpeg: 4:2:0, jpeg_set_quality(q, force_baseline), islow DCT both
# ways, fancy upsampling), in integers.  The entropy coding is lossless and is left out.  DESIGN.md section 11 states the contract;
# tests/test_jpeg_host.py holds it to Pillow's libjpeg-turbo byte for byte.
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
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


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


# ----------------------------------------------------------------------------------------------------------------------- builder
class TrainPairBuilder:
    """Builds the step's inputs from frames.  `pairs` is a (B, 11) table (PAIR_COLUMNS): template frame index, template box xywh,
    search frame index, search box xywh, presence.  Which frames a pair uses is the caller's business."""

    def __init__(self, config: Optional[Dict[str, Any]] = None, device: int = 0, seed: Optional[int] = None):
        self.config = dict(DEFAULT_TRAIN_DATA_CONFIG)
        if config:
            unknown = set(config) - set(self.config)
            if unknown:
                raise KeyError(f"unknown train-data config keys {sorted(unknown)}")
            self.config.update(config)
        self.colour_members = self._members(self.config["colour_members"])
        self.noise_members = self._members(self.config["noise_members"], NOISE_MEMBERS, "noise")
        lo, hi = (int(v) for v in self.config["jpeg_quality"])
        if not 1 <= lo <= hi <= 100:
            raise ValueError("jpeg_quality must be (low, high) with 1 <= low <= high <= 100")
        self._device_colour = any(COLOUR_MEMBERS[m] in DEVICE_COLOUR_KINDS for m in self.colour_members)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.generator = np.random.default_rng(seed)
        self._lib = None
        self._qtable = None

    @staticmethod
    def _members(value, table: Optional[Dict[str, int]] = None, group: str = "colour") -> Tuple[str, ...]:
        """`colour_members` (or, with NOISE_MEMBERS as `table`, `noise_members`) as a tuple of names in the table's order: "all", or any
        non-empty subset (KeyError for a name that is no member)."""
        table = COLOUR_MEMBERS if table is None else table
        if isinstance(value, str):
            value = tuple(table) if value == "all" else (value,)
        names = tuple(value)
        unknown = [m for m in names if m not in table]
        if unknown:
            raise KeyError(f"unknown {group} members {unknown}: the members are {list(table)}")
        if not names or len(set(names)) != len(names):
            raise ValueError(f"{group}_members must name at least one member, each once")
        return tuple(m for m in table if m in names)

    # ------------------------------------------------------------------ draws
    def draw(self, pairs, frame_shapes: Sequence[Tuple[int, ...]], generator: Optional[np.random.Generator] = None) -> TrainPairParams:
        """Every random parameter of a batch, vectorised, from `generator` (the builder's own when None).  The draws mirror the
        reference's: u = U * range + (2 context - range / 2) (tracking_dataset.py:102-105); scale ~ U(-0.35, 0.35), shift ~
        U(-48, 48) (aug.py:90-93); tone at p = 0.05, colour at p = 0.5, each picking uniformly among its members."""
        p = _pairs_array(pairs)
        rng = self.generator if generator is None else generator
        cfg = self.config
        B = p.shape[0]
        rng_ctx = float(cfg["context_range"])
        min_ctx = 2 * float(cfg["search_context"]) - rng_ctx / 2
        context = rng.random(B) * rng_ctx + min_ctx
        sc, sh = float(cfg["search_image_scale"]), float(cfg["search_image_shift"])
        jitter = np.concatenate([rng.uniform(-sc, sc, size=(B, 2)), rng.uniform(-sh, sh, size=(B, 2))], axis=1)
        tone = np.where(rng.random(B) < cfg["tone_p"], 1 + rng.integers(0, 2, size=B), TONE_NONE).astype(np.int32)
        kinds = np.array([COLOUR_MEMBERS[m] for m in self.colour_members])
        colour = np.where(rng.random(B) < cfg["colour_p"], kinds[rng.integers(0, len(kinds), size=B)], COLOUR_NONE).astype(np.int32)
        alpha = 1.0 + rng.uniform(-cfg["contrast_limit"], cfg["contrast_limit"], size=B)
        beta = rng.uniform(-cfg["brightness_limit"], cfg["brightness_limit"], size=B)
        gamma = rng.uniform(cfg["gamma_limit"][0], cfg["gamma_limit"][1], size=B)
        shift = rng.uniform(-cfg["rgb_shift_limit"], cfg["rgb_shift_limit"], size=(B, 3))
        shapes = tuple((int(s[0]), int(s[1])) for s in frame_shapes)
        photo = self._draw_photo(B, rng) if cfg["photometric"] else None       # after every other draw: off consumes nothing
        # the members colour_members adds, after every other draw: the default members consume nothing more
        extra = self._draw_colour(B, rng)
        if photo is not None and "jpeg" in self.noise_members:          # last of all: configurations without it keep their stream
            lo, hi = (int(v) for v in cfg["jpeg_quality"])
            extra["jpeg_quality"] = rng.integers(lo, hi + 1, size=(B, 2)).astype(np.int32)
        return TrainPairParams(context, jitter, tone, colour, alpha, beta, gamma, shift, shapes, photo, **extra)

    def _draw_colour(self, B: int, rng: np.random.Generator) -> Dict[str, np.ndarray]:
        """The values of the configured members beyond the first three (aug.py:35-48), every one for every pair: RandomToneCurve's
        two control heights, HueSaturationValue's three shifts, ColorJitter's three factors, hue shift and the order of its four
        operations (a uniformly random permutation), Emboss's alpha and strength.  Equalize has none."""
        out: Dict[str, np.ndarray] = {}
        if "tone_curve" in self.colour_members:
            out["tone_curve"] = np.stack([rng.uniform(0.15, 0.35, size=B), rng.uniform(0.65, 0.85, size=B)], axis=1)
        if "hsv" in self.colour_members:
            out["hsv"] = np.stack([rng.uniform(-20, 20, size=B), rng.uniform(-30, 30, size=B), rng.uniform(-20, 20, size=B)], axis=1)
        if "colour_jitter" in self.colour_members:
            out["colour_jitter"] = np.concatenate([rng.uniform(0.8, 1.2, size=(B, 3)), rng.uniform(-0.2, 0.2, size=(B, 1))], axis=1)
            out["colour_jitter_order"] = rng.permuted(np.tile(np.arange(4, dtype=np.int32), (B, 1)), axis=1)
        if "emboss" in self.colour_members:
            out["emboss"] = np.stack([rng.uniform(0.2, 0.5, size=B), rng.uniform(0.2, 0.7, size=B)], axis=1)
        return out

    def _colour_ops(self, params: TrainPairParams):
        """The batch's FearColourOp records and tables when a member of fear_colour_u8's is configured, None otherwise."""
        drawn = np.isin(np.asarray(params.colour), DEVICE_COLOUR_KINDS)
        if not self._device_colour:
            if drawn.any():
                raise ValueError("a pair drew a member of fear_colour_u8's, but colour_members configures none of them")
            return None
        return colour_tables(params)

    def _draw_photo(self, B: int, rng: np.random.Generator) -> PhotoParams:
        """The photometric draws, (B, 2): each group at its p, uniform over its members (aug.py:8-25); ksize uniform over the odd
        sizes up to blur_limit; MotionBlur's end points as MotionBlur.get_params draws them (two x, then two y, distinct when the x
        are equal); var and the multiplier uniform over their limits; a fresh 64-bit Philox key per crop.  ImageCompression's quality
        is drawn by `draw`, behind every other draw (`TrainPairParams.jpeg_quality`)."""
        cfg = self.config
        n_k = (int(cfg["blur_limit"]) - 3) // 2 + 1
        if n_k < 1 or n_k > 3:
            raise ValueError("blur_limit must be 3, 5 or 7")
        blur = np.where(rng.random((B, 2)) < cfg["blur_p"], 1 + rng.integers(0, 4, size=(B, 2)), BLUR_NONE).astype(np.int32)
        ksize = (3 + 2 * rng.integers(0, n_k, size=(B, 2))).astype(np.int32)
        xs, xe, ys, ye = (rng.integers(0, ksize) for _ in range(4))
        other = (ys + 1 + rng.integers(0, ksize - 1)) % ksize                  # random.sample(range(k), 2)'s second value
        line = np.stack([xs, ys, xe, np.where(xs == xe, other, ye)], axis=-1).astype(np.int32)
        kinds = np.array([NOISE_MEMBERS[m] for m in self.noise_members])
        noise = np.where(rng.random((B, 2)) < cfg["noise_p"], kinds[rng.integers(0, len(kinds), size=(B, 2))], NOISE_NONE).astype(np.int32)
        var = rng.uniform(cfg["gauss_var_limit"][0], cfg["gauss_var_limit"][1], size=(B, 2))
        mult = rng.uniform(cfg["multiplier"][0], cfg["multiplier"][1], size=(B, 2))
        key = rng.integers(0, 2 ** 32, size=(B, 2, 2), dtype=np.uint64).astype(np.uint32)
        downscale = (rng.random((B, 2)) < cfg["downscale_p"]).astype(np.int32)
        return PhotoParams(blur, ksize, line, noise, var, mult, key, downscale)

    def _photo(self, params: TrainPairParams, B: int) -> Optional[PhotoParams]:
        """The batch's photometric draws when the stage is on, None when it is off."""
        if not self.config["photometric"]:
            return None
        if params.photo is None:
            raise ValueError("the photometric stage is on, but params carry no photometric draws (drawn with it off?)")
        if params.photo.blur.shape != (B, 2):
            raise ValueError(f"photometric draws are shaped {params.photo.blur.shape}, the table has {B} pairs")
        if (np.asarray(params.photo.noise) == NOISE_JPEG).any():
            if "jpeg" not in self.noise_members:
                raise ValueError("a crop drew ImageCompression, but noise_members does not configure it")
            if params.jpeg_quality is None or np.shape(params.jpeg_quality) != (B, 2):
                raise ValueError("a crop drew ImageCompression, but the params carry no quality for it (drawn without it in noise_members?)")
        return params.photo

    # ------------------------------------------------------------------ host tables
    def tables(self, pairs, params: TrainPairParams) -> Dict[str, np.ndarray]:
        """The per-pair host work: context boxes, the 512-crop box, the jittered crop, the moved box (search_bbox), the warp and its
        inverse, the lookup tables and the FearPairGeom records."""
        p = _pairs_array(pairs)
        B = p.shape[0]
        if len(params.context) != B:
            raise ValueError(f"params were drawn for {len(params.context)} pairs, the table has {B}")
        t_box, s_box = p[:, 1:5], p[:, 6:10]
        t_ctx = _extend(t_box, float(self.config["template_bbox_offset"]))
        s_ctx = _extend(s_box, params.context)
        box512 = _box_in_crop(s_box, s_ctx, CONTEXT_SIZE)
        crop = jittered_crop(params.jitter)
        moved = apply_to_bbox(box512, crop)
        b = _ensure(moved, SEARCH_SIZE, SEARCH_SIZE)
        b[:, 2:] = np.maximum(b[:, 2:], 3)                                   # handle_empty_bbox
        search_bbox = _ensure(b, SEARCH_SIZE, SEARCH_SIZE)                    # _transform's final ensure_bbox_boundaries
        M = warp_matrix(crop)
        Minv = invert_affine(M)
        geom = np.zeros(B, dtype=GEOM_DTYPE)
        geom["t_frame"], geom["s_frame"] = p[:, 0].astype(np.int32), p[:, 5].astype(np.int32)
        geom["t_ctx"], geom["s_ctx"], geom["box"] = t_ctx, s_ctx, search_bbox
        geom["presence"] = (p[:, 10] != 0).astype(np.int32)
        geom["tone"] = params.tone
        geom["inv"] = np.stack([Minv[:, 0, 0], Minv[:, 0, 2], Minv[:, 1, 1], Minv[:, 1, 2]], axis=1)
        return dict(t_ctx=t_ctx, s_ctx=s_ctx, box512=box512, crop=crop, moved=moved, search_bbox=search_bbox, M=M, Minv=Minv,
                    lut=colour_luts(params), geom=geom)

    def _params(self, pairs, frames, params):
        shapes = tuple((int(f.shape[0]), int(f.shape[1])) for f in frames)
        if params is None:
            return self.draw(pairs, shapes)
        if params.frame_shapes and tuple(params.frame_shapes) != shapes:
            raise ValueError("params were drawn for other frame shapes")
        return params

    # ------------------------------------------------------------------ host restatement
    def build_host(self, frames: Sequence, pairs, params: Optional[TrainPairParams] = None) -> TrainBatch:
        """numpy restatement of `build` (same arithmetic, term for term): the reference `build` is tested against."""
        host = [f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
        params = self._params(pairs, host, params)
        tab = self.tables(pairs, params)
        geom, lut = tab["geom"], tab["lut"]
        borders = [border_color_u8(np.mean(f[:, :, :3], axis=(0, 1))) if f.shape[0] > 0 and f.shape[1] > 0 else np.zeros(3, np.uint8)
                   for f in host]
        B = len(geom)
        tmpl = np.empty((B, 3, TEMPLATE_SIZE, TEMPLATE_SIZE), dtype=np.float32)
        srch = np.empty((B, 3, SEARCH_SIZE, SEARCH_SIZE), dtype=np.float32)
        photo = self._photo(params, B)
        if photo is not None:
            ops, taps = photo_tables(photo)
            q = normal_quantiles()
        colour = self._colour_ops(params)

        def finish(crop, k, which):          # colour stage -> (photometric stage) -> normalised fp32
            v = _colour_u8(crop, int(geom["tone"][k]), lut[k])
            if colour is not None:
                v = colour_u8_host(v, colour[0][k], colour[1][k])
            if photo is None:
                return _normalise_u8(v)
            quality = int(params.jpeg_quality[k, which]) if ops["noise"][k, which] == NOISE_JPEG else 0
            return photometric_host(v, ops[k, which], taps, q, quality)

        def frame_of(i):
            if 0 <= i < len(host):
                return np.ascontiguousarray(host[i][:, :, :3]), borders[i]
            return None, np.zeros(3, np.uint8)

        for k in range(B):
            f, pad = frame_of(int(geom["t_frame"][k]))
            t = crop_u8(f, pad, geom["t_ctx"][k], TEMPLATE_SIZE)
            tmpl[k] = finish(t, k, 0)
            f, pad = frame_of(int(geom["s_frame"][k]))
            c512 = crop_u8(f, pad, geom["s_ctx"][k], CONTEXT_SIZE)
            s = remap_affine_u8(c512, tab["Minv"][k], (SEARCH_SIZE, SEARCH_SIZE))
            srch[k] = finish(s, k, 1)
        reg, cls, wgt = encode_targets(tab["search_bbox"], geom["presence"], int(self.config["r_pos"]))
        return TrainBatch(tmpl, srch, reg, cls, wgt, tab["search_bbox"].astype(np.int32))

    # ------------------------------------------------------------------ device
    def _library(self):
        if self._lib is None:
            from .train_abi import load_train_library
            self._lib = load_train_library()
        return self._lib

    @torch.no_grad()
    def build(self, frames: Sequence, pairs, params: Optional[TrainPairParams] = None) -> TrainBatch:
        """The batch on the GPU: template (B,3,128,128), search (B,3,256,256), gt_reg (B,4,16,16), gt_cls (B,1,16,16),
        gt_weight (B,16,16) fp32 and search_bbox (B,4) int32, on the current stream, in the layouts `FEARNetTrainHIP.step` takes.
        Frames are uint8 (H, W, 3) numpy arrays or device tensors.  Host frames and the per-pair tables go up non-blocking from
        pinned memory; with device frames the call never waits for the GPU."""
        lib = self._library()
        dev = self.device
        params = self._params(pairs, frames, params)
        tab = self.tables(pairs, params)
        geom, lut = tab["geom"], tab["lut"]
        B, F = len(geom), len(frames)
        photo = self._photo(params, B)
        colour = self._colour_ops(params)
        if photo is not None:
            ops, taps = photo_tables(photo)
        elif colour is not None:               # the crops still leave through fear_photometric_u8: all-"none" records, the normalisation
            ops, taps = np.zeros((B, 2), dtype=PHOTO_DTYPE), np.zeros((0, 49), dtype=np.float32)
        staged_u8 = photo is not None or colour is not None
        # a batch in which a crop drew ImageCompression (the host knows from the draws) runs three launches per side: the chain up to
        # the noise as uint8 (`ops`, the JPEG crops without noise and Downscale), fear_jpeg_u8 (quality 0, a copy, for the other
        # crops), then the JPEG crops' Downscale and everybody's normalisation (`tail`)
        jpeg = photo is not None and bool((ops["noise"] == NOISE_JPEG).any())
        if jpeg:
            drew = ops["noise"] == NOISE_JPEG
            tail = np.zeros((B, 2), dtype=PHOTO_DTYPE)
            tail["downscale"], tail["tap_row"] = np.where(drew, ops["downscale"], 0), -1
            quality = np.where(drew, params.jpeg_quality, 0).astype(np.int32)
            ops["noise"][drew], ops["downscale"][drew] = NOISE_NONE, 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            dframes = [self._frame_on_device(f) for f in frames]
            # one staging buffer, one transfer: frame table | geometry | lookup tables | search_bbox | photometric records | taps |
            # colour records (8-byte aligned: they hold a double) | colour tables | the JPEG path's last records | its qualities
            o_geom = 16 * F
            o_lut = o_geom + 96 * B
            o_box = o_lut + 768 * B
            o_ops = o_box + 16 * B
            o_taps = o_ops + (64 * B if staged_u8 else 0)
            o_cops = (o_taps + (taps.size * 4 if staged_u8 else 0) + 7) // 8 * 8
            o_aux = o_cops + (64 * B if colour is not None else 0)
            o_tail = o_aux + (768 * B if colour is not None else 0)
            if jpeg:
                o_tail = (o_tail + 3) // 4 * 4
            o_quality = o_tail + (64 * B if jpeg else 0)
            total = o_quality + (8 * B if jpeg else 0)
            pinned = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
            hv = pinned.numpy()
            ftab = np.zeros(F, dtype=FRAME_DTYPE)
            for i, f in enumerate(dframes):
                ftab[i] = (f.data_ptr(), f.shape[0], f.shape[1])
            hv[:o_geom] = ftab.view(np.uint8)
            hv[o_geom:o_lut] = geom.view(np.uint8)
            hv[o_lut:o_box] = lut.reshape(-1)
            hv[o_box:o_ops] = tab["search_bbox"].astype(np.int32).view(np.uint8).reshape(-1)
            if staged_u8:                      # templates' records first, then the searches': one call each
                hv[o_ops:o_taps] = np.ascontiguousarray(ops.T).view(np.uint8).reshape(-1)
                hv[o_taps:o_taps + taps.size * 4] = taps.view(np.uint8).reshape(-1)
            if colour is not None:             # one record per pair, shared by its two crops
                hv[o_cops:o_aux] = colour[0].view(np.uint8)
                hv[o_aux:o_aux + 768 * B] = colour[1].reshape(-1)
            if jpeg:                           # templates first, then the searches, as the records in front
                hv[o_tail:o_quality] = np.ascontiguousarray(tail.T).view(np.uint8).reshape(-1)
                hv[o_quality:total] = np.ascontiguousarray(quality.T).view(np.uint8).reshape(-1)
            staged = pinned.to(dev, non_blocking=True)
            base = staged.data_ptr()
            border = torch.empty((max(F, 1), 3), dtype=torch.uint8, device=dev)
            tmpl = torch.empty((B, 3, TEMPLATE_SIZE, TEMPLATE_SIZE), dtype=torch.float32, device=dev)
            srch = torch.empty((B, 3, SEARCH_SIZE, SEARCH_SIZE), dtype=torch.float32, device=dev)
            reg = torch.empty((B, 4, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            cls = torch.empty((B, 1, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            wgt = torch.empty((B, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            st = ctypes.c_void_p(stream.cuda_stream)
            rc = lib.fear_frame_border_u8(ctypes.c_void_p(base), F, ctypes.c_void_p(border.data_ptr()), st)
            if rc != 0:
                raise RuntimeError(f"fear_frame_border_u8 failed with status {rc}")
            if not staged_u8:
                pairs_fn, t_out, s_out = "fear_train_pairs", tmpl, srch
            else:                              # the crops leave the table stage as uint8 HWC for fear_colour_u8 / fear_photometric_u8
                pairs_fn = "fear_train_pairs_u8"
                t_out = torch.empty((B, TEMPLATE_SIZE, TEMPLATE_SIZE, 3), dtype=torch.uint8, device=dev)
                s_out = torch.empty((B, SEARCH_SIZE, SEARCH_SIZE, 3), dtype=torch.uint8, device=dev)
            rc = getattr(lib, pairs_fn)(ctypes.c_void_p(base), F, ctypes.c_void_p(border.data_ptr()), ctypes.c_void_p(base + o_geom),
                                        ctypes.c_void_p(base + o_lut), B, ctypes.c_void_p(t_out.data_ptr()),
                                        ctypes.c_void_p(s_out.data_ptr()), ctypes.c_void_p(reg.data_ptr()),
                                        ctypes.c_void_p(cls.data_ptr()), ctypes.c_void_p(wgt.data_ptr()), st)
            if rc != 0:
                raise RuntimeError(f"{pairs_fn} failed with status {rc}")
            if colour is not None:             # the members that are no table: once for the templates, once for the searches
                t_in, s_in = t_out, s_out
                t_out, s_out = torch.empty_like(t_in), torch.empty_like(s_in)
                for crops, out, side in ((t_in, t_out, TEMPLATE_SIZE), (s_in, s_out, SEARCH_SIZE)):
                    rc = lib.fear_colour_u8(ctypes.c_void_p(crops.data_ptr()), B, side, side, ctypes.c_void_p(base + o_cops),
                                            ctypes.c_void_p(base + o_aux), ctypes.c_void_p(out.data_ptr()), st)
                    if rc != 0:
                        raise RuntimeError(f"fear_colour_u8 failed with status {rc}")
            if staged_u8:
                q = self._quantiles_on_device()
                d_taps = ctypes.c_void_p(base + o_taps) if taps.size else None
                if jpeg:
                    ws_bytes = lib.fear_jpeg_workspace_bytes(B, SEARCH_SIZE, SEARCH_SIZE)      # the larger side's serves both
                    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                for which, (crops, out, side) in enumerate(((t_out, tmpl, TEMPLATE_SIZE), (s_out, srch, SEARCH_SIZE))):
                    o_last = o_ops
                    if jpeg:
                        mid, crops_in = torch.empty_like(crops), crops
                        crops = torch.empty_like(crops)
                        rc = lib.fear_photometric_stage_u8(ctypes.c_void_p(crops_in.data_ptr()), B, side, side,
                                                           ctypes.c_void_p(base + o_ops + 32 * B * which), d_taps,
                                                           ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(mid.data_ptr()), st)
                        if rc != 0:
                            raise RuntimeError(f"fear_photometric_stage_u8 failed with status {rc}")
                        rc = lib.fear_jpeg_u8(ctypes.c_void_p(mid.data_ptr()), B, side, side, ctypes.c_void_p(base + o_quality + 4 * B * which),
                                              ctypes.c_void_p(ws.data_ptr()), ws_bytes, ctypes.c_void_p(crops.data_ptr()), st)
                        if rc != 0:
                            raise RuntimeError(f"fear_jpeg_u8 failed with status {rc}")
                        o_last = o_tail
                    rc = lib.fear_photometric_u8(ctypes.c_void_p(crops.data_ptr()), B, side, side,
                                                 ctypes.c_void_p(base + o_last + 32 * B * which), d_taps, ctypes.c_void_p(q.data_ptr()),
                                                 ctypes.c_void_p(out.data_ptr()), st)
                    if rc != 0:
                        raise RuntimeError(f"fear_photometric_u8 failed with status {rc}")
            for f in dframes:                          # host frames were allocated here; device frames may live on another stream
                f.record_stream(stream)
            box = staged[o_box:o_ops].view(torch.int32).view(B, 4)
        return TrainBatch(tmpl, srch, reg, cls, wgt, box)

    def _quantiles_on_device(self) -> torch.Tensor:
        """GaussNoise's quantile table on the device: uploaded once per builder, non-blocking from pinned memory.  Later builds on
        other streams of the device find it complete only if they are ordered behind the first one, as stream users are."""
        if self._qtable is None:
            pinned = torch.empty(N_QUANTILES, dtype=torch.float32, pin_memory=True)
            np.copyto(pinned.numpy(), normal_quantiles())
            self._qtable = (pinned.to(self.device, non_blocking=True), pinned)     # (the pinned source lives as long as its copy)
        return self._qtable[0]

    def _frame_on_device(self, f) -> torch.Tensor:
        if isinstance(f, torch.Tensor):
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] < 3:
                raise ValueError("device frames must be uint8 (H, W, 3)")
            return f[:, :, :3].to(self.device).contiguous()
        arr = np.asarray(f)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] < 3:
            raise ValueError("host frames must be uint8 (H, W, 3)")
        arr = arr[:, :, :3]
        pinned = torch.empty(arr.shape, dtype=torch.uint8, pin_memory=True)
        np.copyto(pinned.numpy(), arr)
        return pinned.to(self.device, non_blocking=True)
