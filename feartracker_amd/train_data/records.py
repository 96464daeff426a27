"""The data stage's records: sizes, the default configuration, the members' enums and tables, the numpy forms of the ABI's structs
(train_abi) and the replayable draws of a batch."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..train_abi import FearColourOp, FearFrame, FearFrameWindow, FearHlsOp, FearPairGeom, FearPhotoOp

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
    blur_p=0.2,                  # OneOf([Blur, GaussianBlur, MedianBlur, MotionBlur]), and GlassBlur with `glass_blur` below
    noise_p=0.2,                 # OneOf([MultiplicativeNoise, GaussNoise]), or the members named below
    # the members of the noise OneOf, a subset of NOISE_MEMBERS in its order; "all" adds ImageCompression.  ISONoise, the reference's
    # fourth, is `iso_noise` below: no name of this list
    noise_members=("multiplicative", "gauss"),
    jpeg_quality=(50, 100),      # ImageCompression(quality_lower=50): the quality is uniform over these, both ends included
    downscale_p=0.2,             # Downscale(0.5, 0.5)
    blur_limit=7, gauss_var_limit=(10, 35), multiplier=(0.9, 1.1),
    # ISONoise as one more member of the noise OneOf: a crop on which the group fired takes it at 1 / (len(noise_members) + 1)
    iso_noise=False, iso_color_shift=(0.01, 0.05), iso_intensity=(0.1, 0.5),
    # OneOf([RandomRain, RandomShadow], p=0.05) behind the noise: a subset of WEATHER_MEMBERS in its order, "all" = both, () = off
    weather_members=(), weather_p=0.05,
    # GlassBlur (defaults: sigma 0.7, max_delta 4, two iterations, mode "fast") as the fifth member of the blur OneOf: a crop on which
    # the group fired takes it at 1 / 5
    glass_blur=False,
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
BLUR_GLASS = 5                                  # GlassBlur (`glass_blur`): recorded in PhotoParams.blur, applied by fear_glass_u8
GLASS_MAX_DELTA, GLASS_ITERATIONS = 4, 2        # GlassBlur's defaults; its sigma of 0.7 gives cv2's 8-bit kernel GLASS_WEIGHTS
GLASS_WEIGHTS = (2, 53, 146, 53, 2)
NOISE_NONE, NOISE_MULTIPLICATIVE, NOISE_GAUSS, NOISE_JPEG = 0, 1, 2, 3
NOISE_MEMBERS = {"multiplicative": NOISE_MULTIPLICATIVE, "gauss": NOISE_GAUSS, "jpeg": NOISE_JPEG}   # (in the order `noise_members` keeps)
NOISE_ISO = 4                                   # ISONoise (`iso_noise`): recorded in PhotoParams.noise, applied by fear_hls_u8
WEATHER_NONE, WEATHER_RAIN, WEATHER_SHADOW = 0, 1, 2
WEATHER_MEMBERS = {"rain": WEATHER_RAIN, "shadow": WEATHER_SHADOW}                                  # (in the order `weather_members` keeps)
HLS_COPY, HLS_ISO, HLS_RAIN, HLS_SHADOW = 0, 1, 2, 3                                                # FearHlsOp's kinds
SHADOW_POLYGONS, SHADOW_VERTICES = 2, 5         # RandomShadow's defaults: at most two polygons of five vertices
N_QUANTILES = 4096
GAUSS_WEIGHTS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}

# columns of the pairs table
PAIR_COLUMNS = ("template_frame", "tx", "ty", "tw", "th", "search_frame", "sx", "sy", "sw", "sh", "presence")

TrainBatch = namedtuple("TrainBatch", ["template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox"])


# the numpy forms of the device's records, derived from the ctypes mirrors of include/fear_train.h
GEOM_DTYPE, FRAME_DTYPE, WINDOW_DTYPE = np.dtype(FearPairGeom), np.dtype(FearFrame), np.dtype(FearFrameWindow)
PHOTO_DTYPE, COLOUR_DTYPE, HLS_DTYPE = np.dtype(FearPhotoOp), np.dtype(FearColourOp), np.dtype(FearHlsOp)


@dataclass
class PhotoParams:
    """The photometric draws of one batch, every array shaped (B, 2, ...): [:, 0] the template crop, [:, 1] the search crop.  The
    values of all members are drawn; only the drawn member's are used."""
    blur: np.ndarray             # int32, BLUR_* (BLUR_GLASS only with `glass_blur`)
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
    # ISONoise's values per crop, (B, 2, ...); None unless `iso_noise` and the photometric stage are on.  The crops that drew it carry
    # NOISE_ISO in `photo.noise`.  (These
    # fields stand in front of `jpeg_quality`, which stays the last one; their draws come behind its draw.)
    iso_color_shift: Optional[np.ndarray] = None     # (B, 2) float64
    iso_intensity: Optional[np.ndarray] = None       # (B, 2) float64
    iso_key: Optional[np.ndarray] = None             # (B, 2, 2) uint32, the Philox key
    # the weather group per crop, (B, 2, ...); None unless `weather_members` names a member and the photometric stage is on
    weather: Optional[np.ndarray] = None             # (B, 2) int32, WEATHER_*
    rain_slant: Optional[np.ndarray] = None          # (B, 2) int32
    rain_drops: Optional[np.ndarray] = None          # (B, 2, 109, 2) int32: (x, y) per drop; a crop of side s uses the first s s // 600
    shadow_num: Optional[np.ndarray] = None          # (B, 2) int32, 1 or 2 polygons
    shadow_vertices: Optional[np.ndarray] = None     # (B, 2, 2, 5, 2) int32: (x, y) per vertex of both polygons
    # ImageCompression's quality per crop, (B, 2) int32 like the arrays of `photo`; None unless "jpeg" is a configured noise member and
    # the photometric stage is on
    jpeg_quality: Optional[np.ndarray] = None


def _pairs_array(pairs) -> np.ndarray:
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    p = np.asarray(p, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != len(PAIR_COLUMNS):
        raise ValueError(f"pairs must be (B, {len(PAIR_COLUMNS)}): {', '.join(PAIR_COLUMNS)}")
    return p


def scale_pairs(pairs, scale) -> np.ndarray:
    """A (B, 11) pair table for frames decoded at 1 / `scale` (`JpegStore.decode(ids, scale=)`, `decode_rows(..., scale=)`): a float64
    copy with the template box and the search box (x, y, w, h each) divided by `scale`, the frame indices and the presence as they are.
    `frame_rows`, `draw` and `build` then run unchanged on the smaller frames.
    `scale` may also be an (F,) array of per-FRAME scales (`TrainPairBuilder.frame_scales`): the template box is divided by the scale
    of frame pairs[:, 0], the search box by that of frame pairs[:, 5] — the two may differ; a constant array equals the int bit for
    bit.  A frame index outside 0..F-1 is a ValueError."""
    from ..jpeg_frames import _check_scale, _check_scales
    p = _pairs_array(pairs).copy()
    if isinstance(scale, (int, np.integer)):
        scale = _check_scale(scale)
        p[:, 1:5] /= scale
        p[:, 6:10] /= scale
        return p
    scale = _check_scales(scale, len(scale) if hasattr(scale, "__len__") else -1)
    t, s = p[:, 0].astype(np.int64), p[:, 5].astype(np.int64)
    if p.shape[0] and (min(t.min(), s.min()) < 0 or max(t.max(), s.max()) >= scale.size):
        raise ValueError(f"a pair names a frame outside the {scale.size} scales")
    p[:, 1:5] /= scale[t][:, None]
    p[:, 6:10] /= scale[s][:, None]
    return p


@dataclass
class WindowFrames:
    """What `JpegStore.decode_windows` returns: per position a compact tensor that holds a rectangle of the frame.
    `frames[i][y - origin[i, 0], x - origin[i, 1]]` is pixel (y, x) of frame i for every (y, x) of `window[i]`; the rest of a tensor (the
    halo rows and columns, the MCUs' remainder) holds unspecified bytes."""
    frames: List                     # uint8 (wh, ww, 3) device tensors, private; (0, 0, 3) for the empty window
    origin: np.ndarray               # (n, 2) int32: the frame coordinates (y, x) of each tensor's first pixel
    shape: np.ndarray                # (n, 2) int32: the shape of the frames `decode(ids, scale=scale)` returns
    window: np.ndarray               # (n, 4) int64: the clipped request [y0, y1) x [x0, x1), zeros for the empty window

    def __len__(self) -> int:
        return len(self.frames)

    @property
    def nbytes(self) -> int:
        return int(sum(3 * f.shape[0] * f.shape[1] for f in self.frames))


__all__ = [name for name in dir() if name.isupper()] + ["PhotoParams", "TrainPairParams", "TrainBatch", "WindowFrames", "scale_pairs"]     # (every constant above)
