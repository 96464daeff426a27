"""The colour stage on the host: the lookup tables of the first members, cv2's 8-bit HSV, the members of fear_colour_u8, the tone
stage and the normalisation."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..geometry import _INV_STD, _MEAN
from .records import (COLOUR_BRIGHTNESS_CONTRAST, COLOUR_DTYPE, COLOUR_EMBOSS, COLOUR_EQUALIZE, COLOUR_GAMMA, COLOUR_HSV, COLOUR_JITTER,
                      COLOUR_RGB_SHIFT, COLOUR_TONE_CURVE, DEVICE_COLOUR_KINDS, JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION,
                      TONE_GRAY, TONE_SEPIA, TrainPairParams)

_SEPIA = np.array([[0.393, 0.769, 0.189], [0.349, 0.686, 0.168], [0.272, 0.534, 0.131]], dtype=np.float32)


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


def _even_sides(img: np.ndarray, stage: str) -> None:
    if img.shape[0] < 4 or img.shape[1] < 4 or img.shape[0] % 2 or img.shape[1] % 2:
        raise ValueError(f"the {stage} stage takes even sides of at least 4")


def _windows(img: np.ndarray, r: int, mode: str) -> np.ndarray:
    """(H, W, 3) -> (H, W, 3, k, k) windows of the image padded by r (`reflect` = BORDER_REFLECT_101, `edge` = BORDER_REPLICATE)."""
    padded = np.pad(img, ((r, r), (r, r), (0, 0)), mode=mode)
    return np.lib.stride_tricks.sliding_window_view(padded, (2 * r + 1, 2 * r + 1), axis=(0, 1))


def filter2d_u8(img: np.ndarray, taps: np.ndarray, k: int) -> np.ndarray:
    """cv2.filter2D(img, -1, taps) on a uint8 (H, W, 3) crop for k x k taps, as Emboss (k = 3) and MotionBlur (its kernel centred in
    k = 7) use it: correlation, BORDER_REFLECT_101, the non-zero taps in row-major order accumulated in fp32, rint half to even, saturate."""
    win = _windows(img, k // 2, "reflect")
    acc = np.zeros(img.shape, dtype=np.float32)
    for t, wt in enumerate(np.asarray(taps, dtype=np.float32).reshape(k * k)):
        if wt != 0:
            acc = acc + wt * win[..., t // k, t % k].astype(np.float32)
    return _round_u8(acc)


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
    """Emboss on a uint8 (H, W, 3) crop: `filter2d_u8` with the nine taps of `emboss_taps`."""
    return filter2d_u8(img, taps, 3)


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
    _even_sides(v, "colour")
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
        return np.repeat(_gray_u8(rgb)[..., None], 3, axis=-1).astype(np.uint8)
    if tone == TONE_SEPIA:
        v = rgb.astype(np.float32)
        out = []
        for i in range(3):
            acc = _SEPIA[i, 0] * v[..., 0]
            acc = acc + _SEPIA[i, 1] * v[..., 1]
            acc = acc + _SEPIA[i, 2] * v[..., 2]
            out.append(acc)
        return _round_u8(np.stack(out, axis=-1))
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
