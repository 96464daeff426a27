"""The members of the photometric stage that work in HLS, on the host: cv2's RGB <-> HLS (8-bit and fp32), RandomShadow, RandomRain and
ISONoise as DESIGN.md section 11 states them, the FearHlsOp records and the restatement of fear_hls_u8.  Every fp32 or fp64 product, sum
and quotient is rounded on its own (numpy never contracts), as in colour.py."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from .colour import _SECTOR_BGR, _even_sides, _round_u8
from .photometric import philox4x32_10, photometric_u8_host
from .records import (BLUR_BOX, HLS_COPY, HLS_DTYPE, HLS_ISO, HLS_RAIN, HLS_SHADOW, NOISE_ISO, PHOTO_DTYPE, WEATHER_RAIN, WEATHER_SHADOW,
                      TrainPairParams)

_F = np.float32
_EPS = np.finfo(np.float32).eps
RAIN_COLOUR, RAIN_LENGTH, RAIN_BLUR = 200, 20, 7      # albumentations' RandomRain defaults: the drop's value, its height, cv2.blur's side
POISSON_TERMS = 160                                   # the length of ISONoise's CDF: beyond it Poisson(64) holds less than 1e-20
ISO_LAMBDA_MAX = 64.0                                 # sigma_L <= 0.5, intensity <= 0.5: lambda = sigma_L intensity 255 < 64


# ------------------------------------------------------------------------------------------------------------------- RGB <-> HLS
def rgb_to_hls_f32(rgb: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_RGB2HLS) on fp32 (..., 3) in [0, 1]: H in [0, 360), L, S.  l = (max + min) 0.5; s = d / (max + min) when
    l < 0.5, d / ((2 - max) - min) otherwise; h from the maximal channel (r first, then g) with 60 / d, + 360 when negative; a d that
    does not exceed FLT_EPSILON gives h = s = 0."""
    c = np.asarray(rgb, dtype=np.float32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    vmax, vmin = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d, total = vmax - vmin, vmax + vmin
    l = total * _F(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(l < _F(0.5), d / total, d / ((_F(2.0) - vmax) - vmin))
        k = _F(60.0) / d
        h = np.where(vmax == r, (g - b) * k, np.where(vmax == g, (b - r) * k + _F(120.0), (r - g) * k + _F(240.0)))
        h = np.where(h < 0, h + _F(360.0), h)
    flat = ~(d > _EPS)
    out = np.stack([np.where(flat, _F(0.0), h), l, np.where(flat, _F(0.0), s)], axis=-1)
    assert out.dtype == np.float32
    return out


def hls_to_rgb_f32(hls: np.ndarray, hscale: np.float32 = _F(6.0 / 360.0)) -> np.ndarray:
    """cv2.cvtColor(COLOR_HLS2RGB) on fp32 (..., 3), H in degrees (`hscale` = 6 / the hue range): s == 0 is gray; otherwise
    p2 = l (1 + s) when l <= 0.5, (l + s) - l s above, p1 = 2 l - p2, h' = h hscale brought into [0, 6) by one step of 6 either way, and
    cv2's sector table over (p2, p1, p1 + (p2 - p1) (1 - f), p1 + (p2 - p1) f)."""
    c = np.asarray(hls, dtype=np.float32)
    h, l, s = c[..., 0], c[..., 1], c[..., 2]
    one = _F(1.0)
    p2 = np.where(l <= _F(0.5), l * (one + s), (l + s) - l * s)
    p1 = _F(2.0) * l - p2
    hh = h * _F(hscale)
    hh = np.where(hh < 0, hh + _F(6.0), hh)
    hh = np.where(hh >= _F(6.0), hh - _F(6.0), hh)
    sector = np.floor(hh)
    f = hh - sector
    k = np.clip(np.nan_to_num(sector), 0, 5).astype(np.int64)
    span = p2 - p1
    tab = np.stack([p2, p1, p1 + span * (one - f), p1 + span * f], axis=-1)
    bgr = np.take_along_axis(tab, _SECTOR_BGR[k], axis=-1)
    out = np.where((s == 0)[..., None], l[..., None], bgr[..., ::-1])
    assert out.dtype == np.float32
    return out


def rgb_to_hls_u8(rgb: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_RGB2HLS) on uint8 (..., 3), H in [0, 180]: the channels times fp32(1 / 255), `rgb_to_hls_f32`, then
    saturate(rint(h / 2)), saturate(rint(l 255)), saturate(rint(s 255)), half to even."""
    hls = rgb_to_hls_f32(np.asarray(rgb).astype(np.float32) * _F(1.0 / 255.0))
    return np.stack([_round_u8(hls[..., 0] * _F(0.5)), _round_u8(hls[..., 1] * _F(255.0)), _round_u8(hls[..., 2] * _F(255.0))], axis=-1)


def hls_to_rgb_u8(hls: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_HLS2RGB) on uint8 (..., 3) with H in half degrees: h = fp32(H), l and s times fp32(1 / 255), `hls_to_rgb_f32`
    at hscale = 6 / 180, then saturate(rint(c 255))."""
    v = np.asarray(hls)
    f = np.stack([v[..., 0].astype(np.float32), v[..., 1].astype(np.float32) * _F(1.0 / 255.0),
                  v[..., 2].astype(np.float32) * _F(1.0 / 255.0)], axis=-1)
    return _round_u8(hls_to_rgb_f32(f, _F(6.0 / 180.0)) * _F(255.0))


def _scale_lightness_u8(rgb: np.ndarray, factor: float) -> np.ndarray:
    """RGB -> HLS (8-bit), L = trunc(fp32(L) fp32(factor)), HLS -> RGB."""
    hls = rgb_to_hls_u8(rgb)
    hls[..., 1] = (hls[..., 1].astype(np.float32) * _F(factor)).astype(np.uint8)
    return hls_to_rgb_u8(hls)


# ----------------------------------------------------------------------------------------------------------------- masks
def line_points(xs: int, ys: int, xe: int, ye: int) -> np.ndarray:
    """The pixels of `line_u8`'s raster for any end points, (n, 2) int64 of (x, y): OpenCV's 8-connected line, left to right, one pixel per
    step of the longer axis.  Nothing is clipped here."""
    x, y, dx, dy = int(xs), int(ys), int(xe) - int(xs), int(ye) - int(ys)
    if dx < 0:
        x, y, dx, dy = int(xe), int(ye), -dx, -dy
    step_y = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err = major - 2 * minor
    out = np.empty((major + 1, 2), dtype=np.int64)
    for i in range(major + 1):
        out[i] = (x, y)
        diag = err < 0
        err += -2 * minor + (2 * major if diag else 0)
        if steep:
            y += step_y
            x += 1 if diag else 0
        else:
            x += 1
            y += step_y if diag else 0
    return out


def _raster(mask: np.ndarray, segments: np.ndarray) -> None:
    """Set `mask` (H, W) bool along the `line_points` raster of every (x0, y0, x1, y1) row of `segments`, clipped to the mask."""
    H, W = mask.shape
    for seg in np.asarray(segments).reshape(-1, 4):
        p = line_points(*(int(v) for v in seg))
        p = p[(p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)]
        mask[p[:, 1], p[:, 0]] = True


def polygon_edges(vertices: np.ndarray) -> np.ndarray:
    """(n, 2) vertices (x, y) -> (n, 4) edges (x0, y0, x1, y1), the last one closing the polygon."""
    v = np.asarray(vertices).reshape(-1, 2)
    return np.concatenate([v, np.roll(v, -1, axis=0)], axis=1)


def shadow_mask(H: int, W: int, polygons: Sequence[np.ndarray]) -> np.ndarray:
    """RandomShadow's mask, (H, W) bool: the union over `polygons` (each (n, 2) vertices) of the pixels inside by the even-odd rule on
    integer pixel coordinates — an edge counts for pixel (x, y) when y0 <= y < y1 (its ends ordered by y) and (x - x0) (y1 - y0) <
    (y - y0) (x1 - x0), in integers — and of the `line_points` raster of every edge, clipped to the crop."""
    mask = np.zeros((H, W), dtype=bool)
    for poly in polygons:
        mask |= _edges_mask(H, W, polygon_edges(poly).astype(np.int64))
    return mask


def shadow_u8_host(crop: np.ndarray, polygons: Sequence[np.ndarray]) -> np.ndarray:
    """RandomShadow on a uint8 (H, W, 3) crop: where `shadow_mask` is set, RGB -> HLS (8-bit), L = trunc(L 0.5), HLS -> RGB."""
    v = np.ascontiguousarray(crop)
    mask = shadow_mask(v.shape[0], v.shape[1], polygons)
    out = v.copy()
    out[mask] = _scale_lightness_u8(v[mask], 0.5)
    return out


def rain_paint_u8(crop: np.ndarray, drops: np.ndarray) -> np.ndarray:
    """The crop with 200 in all three channels along the raster of every (x0, y0, x1, y1) row of `drops`, clipped."""
    out = np.array(crop, dtype=np.uint8)
    mask = np.zeros(out.shape[:2], dtype=bool)
    _raster(mask, drops)
    out[mask] = RAIN_COLOUR
    return out


_BOX7 = np.zeros((), dtype=PHOTO_DTYPE)
_BOX7["blur"], _BOX7["ksize"], _BOX7["tap_row"] = BLUR_BOX, RAIN_BLUR, -1


def rain_u8_host(crop: np.ndarray, drops: np.ndarray) -> np.ndarray:
    """RandomRain on a uint8 (H, W, 3) crop: the drops painted (`rain_paint_u8`), `photometric_u8_host`'s Blur at k = 7, then on every
    pixel RGB -> HLS (8-bit), L = trunc(fp32(L) fp32(0.7)), HLS -> RGB."""
    v = np.ascontiguousarray(crop)
    _even_sides(v, "weather")
    return _scale_lightness_u8(photometric_u8_host(rain_paint_u8(v, drops), _BOX7, None, None), 0.7)


# ------------------------------------------------------------------------------------------------------------------- ISONoise
_EXP_TABLE = None


def iso_exp_table() -> np.ndarray:
    """ISONoise's table of exp(-i / 16), i = 0 .. 1024: (1025,) float64, made here and uploaded, so that no exponential is evaluated on
    the device."""
    global _EXP_TABLE
    if _EXP_TABLE is None:
        _EXP_TABLE = np.exp(-np.arange(1025, dtype=np.float64) / 16.0)
    return _EXP_TABLE


def iso_lambda_q(crop: np.ndarray, intensity: float) -> float:
    """ISONoise's Poisson mean for a uint8 (H, W, 3) crop: S1 = sum(max + min), S2 = sum((max + min)^2) over the pixels as integers,
    sigma_L = sqrt(max(S2 / N - (S1 / N)^2, 0)) / 510 and lambda = sigma_L intensity 255 in float64, quantised to rint(16 lambda) / 16 and
    clipped to [0, 64]."""
    v = np.asarray(crop).astype(np.int64)
    t = v.max(axis=-1) + v.min(axis=-1)
    n = np.float64(t.size)
    s1, s2 = np.float64(int(t.sum())), np.float64(int((t * t).sum()))
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, np.float64(0.0))
    lam = (np.sqrt(var) / np.float64(510.0)) * np.float64(intensity) * np.float64(255.0)
    lam = np.rint(lam * np.float64(16.0)) / np.float64(16.0)
    return float(lam) if lam >= 0.0 and lam <= ISO_LAMBDA_MAX else (ISO_LAMBDA_MAX if lam > ISO_LAMBDA_MAX else 0.0)


def poisson_cdf(lam_q: float, exp_table: np.ndarray) -> np.ndarray:
    """(160,) float64: p_0 = exp_table[16 lambda_q], p_j = (p_{j-1} lambda_q) / j, summed strictly in order."""
    lam = np.float64(lam_q)
    cdf = np.empty(POISSON_TERMS, dtype=np.float64)
    p = np.float64(exp_table[int(lam * 16.0)])
    acc = p
    cdf[0] = acc
    for j in range(1, POISSON_TERMS):
        p = (p * lam) / np.float64(j)
        acc = acc + p
        cdf[j] = acc
    return cdf


def poisson_from_words(words: np.ndarray, cdf: np.ndarray) -> np.ndarray:
    """Inversion: u = word 2^-32, k = the number of CDF entries <= u, at most 159."""
    u = np.asarray(words).astype(np.float64) * np.float64(2.0 ** -32)
    return np.minimum(np.searchsorted(cdf, u, side="right"), POISSON_TERMS - 1).astype(np.int64)


def iso_hue_scale(color_shift: float, intensity: float) -> np.float32:
    return np.float32(float(color_shift) * 360.0 * float(intensity))


def iso_noise_u8_host(crop: np.ndarray, color_shift: float, intensity: float, key: np.ndarray, q: np.ndarray, exp_table: np.ndarray,
                      hue_scale: Optional[np.float32] = None) -> np.ndarray:
    """ISONoise on a uint8 (H, W, 3) crop.  Per pixel, from Philox4x32-10 at counter (x, y, 0, 0) with the crop's key: word 0 -> a
    Poisson(lambda_q) variate k (`iso_lambda_q`, `poisson_cdf`, `poisson_from_words`), the top 12 bits of word 1 -> a quantile of `q`
    times fp32(color_shift 360 intensity).  On the fp32 HLS of the crop times fp32(1 / 255): h += noise, + 360 when negative, then - 360
    when above 360; l += (fp32(k) fp32(1 / 255)) (1 - l).  Back to RGB, times 255, trunc(clip(., 0, 255))."""
    v = np.ascontiguousarray(crop)
    _even_sides(v, "noise")
    H, W = v.shape[:2]
    scale = iso_hue_scale(color_shift, intensity) if hue_scale is None else np.float32(hue_scale)
    cdf = poisson_cdf(iso_lambda_q(v, intensity), exp_table)
    yy, xx = np.mgrid[0:H, 0:W]
    counter = np.stack([xx, yy, np.zeros_like(xx), np.zeros_like(xx)], axis=-1)
    words = philox4x32_10(counter, np.asarray(key))
    k = poisson_from_words(words[..., 0], cdf)
    noise = np.asarray(q, dtype=np.float32)[words[..., 1] >> np.uint32(20)] * scale
    hls = rgb_to_hls_f32(v.astype(np.float32) * _F(1.0 / 255.0))
    h = hls[..., 0] + noise
    h = np.where(h < 0, h + _F(360.0), h)
    h = np.where(h > _F(360.0), h - _F(360.0), h)
    l = hls[..., 1]
    l = l + (k.astype(np.float32) * _F(1.0 / 255.0)) * (_F(1.0) - l)
    rgb = hls_to_rgb_f32(np.stack([h, l, hls[..., 2]], axis=-1)) * _F(255.0)
    assert rgb.dtype == np.float32
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the operator
def hls_u8_host(crop: np.ndarray, op, segments: np.ndarray, q: np.ndarray, exp_table: np.ndarray) -> np.ndarray:
    """fear_hls_u8's result for one (H, W, 3) uint8 crop and its FearHlsOp record `op` (an HLS_DTYPE scalar): ISONoise from the record's
    scalars, RandomRain over rows seg_offset .. + seg_count of `segments` as drops, RandomShadow over them as polygons (a row
    (n, 0, 0, 0) in front of each polygon's n edges).  Any other kind, and a negative offset or count, copies the crop."""
    v = np.ascontiguousarray(crop)
    _even_sides(v, "HLS")
    kind, off, cnt = int(op["kind"]), int(op["seg_offset"]), int(op["seg_count"])
    if kind == HLS_ISO:
        return iso_noise_u8_host(v, 0.0, float(op["intensity"]), op["key"], q, exp_table, hue_scale=op["hue_scale"])
    if kind not in (HLS_RAIN, HLS_SHADOW) or off < 0 or cnt < 0:
        return v.copy()
    rows = np.asarray(segments).reshape(-1, 4)[off:off + cnt].astype(np.int64)
    if kind == HLS_RAIN:
        return rain_u8_host(v, rows)
    mask = np.zeros(v.shape[:2], dtype=bool)
    i = 0
    while i < len(rows):                       # a polygon: its edge count, then its edges (cut to the rows there are)
        n = int(np.clip(rows[i, 0], 0, len(rows) - i - 1))
        edges = rows[i + 1:i + 1 + n]
        mask |= _edges_mask(v.shape[0], v.shape[1], edges)
        i += 1 + n
    out = v.copy()
    out[mask] = _scale_lightness_u8(v[mask], 0.5)
    return out


def _edges_mask(H: int, W: int, edges: np.ndarray) -> np.ndarray:
    """`shadow_mask` of one polygon given by its edges."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    odd = np.zeros((H, W), dtype=bool)
    for x0, y0, x1, y1 in edges:
        if y0 == y1:
            continue
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        odd ^= (yy >= y0) & (yy < y1) & ((xx - x0) * (y1 - y0) < (yy - y0) * (x1 - x0))
    _raster(odd, edges)
    return odd


def shadow_segments(polygons: Sequence[np.ndarray]) -> np.ndarray:
    """The rows of `segments` for one crop's polygons: (n, 0, 0, 0), then the polygon's n edges, for each polygon; (m, 4) int16."""
    rows = []
    for poly in polygons:
        edges = polygon_edges(poly)
        rows += [np.array([[len(edges), 0, 0, 0]]), edges]
    return np.concatenate(rows).astype(np.int16) if rows else np.zeros((0, 4), dtype=np.int16)


def rain_segments(slant: int, drops: np.ndarray) -> np.ndarray:
    """The rows of `segments` for one crop's drops (n, 2) of (x, y): (x, y, x + slant, y + 20), (n, 4) int16."""
    d = np.asarray(drops).reshape(-1, 2).astype(np.int64)
    return np.concatenate([d, d + np.array([int(slant), RAIN_LENGTH])], axis=1).astype(np.int16)


def rain_drop_count(side: int) -> int:
    return side * side // 600


def hls_tables(params: TrainPairParams, sides: Tuple[int, int]) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], np.ndarray]:
    """The FearHlsOp records of a batch, (B, 2) each, and their segment table: (iso, weather, segments).  `iso` holds the crops that drew
    ISONoise (kind 0 for the others) and is None when none did; `weather` the crops that drew RandomRain or RandomShadow, likewise.  When
    no crop drew both, the two are merged into one set of records, returned as `iso` with `weather` None: fear_hls_u8 then runs once.
    `sides` are the sides of the template and the search crops (a crop's number of drops is side^2 // 600).  `segments` is (m, 4) int16
    with m >= 1."""
    photo = params.photo
    B = photo.noise.shape[0]
    drew_iso = np.asarray(photo.noise) == NOISE_ISO
    kinds = np.zeros((B, 2), dtype=np.int32) if params.weather is None else np.asarray(params.weather)
    drew_rain, drew_shadow = kinds == WEATHER_RAIN, kinds == WEATHER_SHADOW
    iso = weather = None
    rows = [np.zeros((1, 4), dtype=np.int16)]
    n_rows = 1
    if drew_iso.any():
        if params.iso_intensity is None:
            raise ValueError("a crop drew ISONoise, but the params carry no values for it (drawn without iso_noise?)")
        iso = np.zeros((B, 2), dtype=HLS_DTYPE)
        iso["kind"] = np.where(drew_iso, HLS_ISO, HLS_COPY)
        iso["intensity"] = params.iso_intensity
        iso["hue_scale"] = (np.asarray(params.iso_color_shift, dtype=np.float64) * 360.0 * np.asarray(params.iso_intensity, dtype=np.float64)
                            ).astype(np.float32)
        iso["key"] = params.iso_key
    if drew_rain.any() or drew_shadow.any():
        weather = np.zeros((B, 2), dtype=HLS_DTYPE)
        for b, j in np.argwhere(drew_rain | drew_shadow):
            if drew_rain[b, j]:
                seg = rain_segments(int(params.rain_slant[b, j]), params.rain_drops[b, j, :rain_drop_count(sides[j])])
                weather["kind"][b, j] = HLS_RAIN
            else:
                seg = shadow_segments(params.shadow_vertices[b, j, :int(params.shadow_num[b, j])])
                weather["kind"][b, j] = HLS_SHADOW
            weather["seg_offset"][b, j], weather["seg_count"][b, j] = n_rows, len(seg)
            rows.append(seg)
            n_rows += len(seg)
    if iso is not None and weather is not None and not (drew_iso & (drew_rain | drew_shadow)).any():
        iso[~drew_iso] = weather[~drew_iso]
        weather = None
    elif iso is None:
        iso, weather = weather, None
    return iso, weather, np.concatenate(rows)


__all__ = ["rgb_to_hls_f32", "hls_to_rgb_f32", "rgb_to_hls_u8", "hls_to_rgb_u8", "line_points", "polygon_edges", "shadow_mask",
           "shadow_u8_host", "rain_paint_u8", "rain_u8_host", "iso_exp_table", "iso_lambda_q", "poisson_cdf", "poisson_from_words",
           "iso_hue_scale", "iso_noise_u8_host", "hls_u8_host", "shadow_segments", "rain_segments", "rain_drop_count", "hls_tables",
           "POISSON_TERMS", "ISO_LAMBDA_MAX", "RAIN_COLOUR", "RAIN_LENGTH", "RAIN_BLUR"]
