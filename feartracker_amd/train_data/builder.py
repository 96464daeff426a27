"""`TrainPairBuilder`: the draws, the per-pair host tables, the numpy restatement `build_host` and the device's `build`."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ..geometry import border_color_u8
from ..train_abi import launch, load_train_library
from .colour import _colour_u8, _normalise_u8, colour_luts, colour_tables, colour_u8_host
from .hls import hls_tables, iso_exp_table, rain_drop_count
from .photometric import normal_quantiles, photo_tables, photometric_host, split_jpeg_records
from .records import (COLOUR_MEMBERS, COLOUR_NONE, CONTEXT_SIZE, DEFAULT_TRAIN_DATA_CONFIG, DEVICE_COLOUR_KINDS, BLUR_GLASS, BLUR_NONE, FRAME_DTYPE,
                      GEOM_DTYPE, HLS_COPY, N_QUANTILES, NOISE_ISO, NOISE_JPEG, NOISE_MEMBERS, NOISE_NONE, PHOTO_DTYPE, SCORE_SIZE,
                      SEARCH_SIZE, SHADOW_POLYGONS, SHADOW_VERTICES, TEMPLATE_SIZE, TONE_NONE, WEATHER_MEMBERS, WEATHER_NONE, WINDOW_DTYPE, PhotoParams, WindowFrames,
                      TrainBatch, TrainPairParams, _pairs_array)
from .staging import Staging
from .warp import (_box_in_crop, _ensure, _extend, apply_to_bbox, crop_u8, encode_targets, invert_affine, jittered_crop, remap_affine_u8,
                   warp_matrix)


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
        self.colour_members = self._members(self.config["colour_members"], COLOUR_MEMBERS, "colour")
        self.noise_members = self._members(self.config["noise_members"], NOISE_MEMBERS, "noise")
        self.weather_members = self._members(self.config["weather_members"], WEATHER_MEMBERS, "weather", empty=True)
        for name in ("iso_color_shift", "iso_intensity"):
            low, high = (float(v) for v in self.config[name])
            if not 0.0 <= low <= high or (name == "iso_intensity" and high > 0.5):
                raise ValueError(f"{name} must be (low, high) with 0 <= low <= high" + (" <= 0.5" if name == "iso_intensity" else ""))
        lo, hi = (int(v) for v in self.config["jpeg_quality"])
        if not 1 <= lo <= hi <= 100:
            raise ValueError("jpeg_quality must be (low, high) with 1 <= low <= high <= 100")
        self._device_colour = any(COLOUR_MEMBERS[m] in DEVICE_COLOUR_KINDS for m in self.colour_members)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.generator = np.random.default_rng(seed)
        self._qtable = self._exp_table = None

    @staticmethod
    def _members(value, table: Dict[str, int], group: str, empty: bool = False) -> Tuple[str, ...]:
        """`colour_members`, `noise_members` or `weather_members` as a tuple of names in the order of its table (COLOUR_MEMBERS,
        NOISE_MEMBERS, WEATHER_MEMBERS): "all", or any subset (KeyError for a name that is no member), non-empty unless `empty`."""
        if isinstance(value, str):
            value = tuple(table) if value == "all" else (value,)
        names = tuple(value)
        unknown = [m for m in names if m not in table]
        if unknown:
            raise KeyError(f"unknown {group} members {unknown}: the members are {list(table)}")
        if (not names and not empty) or len(set(names)) != len(names):
            raise ValueError(f"{group}_members must name {'its members' if empty else 'at least one member,'} each once")
        return tuple(m for m in table if m in names)

    # ------------------------------------------------------------------ draws
    def draw(self, pairs, frame_shapes: Sequence[Tuple[int, ...]], generator: Optional[np.random.Generator] = None) -> TrainPairParams:
        """Every random parameter of a batch, vectorised, from `generator` (the builder's own when None).  The draws mirror the
        reference's: u = U * range + (2 context - range / 2) (tracking_dataset.py:102-105); scale ~ U(-0.35, 0.35), shift ~
        U(-48, 48) (aug.py:90-93); tone at p = 0.05, colour at p = 0.5, each picking uniformly among its members.
        Of `pairs` the draws read the number of rows B and nothing else, and `frame_shapes` is only recorded: two tables of the same B
        give equal params from the same generator state (what `frame_scales` and `PairLoader(scale="auto")` rely on)."""
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
        if photo is not None:                                           # behind every draw there was before these members
            extra.update(self._draw_hls(B, rng, photo))
        if photo is not None and cfg["glass_blur"]:                     # GlassBlur, behind those again: a blur becomes it at 1 / 5
            u = rng.random((B, 2))
            photo.blur[(photo.blur != BLUR_NONE) & (u < 1.0 / 5)] = BLUR_GLASS
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

    def _draw_hls(self, B: int, rng: np.random.Generator, photo: PhotoParams) -> Dict[str, np.ndarray]:
        """The draws of fear_hls_u8's members, (B, 2, ...), each set only when configured.  ISONoise: a uniform u, color_shift and
        intensity uniform over their limits, a Philox key; a crop on which the noise group fired takes ISONoise in the picked member's
        place when u < 1 / (len(noise_members) + 1) (`photo.noise` becomes NOISE_ISO there).  Weather: a uniform against weather_p and a
        pick among the members; then RandomRain's slant, integers in [-10, 10], and its H W // 600 drops, x an integer in [slant, W] for a
        negative slant and in [0, W - slant] otherwise, y in [0, H - 20]; then RandomShadow's number of polygons, 1 or 2, and five
        vertices for each of two, x an integer in [0, W], y in [H // 2, H].  Every interval includes both of its ends, as Python's
        random.randint does, which albumentations draws these with."""
        cfg, out = self.config, {}
        if cfg["iso_noise"]:
            u = rng.random((B, 2))
            out["iso_color_shift"] = rng.uniform(cfg["iso_color_shift"][0], cfg["iso_color_shift"][1], size=(B, 2))
            out["iso_intensity"] = rng.uniform(cfg["iso_intensity"][0], cfg["iso_intensity"][1], size=(B, 2))
            out["iso_key"] = rng.integers(0, 2 ** 32, size=(B, 2, 2), dtype=np.uint64).astype(np.uint32)
            photo.noise[(photo.noise != NOISE_NONE) & (u < 1.0 / (len(self.noise_members) + 1))] = NOISE_ISO
        if self.weather_members:
            kinds = np.array([WEATHER_MEMBERS[m] for m in self.weather_members])
            fired = rng.random((B, 2)) < cfg["weather_p"]
            out["weather"] = np.where(fired, kinds[rng.integers(0, len(kinds), size=(B, 2))], WEATHER_NONE).astype(np.int32)
            sides = np.array([TEMPLATE_SIZE, SEARCH_SIZE], dtype=np.int64)
            slant = rng.integers(-10, 11, size=(B, 2))
            drops = np.zeros((B, 2, rain_drop_count(SEARCH_SIZE), 2), dtype=np.int32)
            for j, side in enumerate(sides):
                n = rain_drop_count(int(side))
                low, high = np.minimum(slant[:, j], 0)[:, None], (side - np.maximum(slant[:, j], 0))[:, None]
                drops[:, j, :n, 0] = rng.integers(low, high + 1, size=(B, n))
                drops[:, j, :n, 1] = rng.integers(0, side - 20 + 1, size=(B, n))
            out["rain_slant"], out["rain_drops"] = slant.astype(np.int32), drops
            out["shadow_num"] = rng.integers(1, SHADOW_POLYGONS + 1, size=(B, 2)).astype(np.int32)
            shape = (B, 2, SHADOW_POLYGONS, SHADOW_VERTICES)
            x = rng.integers(0, sides[None, :, None, None] + 1, size=shape)
            y = rng.integers(sides[None, :, None, None] // 2, sides[None, :, None, None] + 1, size=shape)
            out["shadow_vertices"] = np.stack([x, y], axis=-1).astype(np.int32)
        return out

    def _hls(self, params: TrainPairParams, photo: Optional[PhotoParams], B: int):
        """The batch's FearHlsOp records (`hls_tables`) when a crop drew ISONoise or a weather member, None otherwise."""
        if photo is None:
            return None
        drew_iso = (np.asarray(photo.noise) == NOISE_ISO).any()
        drew_weather = params.weather is not None and (np.asarray(params.weather) != WEATHER_NONE).any()
        if drew_iso and not self.config["iso_noise"]:
            raise ValueError("a crop drew ISONoise, but iso_noise is not configured")
        if drew_weather:
            if np.shape(params.weather) != (B, 2):
                raise ValueError(f"weather draws are shaped {np.shape(params.weather)}, the table has {B} pairs")
            if params.rain_drops is None or params.rain_slant is None or params.shadow_num is None or params.shadow_vertices is None:
                raise ValueError("a crop drew a weather member, but the params carry no values for it (drawn without weather_members?)")
            names = {v: k for k, v in WEATHER_MEMBERS.items()}
            for kind in np.unique(np.asarray(params.weather)[np.asarray(params.weather) != WEATHER_NONE]):
                if names.get(int(kind)) not in self.weather_members:
                    raise ValueError(f"a crop drew the weather member {int(kind)}, but weather_members does not configure it")
        if not (drew_iso or drew_weather):
            return None
        return hls_tables(params, (TEMPLATE_SIZE, SEARCH_SIZE))

    def _photo(self, params: TrainPairParams, B: int) -> Optional[PhotoParams]:
        """The batch's photometric draws when the stage is on, None when it is off."""
        if not self.config["photometric"]:
            return None
        if params.photo is None:
            raise ValueError("the photometric stage is on, but params carry no photometric draws (drawn with it off?)")
        if params.photo.blur.shape != (B, 2):
            raise ValueError(f"photometric draws are shaped {params.photo.blur.shape}, the table has {B} pairs")
        if (np.asarray(params.photo.blur) == BLUR_GLASS).any() and not self.config["glass_blur"]:
            raise ValueError("a crop drew GlassBlur, but glass_blur is not configured")
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

    def frame_rows(self, pairs, params: TrainPairParams, frame_shapes: Sequence[Tuple[int, ...]]) -> np.ndarray:
        """(F, 2) int64: per frame the pixel rows [y0, y1) a `build` of these pairs reads — the union (as one range) over the pairs that
        use the frame of the rows of their template context box and of their search context box, cut to the frame; (0, 0) for a frame no
        pair uses or touches.  The boxes are `tables()`'s; a crop samples the frame where 0 <= cy + y < fh for y in [0, ch) (warp.crop_u8)
        and nowhere else, whatever the pair's presence.  What `JpegStore.decode_rows` takes."""
        tab = self.tables(pairs, params)
        geom = tab["geom"]
        F = len(frame_shapes)
        heights = np.array([int(s[0]) for s in frame_shapes], dtype=np.int64).reshape(F)
        lo, hi = np.full(F, np.iinfo(np.int64).max), np.full(F, np.iinfo(np.int64).min)
        for frame, ctx in ((geom["t_frame"], tab["t_ctx"]), (geom["s_frame"], tab["s_ctx"])):
            frame, cy, ch = frame.astype(np.int64), ctx[:, 1].astype(np.int64), ctx[:, 3].astype(np.int64)
            ok = (frame >= 0) & (frame < F)
            # a box without height still clamps its taps to the rows cy - 1 and cy
            np.minimum.at(lo, frame[ok], (cy + np.minimum(ch - 1, 0))[ok])
            np.maximum.at(hi, frame[ok], (cy + np.maximum(ch, 1))[ok])
        lo, hi = np.clip(lo, 0, heights), np.clip(hi, 0, heights)
        rows = np.stack([lo, hi], axis=1)
        rows[lo >= hi] = 0
        return rows

    def frame_windows(self, pairs, params: TrainPairParams, frame_shapes: Sequence[Tuple[int, ...]]) -> np.ndarray:
        """(F, 4) int64: per frame the rectangle [y0, y1) x [x0, x1), as (y0, y1, x0, x1), that a `build` of these pairs reads —
        `frame_rows` with the columns added by the same tap rule (a crop samples the frame where 0 <= cx + x < fw for x in [0, cw), and
        a box without width still clamps its taps to the columns cx - 1 and cx): the union, as one rectangle, over the pairs that use
        the frame of their template context box and of their search context box, cut to the frame; (0, 0, 0, 0) for a frame no pair
        uses or touches.  What `JpegStore.decode_windows` takes."""
        tab = self.tables(pairs, params)
        geom = tab["geom"]
        F = len(frame_shapes)
        sides = np.array([[int(s[0]), int(s[1])] for s in frame_shapes], dtype=np.int64).reshape(F, 2)
        big = np.iinfo(np.int64)
        lo, hi = np.full((F, 2), big.max), np.full((F, 2), big.min)              # [:, 0] rows, [:, 1] columns
        for frame, ctx in ((geom["t_frame"], tab["t_ctx"]), (geom["s_frame"], tab["s_ctx"])):
            frame = frame.astype(np.int64)
            ok = (frame >= 0) & (frame < F)
            for axis, (at, size) in enumerate(((1, 3), (0, 2))):                 # the box's y, h | x, w
                c, n = ctx[:, at].astype(np.int64), ctx[:, size].astype(np.int64)
                np.minimum.at(lo[:, axis], frame[ok], (c + np.minimum(n - 1, 0))[ok])
                np.maximum.at(hi[:, axis], frame[ok], (c + np.maximum(n, 1))[ok])
        lo, hi = np.clip(lo, 0, sides), np.clip(hi, 0, sides)
        out = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], axis=1)
        out[(lo >= hi).any(axis=1)] = 0
        return out

    def frame_scales(self, pairs, params: TrainPairParams, frame_shapes: Sequence[Tuple[int, ...]], max_scale: int = 8) -> np.ndarray:
        """(F,) int64: per frame the largest decode scale of {1, 2, 4, 8}, at most `max_scale`, at which no crop `build` reads from
        the frame is upsampled that was a reduction at full size.  `pairs` is the FULL-size table and the context boxes are
        `tables(pairs, params)`'s.  A template use is resized to TEMPLATE_SIZE, a search use to CONTEXT_SIZE (the crop the search
        context is resized to before the jitter); a use admits the largest s with min(context width, context height) >= s * target,
        a frame takes the minimum over its uses, and a frame no pair uses takes 1.  With `scale_pairs(pairs, scales)` the scaled
        context's sides are the full-size ones' divided by a power of two in front of `_extend`'s truncation, so a side that was at least
        s * target stays at least the target.  `draw` reads of the pairs nothing but their number B (it records `frame_shapes` and
        consumes the generator by B and the configuration alone), so the params drawn on the full-size table are the params of the
        scaled one: draw once, `frame_scales`, `scale_pairs`, then `frame_rows` / `frame_windows` on the scaled shapes."""
        from ..jpeg_frames import _check_scale
        max_scale = _check_scale(max_scale)
        tab = self.tables(pairs, params)
        geom = tab["geom"]
        F = len(frame_shapes)
        scales = np.full(F, max_scale, dtype=np.int64)
        used = np.zeros(F, dtype=bool)
        for frame, ctx, target in ((geom["t_frame"], tab["t_ctx"], TEMPLATE_SIZE), (geom["s_frame"], tab["s_ctx"], CONTEXT_SIZE)):
            frame = frame.astype(np.int64)
            ok = (frame >= 0) & (frame < F)
            side = np.minimum(ctx[:, 2], ctx[:, 3]).astype(np.int64)
            admits = np.ones(side.size, dtype=np.int64)
            for s in (2, 4, 8):
                admits[side >= s * target] = s
            np.minimum.at(scales, frame[ok], admits[ok])
            used[frame[ok]] = True
        scales[~used] = 1
        return scales

    def _params(self, pairs, frames, params):
        if isinstance(frames, WindowFrames):
            shapes = tuple((int(h), int(w)) for h, w in np.asarray(frames.shape).reshape(-1, 2).tolist())
        else:
            shapes = tuple((int(f.shape[0]), int(f.shape[1])) for f in frames)
        if params is None:
            return self.draw(pairs, shapes)
        if params.frame_shapes and tuple(params.frame_shapes) != shapes:
            raise ValueError("params were drawn for other frame shapes")
        return params

    # ------------------------------------------------------------------ host restatement
    def build_host(self, frames: Sequence, pairs, params: Optional[TrainPairParams] = None, borders=None) -> TrainBatch:
        """numpy restatement of `build` (same arithmetic, term for term): the reference `build` is tested against.  `borders`, (F, 3)
        uint8, are used as the frames' border colours in place of their means (`build`'s `borders`).  A `WindowFrames` in place of the
        frames needs them; each of its frames is then read as fear_train_pairs_windows reads it: pixel (y, x) inside the frame's shape
        at the window's [y - oy, x - ox], both clamped to the window, and an empty window as a frame without pixels."""
        if isinstance(frames, WindowFrames):
            if borders is None:
                raise ValueError("a WindowFrames needs borders: the mean over a window is not the frame's mean")
            params = self._params(pairs, frames, params)
            host = []
            for f, (oy, ox), (H, W) in zip(frames.frames, np.asarray(frames.origin).tolist(), np.asarray(frames.shape).tolist()):
                w = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
                if w.shape[0] < 1 or w.shape[1] < 1:
                    host.append(np.zeros((0, 0, 3), dtype=np.uint8))
                    continue
                ys, xs = np.clip(np.arange(H) - oy, 0, w.shape[0] - 1), np.clip(np.arange(W) - ox, 0, w.shape[1] - 1)
                host.append(w[ys[:, None], xs[None, :], :3])
        else:
            host = [f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
            params = self._params(pairs, host, params)
        tab = self.tables(pairs, params)
        geom, lut = tab["geom"], tab["lut"]
        if borders is None:
            borders = [border_color_u8(np.mean(f[:, :, :3], axis=(0, 1))) if f.shape[0] > 0 and f.shape[1] > 0 else np.zeros(3, np.uint8)
                       for f in host]
        else:
            borders = self._given_borders(borders, len(host))
        B = len(geom)
        tmpl = np.empty((B, 3, TEMPLATE_SIZE, TEMPLATE_SIZE), dtype=np.float32)
        srch = np.empty((B, 3, SEARCH_SIZE, SEARCH_SIZE), dtype=np.float32)
        photo = self._photo(params, B)
        if photo is not None:
            ops, taps = photo_tables(photo)
            q = normal_quantiles()
        colour = self._colour_ops(params)
        hls = self._hls(params, photo, B)
        if hls is not None:
            exp_table = iso_exp_table()

        def hls_of(k, which):                # the crop's FearHlsOp records, the ISONoise one and the weather one
            if hls is None:
                return None
            first, second, segments = hls
            if second is None:               # one set of records: each crop's is the one or the other
                rec = first[k, which]
                return (rec, None, segments, exp_table) if ops["noise"][k, which] == NOISE_ISO else (None, rec, segments, exp_table)
            return first[k, which], second[k, which], segments, exp_table

        def finish(crop, k, which):          # colour stage -> (photometric stage) -> normalised fp32
            v = _colour_u8(crop, int(geom["tone"][k]), lut[k])
            if colour is not None:
                v = colour_u8_host(v, colour[0][k], colour[1][k])
            if photo is None:
                return _normalise_u8(v)
            quality = int(params.jpeg_quality[k, which]) if ops["noise"][k, which] == NOISE_JPEG else 0
            return photometric_host(v, ops[k, which], taps, q, quality, hls_of(k, which), bool(self.config["glass_blur"]))

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
    @torch.no_grad()
    def build(self, frames: Sequence, pairs, params: Optional[TrainPairParams] = None, borders=None) -> TrainBatch:
        """The batch on the GPU: template (B,3,128,128), search (B,3,256,256), gt_reg (B,4,16,16), gt_cls (B,1,16,16),
        gt_weight (B,16,16) fp32 and search_bbox (B,4) int32, on the current stream, in the layouts `FEARNetTrainHIP.step` takes.
        Frames are uint8 (H, W, 3) numpy arrays or device tensors.  Host frames and the per-pair tables go up non-blocking from
        pinned memory; with device frames the call never waits for the GPU.
        `borders`, an (F, 3) uint8 device tensor or array, gives the frames' border colours (`JpegStore.borders`, computed once per
        file): the call then skips the `fear_frame_border_u8` launch, the only reader of every pixel of a frame, so that frames of
        which only `frame_rows` is defined (`JpegStore.decode_rows`) give the same batch.  None keeps the launch.
        `frames` may be a `WindowFrames` (`JpegStore.decode_windows` of `frame_windows`): compact tensors with their origins, read by
        `fear_train_pairs_windows` — the same kernel body with another frame-fetch policy — and the same batch.  `borders` is then
        required (ValueError otherwise: the mean over a window is not the frame's mean)."""
        lib, dev = load_train_library(), self.device
        windowed = isinstance(frames, WindowFrames)
        if windowed and borders is None:
            raise ValueError("a WindowFrames needs borders: the mean over a window is not the frame's mean")
        params = self._params(pairs, frames, params)
        tab = self.tables(pairs, params)
        B, F = len(tab["geom"]), len(frames)
        photo = self._photo(params, B)
        colour = self._colour_ops(params)
        staged_u8 = photo is not None or colour is not None
        if photo is not None:
            ops, taps = photo_tables(photo)
        elif colour is not None:               # the crops still leave through fear_photometric_u8: all-"none" records, the normalisation
            ops, taps = np.zeros((B, 2), dtype=PHOTO_DTYPE), np.zeros((0, 49), dtype=np.float32)
        # a batch in which a crop drew ImageCompression (the host knows from the draws) runs three launches per side: the chain up to
        # the noise as uint8 (`ops`, the JPEG crops without noise and Downscale), fear_jpeg_u8 (quality 0, a copy, for the other
        # crops), then the JPEG crops' Downscale and everybody's normalisation (`tail`)
        jpeg = photo is not None and bool((ops["noise"] == NOISE_JPEG).any())
        # a batch in which a crop drew ISONoise or a weather member takes the same path, with fear_hls_u8 behind fear_jpeg_u8: once, or
        # twice (the ISONoise records, then the weather ones) when some crop drew both
        hls = self._hls(params, photo, B)
        # a side on which a crop drew GlassBlur runs fear_glass_u8 in front of those launches, to which its records are "none"
        glass = (ops["blur"] == BLUR_GLASS).any(axis=0) if photo is not None else (False, False)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            st = ctypes.c_void_p(stream.cuda_stream)
            if windowed:                       # fear_frame_window records: the frame's shape, the window's origin and shape
                dframes = [self._frame_on_device(f) for f in frames.frames]
                ftab = np.zeros(F, dtype=WINDOW_DTYPE)
                ftab["data"] = [f.data_ptr() if f.numel() else 0 for f in dframes]
                ftab["h"], ftab["w"] = np.asarray(frames.shape, dtype=np.int32).reshape(F, 2).T
                ftab["y0"], ftab["x0"] = np.asarray(frames.origin, dtype=np.int32).reshape(F, 2).T
                ftab["wh"], ftab["ww"] = [f.shape[0] for f in dframes], [f.shape[1] for f in dframes]
            else:
                dframes = [self._frame_on_device(f) for f in frames]
                ftab = np.zeros(F, dtype=FRAME_DTYPE)
                for i, f in enumerate(dframes):
                    ftab[i] = (f.data_ptr(), f.shape[0], f.shape[1])
            stage = Staging()                  # every table of the call: one pinned buffer, one transfer
            stage.add("frames", ftab)
            stage.add("geom", tab["geom"])
            stage.add("lut", tab["lut"])
            stage.add("search_bbox", tab["search_bbox"].astype(np.int32))
            if staged_u8:                      # per-crop records go up transposed: the templates' first, then the searches', one call each
                hls_records = {} if hls is None else {name: rec for name, rec in zip(("hls_first", "hls_second"), hls[:2]) if rec is not None}
                if jpeg or hls_records:
                    later = np.logical_or.reduce([rec["kind"] != HLS_COPY for rec in hls_records.values()]) if hls_records else None
                    ops, tail, quality = split_jpeg_records(ops, params.jpeg_quality if jpeg else None, later)
                    stage.add("tail", tail.T)
                if jpeg:
                    stage.add("quality", quality.T)
                for name, rec in hls_records.items():
                    stage.add(name, rec.T)
                if hls_records:
                    stage.add("segments", hls[2])
                stage.add("ops", ops.T)
                stage.add("taps", taps)
            if colour is not None:             # one record per pair, shared by its two crops
                stage.add("colour_ops", colour[0])
                stage.add("colour_aux", colour[1])
            stage.upload(dev)
            if borders is None:
                border = torch.empty((max(F, 1), 3), dtype=torch.uint8, device=dev)
            elif isinstance(borders, torch.Tensor):
                if borders.dtype != torch.uint8 or tuple(borders.shape) != (F, 3):
                    raise ValueError(f"borders must be uint8 ({F}, 3)")
                border = borders.to(dev).contiguous()
                if F == 0:
                    border = torch.empty((1, 3), dtype=torch.uint8, device=dev)
            else:
                pinned_border = torch.empty((max(F, 1), 3), dtype=torch.uint8, pin_memory=True)
                pinned_border.numpy()[:F] = self._given_borders(borders, F)
                border = pinned_border.to(dev, non_blocking=True)
            tmpl = torch.empty((B, 3, TEMPLATE_SIZE, TEMPLATE_SIZE), dtype=torch.float32, device=dev)
            srch = torch.empty((B, 3, SEARCH_SIZE, SEARCH_SIZE), dtype=torch.float32, device=dev)
            reg = torch.empty((B, 4, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            cls = torch.empty((B, 1, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            wgt = torch.empty((B, SCORE_SIZE, SCORE_SIZE), dtype=torch.float32, device=dev)
            if borders is None:
                launch(lib, "fear_frame_border_u8", stage.ptr("frames"), F, ptr(border), st)
            if not staged_u8:
                pairs_fn, t_out, s_out = "fear_train_pairs_windows" if windowed else "fear_train_pairs", tmpl, srch
            else:                              # the crops leave the table stage as uint8 HWC for the chain below
                pairs_fn = "fear_train_pairs_windows_u8" if windowed else "fear_train_pairs_u8"
                t_out = torch.empty((B, TEMPLATE_SIZE, TEMPLATE_SIZE, 3), dtype=torch.uint8, device=dev)
                s_out = torch.empty((B, SEARCH_SIZE, SEARCH_SIZE, 3), dtype=torch.uint8, device=dev)
            launch(lib, pairs_fn, stage.ptr("frames"), F, ptr(border), stage.ptr("geom"), stage.ptr("lut"), B, ptr(t_out), ptr(s_out),
                   ptr(reg), ptr(cls), ptr(wgt), st)
            if staged_u8:
                q = ptr(self._quantiles_on_device())
                if hls is not None:
                    exp_table = ptr(self._exp_table_on_device())
                d_taps = stage.ptr("taps") if taps.size else None
                if jpeg:
                    ws_bytes = lib.fear_jpeg_workspace_bytes(B, SEARCH_SIZE, SEARCH_SIZE)      # the larger side's serves both
                    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

                def finish(crops, out, side, which):
                    """One side's chain behind the table stage: [fear_colour_u8] -> [fear_glass_u8] -> [fear_photometric_stage_u8 ->
                    [fear_jpeg_u8] -> [fear_hls_u8, once or twice]] -> fear_photometric_u8, `which` 0 for the templates and 1 for the
                    searches (the second half of the per-crop records)."""
                    if colour is not None:     # the members that are no table
                        src, crops = crops, torch.empty_like(crops)
                        launch(lib, "fear_colour_u8", ptr(src), B, side, side, stage.ptr("colour_ops"), stage.ptr("colour_aux"), ptr(crops), st)
                    half, last = which * B * ops.itemsize, "ops"
                    if glass[which]:
                        src, crops = crops, torch.empty_like(crops)
                        launch(lib, "fear_glass_u8", ptr(src), B, side, side, stage.ptr("ops", half), ptr(crops), st)
                    if jpeg or hls is not None:
                        src, crops = crops, torch.empty_like(crops)
                        launch(lib, "fear_photometric_stage_u8", ptr(src), B, side, side, stage.ptr("ops", half), d_taps, q, ptr(crops), st)
                        last = "tail"
                    if jpeg:
                        src, crops = crops, torch.empty_like(crops)
                        launch(lib, "fear_jpeg_u8", ptr(src), B, side, side, stage.ptr("quality", which * B * quality.itemsize), ptr(ws),
                               ws_bytes, ptr(crops), st)
                    for name, rec in hls_records.items():
                        src, crops = crops, torch.empty_like(crops)
                        launch(lib, "fear_hls_u8", ptr(src), B, side, side, stage.ptr(name, which * B * rec.itemsize), stage.ptr("segments"),
                               q, exp_table, ptr(crops), st)
                    launch(lib, "fear_photometric_u8", ptr(crops), B, side, side, stage.ptr(last, half), d_taps, q, ptr(out), st)

                finish(t_out, tmpl, TEMPLATE_SIZE, 0)
                finish(s_out, srch, SEARCH_SIZE, 1)
            for f in dframes:                          # host frames were allocated here; device frames may live on another stream
                f.record_stream(stream)
            if borders is not None:
                border.record_stream(stream)
            box = stage.view("search_bbox", torch.int32, (B, 4))
        return TrainBatch(tmpl, srch, reg, cls, wgt, box)

    @staticmethod
    def _given_borders(borders, F: int) -> np.ndarray:
        if isinstance(borders, torch.Tensor):
            borders = borders.detach().cpu().numpy()
        arr = np.asarray(borders)
        if arr.dtype != np.uint8 or arr.shape != (F, 3):
            raise ValueError(f"borders must be uint8 ({F}, 3)")
        return arr

    def _quantiles_on_device(self) -> torch.Tensor:
        """GaussNoise's quantile table on the device: uploaded once per builder, non-blocking from pinned memory.  Later builds on
        other streams of the device find it complete only if they are ordered behind the first one, as stream users are."""
        if self._qtable is None:
            pinned = torch.empty(N_QUANTILES, dtype=torch.float32, pin_memory=True)
            np.copyto(pinned.numpy(), normal_quantiles())
            self._qtable = (pinned.to(self.device, non_blocking=True), pinned)     # (the pinned source lives as long as its copy)
        return self._qtable[0]

    def _exp_table_on_device(self) -> torch.Tensor:
        """ISONoise's table of exp(-i / 16) on the device, uploaded once per builder as the quantile table is."""
        if self._exp_table is None:
            table = iso_exp_table()
            pinned = torch.empty(len(table), dtype=torch.float64, pin_memory=True)
            np.copyto(pinned.numpy(), table)
            self._exp_table = (pinned.to(self.device, non_blocking=True), pinned)
        return self._exp_table[0]

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
