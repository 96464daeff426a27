"""The HLS members of the photometric stage on the host (feartracker_amd/train_data/hls.py): cv2's 8-bit RGB <-> HLS against a float64
statement of the same formulas over every colour, the shadow mask against a per-pixel loop, RandomRain, ISONoise's Poisson table, and the
draws of `iso_noise` and `weather_members`.  No GPU."""
import colorsys
import dataclasses
import json
import os

import numpy as np
import pytest

from feartracker_amd import train_data as td
from feartracker_amd.train_data import (BLUR_BOX, HLS_DTYPE, HLS_ISO, NOISE_ISO, NOISE_MEMBERS, NOISE_NONE, PHOTO_DTYPE, WEATHER_MEMBERS,
                                        WEATHER_NONE, WEATHER_RAIN, WEATHER_SHADOW, TrainPairBuilder, hls_to_rgb_f32, hls_to_rgb_u8,
                                        hls_u8_host, iso_exp_table, iso_lambda_q, iso_noise_u8_host, line_points, line_u8,
                                        normal_quantiles, philox4x32_10, photometric_u8_host, poisson_cdf, poisson_from_words,
                                        rain_paint_u8, rain_segments, rain_u8_host, rgb_to_hls_f32, rgb_to_hls_u8, shadow_mask,
                                        shadow_segments, shadow_u8_host)

HERE = os.path.dirname(os.path.abspath(__file__))
DRAWS = os.path.join(HERE, "golden", "train_pairs_draws.npz")
SEED, PAIRS, SHAPES = 20240611, 16, ((48, 64), (256, 480))          # tools/make_colour_draws_golden.py's

# The worst cases over all 2^24 inputs, as measured (DESIGN.md section 11 records them).  fp32 against float64: a rounded fp32 value whose
# error is far below half a level cannot differ from the rounded float64 value by more than one level.
RGB2HLS_WORST = (1, 1, 1)            # H (circular, modulo 180), L, S
HLS2RGB_WORST = 1
ROUND_TRIP_WORST = 5


# ------------------------------------------------------------------------------------------------------------------- RGB <-> HLS
def _all_triples():
    a, b, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.stack([a, b, c], axis=-1).reshape(256, 65536, 3)             # 256 slices, so that no temporary is large


def _rgb_to_hls_f64(rgb):
    """The formulas of `rgb_to_hls_u8` in float64: (h / 2, l 255, s 255) before the rounding."""
    c = rgb.astype(np.float64) / 255.0
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    vmax, vmin = c.max(axis=-1), c.min(axis=-1)
    d, total = vmax - vmin, vmax + vmin
    l = total * 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(l < 0.5, d / total, d / (2.0 - vmax - vmin))
        h = np.where(vmax == r, (g - b) * 60.0 / d, np.where(vmax == g, (b - r) * 60.0 / d + 120.0, (r - g) * 60.0 / d + 240.0))
    h = np.where(h < 0, h + 360.0, h)
    flat = d == 0
    return np.where(flat, 0.0, h) * 0.5, l * 255.0, np.where(flat, 0.0, s) * 255.0


def _hls_to_rgb_f64(hls):
    """The formulas of `hls_to_rgb_u8` in float64: (r, g, b) 255 before the rounding."""
    h, l, s = hls[..., 0].astype(np.float64), hls[..., 1] / 255.0, hls[..., 2] / 255.0
    p2 = np.where(l <= 0.5, l * (1.0 + s), l + s - l * s)
    p1 = 2.0 * l - p2
    hh = h / 30.0
    hh = np.where(hh >= 6.0, hh - 6.0, hh)
    sector = np.floor(hh)
    f = hh - sector
    tab = np.stack([p2, p1, p1 + (p2 - p1) * (1.0 - f), p1 + (p2 - p1) * f], axis=-1)
    bgr = np.take_along_axis(tab, np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector.astype(np.int64)], axis=-1)
    return np.where((hls[..., 2] == 0)[..., None], l[..., None], bgr[..., ::-1]) * 255.0


def test_rgb_to_hls_u8_every_colour():
    worst = np.zeros(3, dtype=np.int64)
    for rgb in _all_triples():
        got = rgb_to_hls_u8(rgb).astype(np.int64)
        h, l, s = (np.clip(np.rint(v), 0, 255).astype(np.int64) for v in _rgb_to_hls_f64(rgb))
        dh = np.abs(got[..., 0] - h) % 180
        worst = np.maximum(worst, [np.minimum(dh, 180 - dh).max(), np.abs(got[..., 1] - l).max(), np.abs(got[..., 2] - s).max()])
        assert got[..., 0].max() <= 180
    print("rgb_to_hls_u8 against float64, worst |dH|, |dL|, |dS| in levels:", worst.tolist())
    assert np.all(worst <= 1)
    assert tuple(worst.tolist()) == RGB2HLS_WORST


def test_rgb_to_hls_follows_colorsys():
    """The float64 statement above is colorsys' (h, l, s), and the fp32 one follows it."""
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (2000, 3), dtype=np.uint8)
    rgb[:64] = rng.integers(0, 2, (64, 3)) * 255                           # corners, and grays
    rgb[64:128] = rgb[64:128, :1]
    ref = np.array([colorsys.rgb_to_hls(*(c / 255.0)) for c in rgb])
    h, l, s = _rgb_to_hls_f64(rgb)
    assert np.abs(h - ref[:, 0] * 180.0).max() < 1e-9 and np.abs(l - ref[:, 1] * 255.0).max() < 1e-9 and np.abs(s - ref[:, 2] * 255.0).max() < 1e-9
    f32 = rgb_to_hls_f32(rgb.astype(np.float32) * np.float32(1.0 / 255.0))
    assert f32.dtype == np.float32
    assert np.abs(f32[:, 0] - ref[:, 0] * 360.0).max() < 2e-3 and np.abs(f32[:, 1:] - ref[:, 1:]).max() < 1e-6
    back = np.array([colorsys.hls_to_rgb(*c) for c in ref])
    assert np.abs(hls_to_rgb_f32(f32) - back).max() < 1e-5


def test_hls_to_rgb_u8_every_triple():
    worst = 0
    for hls in _all_triples():
        got = hls_to_rgb_u8(hls).astype(np.int64)
        ref = np.clip(np.rint(_hls_to_rgb_f64(hls)), 0, 255).astype(np.int64)
        worst = max(worst, int(np.abs(got - ref).max()))
    print("hls_to_rgb_u8 against float64, worst difference in levels:", worst)
    assert worst <= 1
    assert worst == HLS2RGB_WORST


def test_round_trip_every_colour():
    worst = 0
    for rgb in _all_triples():
        hls = rgb_to_hls_u8(rgb)
        assert hls.dtype == np.uint8
        worst = max(worst, int(np.abs(hls_to_rgb_u8(hls).astype(np.int64) - rgb).max()))
    print("RGB -> HLS -> RGB in 8 bits, worst difference in levels:", worst)
    assert worst == ROUND_TRIP_WORST


# ----------------------------------------------------------------------------------------------------------------------- shadow
def _brute_mask(H, W, polygons):
    """The rule of `shadow_mask`, one pixel and one edge at a time in Python integers; the rasters from `line_u8` on a canvas that
    holds every vertex."""
    mask = np.zeros((H, W), dtype=bool)
    for poly in polygons:
        pts = [(int(x), int(y)) for x, y in poly]
        edges = list(zip(pts, pts[1:] + pts[:1]))
        for y in range(H):
            for x in range(W):
                crossings = 0
                for (x0, y0), (x1, y1) in edges:
                    if y0 > y1:
                        x0, y0, x1, y1 = x1, y1, x0, y0
                    if y0 <= y < y1 and (x - x0) * (y1 - y0) < (y - y0) * (x1 - x0):
                        crossings += 1
                mask[y, x] |= crossings % 2 == 1
        k = max(H, W, max(max(p) for p in pts) + 1)
        for (x0, y0), (x1, y1) in edges:
            mask |= line_u8(k, x0, y0, x1, y1)[:H, :W].astype(bool)
    return mask


SHADOW_CASES = {
    "a triangle": [[(3, 10), (25, 14), (9, 19)]],
    "a pentagon that crosses itself": [[(2, 10), (28, 10), (6, 19), (15, 4), (24, 19)]],
    "a horizontal edge": [[(4, 12), (20, 12), (26, 18), (12, 19), (2, 16)]],
    "vertices on the border": [[(0, 10), (32, 10), (32, 20), (16, 14), (0, 20)]],
    "two polygons that overlap": [[(2, 10), (20, 11), (18, 19), (4, 18), (10, 14)], [(12, 12), (30, 10), (31, 19), (14, 20), (22, 15)]],
}


@pytest.mark.parametrize("name", list(SHADOW_CASES))
def test_shadow_mask_equals_the_per_pixel_rule(name):
    H, W = 20, 32
    polygons = [np.array(p) for p in SHADOW_CASES[name]]
    mask = shadow_mask(H, W, polygons)
    assert np.array_equal(mask, _brute_mask(H, W, polygons))
    assert mask.any() and not mask.all()
    crop = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = shadow_u8_host(crop, polygons)
    assert np.array_equal(out[~mask], crop[~mask])
    hls = rgb_to_hls_u8(crop[mask])
    hls[..., 1] = (hls[..., 1] * 0.5).astype(np.uint8)
    assert np.array_equal(out[mask], hls_to_rgb_u8(hls))
    # and through the record: the polygons as rows of the segment table
    seg = np.concatenate([np.zeros((2, 4), np.int16), shadow_segments(polygons)])
    op = np.zeros((), dtype=HLS_DTYPE)
    op["kind"], op["seg_offset"], op["seg_count"] = td.HLS_SHADOW, 2, len(seg) - 2
    assert np.array_equal(hls_u8_host(crop, op, seg, None, None), out)


def test_two_polygons_are_a_union():
    a, b = (np.array(p) for p in SHADOW_CASES["two polygons that overlap"][0:2])
    both, one, other = shadow_mask(20, 32, [a, b]), shadow_mask(20, 32, [a]), shadow_mask(20, 32, [b])
    assert (one & other).any() and np.array_equal(both, one | other)


def test_line_points_is_line_u8():
    rng = np.random.default_rng(2)
    for _ in range(200):
        k = int(rng.integers(2, 24))
        xs, ys, xe, ye = (int(v) for v in rng.integers(0, k, 4))
        img = np.zeros((k, k), np.uint8)
        p = line_points(xs, ys, xe, ye)
        img[p[:, 1], p[:, 0]] = 1
        assert np.array_equal(img, line_u8(k, xs, ys, xe, ye))
        assert len(p) == max(abs(xe - xs), abs(ye - ys)) + 1


# ------------------------------------------------------------------------------------------------------------------------- rain
def test_rain():
    H, W = 34, 40
    crop = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    drops = np.concatenate([rain_segments(-10, [[4, 5], [W, 2], [12, H - 20]]),       # out on the left, in from the right, to the last row
                            rain_segments(10, [[W - 4, 8], [20, -6], [3, H - 8]]),    # out on the right, in from above, out below
                            rain_segments(0, [[17, 9]])])                             # slant 0: a vertical drop
    painted = rain_paint_u8(crop, drops)
    on = (painted != crop).any(axis=-1)
    assert np.all(painted[on] == 200) and on[9:30, 17].all() and not on[8, 17] and not on[30, 17]
    for side in (on[:, 0], on[:, -1], on[0], on[-1]):
        assert side.any()                                                             # a drop reaches every side of the crop
    assert on.sum() < sum(21 for _ in drops)                                          # and some of their pixels fell outside
    box = np.zeros((), dtype=PHOTO_DTYPE)
    box["blur"], box["ksize"], box["tap_row"] = BLUR_BOX, 7, -1
    blurred = photometric_u8_host(painted, box, None, None)
    hls = rgb_to_hls_u8(blurred)
    hls[..., 1] = (hls[..., 1].astype(np.float32) * np.float32(0.7)).astype(np.uint8)
    assert np.array_equal(rain_u8_host(crop, drops), hls_to_rgb_u8(hls))
    # no drop: the blur and the darkening alone
    hls = rgb_to_hls_u8(photometric_u8_host(crop, box, None, None))
    hls[..., 1] = (hls[..., 1].astype(np.float32) * np.float32(0.7)).astype(np.uint8)
    assert np.array_equal(rain_u8_host(crop, np.zeros((0, 4), np.int16)), hls_to_rgb_u8(hls))


# --------------------------------------------------------------------------------------------------------------------- ISONoise
def test_iso_noise_on_a_crop_of_one_colour():
    """lambda = 0: every Poisson variate is 0, so L stays; without hue noise the crop is the fp32 round trip of itself."""
    crop = np.broadcast_to(np.array([90, 200, 30], np.uint8), (8, 12, 3)).copy()
    assert iso_lambda_q(crop, 0.5) == 0.0
    cdf = poisson_cdf(0.0, iso_exp_table())
    assert np.all(cdf == 1.0)
    assert not poisson_from_words(np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32), cdf).any()
    q, key = normal_quantiles(), np.array([5, 6], np.uint32)
    still = iso_noise_u8_host(crop, 0.0, 0.5, key, q, iso_exp_table())
    f = crop.astype(np.float32) * np.float32(1.0 / 255.0)
    assert np.array_equal(still, np.clip(hls_to_rgb_f32(rgb_to_hls_f32(f)) * np.float32(255.0), 0, 255).astype(np.uint8))
    assert np.abs(still.astype(int) - crop).max() <= 1
    moved = iso_noise_u8_host(crop, 0.05, 0.5, key, q, iso_exp_table())
    l_of = lambda v: v.max(axis=-1).astype(int) + v.min(axis=-1)
    assert not np.array_equal(moved, still) and np.abs(l_of(moved) - l_of(crop)).max() <= 2     # the hue moved, the lightness did not


def test_iso_lambda():
    rng = np.random.default_rng(4)
    crop = rng.integers(0, 256, (16, 20, 3), dtype=np.uint8)
    l = (crop.max(axis=-1).astype(np.float64) + crop.min(axis=-1)) / 510.0
    for intensity in (0.1, 0.3, 0.5):
        lam = iso_lambda_q(crop, intensity)
        assert lam * 16 == int(lam * 16) and abs(lam - l.std() * intensity * 255.0) <= 1 / 32 + 1e-9
    half = np.zeros((4, 8, 3), np.uint8)
    half[:, 4:] = 255
    assert iso_lambda_q(half, 0.5) == 63.75 and iso_lambda_q(half, 1.0) == 64.0       # sigma_L = 0.5 is the largest; the cap


def test_poisson_table():
    table = iso_exp_table()
    assert table.shape == (1025,) and table.dtype == np.float64 and table[0] == 1.0 and table[16] == np.exp(-1.0)
    for i in range(1025):                                                             # every lambda_q
        cdf = poisson_cdf(i / 16.0, table)
        assert cdf.shape == (td.POISSON_TERMS,) and np.all(np.diff(cdf) >= 0) and abs(cdf[-1] - 1.0) < 1e-12, i
    yy, xx = np.mgrid[0:256, 0:256]
    words = philox4x32_10(np.stack([xx, yy, 0 * xx, 0 * xx], axis=-1), np.array([123, 456], np.uint32))[..., 0]
    n = words.size
    for lam in (0.5, 8.0, 64.0):
        k = poisson_from_words(words, poisson_cdf(lam, table)).astype(np.float64)
        assert abs(k.mean() - lam) < 4 * np.sqrt(lam / n), lam
        assert abs(k.var() - lam) < 4 * np.sqrt((lam + 2 * lam * lam) / n), lam      # Var(s^2) = (mu_4 - sigma^4) / n, mu_4 = lam + 3 lam^2


def test_iso_noise_per_pixel():
    """One pixel at a time from the contract's words, against the vectorised form."""
    rng = np.random.default_rng(6)
    crop = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    q, table, key = normal_quantiles(), iso_exp_table(), np.array([77, 99], np.uint32)
    out = iso_noise_u8_host(crop, 0.04, 0.45, key, q, table)
    cdf = poisson_cdf(iso_lambda_q(crop, 0.45), table)
    scale = np.float32(0.04 * 360.0 * 0.45)
    one, k255 = np.float32(1.0), np.float32(1.0 / 255.0)
    for y, x in ((0, 0), (5, 7), (2, 3)):
        w = philox4x32_10(np.array([x, y, 0, 0]), key)
        k = int(np.sum(cdf <= float(w[0]) / 2.0 ** 32))
        hls = rgb_to_hls_f32(crop[y, x].astype(np.float32) * k255)
        h = hls[0] + q[int(w[1]) >> 20] * scale
        h = h + np.float32(360.0) if h < 0 else h
        h = h - np.float32(360.0) if h > 360 else h
        l = hls[1] + (np.float32(k) * k255) * (one - hls[1])
        rgb = hls_to_rgb_f32(np.array([h, l, hls[2]], np.float32)) * np.float32(255.0)
        assert np.array_equal(out[y, x], np.clip(rgb, 0, 255).astype(np.uint8)), (y, x)
    op = np.zeros((), dtype=HLS_DTYPE)
    op["kind"], op["intensity"], op["hue_scale"], op["key"] = HLS_ISO, 0.45, scale, key
    assert np.array_equal(hls_u8_host(crop, op, np.zeros((1, 4), np.int16), q, table), out)


# ------------------------------------------------------------------------------------------------------------------------ draws
def _draw(config, n=PAIRS, seed=SEED, rng=None):
    return TrainPairBuilder(config, device="cpu").draw(np.zeros((n, 11)), SHAPES, np.random.default_rng(seed) if rng is None else rng)


@pytest.mark.parametrize("photometric", [False, True])
def test_keys_off_draw_as_before(photometric):
    """tests/golden/train_pairs_draws.npz was recorded before these keys existed: at their defaults, named or not, every array is the
    recorded one and nothing more is drawn."""
    golden = np.load(DRAWS)
    prefix = "on_" if photometric else "off_"
    rng = np.random.default_rng(SEED)
    params = _draw(dict(photometric=photometric, iso_noise=False, weather_members=(), weather_p=0.05), rng=rng)
    rng2 = np.random.default_rng(SEED)
    _draw(dict(photometric=photometric), rng=rng2)
    assert rng.random() == rng2.random()
    for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
        assert np.array_equal(getattr(params, name), golden[prefix + name]), name
    if photometric:
        for f in dataclasses.fields(params.photo):
            assert np.array_equal(getattr(params.photo, f.name), golden[prefix + "photo_" + f.name]), f.name
    for name in ("iso_color_shift", "iso_intensity", "iso_key", "weather", "rain_slant", "rain_drops", "shadow_num", "shadow_vertices"):
        assert getattr(params, name) is None, name
    # the stage off: the keys draw nothing
    off = _draw(dict(iso_noise=True, weather_members="all"))
    assert off.photo is None and off.weather is None and off.iso_key is None


def test_recorded_digests_are_untouched():
    """The digests of tests/golden/train_data_digests.json name no configuration with the new keys, and their builders have them off."""
    with open(os.path.join(HERE, "golden", "train_data_digests.json")) as f:
        recorded = json.load(f)
    assert recorded and not any("iso" in name or "weather" in name for name in recorded)
    assert td.DEFAULT_TRAIN_DATA_CONFIG["iso_noise"] is False and td.DEFAULT_TRAIN_DATA_CONFIG["weather_members"] == ()
    assert td.DEFAULT_TRAIN_DATA_CONFIG["weather_p"] == 0.05
    assert td.DEFAULT_TRAIN_DATA_CONFIG["iso_color_shift"] == (0.01, 0.05) and td.DEFAULT_TRAIN_DATA_CONFIG["iso_intensity"] == (0.1, 0.5)


@pytest.mark.parametrize("noise_members", [("multiplicative", "gauss"), "all"])
def test_new_draws_come_last(noise_members):
    """With the keys on, everything drawn before is drawn first and unchanged, but for the noise member picked."""
    base = dict(photometric=True, colour_members="all", noise_members=noise_members)
    rng, rng2 = np.random.default_rng(SEED), np.random.default_rng(SEED)
    N = 256
    before = _draw(base, n=N, rng=rng2)
    params = _draw(dict(base, iso_noise=True, weather_members="all"), n=N, rng=rng)
    for f in dataclasses.fields(td.TrainPairParams):
        if f.name in ("photo", "frame_shapes") or getattr(before, f.name) is None:
            continue
        assert np.array_equal(getattr(params, f.name), getattr(before, f.name)), f.name
    for f in dataclasses.fields(params.photo):
        if f.name != "noise":
            assert np.array_equal(getattr(params.photo, f.name), getattr(before.photo, f.name)), f.name
    changed = params.photo.noise != before.photo.noise
    assert changed.any() and np.all(params.photo.noise[changed] == NOISE_ISO) and np.all(before.photo.noise[changed] != NOISE_NONE)
    # the new draws in their order, from the stream where the configuration without them stopped
    k = len(TrainPairBuilder(base, device="cpu").noise_members)
    u = rng2.random((N, 2))
    assert np.array_equal(changed, (before.photo.noise != NOISE_NONE) & (u < 1.0 / (k + 1)))
    assert np.array_equal(params.iso_color_shift, rng2.uniform(0.01, 0.05, (N, 2)))
    assert np.array_equal(params.iso_intensity, rng2.uniform(0.1, 0.5, (N, 2)))
    assert np.array_equal(params.iso_key, rng2.integers(0, 2 ** 32, (N, 2, 2), dtype=np.uint64).astype(np.uint32))
    fired, pick = rng2.random((N, 2)) < 0.05, rng2.integers(0, 2, (N, 2))
    assert np.array_equal(params.weather, np.where(fired, pick + 1, WEATHER_NONE))
    assert np.array_equal(params.rain_slant, rng2.integers(-10, 11, (N, 2)))
    # weather alone draws nothing of ISONoise's, and the other way round
    only = _draw(dict(base, weather_members=("shadow",)))
    assert only.iso_key is None and set(np.unique(only.weather)) <= {WEATHER_NONE, WEATHER_SHADOW} and only.rain_drops is not None
    only = _draw(dict(base, iso_noise=True))
    assert only.weather is None and only.rain_drops is None and only.iso_key is not None


def test_member_frequencies():
    n = 10000                                                                         # 20 000 crops
    for members in (("multiplicative", "gauss"), "all"):
        k = 2 if members != "all" else 3
        params = _draw(dict(photometric=True, noise_p=1.0, noise_members=members, iso_noise=True), n=n, seed=21 + k)
        noise = params.photo.noise.reshape(-1)
        assert np.all(noise != NOISE_NONE)
        share = 1.0 / (k + 1)
        sigma = np.sqrt(share * (1 - share) / noise.size)
        for kind in [NOISE_ISO] + [NOISE_MEMBERS[m] for m in TrainPairBuilder(dict(noise_members=members), device="cpu").noise_members]:
            assert abs(np.mean(noise == kind) - share) < 4 * sigma, (members, kind)
        # at the reference's p the group still fires on a fifth of the crops
        noise = _draw(dict(photometric=True, noise_members=members, iso_noise=True), n=n, seed=31 + k).photo.noise.reshape(-1)
        assert abs(np.mean(noise != NOISE_NONE) - 0.2) < 4 * np.sqrt(0.2 * 0.8 / noise.size)
    weather = _draw(dict(photometric=True, weather_members="all", weather_p=1.0), n=n, seed=41).weather.reshape(-1)
    for kind in (WEATHER_RAIN, WEATHER_SHADOW):
        assert abs(np.mean(weather == kind) - 0.5) < 4 * np.sqrt(0.25 / weather.size), kind
    weather = _draw(dict(photometric=True, weather_members="all"), n=n, seed=42).weather.reshape(-1)
    assert abs(np.mean(weather != WEATHER_NONE) - 0.05) < 4 * np.sqrt(0.05 * 0.95 / weather.size)
    assert np.all(_draw(dict(photometric=True, weather_members="rain", weather_p=1.0), n=50).weather == WEATHER_RAIN)


def test_limits_of_the_new_values():
    """Every interval of integers includes both of its ends, pinned by the smallest and the largest value drawn."""
    n = 2000
    p = _draw(dict(photometric=True, iso_noise=True, weather_members="all"), n=n, seed=51)
    assert p.iso_color_shift.shape == p.iso_intensity.shape == (n, 2) and p.iso_key.shape == (n, 2, 2) and p.iso_key.dtype == np.uint32
    assert 0.01 <= p.iso_color_shift.min() < 0.0101 and 0.0499 < p.iso_color_shift.max() < 0.05
    assert 0.1 <= p.iso_intensity.min() < 0.101 and 0.499 < p.iso_intensity.max() < 0.5
    assert p.weather.dtype == p.rain_slant.dtype == p.rain_drops.dtype == p.shadow_num.dtype == p.shadow_vertices.dtype == np.int32
    assert (p.rain_slant.min(), p.rain_slant.max()) == (-10, 10)
    assert p.rain_drops.shape == (n, 2, 256 * 256 // 600, 2) and p.shadow_vertices.shape == (n, 2, 2, 5, 2)
    for j, side in enumerate((128, 256)):
        count = side * side // 600
        assert count == (27, 109)[j] and not p.rain_drops[:, j, count:].any()
        x, y, slant = p.rain_drops[:, j, :count, 0], p.rain_drops[:, j, :count, 1], p.rain_slant[:, j]
        assert (y.min(), y.max()) == (0, side - 20)
        assert (x.min(), x.max()) == (-10, side)
        for s in (-10, -1, 0, 1, 10):                                                 # x in [slant, W] below 0, in [0, W - slant] from 0 on
            xs = x[slant == s]
            assert (xs.min(), xs.max()) == (min(s, 0), side - max(s, 0)), (side, s)
        vx, vy = p.shadow_vertices[:, j, ..., 0], p.shadow_vertices[:, j, ..., 1]
        assert (vx.min(), vx.max()) == (0, side) and (vy.min(), vy.max()) == (side // 2, side)
    assert (p.shadow_num.min(), p.shadow_num.max()) == (1, 2)
    narrow = _draw(dict(photometric=True, iso_noise=True, iso_color_shift=(0.02, 0.02), iso_intensity=(0.3, 0.3)), n=8)
    assert np.all(narrow.iso_color_shift == 0.02) and np.all(narrow.iso_intensity == 0.3)


def test_member_names_are_validated():
    assert NOISE_MEMBERS == {"multiplicative": 1, "gauss": 2, "jpeg": 3} and NOISE_ISO == 4 and NOISE_ISO not in NOISE_MEMBERS.values()
    assert WEATHER_MEMBERS == {"rain": 1, "shadow": 2}
    make = lambda **config: TrainPairBuilder(config, device="cpu")
    assert make(noise_members="all").noise_members == ("multiplicative", "gauss", "jpeg")
    assert make().weather_members == () and make(weather_members=()).weather_members == ()
    assert make(weather_members="all").weather_members == ("rain", "shadow")
    assert make(weather_members=("shadow", "rain")).weather_members == ("rain", "shadow")
    assert make(weather_members="shadow").weather_members == ("shadow",)
    with pytest.raises(KeyError):
        make(weather_members=("rain", "snow"))
    with pytest.raises(KeyError):
        make(noise_members=("gauss", "iso"))
    with pytest.raises(ValueError):
        make(weather_members=("rain", "rain"))
    for bad in (dict(iso_intensity=(0.3, 0.2)), dict(iso_intensity=(0.1, 0.6)), dict(iso_color_shift=(-0.1, 0.05))):
        with pytest.raises(ValueError):
            make(**bad)


def test_build_host_applies_the_members_in_order():
    """One pair: ISONoise on the template, rain behind GaussNoise and in front of the Downscale on the search; and draws a builder
    cannot apply are refused."""
    frames = [np.random.default_rng(5).integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    pairs = np.array([[0, 10, 10, 20, 16, 0, 12, 8, 20, 16, 1]], dtype=np.float64)
    builder = TrainPairBuilder(dict(photometric=True, iso_noise=True, weather_members="all"), device="cpu")
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(6))
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:], params.weather[:] = 0, NOISE_NONE, 0, WEATHER_NONE
    plain = builder.build_host(frames, pairs, params)
    ph.noise[0], ph.downscale[0, 1], params.weather[0, 1] = (NOISE_ISO, td.NOISE_GAUSS), 1, WEATHER_RAIN
    got = builder.build_host(frames, pairs, params)
    u8 = lambda t: np.rint(t.transpose(1, 2, 0) / td._INV_STD + td._MEAN).astype(np.uint8)         # the crop in front of the normalisation
    q, table = normal_quantiles(), iso_exp_table()
    want = iso_noise_u8_host(u8(plain.template[0]), params.iso_color_shift[0, 0], params.iso_intensity[0, 0], params.iso_key[0, 0], q, table)
    assert np.array_equal(u8(got.template[0]), want)
    ops, _ = td.photo_tables(ph)
    op = ops[0, 1].copy()
    op["downscale"] = 0
    noisy = photometric_u8_host(u8(plain.search[0]), op, None, q)
    wet = rain_u8_host(noisy, rain_segments(params.rain_slant[0, 1], params.rain_drops[0, 1]))
    assert np.array_equal(u8(got.search[0]), np.repeat(np.repeat(wet[::2, ::2], 2, axis=0), 2, axis=1))
    with pytest.raises(ValueError):                                                   # neither member is configured
        TrainPairBuilder(dict(photometric=True), device="cpu").build_host(frames, pairs, params)
    with pytest.raises(ValueError):
        TrainPairBuilder(dict(photometric=True, iso_noise=True, weather_members="shadow"), device="cpu").build_host(frames, pairs, params)
    params.iso_intensity = None
    with pytest.raises(ValueError):                                                   # no values to apply
        builder.build_host(frames, pairs, params)
