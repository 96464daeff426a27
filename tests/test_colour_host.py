"""The colour members behind `colour_members` on the host (feartracker_amd/train_data/colour.py): each restatement of
`colour_u8_host` against an independent formulation, and the draws.  The references here are written out in this file; none of them is
the code under test."""
import dataclasses
import itertools
import os

import numpy as np
import pytest

from feartracker_amd import train_data as td
from feartracker_amd.train_data import (COLOUR_DTYPE, COLOUR_EMBOSS, COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_JITTER, COLOUR_MEMBERS,
                                        COLOUR_TONE_CURVE, JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_HUE, JITTER_SATURATION,
                                        TrainPairBuilder, colour_luts, colour_tables, colour_u8_host)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_pairs_draws.npz")
SEED, PAIRS, SHAPES = 20240611, 16, ((48, 64), (256, 480))          # tools/make_colour_draws_golden.py's


def _random(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _op(kind, **fields):
    op = np.zeros(1, dtype=COLOUR_DTYPE)
    op["kind"] = kind
    for name, value in fields.items():
        op[name] = value
    return op[0]


# ----------------------------------------------------------------------------------------------------------------------------- HSV
def _exact_hsv(rgb):
    """float64 HSV of uint8 (N, 3): h in [0, 180) half-degrees, s in [0, 255], no rounding."""
    c = rgb.astype(np.float64)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    v = c.max(axis=1)
    d = v - c.min(axis=1)
    dd = np.where(d == 0, 1.0, d)
    h = np.where(v == r, 60.0 * (g - b) / dd, np.where(v == g, 120.0 + 60.0 * (b - r) / dd, 240.0 + 60.0 * (r - g) / dd))
    h = np.where(d == 0, 0.0, np.where(h < 0, h + 360.0, h)) / 2.0
    s = np.where(v == 0, 0.0, 255.0 * d / np.where(v == 0, 1.0, v))
    return h, s, v


def _exact_rgb(hsv):
    """float64 RGB levels (unrounded, 0..255) of uint8 HSV (N, 3) with h < 180."""
    h, s, v = hsv[:, 0] / 30.0, hsv[:, 1] / 255.0, hsv[:, 2].astype(np.float64)
    k = np.floor(h)
    f = h - k
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    k = k.astype(np.int64) % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=1)


def test_hsv_over_every_colour():
    """All 2^24 colours: h < 180, v = max, circular |h - h*| < 1 and |s - s*| < 1 against float64 HSV (the contract's worst cases are
    0.64 and 0.53), and the round trip through both conversions within 5 levels (worst case 5, at dark saturated colours)."""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst_h = worst_s = worst_rt = 0.0
    for r0 in range(0, 256, 16):
        slab = np.stack([np.broadcast_to(np.arange(r0, r0 + 16, dtype=np.uint8)[:, None, None], (16, 256, 256)),
                         np.broadcast_to(g, (16, 256, 256)), np.broadcast_to(b, (16, 256, 256))], axis=-1).reshape(-1, 3)
        hsv = td.rgb_to_hsv_u8(slab)
        assert hsv.dtype == np.uint8 and int(hsv[:, 0].max()) < 180
        assert np.array_equal(hsv[:, 2], slab.max(axis=1))
        h, s, _ = _exact_hsv(slab)
        dh = np.abs(hsv[:, 0] - h)
        dh = np.minimum(dh, 180.0 - dh)
        worst_h = max(worst_h, float(dh.max()))
        worst_s = max(worst_s, float(np.abs(hsv[:, 1] - s).max()))
        back = td.hsv_to_rgb_u8(hsv)
        worst_rt = max(worst_rt, float(np.abs(back.astype(np.int64) - slab.astype(np.int64)).max()))
    print(f"worst |h - h*| {worst_h:.4f}, worst |s - s*| {worst_s:.4f}, worst round trip {worst_rt:.0f} levels")
    assert worst_h < 1.0 and worst_s < 1.0
    assert worst_rt <= 5


def test_hsv_to_rgb_over_every_hsv():
    """Every (h < 180, s, v): within one level of the float64 formula rounded (fp32's error is far below half a level: only ties move)."""
    s, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst = 0
    for h0 in range(0, 180, 12):
        slab = np.stack([np.broadcast_to(np.arange(h0, h0 + 12, dtype=np.uint8)[:, None, None], (12, 256, 256)),
                         np.broadcast_to(s, (12, 256, 256)), np.broadcast_to(v, (12, 256, 256))], axis=-1).reshape(-1, 3)
        got = td.hsv_to_rgb_u8(slab).astype(np.int64)
        ref = np.rint(_exact_rgb(slab)).astype(np.int64)
        worst = max(worst, int(np.abs(got - ref).max()))
    assert worst <= 1
    # a hue the tables cannot produce lands in sector 0 with f = 0: (v, v (1 - s), v (1 - s)) for r, g, b
    odd = td.hsv_to_rgb_u8(np.array([[180, 255, 200], [255, 128, 200]], dtype=np.uint8))
    assert odd[0].tolist() == [200, 0, 0] and odd[1, 0] == 200 and odd[1, 1] == odd[1, 2]


def test_hue_saturation_value_member():
    img = _random(16, 18, seed=1)
    params = _params_with(COLOUR_HSV, hsv=np.array([[-7.25, 12.5, -3.0]]))
    ops, aux = colour_tables(params)
    ramp = np.arange(256)
    assert np.array_equal(aux[0, 0], np.floor(np.mod(ramp - 7.25, 180.0)).astype(np.uint8))
    assert np.array_equal(aux[0, 1], np.clip(np.floor(ramp + 12.5), 0, 255).astype(np.uint8))
    assert np.array_equal(aux[0, 2], np.clip(ramp - 3, 0, 255).astype(np.uint8))
    hsv = td.rgb_to_hsv_u8(img)
    moved = np.stack([aux[0, c][hsv[..., c]] for c in range(3)], axis=-1)
    assert np.array_equal(colour_u8_host(img, ops[0], aux[0]), td.hsv_to_rgb_u8(moved))
    # zero shifts: only the round trip's own error is left
    ops, aux = colour_tables(_params_with(COLOUR_HSV, hsv=np.zeros((1, 3))))
    assert np.abs(colour_u8_host(img, ops[0], aux[0]).astype(int) - img.astype(int)).max() <= 5


# ------------------------------------------------------------------------------------------------------------------------- Equalize
def _equalize_direct(img):
    out = np.empty_like(img)
    for c in range(3):
        plane = img[..., c].ravel()
        hist = np.bincount(plane, minlength=256)
        i0 = int(np.nonzero(hist)[0][0])
        if hist[i0] == plane.size:
            out[..., c] = i0
            continue
        scale = np.float32(255.0) / np.float32(plane.size - hist[i0])
        cum = np.cumsum(hist) - np.cumsum(hist)[i0]
        lut = np.zeros(256, dtype=np.uint8)
        for i in range(i0 + 1, 256):
            lut[i] = np.uint8(min(max(np.rint(np.float32(cum[i]) * scale), 0), 255))
        out[..., c] = lut[img[..., c]]
    return out


def test_equalize():
    op = _op(COLOUR_EQUALIZE)
    aux = np.zeros((3, 256), dtype=np.uint8)
    for seed, (h, w) in enumerate(((4, 4), (34, 70), (128, 128))):
        img = _random(h, w, seed)
        img[..., 1] = img[..., 1] // 3 + 40                     # a channel whose first bin is not 0 and whose range is narrow
        assert np.array_equal(colour_u8_host(img, op, aux), _equalize_direct(img))
    const = np.full((8, 8, 3), (0, 17, 255), dtype=np.uint8)
    assert np.array_equal(colour_u8_host(const, op, aux), const)
    two = np.where((np.add.outer(np.arange(8), np.arange(10)) & 1)[..., None] == 1, np.uint8(90), np.uint8(60)).repeat(3, axis=-1)
    assert sorted(np.unique(colour_u8_host(two, op, aux)).tolist()) == [0, 255]
    ramp = np.broadcast_to((np.arange(256) % 256).astype(np.uint8)[None, :, None], (4, 256, 3)).copy()
    out = colour_u8_host(ramp, op, aux)
    assert np.all(np.diff(out[0, :, 0].astype(int)) >= 0) and out.min() == 0 and out.max() == 255


# ----------------------------------------------------------------------------------------------------------------------- tone curve
def test_tone_curve():
    grid = np.linspace(0.0, 1.0, 256)
    for low, high in ((0.15, 0.65), (0.35, 0.85), (0.15, 0.85), (0.35, 0.65), (0.25, 0.75), (0.2213, 0.7071)):
        lut = td.tone_curve_lut(low, high)
        assert lut.dtype == np.uint8 and lut[0] == 0 and lut[255] == 255
        assert np.all(np.diff(lut.astype(int)) >= 0)
        for i in range(256):
            t = float(grid[i])
            ref = (3 * (1 - t) ** 2 * t * low + 3 * (1 - t) * t ** 2 * high + t ** 3) * 255
            assert int(lut[i]) == int(round(ref)) or abs(ref - np.floor(ref) - 0.5) < 1e-9, (low, high, i)
            assert abs(int(lut[i]) - ref) <= 0.5 + 1e-9
    params = _params_with(COLOUR_TONE_CURVE, tone_curve=np.array([[0.2, 0.8]]))
    assert np.array_equal(colour_luts(params)[0], np.broadcast_to(td.tone_curve_lut(0.2, 0.8), (3, 256)))
    assert int(colour_tables(params)[0]["kind"][0]) == 0          # a lookup-table member: nothing for fear_colour_u8 to do


# ---------------------------------------------------------------------------------------------------------------------- ColorJitter
def _params_with(kind, **fields):
    base = dict(context=np.zeros(1), jitter=np.zeros((1, 4)), tone=np.zeros(1, np.int32), colour=np.array([kind], np.int32),
                alpha=np.ones(1), beta=np.zeros(1), gamma=np.ones(1), shift=np.zeros((1, 3)), frame_shapes=())
    return td.TrainPairParams(**base, **fields)


def test_colour_jitter_every_order():
    img = _random(12, 14, seed=3)
    img[:, :7] //= 4                                             # dark half: brightness moves the mean by a non-integer amount
    factors = np.array([[1.17, 0.83, 1.12, -0.11]])
    results = {}
    for order in itertools.permutations(range(4)):
        params = _params_with(COLOUR_JITTER, colour_jitter=factors, colour_jitter_order=np.array([order], np.int32))
        ops, aux = colour_tables(params)
        assert ops["order"][0].tolist() == list(order) and ops["contrast"][0] == 0.83
        assert ops["alpha"][0] == np.float32(1.12) and ops["beta"][0] == np.float32(1.0 - 1.12)
        got = colour_u8_host(img, ops[0], aux[0])
        v = img
        for o in order:                                          # the plain composition of the four single operations
            if o == JITTER_BRIGHTNESS:
                v = td.jitter_brightness_u8(v, 1.17)
            elif o == JITTER_CONTRAST:
                v = td.jitter_contrast_u8(v, 0.83)
            elif o == JITTER_SATURATION:
                v = td.jitter_saturation_u8(v, np.float32(1.12), np.float32(1.0 - 1.12))
            else:
                v = td.jitter_hue_u8(v, td.jitter_hue_lut(-0.11))
        assert np.array_equal(got, v), order
        results[order] = got
    assert not np.array_equal(results[(0, 1, 2, 3)], results[(1, 0, 2, 3)])       # contrast takes the mean of ITS input


def test_colour_jitter_single_operations():
    img = _random(10, 12, seed=4)
    wide = img.astype(np.int64)
    gray = (4899 * wide[..., 0] + 9617 * wide[..., 1] + 1868 * wide[..., 2] + 8192) >> 14
    assert np.array_equal(td.jitter_saturation_u8(img, np.float32(0.0), np.float32(1.0)), np.repeat(gray[..., None], 3, -1).astype(np.uint8))
    assert np.array_equal(td.jitter_saturation_u8(img, np.float32(1.0), np.float32(0.0)), img)
    # contrast: the table of the crop's own gray mean, float64, truncated
    mean = gray.mean()
    ref = np.clip(img.astype(np.float64) * 0.9 + mean * (1 - 0.9), 0, 255).astype(np.uint8)
    assert np.array_equal(td.jitter_contrast_u8(img, 0.9), ref)
    assert np.array_equal(td.jitter_brightness_u8(img, 1.2), np.clip(img * 1.2, 0, 255).astype(np.uint8))
    assert np.array_equal(td.jitter_hue_lut(0.1)[:180], np.floor(np.mod(np.arange(180) + 18.0, 180.0)).astype(np.uint8))
    # an order that is no permutation copies the crop, as the device does
    bad = _op(COLOUR_JITTER, order=[0, 1, 1, 3], contrast=0.9, alpha=1.0)
    assert np.array_equal(colour_u8_host(img, bad, np.zeros((3, 256), np.uint8)), img)


# --------------------------------------------------------------------------------------------------------------------------- Emboss
def test_emboss():
    from scipy import ndimage
    aux = np.zeros((3, 256), dtype=np.uint8)
    for seed, (alpha, strength) in enumerate(((0.2, 0.2), (0.5, 0.7), (0.37, 0.41))):
        img = _random(34, 70, seed)
        taps = td.emboss_taps(alpha, strength)
        a, s = alpha, strength
        want = (1 - a) * np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]]) + a * np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]])
        assert taps.dtype == np.float32 and np.array_equal(taps.reshape(3, 3), want.astype(np.float32))
        got = colour_u8_host(img, _op(COLOUR_EMBOSS, taps=taps), aux).astype(np.int64)
        kernel = taps.astype(np.float64).reshape(3, 3)
        ref = np.stack([ndimage.correlate(img[..., c].astype(np.float64), kernel, mode="mirror") for c in range(3)], axis=-1)
        assert np.abs(got - np.clip(np.rint(ref), 0, 255)).max() <= 1
    assert np.array_equal(colour_u8_host(img, _op(COLOUR_EMBOSS, taps=td.emboss_taps(0.0, 0.6)), aux), img)


def test_other_kinds_copy():
    img = _random(8, 8, seed=9)
    aux = np.zeros((3, 256), dtype=np.uint8)
    for kind in (0, 1, 4, 9, -1):
        out = colour_u8_host(img, _op(kind), aux)
        assert np.array_equal(out, img) and out is not img


# ---------------------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("photometric", [False, True])
def test_default_members_draw_as_before(photometric):
    """The arrays of tests/golden/train_pairs_draws.npz were recorded on the commit before `colour_members` existed."""
    golden = np.load(GOLDEN)
    prefix = "on_" if photometric else "off_"
    for config in (dict(photometric=photometric), dict(photometric=photometric, colour_members=("brightness_contrast", "gamma", "rgb_shift"))):
        params = TrainPairBuilder(config, device="cpu").draw(np.zeros((PAIRS, 11)), SHAPES, np.random.default_rng(SEED))
        for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
            got = np.asarray(getattr(params, name))
            assert got.dtype == golden[prefix + name].dtype and np.array_equal(got, golden[prefix + name]), name
        if photometric:
            for f in dataclasses.fields(params.photo):
                got = np.asarray(getattr(params.photo, f.name))
                assert got.dtype == golden[prefix + "photo_" + f.name].dtype and np.array_equal(got, golden[prefix + "photo_" + f.name]), f.name
        else:
            assert params.photo is None
        assert params.tone_curve is None and params.hsv is None and params.colour_jitter is None and params.colour_jitter_order is None
        assert params.emboss is None
    assert [f.name for f in dataclasses.fields(td.TrainPairParams)][:10] == ["context", "jitter", "tone", "colour", "alpha", "beta", "gamma",
                                                                            "shift", "frame_shapes", "photo"]


def test_new_draws_come_last():
    """With "all", everything the default configuration draws is drawn first and unchanged, but for the member picked."""
    golden = np.load(GOLDEN)
    params = TrainPairBuilder(dict(photometric=True, colour_members="all"), device="cpu").draw(
        np.zeros((PAIRS, 11)), SHAPES, np.random.default_rng(SEED))
    for name in ("context", "jitter", "tone", "alpha", "beta", "gamma", "shift"):
        assert np.array_equal(getattr(params, name), golden["on_" + name]), name
    assert np.array_equal(params.photo.key, golden["on_photo_key"]) and np.array_equal(params.photo.var, golden["on_photo_var"])
    assert np.array_equal(params.colour == 0, golden["on_colour"] == 0)


def test_all_members_frequencies_and_limits():
    n = 20000
    builder = TrainPairBuilder(dict(colour_members="all", colour_p=1.0), device="cpu")
    assert builder.colour_members == tuple(COLOUR_MEMBERS)
    params = builder.draw(np.zeros((n, 11)), (), np.random.default_rng(7))
    counts = np.bincount(params.colour, minlength=9)
    assert counts[0] == 0
    sigma = np.sqrt(n * (1 / 8) * (7 / 8))
    assert np.all(np.abs(counts[1:] - n / 8) < 4 * sigma), counts
    for values, lo, hi in ((params.tone_curve[:, 0], 0.15, 0.35), (params.tone_curve[:, 1], 0.65, 0.85), (params.hsv[:, 0], -20, 20),
                           (params.hsv[:, 1], -30, 30), (params.hsv[:, 2], -20, 20), (params.colour_jitter[:, :3], 0.8, 1.2),
                           (params.colour_jitter[:, 3], -0.2, 0.2), (params.emboss[:, 0], 0.2, 0.5), (params.emboss[:, 1], 0.2, 0.7)):
        assert values.dtype == np.float64 and values.min() >= lo and values.max() < hi
        assert values.min() < lo + 0.01 * (hi - lo) and values.max() > hi - 0.01 * (hi - lo)      # the whole range is used
    assert np.array_equal(np.sort(params.colour_jitter_order, axis=1), np.broadcast_to(np.arange(4), (n, 4)))
    perms = np.unique(params.colour_jitter_order, axis=0, return_counts=True)[1]
    assert len(perms) == 24 and np.all(np.abs(perms - n / 24) < 4 * np.sqrt(n * (1 / 24) * (23 / 24)))
    half = TrainPairBuilder(dict(colour_members="all"), device="cpu").draw(np.zeros((n, 11)), (), np.random.default_rng(8))
    assert abs(int((half.colour == 0).sum()) - n / 2) < 4 * np.sqrt(n / 4)


def test_member_names():
    with pytest.raises(KeyError):
        TrainPairBuilder(dict(colour_members=("gamma", "clahe")), device="cpu")
    with pytest.raises(KeyError):
        TrainPairBuilder(dict(colour_member="all"), device="cpu")
    with pytest.raises(ValueError):
        TrainPairBuilder(dict(colour_members=()), device="cpu")
    subset = TrainPairBuilder(dict(colour_members=("gamma", "hsv", "emboss"), colour_p=1.0), device="cpu")
    params = subset.draw(np.zeros((600, 11)), (), np.random.default_rng(1))
    assert sorted(np.unique(params.colour).tolist()) == [2, 6, 8]
    assert params.hsv is not None and params.emboss is not None and params.colour_jitter is None and params.tone_curve is None
    # a record that carries a member the configuration lacks is refused, not silently skipped
    default = TrainPairBuilder(device="cpu")
    with pytest.raises(ValueError):
        default.build_host([np.zeros((16, 16, 3), np.uint8)], np.array([[0, 2, 2, 8, 8, 0, 2, 2, 8, 8, 1.0]]), params=_with_colour(default, 6))


def _with_colour(builder, kind):
    params = builder.draw(np.zeros((1, 11)), ((16, 16),), np.random.default_rng(0))
    params.colour[:] = kind
    return params
