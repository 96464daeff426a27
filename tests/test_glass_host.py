"""GlassBlur on the host (feartracker_amd/train_data/glass.py): the 8-bit Gaussian's weights from their formula, `glass_u8_host` — the
gather form the kernel uses — against the literal numpy statement of albumentations' "fast" mode, the tie rule, the offsets, and the draws
of `glass_blur`.  No GPU."""
import dataclasses
import os
import re

import numpy as np
import pytest

from feartracker_amd import train_data as td
from feartracker_amd.train_data import (BLUR_BOX, BLUR_GLASS, BLUR_NONE, GLASS_WEIGHTS, PHOTO_DTYPE, TrainPairBuilder, glass_gauss_u8,
                                        glass_offsets, glass_swap_u8, glass_u8_host, normal_quantiles, philox4x32_10,
                                        photometric_u8_host)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRAWS = os.path.join(HERE, "golden", "train_pairs_draws.npz")
SEED, PAIRS, FRAME_SHAPES = 20240611, 16, ((48, 64), (256, 480))          # tools/make_colour_draws_golden.py's
D = 4
SHAPES = [(4, 4), (8, 8), (10, 10), (12, 18), (34, 70), (128, 128)]
KEY = np.array([0x243F6A88, 0x85A308D3], dtype=np.uint32)


def _op(key=KEY, blur=BLUR_GLASS):
    op = np.zeros((), dtype=PHOTO_DTYPE)
    op["blur"], op["ksize"], op["key"], op["tap_row"] = blur, 3, key, -1
    return op


def _contents(h, w, seed=0):
    """Random, a ramp and a two-level checkerboard: name -> (h, w, 3) uint8."""
    yy, xx = np.mgrid[0:h, 0:w]
    odd = (yy + xx) & 1
    return {"random": np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8),
            "ramp": np.stack([(yy * w + xx) * 255 // (h * w - 1), 255 - xx * 255 // (w - 1), yy * 255 // (h - 1)], axis=-1).astype(np.uint8),
            "checkerboard": np.stack([np.where(odd, 200, 30), np.where(odd, 0, 255), np.where(odd, 90, 91)], axis=-1).astype(np.uint8)}


# ---------------------------------------------------------------------------------------------------------------------- the Gaussian
def test_weights_come_from_the_formula():
    """cv2 at sigma 0.7 on 8 bits: ksize = cvRound(6 sigma + 1) | 1 = 5, the float64 kernel exp(-i^2 / (2 sigma^2)) normalised, then 8
    fractional bits — by rounding the outer taps and giving the centre the remainder, and by diffusing the rounding error from the edge."""
    sigma = 0.7
    ksize = int(np.rint(6 * sigma + 1)) | 1
    assert ksize == 5
    i = np.arange(ksize) - ksize // 2
    g = np.exp(-(i.astype(np.float64) ** 2) / (2 * sigma * sigma))
    g = 256 * g / g.sum()
    assert np.allclose(g, [2.4627, 52.5885, 145.8976, 52.5885, 2.4627], atol=1e-4)
    rounded = np.rint(g).astype(np.int64)
    rounded[ksize // 2] = 256 - (rounded.sum() - rounded[ksize // 2])
    diffused, err = [], 0.0
    for v in g:
        w = int(np.rint(v + err))
        err = v + err - w
        diffused.append(w)
    assert tuple(rounded) == tuple(diffused) == GLASS_WEIGHTS == (2, 53, 146, 53, 2) and sum(GLASS_WEIGHTS) == 256


def _gauss_separable(img):
    """The same pass as two integer passes, rows then columns, with one rounding at the end."""
    w = np.asarray(GLASS_WEIGHTS, dtype=np.int64)
    p = np.pad(img.astype(np.int64), ((2, 2), (2, 2), (0, 0)), mode="reflect")
    H, W = img.shape[:2]
    rows = sum(w[j] * p[:, j:j + W] for j in range(5))
    both = sum(w[i] * rows[i:i + H] for i in range(5))
    return ((both + 32768) >> 16).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_pass(shape):
    for name, img in _contents(*shape, seed=1).items():
        assert np.array_equal(glass_gauss_u8(img), _gauss_separable(img)), name
    flat = np.full(shape + (3,), 201, np.uint8)
    assert np.array_equal(glass_gauss_u8(flat), flat)                                 # the weights sum to 256: a constant stays


# ------------------------------------------------------------------------------------------------------------ the literal statement
def _literal_offsets(H, W, key, i):
    """The index vectors of albumentations' fast mode and their offsets, computed once: h fastest, both descending."""
    hs, ws = np.arange(H - D, D, -1), np.arange(W - D, D, -1)
    h, w = np.tile(hs, len(ws)), np.repeat(ws, len(hs))
    counter = np.stack([w, h, np.full_like(h, 1 + i), np.zeros_like(h)], axis=-1).reshape(-1, 4)
    word = philox4x32_10(counter, key)[:, 0].astype(np.int64) if len(h) else np.zeros(0, np.int64)
    return h, w, (word & 7) - 4, ((word >> 3) & 7) - 4


def _literal(crop, key, first_wins=False):
    x = _gauss_separable(crop)
    for i in range(2):
        h, w, dy, dx = _literal_offsets(*crop.shape[:2], key, i)
        if first_wins:                                                                # the rule flipped: the smallest n wins a target
            a, b = x[h + dy, w + dx], x[h, w]
            x[h, w] = a
            x[(h + dy)[::-1], (w + dx)[::-1]] = b[::-1]
        else:
            x[h, w], x[h + dy, w + dx] = x[h + dy, w + dx], x[h, w]
    return _gauss_separable(x)


@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_literal_statement(shape):
    for name, img in _contents(*shape, seed=shape[1]).items():
        got, want = glass_u8_host(img, _op()), _literal(img, KEY)
        assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: {len(bad)} values differ, first at {bad[0].tolist()}"
        if min(shape) <= 2 * D:                                                       # no interior: the two Gaussians alone
            assert np.array_equal(got, _gauss_separable(_gauss_separable(img))), name
    other = glass_u8_host(_contents(*shape)["random"], _op(key=KEY[::-1]))
    assert (min(shape) <= 2 * D) == np.array_equal(other, glass_u8_host(_contents(*shape)["random"], _op()))     # the key matters


def test_the_tie_rule_is_exercised():
    """34 x 70: in each iteration some target has two or more writers whose values differ, about a quarter of the targets have two or
    more writers, and "first wins" gives another image."""
    H, W = 34, 70
    img = _contents(H, W, seed=70)["random"]
    x = _gauss_separable(img)
    for i in range(2):
        h, w, dy, dx = _literal_offsets(H, W, KEY, i)
        assert len(h) == (H - 2 * D) * (W - 2 * D) and h[0] == H - D and h[1] == H - D - 1 and w[0] == w[1] == W - D
        assert (h + dy).min() >= 1 and (h + dy).max() <= H - 1 and (w + dx).min() >= 1 and (w + dx).max() <= W - 1
        target = (h + dy) * W + (w + dx)
        order = np.argsort(target, kind="stable")
        t, v = target[order], x[h, w][order]
        same = t[1:] == t[:-1]
        contested = np.unique(t[1:][same])
        assert 0.15 < len(contested) / len(np.unique(t)) < 0.40
        assert (same & np.any(v[1:] != v[:-1], axis=-1)).any()                        # two writers of one target, other values
        # the gather and the literal statement agree on this iteration alone, and the last writer in index order is the one kept
        want = x.copy()
        want[h, w], want[h + dy, w + dx] = x[h + dy, w + dx], x[h, w]
        assert np.array_equal(glass_swap_u8(x, *glass_offsets(H, W, KEY, i)), want)
        last = {}
        for n in range(len(h)):
            last[int(target[n])] = n
        for tgt, n in list(last.items())[::37]:
            assert np.array_equal(want[tgt // W, tgt % W], x[h[n], w[n]])
        x = want
    assert np.array_equal(glass_u8_host(img, _op()), _literal(img, KEY))
    assert not np.array_equal(_literal(img, KEY, first_wins=True), _literal(img, KEY))


def test_offsets():
    """Three bits each, uniform on [-4, 3]: every value occurs for dy and for dx on 128 x 128, from word 0 at counter (w, h, 1 + i, 0)."""
    for i in range(2):
        dy, dx = glass_offsets(128, 128, KEY, i)
        assert dy.shape == dx.shape == (128, 128)
        assert sorted(np.unique(dy)) == sorted(np.unique(dx)) == list(range(-4, 4))
        for off in (dy, dx):
            assert np.bincount((off + 4).reshape(-1), minlength=8).min() > 128 * 128 // 8 * 0.9
        for h, w in ((5, 5), (17, 100), (124, 124)):
            word = int(philox4x32_10(np.array([w, h, 1 + i, 0]), KEY)[0])
            assert (dy[h, w], dx[h, w]) == ((word & 7) - 4, ((word >> 3) & 7) - 4)
    assert not np.array_equal(glass_offsets(128, 128, KEY, 0)[0], glass_offsets(128, 128, KEY, 1)[0])
    # apart from GaussNoise's and ISONoise's counter (x, y, 0, 0)
    assert philox4x32_10(np.array([7, 9, 1, 0]), KEY)[0] != philox4x32_10(np.array([7, 9, 0, 0]), KEY)[0]


def test_the_member_in_the_blurs_place():
    """`photometric_u8_host` applies the member only when told to; the noise and the Downscale follow it."""
    img = _contents(34, 70, seed=3)["random"]
    q = normal_quantiles()
    op = _op()
    assert np.array_equal(photometric_u8_host(img, op, None, q), img)                 # "none", as to fear_photometric_u8
    assert np.array_equal(photometric_u8_host(img, op, None, q, glass=True), glass_u8_host(img, op))
    op["ksize"] = 0                                                                    # the record's ksize is not read
    assert np.array_equal(photometric_u8_host(img, op, None, q, glass=True), glass_u8_host(img, op))
    op["noise"], op["scale"], op["downscale"] = td.NOISE_GAUSS, 4.0, 1
    plain = op.copy()
    plain["blur"] = BLUR_NONE
    assert np.array_equal(photometric_u8_host(img, op, None, q, glass=True), photometric_u8_host(glass_u8_host(img, op), plain, None, q))
    box = _op(blur=BLUR_BOX)
    assert np.array_equal(photometric_u8_host(img, box, None, q, glass=True), photometric_u8_host(img, box, None, q))
    with pytest.raises(ValueError):
        glass_u8_host(img[:33], _op())


# ------------------------------------------------------------------------------------------------------------------------ draws
def _draw(config, n=PAIRS, seed=SEED, rng=None):
    return TrainPairBuilder(config, device="cpu").draw(np.zeros((n, 11)), FRAME_SHAPES, np.random.default_rng(seed) if rng is None else rng)


@pytest.mark.parametrize("photometric", [False, True])
def test_key_off_draws_as_before(photometric):
    """tests/golden/train_pairs_draws.npz was recorded before the key existed: with it off, named or not, every array is the recorded one
    and the generator is left where it was."""
    assert td.DEFAULT_TRAIN_DATA_CONFIG["glass_blur"] is False
    golden = np.load(DRAWS)
    prefix = "on_" if photometric else "off_"
    rng, rng2 = np.random.default_rng(SEED), np.random.default_rng(SEED)
    params = _draw(dict(photometric=photometric, glass_blur=False), rng=rng)
    _draw(dict(photometric=photometric), rng=rng2)
    assert rng.bit_generator.state == rng2.bit_generator.state
    for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
        assert np.array_equal(getattr(params, name), golden[prefix + name]), name
    if photometric:
        for f in dataclasses.fields(params.photo):
            assert np.array_equal(getattr(params.photo, f.name), golden[prefix + "photo_" + f.name]), f.name
        assert not (params.photo.blur == BLUR_GLASS).any()
    rng3, rng4 = np.random.default_rng(SEED), np.random.default_rng(SEED)
    off = _draw(dict(glass_blur=True), rng=rng3)                                       # the stage off: the key draws nothing
    _draw(dict(), rng=rng4)
    assert off.photo is None and rng3.bit_generator.state == rng4.bit_generator.state


def test_the_draw_comes_last():
    """With the key on everything else is drawn first and unchanged; then one uniform per crop turns a blur into GlassBlur below 1 / 5."""
    base = dict(photometric=True, colour_members="all", noise_members="all", iso_noise=True, weather_members="all")
    rng, rng2 = np.random.default_rng(SEED), np.random.default_rng(SEED)
    N = 256
    before = _draw(base, n=N, rng=rng2)
    params = _draw(dict(base, glass_blur=True), n=N, rng=rng)
    for f in dataclasses.fields(td.TrainPairParams):
        if f.name in ("photo", "frame_shapes"):
            continue
        assert np.array_equal(getattr(params, f.name), getattr(before, f.name)), f.name
    for f in dataclasses.fields(params.photo):
        if f.name != "blur":
            assert np.array_equal(getattr(params.photo, f.name), getattr(before.photo, f.name)), f.name
    u = rng2.random((N, 2))
    changed = params.photo.blur != before.photo.blur
    assert changed.any() and np.all(params.photo.blur[changed] == BLUR_GLASS)
    assert np.array_equal(changed, (before.photo.blur != BLUR_NONE) & (u < 1.0 / 5))
    assert rng.bit_generator.state == rng2.bit_generator.state


def test_member_frequency():
    n = 10000                                                                          # 20 000 crops
    blur = _draw(dict(photometric=True, blur_p=1.0, glass_blur=True), n=n, seed=61).photo.blur.reshape(-1)
    assert np.all(blur != BLUR_NONE)
    sigma = np.sqrt(0.2 * 0.8 / blur.size)
    for kind in (1, 2, 3, 4, BLUR_GLASS):                                              # the reference's five members, a fifth each
        assert abs(np.mean(blur == kind) - 0.2) < 4 * sigma, kind
    blur = _draw(dict(photometric=True, glass_blur=True), n=n, seed=62).photo.blur.reshape(-1)
    assert abs(np.mean(blur != BLUR_NONE) - 0.2) < 4 * sigma                           # the group still fires at the reference's p
    assert abs(np.mean(blur == BLUR_GLASS) - 0.04) < 4 * np.sqrt(0.04 * 0.96 / blur.size)


def test_build_host_applies_the_member_and_refuses_what_it_cannot():
    frames = [np.random.default_rng(5).integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    pairs = np.array([[0, 10, 10, 20, 16, 0, 12, 8, 20, 16, 1]], dtype=np.float64)
    builder = TrainPairBuilder(dict(photometric=True, glass_blur=True), device="cpu")
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(6))
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:] = BLUR_NONE, td.NOISE_NONE, 0
    plain = builder.build_host(frames, pairs, params)
    ph.blur[0, 0], ph.blur[0, 1], ph.downscale[0, 1] = BLUR_GLASS, BLUR_GLASS, 1
    got = builder.build_host(frames, pairs, params)
    u8 = lambda t: np.rint(t.transpose(1, 2, 0) / td._INV_STD + td._MEAN).astype(np.uint8)         # the crop in front of the normalisation
    ops, _ = td.photo_tables(ph)
    assert ops["blur"][0, 0] == BLUR_GLASS
    assert np.array_equal(u8(got.template[0]), glass_u8_host(u8(plain.template[0]), ops[0, 0]))
    glassy = glass_u8_host(u8(plain.search[0]), ops[0, 1])
    assert np.array_equal(u8(got.search[0]), np.repeat(np.repeat(glassy[::2, ::2], 2, axis=0), 2, axis=1))
    assert not np.array_equal(got.template[0], plain.template[0])
    with pytest.raises(ValueError, match="GlassBlur"):                                 # the member is not configured
        TrainPairBuilder(dict(photometric=True), device="cpu").build_host(frames, pairs, params)
    with pytest.raises(KeyError):
        TrainPairBuilder(dict(glass="yes"), device="cpu")


# -------------------------------------------------------------------------------------------------------------------------- ABI
def test_abi():
    import ctypes
    from feartracker_amd import train_abi
    assert ctypes.sizeof(train_abi.FearPhotoOp) == 32 and PHOTO_DTYPE.itemsize == 32
    args, res = train_abi.TRAIN_SYMBOLS["fear_glass_u8"]
    assert len(args) == 7 and res is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "fear_train.h")).read()
    assert re.search(r"#define\s+FEAR_PHOTO_BLUR_GLASS\s+5\b", header) and BLUR_GLASS == 5
    assert re.search(r"int\s+fear_glass_u8\(const uint8_t\*\s*crops_u8,\s*int n,\s*int H,\s*int W,\s*const FearPhotoOp\*\s*ops,\s*"
                     r"uint8_t\*\s*out_u8,\s*void\*\s*stream\);", header)
