"""The photometric stage's host side (feartracker_amd/train_data/photometric.py): Philox against the Random123 known
answers, every member of `photometric_u8_host` against an independent formulation, GaussNoise's statistics, and the draws."""
import ctypes

import numpy as np
import pytest

from feartracker_amd import train_data as td
from feartracker_amd.train_data import (BLUR_BOX, BLUR_GAUSSIAN, BLUR_MEDIAN, BLUR_MOTION, BLUR_NONE, GAUSS_WEIGHTS, NOISE_GAUSS,
                                        NOISE_MULTIPLICATIVE, NOISE_NONE, PHOTO_DTYPE, TrainPairBuilder, line_u8, motion_kernel,
                                        motion_taps, normal_quantiles, philox4x32_10, photometric_host, photometric_u8_host)

Q = normal_quantiles()


def _op(blur=BLUR_NONE, ksize=3, noise=NOISE_NONE, scale=1.0, key=(0, 0), downscale=0, tap_row=-1):
    op = np.zeros((), dtype=PHOTO_DTYPE)
    op["blur"], op["ksize"], op["noise"], op["scale"], op["key"] = blur, ksize, noise, scale, key
    op["downscale"], op["tap_row"] = downscale, tap_row
    return op


def _image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _window_stack(img, k, mode):
    """(k * k, H, W, 3): the k x k neighbours of every pixel, built shift by shift from np.pad."""
    r = k // 2
    h, w = img.shape[:2]
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode=mode)
    return np.stack([p[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)])


def _pairs(B):
    p = np.zeros((B, 11))
    p[:, 1:5] = [10, 10, 20, 20]
    p[:, 6:10] = [12, 8, 20, 24]
    p[:, 10] = 1
    return p


# ------------------------------------------------------------------------------------------------------------------------- Philox
def _words(text):
    return np.array([int(v, 16) for v in text.split()], dtype=np.uint32)


@pytest.mark.parametrize("counter,key,expected", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expected):
    assert philox4x32_10(_words(counter), _words(key)).tolist() == _words(expected).tolist()


def test_philox_is_vectorised_over_rows():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (5, 7, 4), dtype=np.uint64).astype(np.uint32)
    k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
    out = philox4x32_10(c, k)
    assert out.shape == (5, 7, 4) and out.dtype == np.uint32
    assert out[3, 2].tolist() == philox4x32_10(c[3, 2], k).tolist()


def test_quantile_table():
    assert Q.shape == (4096,) and Q.dtype == np.float32
    assert np.all(np.diff(Q) > 0) and np.array_equal(Q, -Q[::-1])
    assert abs(float(Q[-1]) - 3.668) < 1e-3                                   # the tails end at +-3.67 sigma
    assert abs(float(np.mean(Q.astype(np.float64) ** 2)) - 0.9997) < 1e-4      # the table's variance


def test_record_layout_is_the_c_struct():
    from feartracker_amd.train_abi import FearPhotoOp
    assert PHOTO_DTYPE.itemsize == ctypes.sizeof(FearPhotoOp) == 32
    for name, _ in FearPhotoOp._fields_:
        assert PHOTO_DTYPE.fields[name][1] == getattr(FearPhotoOp, name).offset, name


# ------------------------------------------------------------------------------------------------------------------------ members
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", [(4, 4), (8, 6), (34, 70)])
def test_box_is_the_rounded_window_mean(k, shape):
    img = _image(*shape, seed=k)
    mean = _window_stack(img, k, "reflect").astype(np.float64).mean(axis=0)    # k * k is odd: no ties
    out = photometric_u8_host(img, _op(BLUR_BOX, k), None, Q)
    assert np.array_equal(out, np.rint(mean).astype(np.uint8))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_gaussian_constant_and_impulse(k):
    const = np.full((8, 10, 3), 201, dtype=np.uint8)
    assert np.array_equal(photometric_u8_host(const, _op(BLUR_GAUSSIAN, k), None, Q), const)
    img = np.zeros((16, 18, 3), dtype=np.uint8)
    img[8, 9] = 255
    out = photometric_u8_host(img, _op(BLUR_GAUSSIAN, k), None, Q)
    w = GAUSS_WEIGHTS[k]
    assert sum(w) == 256
    expected = np.zeros((16, 18), dtype=np.int64)
    r = k // 2
    for dy in range(k):
        for dx in range(k):
            expected[8 - r + dy, 9 - r + dx] = (255 * w[dy] * w[dx] + 32768) >> 16
    for c in range(3):
        assert np.array_equal(out[..., c], expected)


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", [(4, 4), (8, 6), (34, 70)])
def test_median_is_np_median_with_replicated_border(k, shape):
    img = _image(*shape, seed=10 + k)
    img[::2, ::3] = 0                                                          # ties
    expected = np.median(_window_stack(img, k, "edge"), axis=0)
    out = photometric_u8_host(img, _op(BLUR_MEDIAN, k), None, Q)
    assert np.array_equal(out, expected.astype(np.uint8))


def _connected(mask):
    pts = {tuple(p) for p in np.argwhere(mask)}
    seen, todo = set(), [next(iter(pts))]
    while todo:
        y, x = todo.pop()
        if (y, x) in seen:
            continue
        seen.add((y, x))
        todo += [(y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (y + dy, x + dx) in pts]
    return seen == pts


@pytest.mark.parametrize("k", [3, 5, 7])
def test_motion_kernel_every_pair_of_end_points(k):
    for xs in range(k):
        for ys in range(k):
            for xe in range(k):
                for ye in range(k):
                    if (xs, ys) == (xe, ye):
                        continue                                              # get_params never draws a point
                    kern = motion_kernel(k, xs, ys, xe, ye)
                    assert kern.dtype == np.float32 and kern.shape == (k, k)
                    n = int(np.count_nonzero(kern))
                    assert 2 <= n <= k and n == max(abs(xe - xs), abs(ye - ys)) + 1
                    assert abs(float(kern.astype(np.float64).sum()) - 1.0) <= n * 2.0 ** -24
                    assert kern[ys, xs] > 0 and kern[ye, xe] > 0
                    assert _connected(kern > 0)
                    assert np.array_equal(line_u8(k, xs, ys, xe, ye), line_u8(k, xe, ye, xs, ys))   # drawn left to right either way


@pytest.mark.parametrize("k", [3, 5, 7])
def test_motion_blur_is_a_centred_correlation(k):
    img = _image(12, 10, seed=20 + k)
    kern = motion_kernel(k, 0, 0, k - 1, k - 2)
    taps = motion_taps(kern)[None]
    out = photometric_u8_host(img, _op(BLUR_MOTION, k, tap_row=0), taps, Q)
    stack = _window_stack(img, k, "reflect").astype(np.float64)                # float64 sum of at most 7 products: exact enough to
    ref = (stack * kern.astype(np.float64).reshape(k * k, 1, 1, 1)).sum(axis=0)   # round the same way except next to a tie
    near_tie = np.abs(ref - np.floor(ref) - 0.5) < 1e-3
    assert np.array_equal(out[~near_tie], np.rint(ref).astype(np.uint8)[~near_tie])
    assert near_tie.mean() < 0.01
    # a motion record without its taps is "none"
    assert np.array_equal(photometric_u8_host(img, _op(BLUR_MOTION, k, tap_row=-1), taps, Q), img)
    assert np.array_equal(photometric_u8_host(img, _op(BLUR_MOTION, k, tap_row=0), None, Q), img)


def test_downscale_repeats_the_even_pixels():
    img = _image(6, 10, seed=30)
    out = photometric_u8_host(img, _op(downscale=1), None, Q)
    assert np.array_equal(out, np.repeat(np.repeat(img[::2, ::2], 2, 0), 2, 1))


@pytest.mark.parametrize("m", [0.9, 0.957, 1.0, 1.1])
def test_multiplicative_is_the_lookup_table(m):
    img = _image(8, 8, seed=31)
    lut = np.array([min(int(np.float32(v) * np.float32(m)), 255) for v in range(256)], dtype=np.uint8)
    assert np.array_equal(photometric_u8_host(img, _op(noise=NOISE_MULTIPLICATIVE, scale=m), None, Q), lut[img])


def test_unknown_records_are_none_and_odd_sides_raise():
    img = _image(8, 8, seed=32)
    for op in (_op(blur=9, ksize=3), _op(blur=BLUR_BOX, ksize=4), _op(blur=BLUR_MEDIAN, ksize=9), _op(noise=7, scale=3.0)):
        assert np.array_equal(photometric_u8_host(img, op, None, Q), img)
    for shape in ((7, 8), (8, 2)):
        with pytest.raises(ValueError):
            photometric_u8_host(_image(*shape), _op(), None, Q)


def test_the_chain_runs_at_the_even_pixel():
    img = _image(10, 12, seed=33)
    op = _op(BLUR_BOX, 5, NOISE_GAUSS, np.sqrt(20.0), key=(7, 9), downscale=1)
    full = photometric_u8_host(img, _op(BLUR_BOX, 5, NOISE_GAUSS, np.sqrt(20.0), key=(7, 9)), None, Q)
    assert np.array_equal(photometric_u8_host(img, op, None, Q), np.repeat(np.repeat(full[::2, ::2], 2, 0), 2, 1))


def test_normalisation_of_the_none_record():
    img = _image(4, 6, seed=34)
    out = photometric_host(img, _op(), None, Q)
    ref = td._colour_normalise(img, td.TONE_NONE, np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256)))
    assert out.dtype == np.float32 and out.shape == (3, 4, 6) and np.array_equal(out, ref)


# --------------------------------------------------------------------------------------------------------------------- GaussNoise
def test_gauss_noise_statistics_and_keys():
    """Constant 128, 256 x 256 x 3, var 25 (N = 196608).  Observed: mean of out - 128 = -0.4927 (expected -0.5: the truncation's
    bias; standard error 0.0113, so +0.6 standard errors), variance 25.0308 (expected 25 + 1/12 = 25.0833: -0.21 %)."""
    img = np.full((256, 256, 3), 128, dtype=np.uint8)
    sigma = np.float32(np.sqrt(25.0))
    out = photometric_u8_host(img, _op(noise=NOISE_GAUSS, scale=sigma, key=(0x1234, 0xabcd)), None, Q)
    d = out.astype(np.float64) - 128.0
    n = d.size
    print(f"GaussNoise: mean {d.mean():.4f} variance {d.var():.4f} over {n}")
    assert abs(d.mean() + 0.5) <= 5 * 5.0 / np.sqrt(n)
    assert abs(d.var() / (25.0 + 1.0 / 12.0) - 1.0) <= 0.02
    again = photometric_u8_host(img, _op(noise=NOISE_GAUSS, scale=sigma, key=(0x1234, 0xabcd)), None, Q)
    other = photometric_u8_host(img, _op(noise=NOISE_GAUSS, scale=sigma, key=(0x1235, 0xabcd)), None, Q)
    assert np.array_equal(out, again)
    assert (out != other).mean() > 0.5
    assert len({out[..., 0].tobytes(), out[..., 1].tobytes(), out[..., 2].tobytes()}) == 3     # words 0, 1, 2: three fields


# -------------------------------------------------------------------------------------------------------------------------- draws
def test_disabled_draw_consumes_what_it_always_did():
    B = 37
    assert td.DEFAULT_TRAIN_DATA_CONFIG["photometric"] is False
    b = TrainPairBuilder()
    rng = np.random.default_rng(5)
    p = b.draw(_pairs(B), [(48, 64, 3)], rng)
    assert p.photo is None
    replay = np.random.default_rng(5)                 # the draws of the stage-less builder, call by call
    replay.random(B)
    replay.uniform(-0.35, 0.35, size=(B, 2)), replay.uniform(-48, 48, size=(B, 2))
    replay.random(B), replay.integers(0, 2, size=B)
    replay.random(B), replay.integers(0, 3, size=B)
    replay.uniform(-0.2, 0.2, size=B), replay.uniform(-0.2, 0.2, size=B), replay.uniform(0.8, 1.2, size=B)
    replay.uniform(-20, 20, size=(B, 3))
    assert rng.random() == replay.random()
    # the enabled draw makes the same draws first
    on = TrainPairBuilder(dict(photometric=True)).draw(_pairs(B), [(48, 64, 3)], np.random.default_rng(5))
    for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
        assert np.array_equal(getattr(on, name), getattr(p, name)), name
    assert on.photo is not None and on.photo.blur.shape == (B, 2)


def test_params_stay_positional():
    z = np.zeros(1)
    p = td.TrainPairParams(z, z, z, z, z, z, z, z, ((4, 4),))
    assert p.photo is None


def _within(count, n, p, what):
    assert abs(count - n * p) <= 5 * np.sqrt(n * p * (1 - p)), f"{what}: {count} of {n} at p = {p}"


def test_enabled_draw_frequencies():
    B = 10000                                          # 20 000 crops
    ph = TrainPairBuilder(dict(photometric=True)).draw(_pairs(B), [(48, 64, 3)], np.random.default_rng(11)).photo
    n = 2 * B
    for name, members, prob in (("blur", 4, 0.2), ("noise", 2, 0.2)):
        kind = getattr(ph, name).ravel()
        drawn = int((kind != 0).sum())
        _within(drawn, n, prob, name)
        for m in range(1, members + 1):
            _within(int((kind == m).sum()), drawn, 1.0 / members, f"{name} member {m}")
        assert kind.min() >= 0 and kind.max() == members
    _within(int(ph.downscale.sum()), n, 0.2, "downscale")
    for k in (3, 5, 7):
        _within(int((ph.ksize == k).sum()), n, 1.0 / 3, f"ksize {k}")
    assert set(np.unique(ph.ksize)) == {3, 5, 7}
    assert ph.var.min() >= 10 and ph.var.max() <= 35 and ph.mult.min() >= 0.9 and ph.mult.max() <= 1.1
    assert ph.key.dtype == np.uint32 and len(np.unique(ph.key.reshape(-1, 2), axis=0)) == n
    xs, ys, xe, ye = (ph.line[..., i] for i in range(4))
    assert ph.line.min() >= 0 and np.all(ph.line.max(axis=-1) < ph.ksize)
    assert not np.any((xs == xe) & (ys == ye))                                 # MotionBlur never draws a point
    # template and search crops draw on their own
    assert 0.1 < np.mean((ph.blur[:, 0] != 0) & (ph.blur[:, 1] != 0)) / 0.04 < 2.0


def test_photo_tables_records():
    b = TrainPairBuilder(dict(photometric=True, blur_p=1.0, noise_p=1.0))
    ph = b.draw(_pairs(64), [(48, 64, 3)], np.random.default_rng(3)).photo
    ops, taps = td.photo_tables(ph)
    assert ops.shape == (64, 2) and taps.dtype == np.float32 and taps.shape == (int((ph.blur == BLUR_MOTION).sum()), 49)
    motion = ph.blur == BLUR_MOTION
    assert sorted(ops["tap_row"][motion].tolist()) == list(range(len(taps))) and np.all(ops["tap_row"][~motion] == -1)
    g = ph.noise == NOISE_GAUSS
    assert np.array_equal(ops["scale"][g], np.sqrt(ph.var[g]).astype(np.float32))
    assert np.array_equal(ops["scale"][~g], ph.mult[~g].astype(np.float32))
    b0, j0 = np.argwhere(motion)[0]
    k = int(ph.ksize[b0, j0])
    o = (7 - k) // 2
    kern = taps[ops["tap_row"][b0, j0]].reshape(7, 7)
    assert np.array_equal(kern[o:o + k, o:o + k], motion_kernel(k, *ph.line[b0, j0])) and np.count_nonzero(kern) <= k


# --------------------------------------------------------------------------------------------------------------------- build_host
def test_build_host_with_the_stage():
    frames = [_image(48, 64, seed=40), _image(40, 56, seed=41)]
    pairs = _pairs(3)
    pairs[:, 0], pairs[:, 5] = [0, 1, 0], [1, 0, 0]
    off, on = TrainPairBuilder(), TrainPairBuilder(dict(photometric=True))
    params = on.draw(pairs, [f.shape for f in frames], np.random.default_rng(2))
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:] = 0, 0, 0
    base = off.build_host(frames, pairs, params)
    none = on.build_host(frames, pairs, params)
    for a, b in zip(base, none):
        assert np.array_equal(a, b)
    ph.downscale[1, 1] = 1
    ph.noise[2, 0], ph.blur[0, 1], ph.ksize[0, 1] = NOISE_GAUSS, BLUR_MEDIAN, 5
    out = on.build_host(frames, pairs, params)
    s = out.search[1]
    assert np.array_equal(s, np.repeat(np.repeat(s[:, ::2, ::2], 2, 1), 2, 2)) and not np.array_equal(s, base.search[1])
    assert np.array_equal(out.template[1], base.template[1]) and np.array_equal(out.search[2], base.search[2])
    assert not np.array_equal(out.template[2], base.template[2]) and not np.array_equal(out.search[0], base.search[0])
    for a, b in zip(out[2:], base[2:]):
        assert np.array_equal(a, b)                                            # targets and search_bbox do not move
    params.photo = None
    with pytest.raises(ValueError):
        on.build_host(frames, pairs, params)
