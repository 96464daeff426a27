"""ImageCompression on the host: `jpeg_roundtrip_u8_host` against Pillow's libjpeg-turbo — the recorded fixture
tests/golden/jpeg_roundtrip.npz (tools/make_jpeg_golden.py) and, where Pillow is installed, a live round trip — byte for byte; the
quantisation tables for every quality; both DCTs against a float64 DCT; and the draws of the noise group with the new member."""
import dataclasses
import io
import os

import numpy as np
import pytest

from feartracker_amd import train_data as td
from feartracker_amd.train_data import (NOISE_GAUSS, NOISE_JPEG, NOISE_MEMBERS, NOISE_MULTIPLICATIVE, NOISE_NONE, PHOTO_DTYPE,
                                        TrainPairBuilder, jpeg_fdct_islow, jpeg_idct_islow, jpeg_quant_tables, jpeg_roundtrip_u8_host,
                                        normal_quantiles, photometric_u8_host)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_roundtrip.npz")
DRAWS = os.path.join(HERE, "golden", "train_pairs_draws.npz")
SEED, PAIRS, SHAPES = 20240611, 16, ((48, 64), (256, 480))          # tools/make_colour_draws_golden.py's


def _pillow_roundtrip(crop, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(crop[..., ::-1])).save(buf, format="JPEG", quality=int(quality), subsampling=2)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))[..., ::-1]


def _mismatch(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} of {ref.size} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"


# --------------------------------------------------------------------------------------------------------------------- round trip
def test_golden_fixture_is_complete():
    z = np.load(GOLDEN)
    assert list(z["qualities"]) == [50, 51, 75, 90, 99, 100]
    assert list(z["contents"]) == ["random", "constant", "ramp_h", "ramp_v", "checker", "saturated"]
    for size in ("16x16", "16x32", "48x32"):
        h, w = (int(v) for v in size.split("x"))
        assert z["in_" + size].shape == (6, h, w, 3) and z["out_" + size].shape == (6, 6, h, w, 3)
    assert os.path.getsize(GOLDEN) < 128 * 1024


@pytest.mark.parametrize("size", ["16x16", "16x32", "48x32"])
def test_roundtrip_equals_the_golden_outputs(size):
    z = np.load(GOLDEN)
    for name, crop, outs in zip(z["contents"], z["in_" + size], z["out_" + size]):
        for q, ref in zip(z["qualities"], outs):
            got = jpeg_roundtrip_u8_host(crop, int(q))
            assert got.dtype == np.uint8 and got.shape == crop.shape
            _mismatch(got, ref, f"{size} {name} quality {q}")


@pytest.mark.parametrize("side", [32, 128])
def test_roundtrip_equals_live_pillow(side):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(side)
    for q in (1, 37, 50, 83, 100):
        crop = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
        _mismatch(jpeg_roundtrip_u8_host(crop, q), _pillow_roundtrip(crop, q), f"{side} x {side} quality {q}")


def test_channel_order_is_bgr_to_libjpeg():
    """Chroma is subsampled and luma is not, and B weighs least in luma: a pure-channel-0 checkerboard loses more than a pure-channel-2
    one only if channel 0 is libjpeg's B — here it is enough that reversing the channels on the way in and out changes the result."""
    crop = np.random.default_rng(3).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    a = jpeg_roundtrip_u8_host(crop, 75)
    b = jpeg_roundtrip_u8_host(np.ascontiguousarray(crop[..., ::-1]), 75)[..., ::-1]
    assert not np.array_equal(a, b)


def test_quantisation_tables_equal_pillows_for_every_quality():
    Image = pytest.importorskip("PIL.Image")
    for q in range(1, 101):
        buf = io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=q, subsampling=2)
        buf.seek(0)
        tables = Image.open(buf).quantization
        luma, chroma = jpeg_quant_tables(q)
        # (Pillow lists a decoded file's tables in natural order or in zigzag order, depending on its version: either is the same set
        # of 64 values, and the natural-order comparison holds on the version whose round trip the other tests are held to)
        assert sorted(tables[0]) == sorted(luma.tolist()) and sorted(tables[1]) == sorted(chroma.tolist()), q
        if list(tables[0][:8]) == luma[:8].tolist():
            assert list(tables[0]) == luma.tolist() and list(tables[1]) == chroma.tolist(), q


def test_quantisation_table_arithmetic():
    for q in (1, 49, 50, 100):
        scale = 5000 // q if q < 50 else 200 - 2 * q
        luma, chroma = jpeg_quant_tables(q)
        assert luma[0] == min(max((16 * scale + 50) // 100, 1), 255) and chroma[63] == min(max((99 * scale + 50) // 100, 1), 255)
    assert np.all(jpeg_quant_tables(100)[0] == 1) and jpeg_quant_tables(1)[0].max() == 255          # both clamps
    assert jpeg_quant_tables(50)[0].tolist() == td.JPEG_LUMA_BASE.tolist()
    for bad in (0, 101, -1):
        with pytest.raises(ValueError):
            jpeg_quant_tables(bad)


def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    m = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    m[0] /= np.sqrt(2.0)
    return m                                                    # orthonormal: m @ m.T = I


def test_forward_dct_is_within_one_of_float64():
    """jfdctint's output is 8 times the orthonormal DCT (the quantiser divides by q << 3): with that factor taken off it is within 1
    of the float64 DCT.  A constant block is exact."""
    m = _dct_matrix()
    blocks = np.random.default_rng(0).integers(-128, 128, (500, 8, 8))
    blocks[0], blocks[1] = -128, 127
    ref = m @ blocks.astype(np.float64) @ m.T
    got = jpeg_fdct_islow(blocks)
    assert np.abs(got / 8.0 - ref).max() <= 1.0
    assert got[0, 0, 0] == -128 * 64 and got[1, 0, 0] == 127 * 64 and not got[:2].reshape(2, 64)[:, 1:].any()


def test_inverse_dct_is_within_one_of_float64():
    """jidctint takes dequantised coefficients, which are the orthonormal DCT's (the quantiser's q << 3 took the forward factor 8 off):
    its samples are within 1 of the float64 inverse DCT.  A lone DC term is exact."""
    m = _dct_matrix()
    rng = np.random.default_rng(1)
    samples = rng.integers(-128, 128, (500, 8, 8)).astype(np.float64)
    coef = np.rint(m @ samples @ m.T).astype(np.int64)
    coef[0], coef[1] = 0, 0
    coef[0, 0, 0], coef[1, 0, 0] = -1024, 1016
    ref = m.T @ coef.astype(np.float64) @ m
    got = jpeg_idct_islow(coef)
    assert np.abs(got - ref).max() <= 1.0
    assert np.all(got[0] == -128) and np.all(got[1] == 127)


@pytest.mark.parametrize("shape", [(16, 24), (24, 16), (8, 8), (0, 16), (17, 32)])
def test_sizes_that_are_no_whole_mcus_raise(shape):
    with pytest.raises(ValueError):
        jpeg_roundtrip_u8_host(np.zeros(shape + (3,), np.uint8), 75)


def test_other_inputs_raise():
    with pytest.raises(ValueError):
        jpeg_roundtrip_u8_host(np.zeros((16, 16, 3), np.float32), 75)
    with pytest.raises(ValueError):
        jpeg_roundtrip_u8_host(np.zeros((16, 16, 3), np.uint8), 0)


def test_a_256_crop_takes_well_under_a_second():
    import time
    crop = np.random.default_rng(2).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    jpeg_roundtrip_u8_host(crop, 60)
    t = time.perf_counter()
    jpeg_roundtrip_u8_host(crop, 60)
    assert time.perf_counter() - t < 0.5


def test_photometric_host_places_jpeg_between_blur_and_downscale():
    q = normal_quantiles()
    img = np.random.default_rng(4).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    op = np.zeros(1, dtype=PHOTO_DTYPE)[0]
    op["blur"], op["ksize"], op["noise"], op["downscale"], op["tap_row"] = td.BLUR_BOX, 3, NOISE_JPEG, 1, -1
    blur_only = op.copy()
    blur_only["noise"], blur_only["downscale"] = NOISE_NONE, 0
    blurred = photometric_u8_host(img, blur_only, None, q)
    jp = jpeg_roundtrip_u8_host(blurred, 62)
    ref = np.repeat(np.repeat(jp[::2, ::2], 2, axis=0), 2, axis=1)
    assert np.array_equal(photometric_u8_host(img, op, None, q, 62), ref)
    # without a quality in 1..100 the member is "none", as it is to the device's photometric kernel
    none = blur_only.copy()
    none["downscale"] = 1
    for quality in (0, 101, -1):
        assert np.array_equal(photometric_u8_host(img, op, None, q, quality), photometric_u8_host(img, none, None, q))
    assert np.array_equal(photometric_u8_host(img, op, None, q), photometric_u8_host(img, none, None, q))


# --------------------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("photometric", [False, True])
def test_default_members_reproduce_the_golden_draws(photometric):
    """tests/golden/train_pairs_draws.npz was recorded before `noise_members` existed: the default members, named or not, consume the
    generator and fill the record as that commit did."""
    golden = np.load(DRAWS)
    prefix = "on_" if photometric else "off_"
    for config in (dict(photometric=photometric), dict(photometric=photometric, noise_members=("multiplicative", "gauss")),
                   dict(photometric=photometric, noise_members=("gauss", "multiplicative"), jpeg_quality=(60, 70))):
        params = TrainPairBuilder(config, device="cpu").draw(np.zeros((PAIRS, 11)), SHAPES, np.random.default_rng(SEED))
        for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
            got = np.asarray(getattr(params, name))
            assert got.dtype == golden[prefix + name].dtype and np.array_equal(got, golden[prefix + name]), name
        if photometric:
            for name in ("blur", "ksize", "line", "noise", "var", "mult", "key", "downscale"):
                got = np.asarray(getattr(params.photo, name))
                assert got.dtype == golden[prefix + "photo_" + name].dtype and np.array_equal(got, golden[prefix + "photo_" + name]), name
        else:
            assert params.photo is None
        assert params.jpeg_quality is None


def test_jpeg_quality_is_drawn_last():
    """With "all" everything the default configuration draws comes first and unchanged but for the noise member picked; the quality
    follows the colour members' values."""
    golden = np.load(DRAWS)
    rng = np.random.default_rng(SEED)
    params = TrainPairBuilder(dict(photometric=True, noise_members="all", colour_members="all"), device="cpu").draw(
        np.zeros((PAIRS, 11)), SHAPES, rng)
    for name in ("blur", "ksize", "line", "var", "mult", "key", "downscale"):
        assert np.array_equal(getattr(params.photo, name), golden["on_photo_" + name]), name
    assert np.array_equal(params.photo.noise == NOISE_NONE, golden["on_photo_noise"] == NOISE_NONE)
    # the same stream without the member, then one more draw, is the quality
    rng2 = np.random.default_rng(SEED)
    TrainPairBuilder(dict(photometric=True, colour_members="all"), device="cpu").draw(np.zeros((PAIRS, 11)), SHAPES, rng2)
    assert np.array_equal(params.jpeg_quality, rng2.integers(50, 101, size=(PAIRS, 2)))
    assert params.jpeg_quality.dtype == np.int32 and params.jpeg_quality.shape == (PAIRS, 2)
    assert rng.random() == rng2.random()
    # the stage off: nothing drawn, whatever the members
    off = TrainPairBuilder(dict(noise_members="all"), device="cpu").draw(np.zeros((PAIRS, 11)), SHAPES, np.random.default_rng(SEED))
    assert off.photo is None and off.jpeg_quality is None
    assert [f.name for f in dataclasses.fields(td.TrainPairParams)][-1] == "jpeg_quality"


def test_noise_member_frequencies_and_quality_range():
    n = 10000                                                   # 20 000 crops
    b = TrainPairBuilder(dict(photometric=True, noise_p=1.0, noise_members="all"), device="cpu")
    assert b.noise_members == ("multiplicative", "gauss", "jpeg")
    params = b.draw(np.zeros((n, 11)), SHAPES, np.random.default_rng(11))
    noise = params.photo.noise.reshape(-1)
    sigma = np.sqrt((1 / 3) * (2 / 3) / noise.size)
    for kind in (NOISE_MULTIPLICATIVE, NOISE_GAUSS, NOISE_JPEG):
        assert abs(np.mean(noise == kind) - 1 / 3) < 4 * sigma, kind
    q = params.jpeg_quality
    assert q.min() == 50 and q.max() == 100
    counts = np.bincount(q.reshape(-1), minlength=101)[50:]
    expected = q.size / 51
    assert np.all(np.abs(counts - expected) < 5 * np.sqrt(expected))          # 51 values: 5 sigma each
    # at the reference's p the group fires on a fifth of the crops
    b = TrainPairBuilder(dict(photometric=True, noise_members="all"), device="cpu")
    noise = b.draw(np.zeros((n, 11)), SHAPES, np.random.default_rng(12)).photo.noise.reshape(-1)
    assert abs(np.mean(noise != NOISE_NONE) - 0.2) < 4 * np.sqrt(0.2 * 0.8 / noise.size)
    narrow = TrainPairBuilder(dict(photometric=True, noise_members="jpeg", jpeg_quality=(70, 72), noise_p=1.0), device="cpu")
    params = narrow.draw(np.zeros((200, 11)), SHAPES, np.random.default_rng(13))
    assert np.all(params.photo.noise == NOISE_JPEG) and set(np.unique(params.jpeg_quality)) == {70, 71, 72}


def test_member_names_are_validated():
    assert NOISE_MEMBERS == {"multiplicative": 1, "gauss": 2, "jpeg": 3} and NOISE_JPEG == 3
    assert TrainPairBuilder(device="cpu").noise_members == ("multiplicative", "gauss")
    assert TrainPairBuilder(dict(noise_members=("jpeg", "gauss")), device="cpu").noise_members == ("gauss", "jpeg")
    with pytest.raises(KeyError):
        TrainPairBuilder(dict(noise_members=("gauss", "iso")), device="cpu")
    with pytest.raises(KeyError):
        TrainPairBuilder(dict(noise_members="webp"), device="cpu")
    for bad in ((), ("gauss", "gauss")):
        with pytest.raises(ValueError):
            TrainPairBuilder(dict(noise_members=bad), device="cpu")
    for bad in ((0, 100), (60, 50), (50, 101)):
        with pytest.raises(ValueError):
            TrainPairBuilder(dict(jpeg_quality=bad), device="cpu")


def test_build_host_refuses_jpeg_draws_it_cannot_apply():
    frames = [np.random.default_rng(5).integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    pairs = np.array([[0, 10, 10, 20, 16, 0, 12, 8, 20, 16, 1]], dtype=np.float64)
    all_members = TrainPairBuilder(dict(photometric=True, noise_members="all"), device="cpu")
    params = all_members.draw(pairs, [f.shape for f in frames], np.random.default_rng(6))
    params.photo.noise[:] = NOISE_JPEG
    with pytest.raises(ValueError):                             # the member is not configured
        TrainPairBuilder(dict(photometric=True), device="cpu").build_host(frames, pairs, params)
    params.jpeg_quality = None
    with pytest.raises(ValueError):                             # no quality to apply
        all_members.build_host(frames, pairs, params)


def test_build_host_applies_jpeg_per_crop():
    """A pair whose template drew ImageCompression and whose search did not: the template differs from the JPEG-less build, the search
    does not, and the template is the round trip of the JPEG-less uint8 crop."""
    frames = [np.random.default_rng(7).integers(0, 256, (96, 128, 3), dtype=np.uint8)]
    pairs = np.array([[0, 30, 20, 40, 30, 0, 34, 24, 40, 30, 1]], dtype=np.float64)
    b = TrainPairBuilder(dict(photometric=True, noise_members="all"), device="cpu")
    params = b.draw(pairs, [f.shape for f in frames], np.random.default_rng(8))
    params.tone[:], params.colour[:] = 0, 0
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:] = 0, NOISE_NONE, 0
    plain = b.build_host(frames, pairs, params)
    ph.noise[0, 0] = NOISE_JPEG
    params.jpeg_quality[0, 0] = 55
    with_jpeg = b.build_host(frames, pairs, params)
    assert np.array_equal(with_jpeg.search, plain.search)
    mean, inv = td._MEAN, td._INV_STD
    u8 = np.rint(plain.template[0].transpose(1, 2, 0) / inv + mean).astype(np.uint8)
    assert np.array_equal(td._normalise_u8(u8), plain.template[0])            # (the uint8 crop recovered exactly)
    assert np.array_equal(with_jpeg.template[0], td._normalise_u8(jpeg_roundtrip_u8_host(u8, 55)))
    assert not np.array_equal(with_jpeg.template, plain.template)
