"""GlassBlur on the GPU (include/fear_train.h: fear_glass_u8): the operator through the C ABI, bit for bit against `glass_u8_host`, and
`TrainPairBuilder` with `glass_blur` against `build_host` and against the launches of the configurations without it."""
import numpy as np
import pytest
import torch

from dataops import (P, SENTINEL_U8 as SENTINEL, _device, equal as _equal, frames as _frames, guarded, inner, inside, pairs as _pairs)
from feartracker_amd.train_data import (BLUR_BOX, BLUR_GAUSSIAN, BLUR_GLASS, BLUR_MOTION, BLUR_NONE, FRAME_DTYPE, NOISE_GAUSS, NOISE_ISO,
                                        NOISE_JPEG, NOISE_NONE, PHOTO_DTYPE, WEATHER_NONE, WEATHER_RAIN, WEATHER_SHADOW, TrainPairBuilder,
                                        glass_u8_host, normal_quantiles, photo_tables)

pytestmark = pytest.mark.gpu

# no interior; a 2 x 2 interior; one tile, no multiple of anything; tiles cut on both axes; 4 x 4 and 8 x 8 tiles, the builder's sizes
SHAPES = [(4, 4), (10, 10), (12, 18), (34, 70), (128, 128), (256, 256)]


@pytest.fixture(scope="module")
def lib():
    from feartracker_amd.train_abi import load_train_library
    return load_train_library()


def _contents(h, w, seed=0):
    """Random, a 0..255 ramp and a two-level checkerboard: (3, h, w, 3) uint8."""
    rnd = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.stack([np.where((yy + xx) & 1, 200, 30), np.where((yy + xx) & 1, 0, 255), np.where((yy + xx) & 1, 90, 91)], axis=-1)
    ramp = np.stack([(yy * w + xx) * 255 // (h * w - 1), 255 - xx * 255 // (w - 1), yy * 255 // (h - 1)], axis=-1)
    return np.stack([rnd, ramp.astype(np.uint8), checker.astype(np.uint8)])


def _records(blurs, seed=0):
    """FearPhotoOp records with these blur kinds, a seeded key each, and values for the members fear_glass_u8 does not read."""
    rng = np.random.default_rng(seed)
    ops = np.zeros(len(blurs), dtype=PHOTO_DTYPE)
    ops["blur"], ops["ksize"], ops["noise"], ops["scale"], ops["downscale"], ops["tap_row"] = blurs, 5, NOISE_GAUSS, 3.0, 1, -1
    ops["key"] = rng.integers(0, 2 ** 32, (len(blurs), 2), dtype=np.uint64).astype(np.uint32)
    return ops


def _run(lib, crops, ops):
    """fear_glass_u8 on (n, H, W, 3) uint8 crops, the guard band around the output checked and the input left alone."""
    n, h, w = crops.shape[:3]
    d_in, d_ops = _device(crops), _device(ops)
    count = n * h * w * 3
    out = guarded(count)
    rc = lib.fear_glass_u8(P(d_in.data_ptr()), n, h, w, P(d_ops.data_ptr()), inner(out), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), crops), "input written"
    return inside(out, count).reshape(n, h, w, 3)


def _check(lib, crops, ops):
    out = _run(lib, crops, ops)
    for i in range(len(crops)):
        ref = glass_u8_host(crops[i], ops[i]) if ops["blur"][i] == BLUR_GLASS else crops[i]
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, (f"crop {i} blur {ops['blur'][i]}: {len(bad)} of {ref.size} values differ, first at {bad[0].tolist()}: "
                               f"{out[i][tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    return out


# ---------------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("shape", SHAPES)
def test_member(lib, shape):
    crops = _contents(*shape, seed=shape[0])
    out = _check(lib, crops, _records([BLUR_GLASS] * 3, seed=shape[1]))
    assert not np.array_equal(out[0], crops[0])                                   # the member did something to the random crop
    one = _run(lib, crops[:1], _records([BLUR_GLASS] * 3, seed=shape[1])[:1])         # n = 1
    assert np.array_equal(one[0], out[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_record_per_crop(lib, shape):
    """n = 5: the member, "none", another blur kind, a kind nobody draws, the member again with another key."""
    c = _contents(*shape, seed=shape[0] + 1)
    crops = np.concatenate([c, c[:1][:, ::-1], c[:1]])
    ops = _records([BLUR_GLASS, BLUR_NONE, BLUR_GAUSSIAN, 9, BLUR_GLASS], seed=shape[1] + 1)
    out = _check(lib, crops, ops)
    for i in (1, 2, 3):
        assert np.array_equal(out[i], crops[i])                                   # copies
    if min(shape) > 8:
        assert not np.array_equal(out[0], out[4])                                 # one crop, two keys
    one = _run(lib, crops[4:5], ops[4:5])                                         # a record other than the first
    assert np.array_equal(one[0], out[4])


def test_copies(lib):
    """Crops without the member leave as they came, whatever else their records hold."""
    for shape in SHAPES[:4]:
        crops = np.concatenate([_contents(*shape, seed=7), _contents(*shape, seed=8)])
        ops = _records([BLUR_NONE, BLUR_BOX, BLUR_MOTION, -1, 6, 1 << 20], seed=9)
        assert np.array_equal(_check(lib, crops, ops), crops)


def test_argument_checks(lib):
    crops = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    d_ops = _device(_records([BLUR_GLASS, BLUR_NONE]))
    out = torch.full((2, 8, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        return lib.fear_glass_u8(kw.get("crops", P(crops.data_ptr())), kw.get("n", 2), kw.get("h", 8), kw.get("w", 8),
                                 kw.get("ops", P(d_ops.data_ptr())), kw.get("out", P(out.data_ptr())), st)

    for bad in (dict(h=7), dict(w=7), dict(w=2), dict(h=2), dict(h=0), dict(n=-1), dict(n=65536), dict(h=258), dict(w=258),
                dict(out=P(crops.data_ptr()))):
        assert call(**bad) == -2, bad
    for name in ("crops", "ops", "out"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, crops=None, ops=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                          # refused calls and n = 0 write nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ----------------------------------------------------------------------------------------------------------------------- builder
@pytest.mark.parametrize("others", [False, True])
def test_build_equals_build_host(others):
    """B = 8 with every crop forced to the member; with `others` the noise group's and the weather group's members run behind it on some
    crops, which pins the order: GlassBlur, noise, weather, Downscale."""
    frames = _frames(2)
    pairs = _pairs(8, seed=3)
    config = dict(photometric=True, glass_blur=True)
    if others:
        config.update(noise_members="all", iso_noise=True, weather_members="all")
    builder = TrainPairBuilder(config, device=0)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(4))
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:] = BLUR_GLASS, NOISE_NONE, 0
    ph.downscale[4, 1], ph.downscale[6, 0] = 1, 1
    if others:
        params.weather[:] = WEATHER_NONE
        ph.noise[0, 1], ph.noise[1, 0], ph.noise[2, 1], ph.noise[3, 0] = NOISE_ISO, NOISE_JPEG, NOISE_GAUSS, NOISE_JPEG
        params.weather[2, 1], params.weather[3, 0], params.weather[5, 0] = WEATHER_RAIN, WEATHER_SHADOW, WEATHER_RAIN
    host = builder.build_host(frames, pairs, params)
    if not others:                                                                # the member does something to every crop
        ph.blur[:] = BLUR_NONE
        untouched = builder.build_host(frames, pairs, params)
        ph.blur[:] = BLUR_GLASS
        for k in range(8):
            assert not np.array_equal(host.template[k], untouched.template[k]) and not np.array_equal(host.search[k], untouched.search[k]), k
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    _equal(builder.build(frames, pairs, params), host)                            # host frames (and the allocators warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dev = builder.build(dev_frames, pairs, params)                            # device frames: no wait for the GPU
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _equal(dev, host)


def test_one_side_alone_draws_the_member():
    """The launch is decided per side: only a template drew the member, then only a search."""
    frames = _frames(3)
    pairs = _pairs(4, seed=5)
    builder = TrainPairBuilder(dict(photometric=True, glass_blur=True), device=0)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(8))
    for which in (0, 1):
        params.photo.blur[:] = [[BLUR_BOX, BLUR_NONE], [BLUR_NONE, BLUR_MOTION], [BLUR_NONE, BLUR_NONE], [BLUR_GAUSSIAN, BLUR_BOX]]
        params.photo.blur[2, which] = BLUR_GLASS
        _equal(builder.build(frames, pairs, params), builder.build_host(frames, pairs, params))
    with pytest.raises(ValueError, match="GlassBlur"):
        TrainPairBuilder(dict(photometric=True), device=0).build(frames, pairs, params)


def test_builds_without_the_key_are_the_launches_of_before(lib):
    """With glass_blur at its default `build` is fear_frame_border_u8 + fear_train_pairs, and with photometric=True
    fear_frame_border_u8 + fear_train_pairs_u8 + one fear_photometric_u8 per side, on the same tables, bit for bit; and so is a build with
    the key on in which no crop drew the member."""
    frames = _frames(5)
    pairs = _pairs(4, seed=6)
    B, F = 4, len(frames)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    qtable = torch.from_numpy(normal_quantiles().copy()).cuda()
    ftab = np.zeros(F, dtype=FRAME_DTYPE)
    for i, f in enumerate(d_frames):
        ftab[i] = (f.data_ptr(), f.shape[0], f.shape[1])
    st = P(torch.cuda.current_stream().cuda_stream)
    for photometric, key in ((False, False), (True, False), (True, True)):
        builder = TrainPairBuilder(dict(photometric=photometric, glass_blur=key), device=0, seed=9)
        params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(9))
        if photometric:
            params.photo.noise[:, 0], params.photo.blur[:, 1], params.photo.blur[:, 0] = [0, 1, 2, 0], [1, 2, 3, 4], 0
        got = builder.build(frames, pairs, params)
        tab = builder.tables(pairs, params)
        d_ftab, d_geom, d_lut = _device(ftab), _device(tab["geom"]), _device(tab["lut"])
        border = torch.empty((F, 3), dtype=torch.uint8, device="cuda")
        outs = [torch.empty(s, device="cuda") for s in ((B, 3, 128, 128), (B, 3, 256, 256), (B, 4, 16, 16), (B, 1, 16, 16), (B, 16, 16))]
        assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), F, P(border.data_ptr()), st) == 0
        if not photometric:
            assert lib.fear_train_pairs(P(d_ftab.data_ptr()), F, P(border.data_ptr()), P(d_geom.data_ptr()), P(d_lut.data_ptr()), B,
                                        *[P(o.data_ptr()) for o in outs], st) == 0
        else:
            u8 = [torch.empty((B, s, s, 3), dtype=torch.uint8, device="cuda") for s in (128, 256)]
            assert lib.fear_train_pairs_u8(P(d_ftab.data_ptr()), F, P(border.data_ptr()), P(d_geom.data_ptr()), P(d_lut.data_ptr()), B,
                                           *[P(o.data_ptr()) for o in u8 + outs[2:]], st) == 0
            ops, taps = photo_tables(params.photo)
            d_taps = _device(taps) if taps.size else None
            for which, side in enumerate((128, 256)):
                d_ops = _device(np.ascontiguousarray(ops[:, which]))
                assert lib.fear_photometric_u8(P(u8[which].data_ptr()), B, side, side, P(d_ops.data_ptr()),
                                               P(d_taps.data_ptr()) if d_taps is not None else None, P(qtable.data_ptr()),
                                               P(outs[which].data_ptr()), st) == 0
        torch.cuda.synchronize()
        for name, ref in zip(("template", "search", "gt_reg", "gt_cls", "gt_weight"), outs):
            assert torch.equal(getattr(got, name), ref), (photometric, key, name)
