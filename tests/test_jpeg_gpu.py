"""ImageCompression on the GPU (include/fear_train.h: fear_jpeg_u8, fear_photometric_stage_u8): the operators through the C ABI, bit for
bit against `jpeg_roundtrip_u8_host` and `photometric_u8_host`, and `TrainPairBuilder` with crops that drew the member against
`build_host`."""
import os

import numpy as np
import pytest
import torch

from dataops import P, SENTINEL_U8 as SENTINEL, equal as _equal, frames as _frames, pairs as _pairs, run_jpeg as _run_jpeg, run_stage as _run_stage
from feartracker_amd.train_data import (BLUR_BOX, BLUR_GAUSSIAN, BLUR_MEDIAN, BLUR_MOTION, BLUR_NONE, NOISE_GAUSS, NOISE_JPEG,
                                        NOISE_MULTIPLICATIVE, NOISE_NONE, PHOTO_DTYPE, TrainPairBuilder, jpeg_roundtrip_u8_host,
                                        motion_kernel, motion_taps, normal_quantiles, photometric_u8_host)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_roundtrip.npz")


@pytest.fixture(scope="module")
def lib():
    from feartracker_amd.train_abi import load_train_library
    return load_train_library()


@pytest.fixture(scope="module")
def qtable():
    return torch.from_numpy(normal_quantiles().copy()).cuda()


def _check_jpeg(lib, crops, quality):
    out = _run_jpeg(lib, crops, quality)
    for i, q in enumerate(quality):
        ref = jpeg_roundtrip_u8_host(crops[i], int(q)) if 1 <= q <= 100 else crops[i]
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, (f"crop {i} quality {q}: {len(bad)} of {ref.size} bytes differ, first at {bad[0].tolist()}: "
                               f"{out[i][tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    return out


def _contents(h, w, seed):
    """Five crops: random, a ramp on both axes, a 1-pixel checkerboard, 8 x 8 blocks saturated at 0 and 255 side by side, a constant."""
    yy, xx = np.mgrid[0:h, 0:w]
    rnd = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ramp = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), 255 - (xx + yy) * 255 // (h + w - 2)], axis=-1).astype(np.uint8)
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    sat = np.repeat(((((yy // 8) + (xx // 8)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    sat[..., 1] = 255 - sat[..., 1]
    const = np.broadcast_to(np.array([201, 17, 94], dtype=np.uint8), (h, w, 3))
    return np.stack([rnd, ramp, checker, sat, const])


# ---------------------------------------------------------------------------------------------------------------------- fear_jpeg_u8
@pytest.mark.parametrize("size", ["16x16", "16x32", "48x32"])
def test_fixture_contents_equal_pillow(lib, size):
    """The fixture's crops, every content in one call per quality: the device equals Pillow's recorded bytes (and so the host's)."""
    z = np.load(GOLDEN)
    crops = z["in_" + size]
    for j, q in enumerate(z["qualities"]):
        out = _run_jpeg(lib, crops, [int(q)] * len(crops))
        assert np.array_equal(out, z["out_" + size][:, j]), f"{size} quality {q}"


@pytest.mark.parametrize("shape", [(16, 16), (16, 32), (48, 32), (128, 128), (256, 256)])
def test_five_crops_with_a_quality_each(lib, shape):
    """n = 5, a different quality per crop; 0, 101 and -1 copy.  48 x 32 has 6 MCUs: a workgroup's group of four ends inside the crop."""
    crops = _contents(*shape, seed=shape[0] + shape[1])
    for quality in ([50, 100, 0, 75, 1], [101, 51, 99, -1, 90]):
        out = _check_jpeg(lib, crops, quality)
        for i, q in enumerate(quality):
            if not 1 <= q <= 100:
                assert np.array_equal(out[i], crops[i])


@pytest.mark.parametrize("shape", [(16, 16), (48, 32), (32, 80)])
def test_single_crop(lib, shape):
    crops = _contents(*shape, seed=7)
    for i, q in ((0, 63), (3, 100), (2, 50), (1, 0)):
        _check_jpeg(lib, crops[i:i + 1], [q])


def test_jpeg_argument_checks(lib):
    crops = torch.zeros((2, 16, 32, 3), dtype=torch.uint8, device="cuda")
    quality = torch.tensor([50, 90], dtype=torch.int32, device="cuda")
    need = lib.fear_jpeg_workspace_bytes(2, 16, 32)
    assert need >= 2 * 16 * 32 * 3 // 2
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 16, 32, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        return lib.fear_jpeg_u8(kw.get("crops", P(crops.data_ptr())), kw.get("n", 2), kw.get("h", 16), kw.get("w", 32),
                                kw.get("quality", P(quality.data_ptr())), kw.get("ws", P(ws.data_ptr())), kw.get("ws_bytes", need),
                                kw.get("out", P(out.data_ptr())), st)

    for bad in (dict(h=8), dict(w=24), dict(h=0), dict(w=0), dict(h=-16), dict(h=17), dict(n=-1), dict(n=65536), dict(out=P(crops.data_ptr()))):
        assert call(**bad) == -2, bad
    for name in ("crops", "quality", "out"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -7, bad
    assert call(n=0, crops=None, quality=None, out=None, ws=None, ws_bytes=0) == 0
    for bad in ((2, 8, 32), (2, 16, 24), (-1, 16, 16), (65536, 16, 16)):
        assert lib.fear_jpeg_workspace_bytes(*bad) == 0, bad
    assert lib.fear_jpeg_workspace_bytes(0, 16, 16) <= 16
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                         # refused calls and n = 0 write nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out.view(-1, 3)[:, 0] != SENTINEL).all())                       # (a black crop decodes to black)


# --------------------------------------------------------------------------------------------------------- fear_photometric_stage_u8
def _ops(n, **fields):
    ops = np.zeros(n, dtype=PHOTO_DTYPE)
    ops["ksize"], ops["scale"], ops["tap_row"] = 3, 1.0, -1
    for name, value in fields.items():
        ops[name] = value
    return ops


def _chain_records(seed):
    """Five crops, a three-stage chain each: every blur member, both noises, Downscale; and one record that is "none" throughout."""
    ops = _ops(6)
    ops["blur"] = [BLUR_MOTION, BLUR_MEDIAN, BLUR_BOX, BLUR_MOTION, BLUR_GAUSSIAN, BLUR_NONE]
    ops["ksize"] = [7, 5, 3, 3, 7, 3]
    ops["noise"] = [NOISE_GAUSS, NOISE_MULTIPLICATIVE, NOISE_GAUSS, NOISE_MULTIPLICATIVE, NOISE_GAUSS, NOISE_JPEG]    # JPEG: "none" here
    ops["scale"] = [np.sqrt(35.0), 1.07, np.sqrt(10.0), 0.93, np.sqrt(20.0), 1.0]
    ops["key"] = np.random.default_rng(seed).integers(0, 2 ** 32, (6, 2), dtype=np.uint64).astype(np.uint32)
    ops["downscale"] = [1, 1, 1, 1, 1, 0]
    taps = np.zeros((2, 49), dtype=np.float32)
    ops["tap_row"][0], ops["tap_row"][3] = 1, 0
    taps[1] = motion_taps(motion_kernel(7, 6, 1, 0, 5))
    taps[0] = motion_taps(motion_kernel(3, 1, 0, 1, 2))
    return ops, taps


@pytest.mark.parametrize("shape", [(8, 8), (34, 70)])
def test_stage_u8_equals_photometric_u8_host(lib, qtable, shape):
    ops, taps = _chain_records(shape[0])
    rng = np.random.default_rng(shape[1])
    crops = rng.integers(0, 256, (6,) + shape + (3,), dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    crops[1] = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    out = _run_stage(lib, qtable, crops, ops, taps)
    q = normal_quantiles()
    for i in range(len(crops)):
        ref = photometric_u8_host(crops[i], ops[i], taps, q)
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, f"crop {i} {ops[i]}: {len(bad)} of {ref.size} bytes differ, first at {bad[0].tolist()}"
    assert np.array_equal(out[5], crops[5])


def test_stage_u8_argument_checks(lib, qtable):
    crops = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    ops = torch.from_numpy(_ops(2).view(np.uint8).copy()).cuda()
    out = torch.full((2, 8, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        return lib.fear_photometric_stage_u8(kw.get("crops", P(crops.data_ptr())), kw.get("n", 2), kw.get("h", 8), kw.get("w", 8),
                                             kw.get("ops", P(ops.data_ptr())), None, kw.get("q", P(qtable.data_ptr())),
                                             kw.get("out", P(out.data_ptr())), st)

    for bad in (dict(h=7), dict(w=7), dict(w=2), dict(h=2), dict(h=0), dict(n=-1), dict(n=65536), dict(out=P(crops.data_ptr()))):
        assert call(**bad) == -2, bad
    for name in ("crops", "ops", "q", "out"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, crops=None, ops=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ----------------------------------------------------------------------------------------------------------------------- builder
def _forced_params(builder, frames, pairs, seed):
    """B = 8 draws with ImageCompression forced on some crops — a blur in front and a Downscale behind among them — while the other
    crops keep chains of their own."""
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(seed))
    params.tone[:] = [0, 1, 2, 0, 0, 1, 2, 0]
    ph = params.photo
    ph.blur[:] = [[BLUR_BOX, BLUR_GAUSSIAN], [BLUR_MEDIAN, BLUR_MOTION], [BLUR_MOTION, BLUR_NONE], [BLUR_NONE, BLUR_MEDIAN],
                  [BLUR_NONE, BLUR_NONE], [BLUR_GAUSSIAN, BLUR_BOX], [BLUR_NONE, BLUR_MOTION], [BLUR_MEDIAN, BLUR_NONE]]
    ph.ksize[:] = [[3, 5], [7, 7], [3, 5], [3, 3], [3, 3], [7, 3], [5, 5], [5, 7]]
    ph.line[1, 1], ph.line[2, 0], ph.line[6, 1] = (0, 6, 5, 0), (2, 0, 2, 2), (4, 0, 0, 3)
    ph.noise[:] = [[NOISE_JPEG, NOISE_MULTIPLICATIVE], [NOISE_NONE, NOISE_JPEG], [NOISE_JPEG, NOISE_JPEG], [NOISE_GAUSS, NOISE_MULTIPLICATIVE],
                   [NOISE_NONE, NOISE_NONE], [NOISE_GAUSS, NOISE_JPEG], [NOISE_JPEG, NOISE_GAUSS], [NOISE_MULTIPLICATIVE, NOISE_JPEG]]
    ph.downscale[:] = [[1, 1], [0, 1], [0, 0], [1, 0], [0, 1], [1, 1], [1, 0], [0, 0]]
    params.jpeg_quality[:] = [[50, 60], [100, 70], [99, 51], [80, 80], [55, 65], [75, 90], [100, 50], [85, 95]]
    return params


def test_build_with_jpeg_equals_build_host():
    frames = _frames(3)
    pairs = _pairs(8, seed=4)
    builder = TrainPairBuilder(dict(photometric=True, noise_members="all"), device=0)
    params = _forced_params(builder, frames, pairs, seed=5)
    host = builder.build_host(frames, pairs, params)
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    _equal(builder.build(frames, pairs, params), host)                 # host frames (and the allocators warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dev = builder.build(dev_frames, pairs, params)                 # device frames: no wait for the GPU
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _equal(dev, host)
    # the member does something: the same draws with it taken off differ on exactly the crops that drew it
    drew = params.photo.noise == NOISE_JPEG
    params.photo.noise[drew] = NOISE_NONE
    plain = builder.build_host(frames, pairs, params)
    for k in range(8):
        assert np.array_equal(plain.template[k], host.template[k]) == (not drew[k, 0]), k
        assert np.array_equal(plain.search[k], host.search[k]) == (not drew[k, 1]), k


def test_build_with_jpeg_and_device_colour_members():
    """The colour stage's own launches in front of the three-launch path: the records of both ride in the one transfer."""
    frames = _frames(6)
    pairs = _pairs(8, seed=7)
    builder = TrainPairBuilder(dict(photometric=True, noise_members="all", colour_members="all"), device=0)
    params = _forced_params(builder, frames, pairs, seed=8)
    params.colour[:] = [5, 6, 7, 8, 0, 4, 1, 6]
    host = builder.build_host(frames, pairs, params)
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    builder.build(dev_frames, pairs, params)                           # (the quantile table and the allocators warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dev = builder.build(dev_frames, pairs, params)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _equal(dev, host)


def test_a_batch_without_a_jpeg_draw_equals_the_default_members_build():
    frames = _frames(9)
    pairs = _pairs(8, seed=10)
    with_all = TrainPairBuilder(dict(photometric=True, noise_members="all"), device=0)
    default = TrainPairBuilder(dict(photometric=True), device=0)
    params = _forced_params(with_all, frames, pairs, seed=11)
    ph = params.photo
    ph.noise[ph.noise == NOISE_JPEG] = NOISE_GAUSS
    a = with_all.build(frames, pairs, params)
    b = default.build(frames, pairs, params)
    torch.cuda.synchronize()
    _equal(a, b)
    _equal(a, default.build_host(frames, pairs, params))
