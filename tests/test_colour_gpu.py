"""The colour members that are no lookup table on the GPU (include/fear_train.h: fear_colour_u8): the operator through the C ABI, bit for
bit against `colour_u8_host`, and `TrainPairBuilder` with `colour_members` against `build_host` and against the two-launch path."""
import itertools

import numpy as np
import pytest
import torch

from dataops import P, SENTINEL_U8 as SENTINEL, equal as _equal, frames as _frames, pairs as _pairs, run_colour as _run
from feartracker_amd.train_data import (BLUR_GAUSSIAN, BLUR_MEDIAN, BLUR_NONE, COLOUR_DTYPE, COLOUR_EMBOSS, COLOUR_EQUALIZE, COLOUR_HSV,
                                        COLOUR_JITTER, COLOUR_TONE_CURVE, FRAME_DTYPE, NOISE_GAUSS, NOISE_NONE, TrainPairBuilder,
                                        TrainPairParams, colour_tables, colour_u8_host)

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (8, 8), (34, 70), (128, 128), (256, 256)]


@pytest.fixture(scope="module")
def lib():
    from feartracker_amd.train_abi import load_train_library
    return load_train_library()


def _contents(h, w, seed=0):
    """Random, constant (Equalize's single-bin branch), a two-level checkerboard and a 0..255 ramp: (4, h, w, 3) uint8."""
    rnd = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    const = np.broadcast_to(np.array([37, 0, 255], np.uint8), (h, w, 3))
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.stack([np.where((yy + xx) & 1, 200, 30), np.where((yy + xx) & 1, 0, 255), np.where((yy + xx) & 1, 90, 91)], axis=-1)
    ramp = np.stack([(yy * w + xx) * 255 // (h * w - 1), 255 - xx * 255 // (w - 1), yy * 255 // (h - 1)], axis=-1)
    return np.stack([rnd, const, checker.astype(np.uint8), ramp.astype(np.uint8)])


def _records(kinds, seed=0):
    """Records and tables for crops that drew `kinds`, with seeded member values inside the draw limits."""
    rng = np.random.default_rng(seed)
    n = len(kinds)
    params = TrainPairParams(context=np.zeros(n), jitter=np.zeros((n, 4)), tone=np.zeros(n, np.int32), colour=np.asarray(kinds, np.int32),
                             alpha=np.ones(n), beta=np.zeros(n), gamma=np.ones(n), shift=np.zeros((n, 3)), frame_shapes=(),
                             hsv=np.stack([rng.uniform(-20, 20, n), rng.uniform(-30, 30, n), rng.uniform(-20, 20, n)], axis=1),
                             colour_jitter=np.concatenate([rng.uniform(0.8, 1.2, (n, 3)), rng.uniform(-0.2, 0.2, (n, 1))], axis=1),
                             colour_jitter_order=rng.permuted(np.tile(np.arange(4, dtype=np.int32), (n, 1)), axis=1),
                             emboss=np.stack([rng.uniform(0.2, 0.5, n), rng.uniform(0.2, 0.7, n)], axis=1))
    return (params,) + colour_tables(params)


def _check(lib, crops, ops, aux):
    out = _run(lib, crops, ops, aux)
    for i in range(len(crops)):
        ref = colour_u8_host(crops[i], ops[i], aux[i])
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, (f"crop {i} kind {ops['kind'][i]} order {ops['order'][i]}: {len(bad)} of {ref.size} values differ, first at "
                               f"{bad[0].tolist()}: {out[i][tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    return out


# ---------------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_EMBOSS])
def test_members(lib, kind, shape):
    crops = _contents(*shape, seed=kind)
    _, ops, aux = _records([kind] * 4, seed=shape[1])
    out = _check(lib, crops, ops, aux)
    if kind == COLOUR_EQUALIZE:
        assert np.array_equal(out[1], crops[1])                                   # one bin holds every pixel: unchanged
        assert sorted(np.unique(out[2][..., 0]).tolist()) == [0, 255]             # two levels spread to the ends


@pytest.mark.parametrize("shape", SHAPES)
def test_colour_jitter_every_order(lib, shape):
    """24 crops in one call, one order each."""
    orders = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
    params, _, _ = _records([COLOUR_JITTER] * 24, seed=shape[0])
    params.colour_jitter_order = orders
    ops, aux = colour_tables(params)
    assert np.array_equal(ops["order"], orders)
    crops = _contents(*shape, seed=5)[np.arange(24) % 4]
    crops[4:8] = _contents(*shape, seed=6)
    _check(lib, crops, ops, aux)


def test_other_kinds_copy(lib):
    for shape in SHAPES[:3]:
        crops = np.concatenate([_contents(*shape, seed=7), _contents(*shape, seed=8)[:2]])
        _, ops, aux = _records([COLOUR_JITTER] * 6)
        ops["kind"][:5] = [0, COLOUR_TONE_CURVE, 9, -1, 1 << 20]                  # and a ColorJitter whose order is no permutation
        ops["order"][5] = [0, 1, 1, 3]
        out = _check(lib, crops, ops, aux)
        assert np.array_equal(out, crops)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_record_per_crop(lib, shape):
    kinds = [COLOUR_EMBOSS, COLOUR_JITTER, 0, COLOUR_EQUALIZE, COLOUR_HSV]
    c = _contents(*shape, seed=shape[0] + 1)
    crops = np.concatenate([c, c[:1][:, ::-1]])
    _, ops, aux = _records(kinds, seed=shape[1] + 1)
    out = _check(lib, crops, ops, aux)
    assert not np.array_equal(out[0], out[4])
    for i in (0, 1, 3, 4):                                                        # n = 1, every kind, a record other than the first
        one = _run(lib, crops[i:i + 1], ops[i:i + 1], aux[i:i + 1])
        assert np.array_equal(one[0], out[i])


def test_statistics_are_per_crop(lib):
    """Two crops with the same record and different content: each gets its own histogram and its own mean."""
    a = _contents(34, 70, seed=11)[0]
    crops = np.stack([a, a // 2, a])
    for kind in (COLOUR_EQUALIZE, COLOUR_JITTER):
        _, ops, aux = _records([kind] * 3, seed=3)
        ops[:], aux[:] = ops[0], aux[0]
        out = _check(lib, crops, ops, aux)
        assert np.array_equal(out[0], out[2])


def test_argument_checks(lib):
    crops = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    _, ops, aux = _records([COLOUR_HSV, COLOUR_EMBOSS])
    d_ops, d_aux = torch.from_numpy(ops.view(np.uint8).copy()).cuda(), torch.from_numpy(aux).cuda()
    out = torch.full((2, 8, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        return lib.fear_colour_u8(kw.get("crops", P(crops.data_ptr())), kw.get("n", 2), kw.get("h", 8), kw.get("w", 8),
                                  kw.get("ops", P(d_ops.data_ptr())), kw.get("aux", P(d_aux.data_ptr())), kw.get("out", P(out.data_ptr())), st)

    for bad in (dict(h=7), dict(w=7), dict(w=2), dict(h=2), dict(h=0), dict(n=-1), dict(n=65536), dict(out=P(crops.data_ptr()))):
        assert call(**bad) == -2, bad
    for name in ("crops", "ops", "aux", "out"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, crops=None, ops=None, aux=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                          # refused calls and n = 0 write nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------- builder
@pytest.mark.parametrize("photometric", [False, True])
def test_all_members_build_equals_build_host(photometric):
    """B = 8, every member once (the tone-curve member runs here only: it is a table of the first stage), every tone branch."""
    frames = _frames(2)
    pairs = _pairs(8, seed=3)
    builder = TrainPairBuilder(dict(colour_members="all", photometric=photometric), device=0)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(4))
    params.colour[:] = [7, 5, 4, 8, 6, 1, 2, 3]
    params.tone[:] = [0, 1, 2, 0, 0, 0, 1, 0]
    if photometric:
        ph = params.photo
        ph.blur[:], ph.noise[:], ph.downscale[:] = BLUR_NONE, NOISE_NONE, 0
        ph.blur[0], ph.blur[3, 1], ph.ksize[:] = (BLUR_GAUSSIAN, BLUR_MEDIAN), BLUR_MEDIAN, 3
        ph.noise[1, 0], ph.downscale[4, 1] = NOISE_GAUSS, 1
    host = builder.build_host(frames, pairs, params)
    plain = TrainPairBuilder(dict(photometric=photometric), device=0)
    params.colour[:] = 0
    untouched = plain.build_host(frames, pairs, params)
    params.colour[:] = [7, 5, 4, 8, 6, 1, 2, 3]
    for k in range(8):                                                            # every member does something to its pair
        assert not np.array_equal(host.search[k], untouched.search[k]), k
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


def test_default_members_build_is_the_two_launch_result(lib):
    """The default configuration still is fear_frame_border_u8 + fear_train_pairs on the same tables, bit for bit; and the three-stage
    path of "all" gives those bits too for pairs that drew a lookup-table member or none."""
    frames = _frames(5)
    pairs = _pairs(4, seed=6)
    builder = TrainPairBuilder(device=0, seed=9)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(9))
    params.colour[:] = [0, 1, 2, 3]
    got = builder.build(frames, pairs, params)
    tab = builder.tables(pairs, params)
    B, F = 4, len(frames)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    ftab = np.zeros(F, dtype=FRAME_DTYPE)
    for i, f in enumerate(d_frames):
        ftab[i] = (f.data_ptr(), f.shape[0], f.shape[1])
    d_ftab = torch.from_numpy(ftab.view(np.uint8).copy()).cuda()
    d_geom = torch.from_numpy(tab["geom"].view(np.uint8).copy()).cuda()
    d_lut = torch.from_numpy(tab["lut"].copy()).cuda()
    border = torch.empty((F, 3), dtype=torch.uint8, device="cuda")
    outs = [torch.empty(s, device="cuda") for s in ((B, 3, 128, 128), (B, 3, 256, 256), (B, 4, 16, 16), (B, 1, 16, 16), (B, 16, 16))]
    st = P(torch.cuda.current_stream().cuda_stream)
    assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), F, P(border.data_ptr()), st) == 0
    assert lib.fear_train_pairs(P(d_ftab.data_ptr()), F, P(border.data_ptr()), P(d_geom.data_ptr()), P(d_lut.data_ptr()), B,
                                *[P(o.data_ptr()) for o in outs], st) == 0
    torch.cuda.synchronize()
    for name, ref in zip(("template", "search", "gt_reg", "gt_cls", "gt_weight"), outs):
        assert torch.equal(getattr(got, name), ref), name
    wide = TrainPairBuilder(dict(colour_members="all"), device=0)
    wide_params = wide.draw(pairs, [f.shape for f in frames], np.random.default_rng(9))
    for name in ("context", "jitter", "tone", "alpha", "beta", "gamma", "shift"):
        setattr(wide_params, name, getattr(params, name))
    wide_params.colour[:] = [0, 1, 2, 3]
    _equal(wide.build(frames, pairs, wide_params), got)
