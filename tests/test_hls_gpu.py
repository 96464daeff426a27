"""ISONoise, RandomRain and RandomShadow on the GPU (include/fear_train.h: fear_hls_u8): the operator through the C ABI, bit for bit
against `hls_u8_host`, and `TrainPairBuilder` with `iso_noise` and `weather_members` against `build_host` and against the launches of the
configurations without them."""
import numpy as np
import pytest
import torch

from dataops import (P, SENTINEL_U8 as SENTINEL, _device, equal as _equal, frames as _frames, guarded, inner, inside, pairs as _pairs)
from feartracker_amd.train_data import (BLUR_BOX, BLUR_NONE, FRAME_DTYPE, HLS_COPY, HLS_DTYPE, HLS_ISO, HLS_RAIN, HLS_SHADOW, NOISE_GAUSS,
                                        NOISE_ISO, NOISE_JPEG, NOISE_MULTIPLICATIVE, NOISE_NONE, WEATHER_NONE, WEATHER_RAIN, WEATHER_SHADOW,
                                        TrainPairBuilder, hls_u8_host, iso_exp_table, iso_hue_scale, iso_lambda_q, normal_quantiles,
                                        photo_tables, rain_segments, hls_to_rgb_u8, rgb_to_hls_u8, shadow_segments)

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (8, 8), (34, 70), (128, 128), (256, 256)]


@pytest.fixture(scope="module")
def lib():
    from feartracker_amd.train_abi import load_train_library
    return load_train_library()


@pytest.fixture(scope="module")
def tables():
    """The quantile table and exp(-i / 16), on the host and on the device."""
    q, e = normal_quantiles(), iso_exp_table()
    return q, e, torch.from_numpy(q.copy()).cuda(), torch.from_numpy(e.copy()).cuda()


def _contents(h, w, seed=0):
    """Random, constant, a two-level checkerboard and a 0..255 ramp: (4, h, w, 3) uint8."""
    rnd = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    const = np.broadcast_to(np.array([37, 0, 255], np.uint8), (h, w, 3))
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.stack([np.where((yy + xx) & 1, 200, 30), np.where((yy + xx) & 1, 0, 255), np.where((yy + xx) & 1, 90, 91)], axis=-1)
    ramp = np.stack([(yy * w + xx) * 255 // (h * w - 1), 255 - xx * 255 // (w - 1), yy * 255 // (h - 1)], axis=-1)
    return np.stack([rnd, const, checker.astype(np.uint8), ramp.astype(np.uint8)])


def _drops(h, w, rng, count=None):
    """Drops as the builder draws them where the crop is tall enough, and a few that leave a small crop on every side otherwise."""
    slant = int(rng.integers(-10, 11))
    if count is None:
        count = max(h * w // 600, 3)
    if h > 20:
        x = rng.integers(min(slant, 0), w - max(slant, 0) + 1, count)
        y = rng.integers(0, h - 20 + 1, count)
    else:
        x, y = rng.integers(-12, w + 12, count), rng.integers(-22, h + 2, count)
    return rain_segments(slant, np.stack([x, y], axis=1))


def _polygons(h, w, rng):
    n = int(rng.integers(1, 3))
    return [np.stack([rng.integers(0, w + 1, 5), rng.integers(h // 2, h + 1, 5)], axis=1) for _ in range(n)]


def _records(kinds, h, w, seed=0):
    """FearHlsOp records for crops that drew `kinds` and their segment table, with seeded member values inside the draw limits."""
    rng = np.random.default_rng(seed)
    ops = np.zeros(len(kinds), dtype=HLS_DTYPE)
    rows, n_rows = [np.zeros((1, 4), dtype=np.int16)], 1
    for i, kind in enumerate(kinds):
        ops["kind"][i] = kind
        intensity = rng.uniform(0.1, 0.5)
        ops["intensity"][i], ops["hue_scale"][i] = intensity, iso_hue_scale(rng.uniform(0.01, 0.05), intensity)
        ops["key"][i] = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        seg = _drops(h, w, rng) if kind == HLS_RAIN else shadow_segments(_polygons(h, w, rng))
        ops["seg_offset"][i], ops["seg_count"][i] = n_rows, len(seg)
        rows.append(seg)
        n_rows += len(seg)
    return ops, np.concatenate(rows)


def _run(lib, tables, crops, ops, segments):
    """fear_hls_u8 on (n, H, W, 3) uint8 crops, the guard band around the output checked and the input left alone."""
    n, h, w = crops.shape[:3]
    d_in, d_ops, d_seg = _device(crops), _device(ops), _device(segments)
    count = n * h * w * 3
    out = guarded(count)
    rc = lib.fear_hls_u8(P(d_in.data_ptr()), n, h, w, P(d_ops.data_ptr()), P(d_seg.data_ptr()), P(tables[2].data_ptr()),
                         P(tables[3].data_ptr()), inner(out), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), crops), "input written"
    return inside(out, count).reshape(n, h, w, 3)


def _check(lib, tables, crops, ops, segments):
    out = _run(lib, tables, crops, ops, segments)
    for i in range(len(crops)):
        ref = hls_u8_host(crops[i], ops[i], segments, tables[0], tables[1])
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, (f"crop {i} kind {ops['kind'][i]}: {len(bad)} of {ref.size} values differ, first at {bad[0].tolist()}: "
                               f"{out[i][tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    return out


# ---------------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [HLS_ISO, HLS_RAIN, HLS_SHADOW])
def test_members(lib, tables, kind, shape):
    crops = _contents(*shape, seed=kind)
    ops, seg = _records([kind] * 4, *shape, seed=shape[1] + kind)
    out = _check(lib, tables, crops, ops, seg)
    if shape[0] >= 8:
        assert not np.array_equal(out[0], crops[0])                               # the member did something to the random crop


@pytest.mark.parametrize("shape", SHAPES)
def test_a_record_per_crop(lib, tables, shape):
    kinds = [HLS_RAIN, HLS_ISO, HLS_COPY, HLS_SHADOW, HLS_ISO]
    c = _contents(*shape, seed=shape[0] + 1)
    crops = np.concatenate([c, c[:1][:, ::-1]])
    ops, seg = _records(kinds, *shape, seed=shape[1] + 1)
    out = _check(lib, tables, crops, ops, seg)
    assert np.array_equal(out[2], crops[2])
    for i in (0, 1, 3, 4):                                                        # n = 1, every kind, a record other than the first
        one = _run(lib, tables, crops[i:i + 1], ops[i:i + 1], seg)
        assert np.array_equal(one[0], out[i])


def test_statistics_are_per_crop(lib, tables):
    """Three crops with one ISONoise record: each gets its own lambda; a crop of one colour gets lambda 0 and keeps its lightness."""
    a = _contents(34, 70, seed=11)[0]
    crops = np.stack([a, a // 4, a, _contents(34, 70)[1]])
    ops, seg = _records([HLS_ISO] * 4, 34, 70, seed=3)
    ops[:] = ops[0]
    assert iso_lambda_q(crops[0], ops["intensity"][0]) != iso_lambda_q(crops[1], ops["intensity"][0])
    out = _check(lib, tables, crops, ops, seg)
    assert np.array_equal(out[0], out[2]) and iso_lambda_q(crops[3], 0.5) == 0.0


def test_all_colours_under_a_shadow(lib, tables):
    """Every colour, 256 crops of 256 x 256: under one polygon that covers the whole crop, and under one that covers nothing."""
    b, g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    crops = np.ascontiguousarray(np.stack([r, g, b], axis=-1))                    # crop = blue, row = green, column = red
    seg = np.concatenate([np.zeros((1, 4), np.int16), shadow_segments([np.array([[0, 0], [256, 0], [256, 256], [0, 256]])]),
                          shadow_segments([np.array([[256, 300], [300, 300], [300, 256], [280, 270], [270, 290]])])])
    ops = np.zeros(256, dtype=HLS_DTYPE)
    ops["kind"], ops["seg_offset"], ops["seg_count"] = HLS_SHADOW, 1, 5
    out = _run(lib, tables, crops, ops, seg)
    assert np.array_equal(out[7], hls_u8_host(crops[7], ops[7], seg, tables[0], tables[1]))
    for i in range(0, 256, 16):                                                   # the whole crop is in shadow: the round trip alone
        hls = rgb_to_hls_u8(crops[i:i + 16])
        hls[..., 1] >>= 1
        bad = np.argwhere(out[i:i + 16] != hls_to_rgb_u8(hls))
        assert bad.size == 0, f"crops {i}..: {len(bad)} values differ, first at {bad[0].tolist()}"
    assert out.mean() < 0.6 * crops.mean()
    ops["seg_offset"], ops["seg_count"] = 6, 6
    assert np.array_equal(_run(lib, tables, crops, ops, seg), crops)


def test_rain_drop_counts(lib, tables):
    """No drop (the blur and the darkening alone) and the H W // 600 drops of the builder, at both of its crop sizes."""
    for h, w in ((128, 128), (256, 256)):
        crops = _contents(h, w, seed=h)[:2]
        rng = np.random.default_rng(w)
        full = _drops(h, w, rng, h * w // 600)
        assert len(full) == h * w // 600
        seg = np.concatenate([np.zeros((1, 4), np.int16), full])
        ops = np.zeros(2, dtype=HLS_DTYPE)
        ops["kind"], ops["seg_offset"], ops["seg_count"] = HLS_RAIN, 1, [0, len(full)]
        out = _check(lib, tables, crops, ops, seg)
        assert not np.array_equal(out[0], crops[0])


def test_iso_noise_extremes(lib, tables):
    """A crop of one colour (lambda 0: the hue noise alone), and crops of black and white halves at the largest intensity and beyond
    it, where lambda meets its cap of 64."""
    h, w = 34, 70
    half = np.zeros((h, w, 3), np.uint8)
    half[:, w // 2:] = 255
    tinted = half.copy()
    tinted[..., 1] //= 2
    crops = np.stack([_contents(h, w)[1], half, tinted, tinted])
    ops, seg = _records([HLS_ISO] * 4, h, w, seed=5)
    ops["intensity"] = [0.5, 0.5, 0.5, 0.75]
    assert iso_lambda_q(crops[0], 0.5) == 0.0 and iso_lambda_q(crops[1], 0.5) == 63.75 and iso_lambda_q(crops[3], 0.75) == 64.0
    _check(lib, tables, crops, ops, seg)


def test_copies(lib, tables):
    """Kind 0, unknown kinds, a count of 0 for the shadow and negative offsets or counts all copy the crop."""
    for shape in SHAPES[:3]:
        crops = np.concatenate([_contents(*shape, seed=7), _contents(*shape, seed=8)])
        ops, seg = _records([HLS_SHADOW] * 8, *shape, seed=9)
        ops["kind"][:4] = [HLS_COPY, 4, -1, 1 << 20]
        ops["seg_count"][4] = 0
        ops["seg_count"][5], ops["seg_offset"][6] = -3, -1
        ops["kind"][7], ops["seg_count"][7] = HLS_RAIN, -1
        out = _check(lib, tables, crops, ops, seg)
        assert np.array_equal(out, crops)


def test_argument_checks(lib, tables):
    crops = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    ops, seg = _records([HLS_ISO, HLS_RAIN], 8, 8)
    d_ops, d_seg = _device(ops), _device(seg)
    out = torch.full((2, 8, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        return lib.fear_hls_u8(kw.get("crops", P(crops.data_ptr())), kw.get("n", 2), kw.get("h", 8), kw.get("w", 8),
                               kw.get("ops", P(d_ops.data_ptr())), kw.get("seg", P(d_seg.data_ptr())), kw.get("q", P(tables[2].data_ptr())),
                               kw.get("exp", P(tables[3].data_ptr())), kw.get("out", P(out.data_ptr())), st)

    for bad in (dict(h=7), dict(w=7), dict(w=2), dict(h=2), dict(h=0), dict(n=-1), dict(n=65536), dict(h=258), dict(w=258),
                dict(out=P(crops.data_ptr()))):
        assert call(**bad) == -2, bad
    for name in ("crops", "ops", "seg", "q", "exp", "out"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, crops=None, ops=None, seg=None, q=None, exp=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                          # refused calls and n = 0 write nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------- builder
@pytest.mark.parametrize("noise_members,two_calls", [(("multiplicative", "gauss"), True), ("all", True), (("multiplicative", "gauss"), False)])
def test_build_equals_build_host(noise_members, two_calls):
    """B = 8 with every member forced through the params; with `two_calls` one search crop draws ISONoise and rain, which takes
    fear_hls_u8 twice per side; without, one set of records serves both members."""
    frames = _frames(2)
    pairs = _pairs(8, seed=3)
    config = dict(photometric=True, iso_noise=True, weather_members="all", noise_members=noise_members)
    builder = TrainPairBuilder(config, device=0)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(4))
    ph = params.photo
    ph.blur[:], ph.noise[:], ph.downscale[:], params.weather[:] = BLUR_NONE, NOISE_NONE, 0, WEATHER_NONE
    ph.noise[0, 1], ph.noise[1, 0], ph.noise[2, 1], ph.noise[3, 0] = NOISE_ISO, NOISE_ISO, NOISE_GAUSS, NOISE_MULTIPLICATIVE
    params.weather[2, 1], params.weather[3, 0] = WEATHER_RAIN, WEATHER_SHADOW
    params.weather[4, 1], params.weather[5, 0] = WEATHER_SHADOW, WEATHER_RAIN
    ph.blur[4, 1], ph.ksize[4, 1], ph.downscale[4, 1], ph.downscale[0, 1], ph.downscale[6, 0] = BLUR_BOX, 5, 1, 1, 1
    if two_calls:
        params.weather[0, 1], params.weather[1, 0] = WEATHER_RAIN, WEATHER_SHADOW
    if noise_members == "all":
        ph.noise[5, 0], ph.noise[7, 1] = NOISE_JPEG, NOISE_JPEG               # ImageCompression in front of the rain, and on its own
    host = builder.build_host(frames, pairs, params)
    plain = TrainPairBuilder(dict(photometric=True, noise_members=noise_members), device=0)
    saved = ph.noise.copy(), params.weather.copy()
    ph.noise[ph.noise == NOISE_ISO], params.weather[:] = NOISE_NONE, WEATHER_NONE
    untouched = plain.build_host(frames, pairs, params)
    ph.noise[:], params.weather[:] = saved
    for k, name in ((0, "search"), (1, "template"), (2, "search"), (3, "template"), (4, "search"), (5, "template")):
        assert not np.array_equal(getattr(host, name)[k], getattr(untouched, name)[k]), (k, name)      # every member does something
    assert np.array_equal(host.template[6], untouched.template[6]) and np.array_equal(host.search[7], untouched.search[7])
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


def test_builds_without_the_keys_are_the_launches_of_before(lib, tables):
    """With iso_noise and weather_members at their defaults `build` is fear_frame_border_u8 + fear_train_pairs, and with photometric=True
    fear_frame_border_u8 + fear_train_pairs_u8 + one fear_photometric_u8 per side, on the same tables, bit for bit."""
    frames = _frames(5)
    pairs = _pairs(4, seed=6)
    B, F = 4, len(frames)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    ftab = np.zeros(F, dtype=FRAME_DTYPE)
    for i, f in enumerate(d_frames):
        ftab[i] = (f.data_ptr(), f.shape[0], f.shape[1])
    st = P(torch.cuda.current_stream().cuda_stream)
    for photometric in (False, True):
        builder = TrainPairBuilder(dict(photometric=photometric, iso_noise=False, weather_members=()), device=0, seed=9)
        params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(9))
        assert params.weather is None and params.iso_key is None
        if photometric:
            params.photo.noise[:, 0], params.photo.blur[:, 1] = [0, 1, 2, 0], [1, 2, 3, 4]
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
                                               P(d_taps.data_ptr()) if d_taps is not None else None, P(tables[2].data_ptr()),
                                               P(outs[which].data_ptr()), st) == 0
        torch.cuda.synchronize()
        for name, ref in zip(("template", "search", "gt_reg", "gt_cls", "gt_weight"), outs):
            assert torch.equal(getattr(got, name), ref), (photometric, name)
