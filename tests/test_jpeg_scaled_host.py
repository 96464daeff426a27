"""Reduced-size JPEG decoding on the host ("Reduced-size decoding"): `jpeg_decode_host(scale=)` against Pillow's
`draft` decode — the recorded fixture tests/golden/jpeg_scaled.npz (tools/make_jpeg_scaled_golden.py) and, where Pillow is installed, a
live decode — byte for byte; the transform size per component; bands of MCU rows through `jpeg_pixels_host(scale=)`; the plans of
`JpegStore` at a scale, and that they are what they were at scale 1; the refused scales; `scale_pairs`."""
import io

import numpy as np
import pytest

import jpegdec
import jpegscaled
from jpegscaled import SCALES
from feartracker_amd import (jpeg_decode_host, jpeg_pixels_host, jpeg_scaled_shape, jpeg_scaled_transforms, plan_decode, plan_decode_rows)
from feartracker_amd import jpeg_frames as jf
from feartracker_amd.jpeg_store import COLUMNS, KIND_PIXELS, KIND_SCAN
from feartracker_amd.train_data import scale_pairs


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[:3].tolist()}"


def test_the_fixture_pins_every_pair_draft_can_take():
    """Pillow's draft cannot force a scale above a file's smaller side: of the 129 file x scale pairs of the old fixture exactly 16 are
    not pinned — the four 1 x 1 files at every scale and the four 7 x 5 files at 1/8."""
    old = [name for name, _, _ in jpegdec.supported()]
    assert len(old) == 43
    missing = {f"{name}@{s}" for name in old for s in SCALES} - set(jpegscaled.pinned())
    want = {f"{name}@{s}" for name in old for s in SCALES if name.startswith("1x1_") or (name.startswith("7x5_") and s == 8)}
    assert len(want) == 16 and missing == want
    for name, _ in jpegscaled.new_files():
        assert all(f"{name}@{s}" in jpegscaled.pinned() for s in SCALES), name


def test_host_model_equals_the_fixture():
    seen = 0
    for name, data in jpegscaled.files(progressive=True):
        hd = jf._parse(data) if "progressive" not in name else None
        for s in SCALES:
            want, is_pinned = jpegscaled.expected(name, data, s)
            if hd is not None:
                assert want.shape == jpeg_scaled_shape(hd.height, hd.width, s), (name, s)
            if is_pinned:
                _same(jpeg_decode_host(data, progressive="progressive" in name, scale=s), want, f"{name} at 1/{s}")
                seen += 1
    assert seen == 128
    name, data, px = jpegdec.case("17x23_420")
    _same(jpeg_decode_host(data, scale=1), px, name)                                  # scale 1 is the full decode


def test_host_model_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for name, data in jpegscaled.files(progressive=True):
        for s in SCALES:
            im = Image.open(io.BytesIO(data))
            w, h = im.size
            if min(w, h) < s:
                continue
            im.draft(im.mode, (max(1, w // s), max(1, h // s)))
            im.load()
            assert im.size == (-(-w // s), -(-h // s)), (name, s)
            _same(jpeg_decode_host(data, progressive="progressive" in name, scale=s), np.asarray(im.convert("RGB")), f"{name} at 1/{s}")
            seen += 1
    assert seen == 128


def test_the_cases_that_the_new_files_are_for():
    """Scaled 4:2:2 chroma planes exactly 3 and exactly 2 wide (fancy upsampling | replication), and one above 2 at 1/8, where libjpeg
    upsamples without the filter: the fancy rule there would change the pixels."""
    by_name = dict(jpegscaled.new_files())
    widths = {(name, s): -(-jf._parse(data).width * (8 // s) // 16) for name, data in by_name.items() if "progressive" not in name for s in SCALES}
    assert widths["12x9_422_random_q90_cw3_cw2", 2] == 3 and widths["12x9_422_random_q90_cw3_cw2", 4] == 2
    assert widths["24x10_422_smooth_q75_cw3", 4] == 3
    assert widths["48x16_422_random_q90_wide", 8] == 3 and widths["64x40_422_smooth_q95_wide", 8] == 4
    data = by_name["48x16_422_random_q90_wide"]
    hd, coef = jf.jpeg_coefficients_host(data)
    assert hd.width > 32 and (hd.h[0], hd.v[0]) == (2, 1)
    plane = np.arange(3 * 2, dtype=np.int64).reshape(2, 3) * 40
    assert not np.array_equal(jf._upsample_h2v1(plane), np.repeat(plane, 2, axis=1))


def test_transform_size_per_component():
    table = {"gray": ([1], [1]), "444": ([1, 1, 1], [1, 1, 1]), "422": ([2, 1, 1], [1, 1, 1]), "420": ([2, 1, 1], [2, 1, 1])}
    for s in SCALES:
        m = 8 // s
        assert jpeg_scaled_transforms(*table["gray"], s) == [m]
        assert jpeg_scaled_transforms(*table["444"], s) == [m, m, m]
        assert jpeg_scaled_transforms(*table["422"], s) == [m, m, m]
        assert jpeg_scaled_transforms(*table["420"], s) == [m, 2 * m, 2 * m]
    assert jpeg_scaled_transforms(*table["420"], 1) == [8, 8, 8]
    assert jpeg_scaled_shape(7, 5, 2) == (4, 3, 3) and jpeg_scaled_shape(7, 5, 8) == (1, 1, 3) and jpeg_scaled_shape(720, 1280, 4) == (180, 320, 3)
    assert jpeg_scaled_shape(33, 31, 1) == (33, 31, 3)


def test_reduced_transforms_on_flat_and_full_blocks():
    """A block with its dc alone is flat at DESCALE(dc, 3) + rounding of the two passes at every size, and ss == 8 is the islow
    transform.  (The bytes of real files are pinned by the fixture.)"""
    x = np.zeros((5, 8, 8), dtype=np.int64)
    x[:, 0, 0] = [-1024, -9, 0, 8, 1016]
    for ss in (4, 2, 1):
        got = jf.jpeg_idct_scaled(x, ss)
        assert got.shape == (5, ss, ss) and np.array_equal(got, np.broadcast_to(((x[:, 0, 0] + 4) >> 3)[:, None, None], got.shape)), ss
    rng = np.random.default_rng(5)
    x = rng.integers(-300, 300, (50, 8, 8))
    assert np.array_equal(jf.jpeg_idct_scaled(x, 8), jf.jpeg_idct_islow(x))
    for ss, unread in ((4, (4,)), (2, (2, 4, 6))):                                    # rows and columns the transform never reads
        y = x.copy()
        for k in unread:
            y[:, k, :] = 7777
            y[:, :, k] = -7777
        assert np.array_equal(jf.jpeg_idct_scaled(x, ss), jf.jpeg_idct_scaled(y, ss)), ss


def _band(coef, hd, a, b):
    return [c[a * hd.v[i]:b * hd.v[i]] for i, c in enumerate(coef)]


def test_every_band_of_mcu_rows_is_a_slice_of_the_scaled_decode():
    """What `decode_rows(scale=)` relies on: the MCU rows a .. b) as an image of their own, of the band's full-size height, give the rows
    a v m .. of the scaled frame — at a scale no supported mode reads a chroma row of a neighbouring MCU row."""
    bands = 0
    for name, data in jpegscaled.files():
        hd, coef = jf.jpeg_coefficients_host(data)
        mcu_h = 8 * hd.v[0]
        for s in SCALES:
            full, _ = jpegscaled.expected(name, data, s)
            step = mcu_h * (8 // s) // 8
            for a in range(hd.mcus_y):
                for b in range(a + 1, hd.mcus_y + 1):
                    high = min(b * mcu_h, hd.height) - a * mcu_h
                    got = jpeg_pixels_host(hd, _band(coef, hd, a, b), height=high, scale=s)
                    _same(got, full[a * step:min(b * step, full.shape[0])], f"{name} at 1/{s}: MCU rows {a}..{b}")
                    bands += 1
    assert bands > 1000


def _columns():
    """A mirror of five entries: 4:2:0 80 x 72, 4:2:2 33 x 31, gray 7 x 5, an entry kept as pixels, 4:4:4 1280 x 720."""
    col = np.zeros(5, dtype=COLUMNS)
    rows, at = [], 0
    for k, (w, h, hs, vs, nc) in enumerate(((80, 72, 2, 2, 3), (33, 31, 2, 1, 3), (7, 5, 1, 1, 1), (0, 0, 0, 0, 0), (1280, 720, 1, 1, 3))):
        if k == 3:
            col[k]["H"], col[k]["W"], col[k]["kind"] = 20, 30, KIND_PIXELS
            continue
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        slots = hs * vs + 2 if nc == 3 else 1
        col[k] = (1, 4 * my, mx * my * slots, h, w, KIND_SCAN, mx, my, 8 * vs, slots, vs == 2, at)
        rows.append(np.arange(my + 1, dtype=np.uint32) * 4)
        at += my + 1
    return col, np.concatenate(rows)


def _plans_equal(one, two):
    assert len(one) == len(two)
    for p, q in zip(one, two):
        assert p.keys() == q.keys()
        for key in p:
            a, b = np.asarray(p[key]), np.asarray(q[key])
            assert a.dtype == b.dtype and np.array_equal(a, b), key


def test_plans_at_scale_1_are_what_they_were():
    """`scale=1` changes nothing: the same plans as without the argument, and the fields a scale touches still hold the full-size
    values the plans have always held (H W pixels per frame, bands in pixel rows with their halo)."""
    col, row_sub = _columns()
    ids = np.array([4, 0, 1, 3, 2, 0, 1])
    for limit in (1 << 40, 128 * 60, 0):
        _plans_equal(plan_decode(col, ids, limit), plan_decode(col, ids, limit, scale=1))
    plan, = plan_decode(col, ids, 1 << 40, scale=1)
    px = np.array([720 * 1280, 72 * 80, 31 * 33, 5 * 7, 72 * 80, 31 * 33])
    assert np.array_equal(plan["pixel_prefix"], np.concatenate([[0], np.cumsum(-(-px // 256))]))
    sizes = np.array([720 * 1280, 72 * 80, 31 * 33, 20 * 30, 5 * 7, 72 * 80, 31 * 33]) * 3
    assert plan["out_bytes"] == int((-(-sizes // 16) * 16).sum())
    rows = np.array([[100, 300], [17, 40], [0, 31], [0, 20], [2, 3], [0, 0], [30, 31]])
    for limit in (1 << 40, 128 * 60, 0):
        _plans_equal(plan_decode_rows(col, row_sub, ids, rows, limit), plan_decode_rows(col, row_sub, ids, rows, limit, scale=1))
    plan, = plan_decode_rows(col, row_sub, ids, rows, 1 << 40, scale=1)
    assert plan["scan"].tolist() == [0, 1, 2, 4, 6]
    assert plan["mcu_row0"].tolist() == [12, 0, 0, 0, 3] and plan["mcu_rows"].tolist() == [26, 4, 4, 1, 1]      # the 4:2:0 band has its halo
    assert plan["band_height"].tolist() == [208, 64, 31, 5, 7] and plan["band_y0"].tolist() == [96, 0, 0, 0, 24]
    assert plan["band_out"].tolist() == [3 * 1280 * 96, 0, 0, 0, 3 * 33 * 24]


def test_plans_at_a_scale():
    col, row_sub = _columns()
    ids = np.array([4, 0, 1, 2])
    for s in SCALES:
        m = 8 // s
        full, = plan_decode(col, ids, 1 << 40)
        plan, = plan_decode(col, ids, 1 << 40, scale=s)
        shapes = [jpeg_scaled_shape(h, w, s) for h, w in ((720, 1280), (72, 80), (31, 33), (5, 7))]
        px = np.array([h * w for h, w, _ in shapes])
        assert np.array_equal(plan["pixel_prefix"], np.concatenate([[0], np.cumsum(-(-px // 256))]))
        assert plan["out_bytes"] == int((-(-3 * px // 16) * 16).sum()) and plan["out_offset"][1] == -(-3 * px[0] // 16) * 16
        for key in ("sub_prefix", "block_prefix", "coef_offset", "values", "plane_offset", "workspace_bytes", "most"):
            assert np.array_equal(np.asarray(plan[key]), np.asarray(full[key])), key    # the blocks are the file's
        # rows of the scaled frame; a scaled MCU row is v m of them and no band has a halo
        rows = np.array([[10 * m, 30 * m], [2 * m, 2 * m + 1], [0, 1000], [0, 1]])
        plan, = plan_decode_rows(col, row_sub, ids, rows, 1 << 40, scale=s)
        assert plan["mcu_row0"].tolist() == [10, 1, 0, 0] and plan["mcu_rows"].tolist() == [20, 1, 4, 1]      # (2 m is MCU row 1 of the 4:2:0 file)
        assert plan["band_height"].tolist() == [160, 16, 31, 5]                         # full-size: what the record holds
        assert plan["band_y0"].tolist() == [10 * m, 2 * m, 0, 0]
        assert plan["band_out"].tolist() == [3 * shapes[0][1] * 10 * m, 3 * shapes[1][1] * 2 * m, 0, 0]
        band_px = np.array([20 * m * shapes[0][1], 2 * m * shapes[1][1], shapes[2][0] * shapes[2][1], shapes[3][0] * shapes[3][1]])
        assert np.array_equal(plan["pixel_prefix"], np.concatenate([[0], np.cumsum(-(-band_px // 256))]))
        assert plan["out_bytes"] == int((-(-3 * px // 16) * 16).sum())


def test_other_scales_are_refused():
    name, data, _ = jpegdec.case("16x16_420")
    hd, coef = jf.jpeg_coefficients_host(data)
    col, row_sub = _columns()
    for bad in (0, 3, 16, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="scale"):
            jpeg_decode_host(data, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            jpeg_decode_host(b"no jpeg at all", scale=bad)                            # refused before anything is parsed
        with pytest.raises(ValueError, match="scale"):
            jpeg_pixels_host(hd, coef, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            jpeg_scaled_shape(16, 16, bad)
        with pytest.raises(ValueError, match="scale"):
            plan_decode(col, [0], 1 << 30, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            plan_decode_rows(col, row_sub, [0], [[0, 1]], 1 << 30, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            scale_pairs(np.zeros((1, 11)), bad)


def test_scale_pairs():
    pairs = np.array([[0, 100, 60, 40, 20, 1, 120, 80, 44, 22, 1], [3, 7, 5, 3, 1, 2, 0, 0, 9, 9, 0]], dtype=np.float64)
    keep = pairs.copy()
    for s in (1, 2, 4, 8):
        got = scale_pairs(pairs, s)
        assert got.dtype == np.float64 and got.shape == pairs.shape and np.array_equal(pairs, keep)
        assert np.array_equal(got[:, [0, 5, 10]], pairs[:, [0, 5, 10]])
        assert np.array_equal(got[:, 1:5] * s, pairs[:, 1:5]) and np.array_equal(got[:, 6:10] * s, pairs[:, 6:10])
    assert np.array_equal(scale_pairs(pairs.tolist(), 2), scale_pairs(pairs, 2))
    with pytest.raises(ValueError):
        scale_pairs(np.zeros((2, 10)), 2)
