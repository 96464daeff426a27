"""Host side of the training-pair builder (feartracker_amd/train_data/): geometry and targets against the reference's own Python
(tests/golden/train_pairs_geometry.npz, tools/make_train_pairs_golden.py), the vectorised warpAffine against an independent
scalar restatement of OpenCV's remap, and the colour draws.  No GPU."""
import os

import numpy as np
import pytest

from feartracker_amd import geometry
from feartracker_amd.train_data import (COLOUR_BRIGHTNESS_CONTRAST, COLOUR_GAMMA, COLOUR_NONE, COLOUR_RGB_SHIFT, TONE_GRAY,
                                        TONE_NONE, TONE_SEPIA, TrainPairBuilder, TrainPairParams, apply_tone, colour_luts,
                                        crop_u8, encode_targets, remap_affine_u8, warp_affine_u8, warp_matrix)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_pairs_geometry.npz")


def _params(context, jitter, shapes=()):
    B = len(context)
    z = np.zeros(B)
    return TrainPairParams(np.asarray(context, np.float64), np.asarray(jitter, np.float64), np.zeros(B, np.int32),
                           np.zeros(B, np.int32), z + 1.0, z, z + 1.0, np.zeros((B, 3)), tuple(shapes))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------------------ geometry + targets
def test_golden_fixture_covers_the_cases(golden):
    assert len(golden["pairs"]) >= 250
    assert (golden["pairs"][:, 10] == 0).any() and (golden["pairs"][:, 10] == 1).any()
    assert (np.abs(golden["jitter"][:, :2]) == 0.35).any() and (np.abs(golden["jitter"][:, 2:]) == 48).any()
    assert (golden["s_ctx"][:, 0] < 0).any() and (golden["s_ctx"][:, 1] < 0).any()         # contexts leaving the frame
    assert (golden["pairs"][:, 8] <= 3).any()                                               # 1-3 px search boxes


def test_search_context_draw_is_the_references(golden):
    assert np.array_equal(golden["r_context"] * 3 + (2 * 2 - 3 / 2), golden["context"])


def test_tables_equal_the_reference_geometry(golden):
    b = TrainPairBuilder()
    tab = b.tables(golden["pairs"], _params(golden["context"], golden["jitter"]))
    assert np.array_equal(tab["t_ctx"], golden["t_ctx"])
    assert np.array_equal(tab["s_ctx"], golden["s_ctx"])
    assert np.array_equal(tab["box512"], golden["box512"])
    assert np.array_equal(tab["crop"], golden["crop"])
    assert np.array_equal(tab["M"], golden["M"])
    assert np.array_equal(tab["moved"], golden["moved"])
    assert np.array_equal(tab["search_bbox"], golden["search_bbox"])
    assert np.array_equal(tab["geom"]["box"], golden["search_bbox"])


def test_targets_equal_the_reference(golden):
    reg, cls, wgt = encode_targets(golden["search_bbox"], golden["pairs"][:, 10])
    assert np.array_equal(reg, golden["gt_reg"].astype(np.float32))
    assert np.array_equal(cls, golden["gt_cls"].astype(np.float32))
    assert np.array_equal(wgt, golden["gt_weight"].astype(np.float32))
    assert reg.dtype == cls.dtype == wgt.dtype == np.float32


def test_inverse_warp_is_the_cv2_order(golden):
    """The device reads inv = (M0, M2, M4, M5) of the inverted matrix; for the reference's form the cross terms are zeros."""
    b = TrainPairBuilder()
    tab = b.tables(golden["pairs"], _params(golden["context"], golden["jitter"]))
    Mi = tab["Minv"]
    assert np.all(Mi[:, 0, 1] == 0) and np.all(Mi[:, 1, 0] == 0)
    M = golden["M"]
    D = 1.0 / (M[:, 0, 0] * M[:, 1, 1])
    assert np.array_equal(Mi[:, 0, 0], M[:, 1, 1] * D)
    assert np.array_equal(Mi[:, 0, 2], -Mi[:, 0, 0] * M[:, 0, 2])
    assert np.array_equal(tab["geom"]["inv"], np.stack([Mi[:, 0, 0], Mi[:, 0, 2], Mi[:, 1, 1], Mi[:, 1, 2]], axis=1))


# ----------------------------------------------------------------------------------------------------------------------- warp
def _scalar_bilinear_tab():
    """initInterTab2D(INTER_LINEAR, fixpt) of OpenCV 4.x imgwarp.cpp, literally: float 1-D table, products saturate_cast to short,
    the sum correction over the centre 2 x 2 (for ksize 2 its scan reaches into the following, still zero, entries)."""
    INTER_TAB_SIZE, SCALE = 32, 32768
    tab1 = []
    for i in range(INTER_TAB_SIZE):
        x = np.float32(i) * np.float32(1.0 / INTER_TAB_SIZE)
        tab1 += [np.float32(1.0) - x, x]
    itab = np.zeros(INTER_TAB_SIZE * INTER_TAB_SIZE * 4 + 8, dtype=np.int64)        # zero-initialised static table (+ slack)
    ksize = 2
    for i in range(INTER_TAB_SIZE):
        for j in range(INTER_TAB_SIZE):
            base = (i * INTER_TAB_SIZE + j) * 4
            isum = 0
            for k1 in range(ksize):
                vy = tab1[i * ksize + k1]
                for k2 in range(ksize):
                    v = np.float32(vy * tab1[j * ksize + k2])
                    iv = int(min(max(np.rint(np.float32(v * np.float32(SCALE))), -32768), 32767))
                    itab[base + k1 * ksize + k2] = iv
                    isum += iv
            if isum != SCALE:
                diff = isum - SCALE
                ksize2 = ksize // 2
                Mk1 = Mk2 = mk1 = mk2 = ksize2
                for k1 in range(ksize2, ksize2 + 2):
                    for k2 in range(ksize2, ksize2 + 2):
                        if itab[base + k1 * ksize + k2] < itab[base + mk1 * ksize + mk2]:
                            mk1, mk2 = k1, k2
                        elif itab[base + k1 * ksize + k2] > itab[base + Mk1 * ksize + Mk2]:
                            Mk1, Mk2 = k1, k2
                if diff < 0:
                    itab[base + Mk1 * ksize + Mk2] -= diff
                else:
                    itab[base + mk1 * ksize + mk2] -= diff
    return itab[: INTER_TAB_SIZE * INTER_TAB_SIZE * 4].reshape(-1, 4)


def _scalar_warp(src, M, dsize):
    """cv2.warpAffine INTER_LINEAR / BORDER_CONSTANT 0 on uint8, pixel by pixel: WarpAffineInvoker + remapBilinear."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(-1)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    tab = _scalar_bilinear_tab()
    h, w = src.shape[:2]
    out = np.zeros((dsize[1], dsize[0], src.shape[2]), np.uint8)
    for y in range(dsize[1]):
        X0 = int(np.rint((m[1] * y + m[2]) * 1024)) + 16
        Y0 = int(np.rint((m[4] * y + m[5]) * 1024)) + 16
        for x in range(dsize[0]):
            X = (X0 + int(np.rint(m[0] * x * 1024))) >> 5
            Y = (Y0 + int(np.rint(m[3] * x * 1024))) >> 5
            sx, sy = X >> 5, Y >> 5
            wt = tab[(Y & 31) * 32 + (X & 31)]
            if sx >= w or sx + 1 < 0 or sy >= h or sy + 1 < 0:
                continue                                               # all four taps outside: the border value
            for c in range(src.shape[2]):
                acc = 0
                for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    yy, xx = sy + oy, sx + ox
                    v = int(src[yy, xx, c]) if 0 <= yy < h and 0 <= xx < w else 0
                    acc += v * int(wt[k])
                out[y, x, c] = (acc + (1 << 14)) >> 15
    return out


def test_bilinear_table_matches_the_scalar_construction():
    from feartracker_amd.train_data import _TAB
    assert np.array_equal(_TAB, _scalar_bilinear_tab())
    assert np.all(_TAB.sum(axis=1) == 32768)


@pytest.mark.parametrize("seed", range(6))
def test_warp_equals_scalar_restatement(seed):
    rng = np.random.default_rng(seed)
    h, w = rng.integers(24, 48, 2)
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = int(rng.integers(12, 24))
    # the reference's form: a jittered crop box, partly off the source on some seeds
    x, y = rng.uniform(-10, w * 0.6), rng.uniform(-10, h * 0.6)
    cw, ch = rng.uniform(4, w * 1.3), rng.uniform(4, h * 1.3)
    M = warp_matrix(np.array([[x, y, cw, ch]]), out_size=out)[0]
    assert np.array_equal(warp_affine_u8(src, M, (out, out)), _scalar_warp(src, M, (out, out)))


def test_warp_identity_copies():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    assert np.array_equal(warp_affine_u8(src, np.array([[1.0, 0, 0], [0, 1.0, 0]]), (30, 20)), src)


def test_warp_integer_translation_shifts_with_zero_border():
    rng = np.random.default_rng(2)
    src = rng.integers(1, 256, (20, 30, 3), dtype=np.uint8)
    out = warp_affine_u8(src, np.array([[1.0, 0, 3], [0, 1.0, -2]]), (30, 20))
    ref = np.zeros_like(src)
    ref[0:18, 3:30] = src[2:20, 0:27]
    assert np.array_equal(out, ref)


def test_remap_takes_the_inverted_matrix():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    assert np.array_equal(remap_affine_u8(src, np.array([[1.0, 0, 2], [0, 1.0, 0]]), (16, 16))[:, :14], src[:, 2:])


# ----------------------------------------------------------------------------------------------------------------------- crops
@pytest.mark.parametrize("seed", range(4))
def test_crop_equals_get_extended_crop(seed):
    """The per-tap crop the device computes equals geometry.get_extended_crop (pinned against cv_ref.c elsewhere), including the
    identity and exact-2x cases and contexts off the frame."""
    rng = np.random.default_rng(seed)
    H, W = rng.integers(30, 90, 2)
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pad = geometry.border_color_u8(np.mean(f, (0, 1)))
    for box, off, S in (([rng.integers(0, W - 8), rng.integers(0, H - 8), 7, 5], 2.5, 32), ([0, 0, 16, 16], 0.0, 16),
                        ([W - 9, H - 9, 8, 8], 0.5, 8), ([3, 4, 20, 20], 0.0, 10)):
        ref, _, ctx = geometry.get_extended_crop(f, np.array(box, float), S, off)
        assert np.array_equal(crop_u8(f, pad, ctx, S), ref)


def test_crop_of_a_missing_frame_is_zero():
    assert not crop_u8(None, (0, 0, 0), (5, 5, 40, 30), 16).any()


# ----------------------------------------------------------------------------------------------------------------------- colour
def _pairs(B):
    p = np.zeros((B, 11))
    p[:, 1:5] = [10, 10, 20, 20]
    p[:, 6:10] = [10, 10, 20, 20]
    p[:, 5] = 0
    p[:, 10] = 1
    return p


def test_draw_is_deterministic_under_a_seed():
    b = TrainPairBuilder()
    a1 = b.draw(_pairs(64), [(48, 64, 3)], np.random.default_rng(5))
    a2 = b.draw(_pairs(64), [(48, 64, 3)], np.random.default_rng(5))
    a3 = b.draw(_pairs(64), [(48, 64, 3)], np.random.default_rng(6))
    for k in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
        assert np.array_equal(getattr(a1, k), getattr(a2, k)), k
    assert not np.array_equal(a1.context, a3.context)
    assert a1.frame_shapes == ((48, 64),)


def test_draw_ranges_and_branch_frequencies():
    B = 40000
    p = TrainPairBuilder().draw(_pairs(B), [(48, 64, 3)], np.random.default_rng(0))
    assert p.context.min() >= 2.5 and p.context.max() < 5.5
    assert np.abs(p.jitter[:, :2]).max() <= 0.35 and np.abs(p.jitter[:, 2:]).max() <= 48
    assert p.alpha.min() >= 0.8 and p.alpha.max() <= 1.2 and np.abs(p.beta).max() <= 0.2
    assert p.gamma.min() >= 0.8 and p.gamma.max() <= 1.2 and np.abs(p.shift).max() <= 20
    tone = np.bincount(p.tone, minlength=3) / B
    assert abs(tone[TONE_NONE] - 0.95) < 0.006 and abs(tone[TONE_GRAY] - 0.025) < 0.004 and abs(tone[TONE_SEPIA] - 0.025) < 0.004
    col = np.bincount(p.colour, minlength=4) / B
    assert abs(col[COLOUR_NONE] - 0.5) < 0.01
    for k in (COLOUR_BRIGHTNESS_CONTRAST, COLOUR_GAMMA, COLOUR_RGB_SHIFT):
        assert abs(col[k] - 1 / 6) < 0.01


def test_luts_per_branch():
    B = 4
    p = _params(np.full(B, 3.0), np.zeros((B, 4)))
    p.colour[:] = [COLOUR_NONE, COLOUR_BRIGHTNESS_CONTRAST, COLOUR_GAMMA, COLOUR_RGB_SHIFT]
    p.alpha[:] = 1.1
    p.beta[:] = -0.1
    p.gamma[:] = 0.9
    p.shift[:] = [7.5, -20.0, 0.25]
    lut = colour_luts(p)
    v = np.arange(256)
    assert np.array_equal(lut[0], np.broadcast_to(v, (3, 256)))                           # no-op branch: identity
    bc = np.clip(v.astype(np.float32) * np.float32(1.1) + np.float32(-0.1 * 255), 0, 255).astype(np.uint8)
    assert np.array_equal(lut[1], np.broadcast_to(bc, (3, 256)))
    gm = ((v / 255.0) ** 0.9 * 255.0).astype(np.uint8)
    assert np.array_equal(lut[2], np.broadcast_to(gm, (3, 256)))
    assert lut[3, 0, 0] == 7 and lut[3, 0, 250] == 255 and lut[3, 1, 19] == 0 and lut[3, 1, 100] == 80 and lut[3, 2, 10] == 10


def test_tone_stage():
    white = np.full((1, 1, 3), 255, np.uint8)
    assert np.array_equal(apply_tone(white, TONE_GRAY), white)
    assert np.array_equal(apply_tone(np.zeros((1, 1, 3), np.uint8), TONE_GRAY), np.zeros((1, 1, 3), np.uint8))
    px = np.array([[[200, 100, 50]]], np.uint8)
    g = (4899 * 200 + 9617 * 100 + 1868 * 50 + 8192) >> 14
    assert np.array_equal(apply_tone(px, TONE_GRAY), np.full((1, 1, 3), g, np.uint8))
    s = apply_tone(px, TONE_SEPIA)[0, 0]
    assert list(s) == [min(255, round(0.393 * 200 + 0.769 * 100 + 0.189 * 50)), round(0.349 * 200 + 0.686 * 100 + 0.168 * 50),
                       round(0.272 * 200 + 0.534 * 100 + 0.131 * 50)]
    assert np.array_equal(apply_tone(px, TONE_NONE), px)


def _u8_of(normalised):
    """Undo the normalisation of a (3, H, W) crop: the uint8 values after the colour stage."""
    from feartracker_amd.geometry import _INV_STD, _MEAN
    return np.rint(normalised.transpose(1, 2, 0) / _INV_STD + _MEAN).astype(np.int64)


def test_a_pairs_two_crops_share_the_colour_draw():
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    b = TrainPairBuilder()
    pairs = _pairs(2)
    p = b.draw(pairs, [f.shape for f in frames], np.random.default_rng(0))
    p.tone[:] = [TONE_GRAY, TONE_NONE]
    p.colour[:] = [COLOUR_NONE, COLOUR_RGB_SHIFT]
    p.shift[1] = [-20.0, 0.0, 20.0]
    out = b.build_host(frames, pairs, p)
    for crop in (out.template[0], out.search[0]):                 # gray on both crops
        u8 = _u8_of(crop)
        assert np.array_equal(u8[..., 0], u8[..., 1]) and np.array_equal(u8[..., 1], u8[..., 2])
    ref = b.build_host(frames, pairs, _params(p.context, p.jitter, p.frame_shapes))
    for got, base in ((out.template[1], ref.template[1]), (out.search[1], ref.search[1])):    # the same shift on both crops
        g, r = _u8_of(got), _u8_of(base)
        assert np.array_equal(g[..., 0], np.clip(r[..., 0] - 20, 0, 255)) and np.array_equal(g[..., 1], r[..., 1])
        assert np.array_equal(g[..., 2], np.clip(r[..., 2] + 20, 0, 255))


def test_build_host_shapes_and_presence():
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    pairs = _pairs(3)
    pairs[1, 10] = 0
    out = TrainPairBuilder(seed=1).build_host(frames, pairs)
    assert out.template.shape == (3, 3, 128, 128) and out.search.shape == (3, 3, 256, 256)
    assert out.gt_reg.shape == (3, 4, 16, 16) and out.gt_cls.shape == (3, 1, 16, 16) and out.gt_weight.shape == (3, 16, 16)
    assert out.search_bbox.shape == (3, 4) and out.search_bbox.dtype == np.int32
    assert not out.gt_reg[1].any() and not out.gt_cls[1].any() and not out.gt_weight[1].any()
    assert out.gt_weight[0].sum() > 0 and out.gt_cls[0].sum() > 0
