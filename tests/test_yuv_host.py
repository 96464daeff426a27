"""YUV video frames without a GPU: YUVFrame construction and validation, the numpy conversion against fixed anchors and an
independent per-pixel restatement of cv2's integer BT.601 conversion, the packed layouts, and both trackers on the CPU oracle fed
NV12 / I420 clips against the same trackers on the clips' RGB conversion."""
import os

import numpy as np
import pytest
import torch

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARTracker, YUVFrame, hip_backend
from feartracker_amd.frames import FMT_I420, FMT_NV12, yuv_to_rgb_numpy
from yuvgen import full_chroma_frame, i420_packed, nv12_packed, rgb_to_yuv420

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Y, U, V) -> (R, G, B) of the integer formula (include/fear_hip.h)
ANCHORS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)),
           ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)),
           ((0, 0, 0), (0, 154, 0)), ((255, 0, 255), (255, 225, 20))]


def _pixel(y, u, v):
    """One pixel of cv2's YUV420 -> RGB (color_yuv.simd.hpp, uvToRGBuv + yRGBuvToRGBA), in Python integers."""
    def sat(x):
        return 0 if x < 0 else 255 if x > 255 else x
    uu, vv = u - 128, v - 128
    ruv = (1 << 19) + 1673527 * vv
    guv = (1 << 19) - 852492 * vv - 409993 * uu
    buv = (1 << 19) + 2116026 * uu
    yy = max(0, y - 16) * 1220542
    return sat((yy + ruv) >> 20), sat((yy + guv) >> 20), sat((yy + buv) >> 20)


def _frame(y, u, v, fmt):
    return YUVFrame.nv12(y, np.stack([u, v], -1).reshape(u.shape[0], -1)) if fmt == "nv12" else YUVFrame.i420(y, u, v)


# ------------------------------------------------------------------ construction and validation
def test_constructors_and_shape():
    rng = np.random.RandomState(0)
    y = rng.randint(0, 256, (6, 8)).astype(np.uint8)
    u = rng.randint(0, 256, (3, 4)).astype(np.uint8)
    v = rng.randint(0, 256, (3, 4)).astype(np.uint8)
    uv = np.stack([u, v], -1)
    a = YUVFrame.nv12(y, uv.reshape(3, 8))
    b = YUVFrame.nv12(y, uv)                                   # (H/2, W/2, 2) is the same plane
    c = YUVFrame.i420(y, u, v)
    for f in (a, b, c):
        assert f.shape == (6, 8, 3) and not f.is_cuda
        np.testing.assert_array_equal(f.to_rgb(), yuv_to_rgb_numpy(y, u, v))
    assert a.format == FMT_NV12 and c.format == FMT_I420
    assert a.pitches() == (8, 8, 0) and c.pitches() == (8, 4, 4)


def test_pitched_planes_are_views():
    rng = np.random.RandomState(1)
    wide = rng.randint(0, 256, (12, 20)).astype(np.uint8)          # a surface with a 20-byte pitch holding a 8 x 16 frame
    y, uv = wide[:8, :16], wide[8:, :16]
    f = YUVFrame.nv12(y, uv)
    assert f.planes[0] is y and f.pitches()[:2] == (20, 20)
    u, v = uv.reshape(4, 8, 2)[..., 0], uv.reshape(4, 8, 2)[..., 1]
    np.testing.assert_array_equal(f.to_rgb(), yuv_to_rgb_numpy(np.ascontiguousarray(y), u, v))
    fi = YUVFrame.i420(y, wide[8:, :8], wide[8:, 8:16])          # chroma planes with the surface's pitch too
    assert fi.pitches() == (20, 20, 20)


@pytest.mark.parametrize("bad", ["odd_h", "odd_w", "tiny", "dtype", "uv_shape", "u_shape", "ndim", "column_stride", "flipped",
                                 "mixed_sides", "cpu_tensor"])
def test_validation(bad):
    y = np.zeros((4, 6), np.uint8)
    u = np.zeros((2, 3), np.uint8)
    uv = np.zeros((2, 6), np.uint8)
    err = (ValueError, TypeError)
    with pytest.raises(err):
        if bad == "odd_h":
            YUVFrame.nv12(np.zeros((5, 6), np.uint8), np.zeros((2, 6), np.uint8))
        elif bad == "odd_w":
            YUVFrame.i420(np.zeros((4, 7), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8))
        elif bad == "tiny":
            YUVFrame.from_packed(np.zeros(0, np.uint8), 0, 0)
        elif bad == "dtype":
            YUVFrame.i420(y.astype(np.uint16), u, u)
        elif bad == "uv_shape":
            YUVFrame.nv12(y, np.zeros((2, 3), np.uint8))
        elif bad == "u_shape":
            YUVFrame.i420(y, u, np.zeros((3, 3), np.uint8))
        elif bad == "ndim":
            YUVFrame.nv12(np.zeros((4, 6, 1), np.uint8), uv)
        elif bad == "column_stride":
            YUVFrame.i420(np.zeros((4, 12), np.uint8)[:, ::2], u, u)
        elif bad == "flipped":
            YUVFrame.nv12(y[::-1], uv)
        elif bad == "mixed_sides":
            YUVFrame.i420(y, torch.from_numpy(u), u)
        elif bad == "cpu_tensor":
            YUVFrame.i420(torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(u))


def test_from_packed_round_trips():
    rng = np.random.RandomState(2)
    y = rng.randint(0, 256, (10, 14)).astype(np.uint8)
    u = rng.randint(0, 256, (5, 7)).astype(np.uint8)
    v = rng.randint(0, 256, (5, 7)).astype(np.uint8)
    for packed, fmt in ((nv12_packed(y, u, v), "nv12"), (i420_packed(y, u, v), "i420")):
        for buf in (packed, packed.reshape(-1)):
            f = YUVFrame.from_packed(buf, 10, 14, fmt)
            assert f.shape == (10, 14, 3)
            fu, fv = f.chroma()
            np.testing.assert_array_equal(np.asarray(f.planes[0]), y)
            np.testing.assert_array_equal(np.asarray(fu), u)
            np.testing.assert_array_equal(np.asarray(fv), v)
        f = YUVFrame.from_packed(packed, 10, 14, fmt)
        assert np.shares_memory(f.planes[0], packed)                # views, no copy
        np.testing.assert_array_equal(f.to_rgb(), yuv_to_rgb_numpy(y, u, v))
    with pytest.raises(ValueError):
        YUVFrame.from_packed(nv12_packed(y, u, v), 10, 14, "nv21")
    with pytest.raises(ValueError):
        YUVFrame.from_packed(nv12_packed(y, u, v)[:-1], 10, 14, "nv12")


# ------------------------------------------------------------------ the conversion
def test_conversion_anchors():
    for (yy, uu, vv), rgb in ANCHORS:
        assert _pixel(yy, uu, vv) == rgb
        f = YUVFrame.i420(np.full((2, 2), yy, np.uint8), np.full((1, 1), uu, np.uint8), np.full((1, 1), vv, np.uint8))
        assert (f.to_rgb() == np.array(rgb, np.uint8)).all(), (yy, uu, vv)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_every_chroma_pair_against_the_per_pixel_formula(fmt):
    y, u, v = full_chroma_frame()
    got = _frame(y, u, v, fmt).to_rgb()
    # every (U, V) pair with a spread of luma: the 2 x 2 block of chroma sample (cx, cy) holds 4 seeded Y values; the fixed Y
    # levels go through the formula for every pair as well
    for yl in (0, 15, 16, 17, 81, 126, 235, 236, 255):
        ref = np.array([[_pixel(yl, int(uu), int(vv)) for uu in range(256)] for vv in range(256)], np.uint8)
        f = _frame(np.full((512, 512), yl, np.uint8), u, v, fmt).to_rgb()
        np.testing.assert_array_equal(f[::2, ::2], ref, err_msg=f"Y={yl}")
    ys = np.arange(0, 512, 37)
    for py in ys:
        for px in range(512):
            assert tuple(got[py, px]) == _pixel(int(y[py, px]), int(u[py // 2, px // 2]), int(v[py // 2, px // 2])), (py, px)


def test_matches_opencv_where_installed():
    cv2 = pytest.importorskip("cv2")
    y, u, v = full_chroma_frame()
    np.testing.assert_array_equal(YUVFrame.nv12(y, np.stack([u, v], -1).reshape(256, 512)).to_rgb(),
                                  cv2.cvtColor(nv12_packed(y, u, v), cv2.COLOR_YUV2RGB_NV12))
    np.testing.assert_array_equal(YUVFrame.i420(y, u, v).to_rgb(), cv2.cvtColor(i420_packed(y, u, v), cv2.COLOR_YUV2RGB_I420))


# ------------------------------------------------------------------ the trackers on the CPU oracle
def _yuv_clip(golden_dir, n, fmt):
    from clipgen import demo_clip
    frames, _ = demo_clip(n)
    yuv = []
    for t, f in enumerate(frames):
        y, u, v = rgb_to_yuv420(f, seed=t)
        yuv.append(_frame(y, u, v, fmt))
    return yuv, np.stack([f.to_rgb() for f in yuv])


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_tracker_on_yuv_equals_tracker_on_its_rgb_conversion(oracle_net, golden_dir, fmt):
    yuv, rgb = _yuv_clip(golden_dir, 16, fmt)
    box = np.array([163, 53, 45, 174])
    out = []
    for frames in (yuv, rgb):
        trk = FEARTracker(oracle_net, cuda_id="cpu", **DEFAULT_TRACKING_CONFIG)
        trk.initialize(frames[0], box.copy())
        np.testing.assert_array_equal(trk.tracking_state.mean_color, np.mean(rgb[0], axis=(0, 1)))
        out.append(np.stack([trk.update(f)["bbox"] for f in frames[1:]]))
    np.testing.assert_array_equal(out[0], out[1])


def test_multi_tracker_host_path_on_yuv_streams(oracle_net, golden_dir):
    nv, rgb = _yuv_clip(golden_dir, 12, "nv12")
    i4, _ = _yuv_clip(golden_dir, 12, "i420")
    boxes = [np.array([163, 53, 45, 174]), np.array([300, 100, 40, 50])]
    res = {}
    for name, s0, s1 in (("yuv", nv, i4), ("rgb", rgb, rgb)):
        mt = FEARMultiTracker(oracle_net, cuda_id="cpu", **dict(DEFAULT_TRACKING_CONFIG, device_crop=False))
        assert not mt.device_path
        ids = mt.add(s0[0], boxes[0], stream=0) + mt.add(s1[0], boxes[1], stream=1)
        res[name] = [mt.update([s0[t], s1[t]]) for t in range(1, 12)]
    for a, b in zip(res["yuv"], res["rgb"]):
        for i in ids:
            np.testing.assert_array_equal(a[i], b[i])


def test_planar_entry_points_are_declared_and_check_the_handle():
    header = open(os.path.join(ROOT, "include", "fear_hip.h")).read()
    for sym in ("fear_yuv_to_rgb", "fear_crop_normalize_planar"):
        assert f"int {sym}(" in header
        assert sym in hip_backend.EXPORTED_SYMBOLS
    assert hip_backend.PLANAR_FRAME_DTYPE.itemsize == 48
    lib = hip_backend.load_library()
    assert lib.fear_yuv_to_rgb(None, None, None, None) == -1
    assert lib.fear_crop_normalize_planar(None, None, 1, None, None, None, 1, 256, None, None) == -1
