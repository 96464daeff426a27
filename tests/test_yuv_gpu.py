"""YUV video frames on the HIP engine: fear_yuv_to_rgb against the numpy conversion byte for byte, fear_crop_normalize_planar
against fear_crop_normalize_frames on the converted frames bit for bit, and both trackers on NV12 / I420 clips against the same
trackers on the clips' RGB conversion."""
import numpy as np
import pytest
import torch

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARTracker, YUVFrame
from feartracker_amd.frames import yuv_to_rgb_numpy
from yuvgen import full_chroma_frame, rgb_to_yuv420

pytestmark = pytest.mark.gpu

# the twelve boxes of tests/test_multi_tracker.py on the demo clip's 480 x 256 frames
DEMO_BOXES = [(163, 53, 45, 174), (440, 100, 60, 80), (-10, -5, 40, 40), (200, 120, 3, 3), (100, 200, 5, 4), (0, 0, 480, 256),
              (300, 30, 70, 50), (20, 150, 90, 100), (470, 240, 20, 20), (240, 5, 25, 12), (380, 180, 50, 60), (60, 60, 12, 30)]


def _planes(h, w, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8),
            rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8))


def _device_frame(y, u, v, fmt, pitch_pad=0):
    """The planes as CUDA tensors; with pitch_pad > 0 each plane is a slice of a wider buffer (a pitched decoder surface)."""
    def up(p):
        if not pitch_pad:
            return torch.from_numpy(np.ascontiguousarray(p)).cuda()
        buf = torch.full((p.shape[0], p.shape[1] + pitch_pad), 77, dtype=torch.uint8, device="cuda")
        buf[:, : p.shape[1]] = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        return buf[:, : p.shape[1]]
    if fmt == "nv12":
        return YUVFrame.nv12(up(y), up(np.stack([u, v], -1).reshape(u.shape[0], -1)))
    return YUVFrame.i420(up(y), up(u), up(v))


def _host_frame(y, u, v, fmt):
    return YUVFrame.nv12(y, np.stack([u, v], -1).reshape(u.shape[0], -1)) if fmt == "nv12" else YUVFrame.i420(y, u, v)


# ------------------------------------------------------------------ fear_yuv_to_rgb
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("size", [(2, 2), (256, 480), (1080, 1920)])
@pytest.mark.parametrize("pitch_pad", [0, 24])
def test_yuv_to_rgb_matches_numpy(hip_net, fmt, size, pitch_pad):
    y, u, v = _planes(*size, seed=size[0] + pitch_pad)
    got = hip_net.yuv_to_rgb(_device_frame(y, u, v, fmt, pitch_pad))
    assert torch.equal(got.cpu(), torch.from_numpy(yuv_to_rgb_numpy(y, u, v)))


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_to_rgb_every_chroma_pair(hip_net, fmt):
    y, u, v = full_chroma_frame()
    ref = torch.from_numpy(yuv_to_rgb_numpy(y, u, v))
    assert torch.equal(hip_net.yuv_to_rgb(_device_frame(y, u, v, fmt)).cpu(), ref)
    assert torch.equal(hip_net.yuv_to_rgb(_host_frame(y, u, v, fmt)).cpu(), ref)        # host planes are uploaded first


# ------------------------------------------------------------------ fear_crop_normalize_planar
def _contexts(n, frames_hw, fidx, rng, S):
    """Contexts inside, straddling and outside their frames, identity (S x S) and exact-half (2S x 2S) sizes, up- and
    down-scales, anisotropic ones."""
    ctx = np.zeros((n, 4), np.int32)
    sides = [S, 2 * S, 17, 100, 225, 870, 2 * S + 1, S - 1]
    for i in range(n):
        h, w = frames_hw[fidx[i]]
        kind = i % 4
        cw = sides[rng.randint(len(sides))]
        ch = cw if kind < 2 else sides[rng.randint(len(sides))]
        if kind == 0:                                       # inside (when it fits)
            x, y = rng.randint(0, max(1, w - cw)), rng.randint(0, max(1, h - ch))
        elif kind == 1 or kind == 2:                        # anywhere, straddling edges
            x, y = rng.randint(-cw, w), rng.randint(-ch, h)
        else:                                               # outside the frame
            x, y = w + rng.randint(0, 50), -ch - rng.randint(1, 50)
        ctx[i] = (x, y, cw, ch)
    return ctx


def _mixed_frames(seed):
    """An RGB frame, an NV12 frame with pitched planes and an I420 frame, of different sizes, with the RGB conversions."""
    y0, u0, v0 = _planes(256, 480, seed)
    y1, u1, v1 = _planes(192, 320, seed + 1)
    y2, u2, v2 = _planes(98, 62, seed + 2)
    rgb = torch.from_numpy(yuv_to_rgb_numpy(y0, u0, v0)).cuda()
    nv = _device_frame(y1, u1, v1, "nv12", pitch_pad=40)
    i4 = _device_frame(y2, u2, v2, "i420")
    return [rgb, nv, i4]


@pytest.mark.parametrize("n", [1, 5, 256])
@pytest.mark.parametrize("S", [256, 128])
def test_planar_crop_equals_rgb_crop_of_the_conversion(hip_net, n, S):
    rng = np.random.RandomState(n + S)
    frames = _mixed_frames(n)
    conv = [frames[0]] + [hip_net.yuv_to_rgb(f) for f in frames[1:]]
    hw = [tuple(f.shape[:2]) for f in frames]
    fidx = rng.randint(0, 3, n).astype(np.int32)
    ctx = _contexts(n, hw, fidx, rng, S)
    pad = rng.randint(0, 256, (n, 3)).astype(np.uint8)
    fi, cx, pd = (torch.from_numpy(a).cuda() for a in (fidx, ctx, pad))
    got = hip_net.crop_normalize_planar(hip_net.frame_table_planar(frames), fi, cx, pd, S)
    ref = hip_net.crop_normalize_frames(hip_net.frame_table(conv), fi, cx, pd, S)
    assert torch.equal(got, ref)
    # one-format tables too: every crop out of the NV12 frame, then the I420 one
    for k in (1, 2):
        one = torch.full((n,), k, dtype=torch.int32, device="cuda")
        ctx_k = torch.from_numpy(_contexts(n, hw, np.full(n, k), rng, S)).cuda()
        assert torch.equal(hip_net.crop_normalize_planar(hip_net.frame_table_planar([frames[k]]), one - k, ctx_k, pd, S),
                           hip_net.crop_normalize_frames(hip_net.frame_table([conv[k]]), one - k, ctx_k, pd, S))


def test_bad_index_and_bad_format_rows_are_all_border(hip_net):
    frames = _mixed_frames(9)
    table = hip_net.frame_table_planar(frames)
    raw = table.cpu().numpy().copy()
    rec = raw.view(np.dtype([("plane", "<u8", (3,)), ("pitch", "<i4", (3,)), ("h", "<i4"), ("w", "<i4"), ("format", "<i4")]))
    rec[1]["format"] = 7                                   # unknown format
    rec[2]["h"] = 97                                       # odd height for I420
    bad_table = torch.from_numpy(raw).cuda()
    n = 6
    fidx = torch.tensor([1, 2, -1, 3, 99, 0], dtype=torch.int32, device="cuda")
    ctx = torch.tensor([[10, 10, 100, 100]] * n, dtype=torch.int32, device="cuda")
    pad = torch.tensor([[10, 200, 30]] * n, dtype=torch.uint8, device="cuda")
    got = hip_net.crop_normalize_planar(bad_table, fidx, ctx, pad, 64)
    # an RGB table read with an index outside it gives the all-border crop
    border = hip_net.crop_normalize_frames(hip_net.frame_table([frames[0]]), torch.full((n,), 5, dtype=torch.int32,
                                                                                         device="cuda"), ctx, pad, 64)
    assert torch.equal(got[:5], border[:5])
    assert not torch.equal(got[5], border[5])              # the intact RGB row reads its frame
    assert torch.equal(got[5:], hip_net.crop_normalize_frames(hip_net.frame_table([frames[0]]), fidx[5:] * 0, ctx[5:], pad[5:], 64))


def test_crop_normalize_yuv_host_and_device_equal_crop_normalize(hip_net):
    rng = np.random.RandomState(4)
    y, u, v = _planes(256, 480, 4)
    rgb = yuv_to_rgb_numpy(y, u, v)
    for fmt in ("nv12", "i420"):
        for ctx in ([73, -295, 225, 870], [101, 33, 61, 47], [-40, 200, 512, 512], [479, 255, 3, 3], [600, 10, 50, 50]):
            pad = rng.randint(0, 256, (1, 3)).astype(np.uint8)
            ref = hip_net.crop_normalize(rgb, np.array([ctx]), pad, 256)
            for frame in (_host_frame(y, u, v, fmt), _device_frame(y, u, v, fmt, pitch_pad=8)):
                assert torch.equal(hip_net.crop_normalize_yuv(frame, np.array([ctx]), pad, 256), ref), (fmt, ctx)
    several = np.array([[73, -295, 225, 870], [301, 33, 61, 47], [5, 7, 128, 128]])
    pads = rng.randint(0, 256, (3, 3)).astype(np.uint8)
    assert torch.equal(hip_net.crop_normalize_yuv(_host_frame(y, u, v, "nv12"), several, pads, 128),
                       hip_net.crop_normalize(rgb, several, pads, 128))


# ------------------------------------------------------------------ the trackers
def _demo_yuv(golden_dir, n):
    from clipgen import demo_clip
    frames, _ = demo_clip(n)
    planes = [rgb_to_yuv420(f, seed=t) for t, f in enumerate(frames)]
    rgb = [yuv_to_rgb_numpy(*p) for p in planes]
    return planes, rgb


def _single(net, frames, box, smooth):
    trk = FEARTracker(net, cuda_id=0, **dict(DEFAULT_TRACKING_CONFIG, smooth=smooth))
    trk.initialize(frames[0], np.array(box))
    mean = trk.tracking_state.mean_color
    return np.stack([np.array(trk.update(f)["bbox"]) for f in frames[1:]]), mean


@pytest.mark.parametrize("smooth", [False, True])
def test_tracker_on_nv12_equals_tracker_on_rgb(hip_net, golden_dir, smooth):
    planes, rgb = _demo_yuv(golden_dir, 40)
    ref, mean = _single(hip_net, rgb, DEMO_BOXES[0], smooth)
    np.testing.assert_array_equal(mean, np.mean(rgb[0], axis=(0, 1)))
    for device in (False, True):
        frames = [_device_frame(*p, "nv12") if device else _host_frame(*p, "nv12") for p in planes]
        got, m = _single(hip_net, frames, DEMO_BOXES[0], smooth)
        assert m.tobytes() == mean.tobytes()
        np.testing.assert_array_equal(got, ref, err_msg=f"device planes: {device}")


def test_multi_tracker_mixed_format_streams_equal_rgb_runs(hip_net, golden_dir):
    planes, rgb = _demo_yuv(golden_dir, 30)
    streams = [[_host_frame(*p, "nv12") for p in planes],                    # host NV12
               [_device_frame(*p, "i420", pitch_pad=16) for p in planes],    # pitched device I420
               [torch.from_numpy(f).cuda() for f in rgb]]                    # device RGB
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    ids = [mt.add(streams[s][0], np.array(DEMO_BOXES[4 * s: 4 * s + 4]), stream=s) for s in range(3)]
    rows = [mt.update([streams[s][t] for s in range(3)]) for t in range(1, 30)]
    for s in range(3):
        ref = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
        rid = ref.add(rgb[0], np.array(DEMO_BOXES[4 * s: 4 * s + 4]))
        ref_rows = [ref.update(rgb[t]) for t in range(1, 30)]
        for i, j in zip(ids[s], rid):
            np.testing.assert_array_equal(np.stack([r[i] for r in rows]), np.stack([r[j] for r in ref_rows]), err_msg=f"{s}")


@pytest.mark.parametrize("copies", [1, 3])                 # 12 targets: the planar crop; 36: fear_yuv_to_rgb + the RGB crop
@pytest.mark.parametrize("device_frames", [False, True])
def test_submit_with_yuv_frames_never_synchronises(hip_net, golden_dir, device_frames, copies):
    from feartracker_amd.multi_tracker import PLANAR_CROP_MAX_TARGETS
    boxes = np.array(DEMO_BOXES * copies)
    assert (len(boxes) < PLANAR_CROP_MAX_TARGETS) == (copies == 1)
    planes, rgb = _demo_yuv(golden_dir, 12)
    ref = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    rid = ref.add(rgb[0], boxes)
    ref_rows = [ref.update(f) for f in rgb[1:]]
    src = [_device_frame(*p, "nv12") if device_frames else _host_frame(*p, "i420") for p in planes]
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    ids = mt.add(src[0], boxes)
    torch.cuda.synchronize()
    pending = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in src[1:]:
            pending.append(mt.submit(f))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = [p.result() for p in pending]
    for i, j in zip(ids, rid):
        np.testing.assert_array_equal(np.stack([r[i] for r in rows]), np.stack([r[j] for r in ref_rows]))
