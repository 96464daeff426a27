"""The training-pair builder on the GPU (include/fear_train.h: fear_frame_border_u8, fear_train_pairs): bit-exact against its numpy
restatement `build_host`, free of host waits on device frames, feeding `FEARNetTrainHIP.step`, and the C ABI's edges."""
import ctypes

import numpy as np
import pytest
import torch

from feartracker_amd.train_data import (COLOUR_NONE, GEOM_DTYPE, FRAME_DTYPE, TONE_NONE, TrainPairBuilder)

pytestmark = pytest.mark.gpu

SHAPES = [(1080, 1920), (256, 480), (48, 64)]


def _frames(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SHAPES:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) % 256], axis=-1)
        noise = rng.integers(0, 64, (h, w, 3))
        out.append(np.clip(base + noise - 32, 0, 255).astype(np.uint8))
    return out


def _pairs(B, seed=1):
    """Boxes in every frame size, with absent targets, contexts far outside the frame and exact-size / 2x stage-1 contexts."""
    rng = np.random.default_rng(seed)
    p = np.zeros((B, 11))
    for k in range(B):
        tf, sf = k % 3, (k // 3) % 3
        H, W = SHAPES[tf]
        tw, th = rng.integers(2, max(3, W // 3)), rng.integers(2, max(3, H // 3))
        p[k, :5] = [tf, rng.integers(0, W - tw + 1), rng.integers(0, H - th + 1), tw, th]
        H, W = SHAPES[sf]
        sw, sh = rng.integers(1, max(2, W // 3)), rng.integers(1, max(2, H // 3))
        if k % 9 == 4:                                       # a small box in a corner: the context lies mostly outside
            sw, sh = rng.integers(1, 6), rng.integers(1, 6)
            p[k, 5:10] = [sf, W - sw, 0, sw, sh]
        else:
            p[k, 5:10] = [sf, rng.integers(0, W - sw + 1), rng.integers(0, H - sh + 1), sw, sh]
        p[k, 10] = 0 if k % 8 == 7 else 1
    return p


def _params(builder, frames, pairs, seed=2):
    B = len(pairs)
    p = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(seed))
    p.tone[:] = np.arange(B) % 3                              # every tone ...
    p.colour[:] = (np.arange(B) // 3) % 4                     # ... with every colour member in turn
    if B > 16:
        p.context[5::17] = 5.5                                # the widest context
        pairs[10, 5:10] = [0, 300, 200, 128, 128]             # 128 * (1 + 3.5 + 3.5) = 1024: stage 1 is an exact 2x decimation
        p.context[10] = 3.5
        pairs[11, 5:10] = [1, 100, 50, 64, 64]                # 64 * 8 = 512: stage 1 is the identity
        p.context[11] = 3.5
    return p


def _assert_equal(dev, host):
    for name in ("template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox"):
        d = getattr(dev, name).cpu().numpy()
        h = getattr(host, name)
        assert d.shape == h.shape and d.dtype == h.dtype, name
        bad = np.argwhere(d != h)
        assert bad.size == 0, f"{name}: {len(bad)} values differ, first at {bad[:3].tolist()}: {d[tuple(bad[0])]} vs {h[tuple(bad[0])]}"


@pytest.mark.parametrize("B", [1, 128])
def test_build_equals_build_host(B):
    frames = _frames()
    builder = TrainPairBuilder(device=0)
    pairs = _pairs(B)
    params = _params(builder, frames, pairs)
    mixed = [torch.from_numpy(frames[0]).cuda(), frames[1], torch.from_numpy(frames[2]).cuda()]      # device and host frames
    dev = builder.build(mixed, pairs, params)
    torch.cuda.synchronize()
    _assert_equal(dev, builder.build_host(frames, pairs, params))


def test_build_every_branch_single_pairs():
    frames = _frames(3)
    builder = TrainPairBuilder(device=0)
    for tone in range(3):
        for colour in range(4):
            pairs = _pairs(1, seed=10 * tone + colour)
            p = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(tone * 4 + colour))
            p.tone[:], p.colour[:] = tone, colour
            dev = builder.build(frames, pairs, p)
            torch.cuda.synchronize()
            _assert_equal(dev, builder.build_host(frames, pairs, p))


def test_build_on_device_frames_does_not_wait():
    frames = [torch.from_numpy(f).cuda() for f in _frames(4)]
    builder = TrainPairBuilder(device=0, seed=0)
    pairs = _pairs(32, seed=5)
    builder.build(frames, pairs)                              # warm the pinned and device allocators
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = builder.build(frames, pairs)
        out2 = builder.build(frames, pairs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.search.shape == (32, 3, 256, 256) and out2.template.shape == (32, 3, 128, 128)


def test_step_on_built_pairs():
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    frames = _frames(6)
    builder = TrainPairBuilder(device=0)
    pairs = _pairs(16, seed=7)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(8))
    dev = builder.build(frames, pairs, params)
    host = builder.build_host(frames, pairs, params)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    a = net.step(*dev[:5])
    b = net.step(*(torch.from_numpy(x).cuda() for x in host[:5]))
    la = (float(a["loss_cls"]), float(a["loss_reg"]))
    lb = (float(b["loss_cls"]), float(b["loss_reg"]))
    assert np.all(np.isfinite(la)) and la == lb
    AdamHIP(net, lr=1e-4).step(a["grads"])
    torch.cuda.synchronize()


def _geom(B, t_frame, s_frame):
    g = np.zeros(B, dtype=GEOM_DTYPE)
    g["t_frame"], g["s_frame"] = t_frame, s_frame
    g["t_ctx"] = [4, 4, 40, 30]
    g["s_ctx"] = [-100, -50, 600, 600]
    g["box"] = [100, 100, 50, 50]
    g["presence"] = 1
    g["tone"] = TONE_NONE
    g["inv"] = [2.0, 0.0, 2.0, 0.0]
    return g


def test_abi_edges():
    from feartracker_amd.train_head import load_train_library
    lib = load_train_library()
    P = ctypes.c_void_p
    frame = torch.from_numpy(_frames(9)[2]).cuda()
    ftab = np.zeros(1, dtype=FRAME_DTYPE)
    ftab[0] = (frame.data_ptr(), frame.shape[0], frame.shape[1])
    d_ftab = torch.from_numpy(ftab.view(np.uint8).copy()).cuda()
    border = torch.zeros((1, 3), dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    assert lib.fear_frame_border_u8(None, 1, P(border.data_ptr()), st) == -1
    assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), 1, None, st) == -1
    assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), 0, None, st) == 0
    assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), -1, P(border.data_ptr()), st) == -2
    assert lib.fear_frame_border_u8(P(d_ftab.data_ptr()), 1, P(border.data_ptr()), st) == 0
    torch.cuda.synchronize()
    ref = np.clip(np.rint(np.mean(frame.cpu().numpy(), axis=(0, 1))), 0, 255).astype(np.uint8)
    assert np.array_equal(border.cpu().numpy()[0], ref)

    B = 2
    geom = torch.from_numpy(_geom(B, [0, 7], [5, 0]).view(np.uint8).copy()).cuda()   # frame indices 7 and 5 are outside the table
    lut = torch.from_numpy(np.broadcast_to(np.arange(256, dtype=np.uint8), (B, 3, 256)).copy()).cuda()
    outs = [torch.full(s, 7.0, device="cuda") for s in ((B, 3, 128, 128), (B, 3, 256, 256), (B, 4, 16, 16), (B, 1, 16, 16), (B, 16, 16))]
    ptrs = [P(o.data_ptr()) for o in outs]
    args = lambda **kw: [kw.get("frames", P(d_ftab.data_ptr())), kw.get("nf", 1), kw.get("border", P(border.data_ptr())),
                         kw.get("geom", P(geom.data_ptr())), kw.get("lut", P(lut.data_ptr())), kw.get("n", B)] + \
        [kw.get(f"o{i}", ptrs[i]) for i in range(5)] + [st]
    assert lib.fear_train_pairs(*args(geom=None)) == -1
    assert lib.fear_train_pairs(*args(lut=None)) == -1
    for i in range(5):
        assert lib.fear_train_pairs(*args(**{f"o{i}": None})) == -1
    assert lib.fear_train_pairs(*args(frames=None)) == -1
    assert lib.fear_train_pairs(*args(n=-1)) == -2
    assert lib.fear_train_pairs(*args(n=0, geom=None, lut=None)) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                  # n = 0 and refused calls write nothing
    assert lib.fear_train_pairs(*args()) == 0
    torch.cuda.synchronize()
    mean = np.array([0.485, 0.456, 0.406], np.float32) * np.float32(255.0)
    inv = np.reciprocal(np.array([0.229, 0.224, 0.225], np.float32) * np.float32(255.0), dtype=np.float32)
    zero = (np.float32(0.0) - mean) * inv                               # a pixel of value 0, normalised
    t, s = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    for c in range(3):
        assert np.all(t[1, c] == zero[c])                              # template of pair 1: frame 7 does not exist -> all zero pixels
        assert np.all(s[0, c] == zero[c])                              # search of pair 0: frame 5 does not exist
    assert not np.all(t[0] == t[0, :, :1, :1])                          # frame 0 exists: a real crop
    assert outs[4].sum().item() > 0                                    # targets of present pairs
