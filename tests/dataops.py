"""Plumbing shared by the data stage's GPU tests (test_photometric_gpu, test_colour_gpu, test_jpeg_gpu): guard-banded output buffers, one
runner per operator of include/fear_train.h — upload, launch, synchronise, check the guards, reshape — and the frames, pairs and
comparison of the builder tests.  A plain module, imported by name as headref and syncref are."""
import ctypes

import numpy as np
import torch

P = ctypes.c_void_p
GUARD = 4096                       # elements of sentinel on either side of a guarded buffer
SENTINEL_U8, SENTINEL_F32 = 0xA5, -12345.0
_SENTINEL = {torch.uint8: SENTINEL_U8, torch.float32: SENTINEL_F32}


def guarded(count, dtype=torch.uint8):
    return torch.full((count + 2 * GUARD,), _SENTINEL[dtype], dtype=dtype, device="cuda")


def inner(buf):
    return P(buf.data_ptr() + GUARD * buf.element_size())


def inside(buf, count, what="output"):
    host = buf.cpu().numpy()
    sentinel = host.dtype.type(_SENTINEL[buf.dtype])
    assert np.all(host[:GUARD] == sentinel) and np.all(host[GUARD + count:] == sentinel), f"guard band of the {what} written"
    return host[GUARD:GUARD + count]


def _device(array):
    """A host array (records as their bytes) on the device; None stays None."""
    if array is None:
        return None
    a = np.ascontiguousarray(array)
    return torch.from_numpy((a.view(np.uint8) if a.dtype.names else a).copy()).cuda()


def run_photometric(lib, qtable, crops, ops, taps, fn="fear_photometric_u8"):
    """fear_photometric_u8 on (n, H, W, 3) uint8 crops -> (n, 3, H, W) fp32, or fear_photometric_stage_u8 -> (n, H, W, 3) uint8; the
    guard band around the output checked."""
    n, h, w = crops.shape[:3]
    d_in, d_ops, d_taps = _device(crops), _device(ops), _device(taps)
    count, fp32 = n * 3 * h * w, fn == "fear_photometric_u8"
    out = guarded(count, torch.float32 if fp32 else torch.uint8)
    rc = getattr(lib, fn)(P(d_in.data_ptr()), n, h, w, P(d_ops.data_ptr()), P(d_taps.data_ptr()) if d_taps is not None else None,
                          P(qtable.data_ptr()), inner(out), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return inside(out, count).reshape((n, 3, h, w) if fp32 else (n, h, w, 3))


def run_stage(lib, qtable, crops, ops, taps):
    return run_photometric(lib, qtable, crops, ops, taps, fn="fear_photometric_stage_u8")


def run_colour(lib, crops, ops, aux):
    """fear_colour_u8 on (n, H, W, 3) uint8 crops, the guard band around the output checked."""
    n, h, w = crops.shape[:3]
    d_in, d_ops, d_aux = _device(crops), _device(ops), _device(aux)
    count = n * h * w * 3
    out = guarded(count)
    rc = lib.fear_colour_u8(P(d_in.data_ptr()), n, h, w, P(d_ops.data_ptr()), P(d_aux.data_ptr()), inner(out), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), crops), "input written"
    return inside(out, count).reshape(n, h, w, 3)


def run_jpeg(lib, crops, quality):
    """fear_jpeg_u8 on (n, H, W, 3) uint8 crops and (n,) qualities, the guard bands around the output and the workspace checked."""
    n, h, w = crops.shape[:3]
    d_in, d_q = _device(crops), _device(np.asarray(quality, dtype=np.int32))
    count = n * h * w * 3
    ws_bytes = lib.fear_jpeg_workspace_bytes(n, h, w)
    assert ws_bytes >= n * h * w * 3 // 2
    out, ws = guarded(count), guarded(ws_bytes)
    rc = lib.fear_jpeg_u8(P(d_in.data_ptr()), n, h, w, P(d_q.data_ptr()), inner(ws), ws_bytes, inner(out), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    return inside(out, count).reshape(n, h, w, 3)


# ----------------------------------------------------------------------------------------------------------------------- builder
FRAME_SHAPES = ((48, 64), (256, 480))


def frames(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in FRAME_SHAPES:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) % 256], axis=-1)
        out.append(np.clip(base + rng.integers(0, 64, (h, w, 3)) - 32, 0, 255).astype(np.uint8))
    return out


def pairs(B, seed=1):
    rng = np.random.default_rng(seed)
    p = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % 2), (5, (k + 1) % 2)):
            h, w = FRAME_SHAPES[f]
            bw, bh = rng.integers(4, w // 3), rng.integers(4, h // 3)
            p[k, col:col + 5] = [f, rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1), bw, bh]
        p[k, 10] = 1
    return p


def equal(dev, host):
    for name in ("template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox"):
        d = getattr(dev, name)
        d = d.cpu().numpy() if isinstance(d, torch.Tensor) else d
        h = getattr(host, name)
        h = h.cpu().numpy() if isinstance(h, torch.Tensor) else h
        assert d.shape == h.shape and d.dtype == h.dtype, name
        bad = np.argwhere(d != h)
        assert bad.size == 0, f"{name}: {len(bad)} values differ, first at {bad[:3].tolist()}"
