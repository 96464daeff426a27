"""`TrainPairBuilder.build` on a `WindowFrames` (include/fear_train.h: fear_train_pairs_windows, fear_train_pairs_windows_u8; DESIGN.md
section 14, "Windows"): the batch built from the compact frames `JpegStore.decode_windows` returns for `frame_windows` equals the batch
built from whole frames, tensor for tensor and on the uint8 crops, with the default config and with the photometric stage."""
import ctypes

import numpy as np
import pytest
import torch

import jpegwin
from feartracker_amd import JpegStore
from feartracker_amd import train_abi as abi
from feartracker_amd.train_data import TrainPairBuilder
from feartracker_amd.train_data.records import GEOM_DTYPE, SEARCH_SIZE, TEMPLATE_SIZE, WINDOW_DTYPE, FRAME_DTYPE

pytestmark = pytest.mark.gpu
NAMES = ("97x65_420", "97x65_422_restart", "50x37_444", "97x65_gray", "noise_400x48_420_q95", "50x37_420_restart")
# 8 pairs over 6 frames: frames 0 and 4 shared by several pairs, frame 5 used by none; boxes inside, partly outside, wholly outside
PAIRS = np.array([
    # t_frame, box xywh,        s_frame, box xywh,        presence
    [0, 30, 20, 16, 12,         1, 40, 30, 18, 14,        1],
    [4, 200, 10, 40, 20,        4, 220, 14, 30, 18,       1],
    [0, 60, 40, 20, 20,         2, 20, 10, 14, 10,        1],
    [3, -6, 50, 20, 20,         4, 380, 30, 30, 16,       1],     # partly outside: left and bottom | right and bottom
    [2, 5, 5, 10, 10,           0, 2, 2, 12, 9,           0],     # presence == 0
    [1, 30, 300, 12, 12,        3, 30, -200, 12, 12,      1],     # wholly outside: below | above
    [4, 100, 20, 24, 20,        0, 70, 30, 20, 18,        1],
    [1, 50, 30, 10, 12,         1, 10, 10, 30, 28,        1],
], dtype=np.float64)


@pytest.fixture(scope="module")
def held():
    store = JpegStore(device=0, threads=2)
    ids = store.add([jpegwin.named(n)[1] for n in NAMES])
    yield store, ids, store.decode(ids, check=True), store.borders(ids)
    store.close()


def _same_batches(a, b):
    for name, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("photometric", [False, True])
def test_a_batch_from_windows_equals_the_batch_from_whole_frames(held, photometric):
    store, ids, full, borders = held
    builder = TrainPairBuilder(dict(photometric=True) if photometric else None, device=0)
    shapes = store.shape(ids)
    params = builder.draw(PAIRS, shapes, np.random.default_rng(11 + photometric))
    wins = builder.frame_windows(PAIRS, params, shapes)
    assert wins[5].tolist() == [0, 0, 0, 0] and (wins[4, 3] - wins[4, 2]) < 400
    compact = store.decode_windows(ids, wins, check=True)
    assert compact.nbytes < sum(f.numel() for f in full) and tuple(compact.frames[5].shape) == (0, 0, 3)
    want = builder.build(full, PAIRS, params, borders=borders)
    got = builder.build(compact, PAIRS, params, borders=borders)
    _same_batches(got, want)
    assert torch.isfinite(got.template).all() and got.search.abs().sum() > 0
    with pytest.raises(ValueError):
        builder.build(compact, PAIRS, params)                            # the mean over a window is not the frame's mean


def test_the_u8_crops_from_windows_equal_those_from_whole_frames(held):
    """fear_train_pairs_windows_u8 against fear_train_pairs_u8 through the C ABI, on the tables `build` would upload."""
    store, ids, full, borders = held
    lib = abi.load_train_library()
    builder = TrainPairBuilder(device=0)
    shapes = store.shape(ids)
    params = builder.draw(PAIRS, shapes, np.random.default_rng(3))
    compact = store.decode_windows(ids, builder.frame_windows(PAIRS, params, shapes), check=True)
    tab = builder.tables(PAIRS, params)
    B, F = len(PAIRS), len(ids)
    frames, windows = np.zeros(F, dtype=FRAME_DTYPE), np.zeros(F, dtype=WINDOW_DTYPE)
    for i, (f, c) in enumerate(zip(full, compact.frames)):
        frames[i] = (f.data_ptr(), f.shape[0], f.shape[1])
        windows[i] = (c.data_ptr() if c.numel() else 0, f.shape[0], f.shape[1], compact.origin[i, 0], compact.origin[i, 1], c.shape[0], c.shape[1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_frames, d_windows, d_geom, d_lut = up(frames), up(windows), up(tab["geom"].astype(GEOM_DTYPE)), up(tab["lut"])
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for name, table in (("fear_train_pairs_u8", d_frames), ("fear_train_pairs_windows_u8", d_windows)):
        t = torch.zeros((B, TEMPLATE_SIZE, TEMPLATE_SIZE, 3), dtype=torch.uint8, device="cuda")
        s = torch.zeros((B, SEARCH_SIZE, SEARCH_SIZE, 3), dtype=torch.uint8, device="cuda")
        reg, cls = torch.zeros((B, 4, 16, 16), device="cuda"), torch.zeros((B, 1, 16, 16), device="cuda")
        wgt = torch.zeros((B, 16, 16), device="cuda")
        abi.launch(lib, name, P(table), F, P(borders), P(d_geom), P(d_lut), B, P(t), P(s), P(reg), P(cls), P(wgt), None)
        torch.cuda.synchronize()
        out[name] = (t, s, reg, cls, wgt)
    for x, y in zip(out["fear_train_pairs_u8"], out["fear_train_pairs_windows_u8"]):
        assert torch.equal(x, y)
    assert out["fear_train_pairs_u8"][0].float().std() > 1               # pictures, not constants
    # the checks are fear_train_pairs': no launch for a null table or a bad count
    t, s, reg, cls, wgt = out["fear_train_pairs_windows_u8"]
    args = (P(borders), P(d_geom), P(d_lut), B, P(t), P(s), P(reg), P(cls), P(wgt), None)
    assert lib.fear_train_pairs_windows_u8(None, F, *args) == -1
    assert lib.fear_train_pairs_windows_u8(P(d_windows), -1, *args) == -2
