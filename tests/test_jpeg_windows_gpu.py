"""Windows from the resident JPEG store on the GPU (include/fear_train.h: fear_jpeg_huffman_indexed_windows; DESIGN.md section 14,
"Windows"): `JpegStore.decode_windows` against the rectangle of `decode`, byte for byte, for every file and window of jpegwin at scale
1, 2 and 8; a call cut into three groups; an entry kept as pixels; the statuses; and the refusals of the C entry point."""
import ctypes

import numpy as np
import pytest
import torch

import jpegwin
from feartracker_amd import JpegStore, UnsupportedJPEG
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_store import WindowFrames, plan_decode_windows

pytestmark = pytest.mark.gpu
OK, ERR_NULL, ERR_SHAPE = 0, -1, -2


@pytest.fixture(scope="module")
def held():
    """A store with every file of jpegwin (the progressive one through its baseline transcode) and, last, one kept as pixels; the
    headers; the full decode of every entry at each scale, made once and left unchanged."""
    files = jpegwin.files()
    store = JpegStore(device=0, threads=2, progressive=True)
    kept = np.random.default_rng(1).integers(0, 256, (21, 35, 3), dtype=np.uint8)
    ids = store.add([data for _, data, _ in files] + [jpegwin.unsupported()], fallback=lambda data: kept)
    assert store.kinds[ids].tolist() == ["scan"] * len(files) + ["pixels"]
    headers = [jpegwin.sampling(name) for name, _, _ in files]          # (h, v) per file
    full = {scale: store.decode(ids[:-1], check=True, scale=scale) for scale in (1, 2, 8)}
    full[1] = full[1] + [torch.from_numpy(kept).cuda()]
    yield store, ids, files, headers, full
    store.close()


def _holds(got: WindowFrames, i: int, full) -> None:
    """The contract sentence: the window's pixels of tensor i are the rectangle of the full frame."""
    y0, y1, x0, x1 = got.window[i].tolist()
    oy, ox = got.origin[i].tolist()
    frame = got.frames[i]
    assert frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()
    if y0 == y1:
        assert tuple(frame.shape) == (0, 0, 3)
        return
    assert 0 <= oy <= y0 and 0 <= ox <= x0 and y1 - oy <= frame.shape[0] and x1 - ox <= frame.shape[1]
    assert oy + frame.shape[0] <= full.shape[0] and ox + frame.shape[1] <= full.shape[1]
    assert torch.equal(frame[y0 - oy:y1 - oy, x0 - ox:x1 - ox], full[y0:y1, x0:x1])


@pytest.mark.parametrize("scale", [1, 2, 8])
def test_every_window_of_every_file_is_the_rectangle_of_the_full_decode(held, scale):
    """One call: every window of every file, ids repeated.  The windows are given in pixels of the scaled frame."""
    store, ids, files, headers, full = held
    m = 8 // scale
    which, wins = [], []
    for k, (h, v) in enumerate(headers):
        H, W = full[scale][k].shape[:2]
        w = jpegwin.windows(H, W, v * m, h * m)
        which += [k] * len(w)
        wins.append(w)
    which, wins = np.array(which), np.concatenate(wins)
    got = store.decode_windows(ids[which], wins, scale=scale)
    store.check()                                                        # silent
    assert isinstance(got, WindowFrames) and len(got) == len(which)
    assert got.origin.dtype == np.int32 and got.origin.shape == (len(which), 2) and got.window.shape == (len(which), 4)
    assert np.array_equal(got.shape, store.shape(ids[which], scale))
    compact = 0
    for i, k in enumerate(which.tolist()):
        H, W = full[scale][k].shape[:2]
        assert got.window[i].tolist() == list(jpegwin.clipped(wins[i], H, W)), (files[k][0], wins[i].tolist())
        _holds(got, i, full[scale][k])
        compact += got.frames[i].numel() < full[scale][k].numel()
    assert compact > len(which) // 2                                     # compact tensors, not full frames
    # private tensors: writing one changes neither a neighbour nor a second decode
    before = [f.clone() for f in got.frames[:4]]
    got.frames[1].fill_(7)
    assert torch.equal(got.frames[0], before[0]) and torch.equal(got.frames[2], before[2])


def test_a_noise_file_skips_lanes_and_still_decodes_every_column(held):
    """The 400 x 48 noise file: every single MCU column as a window of its own, both MCU rows."""
    store, ids, files, headers, full = held
    k = next(i for i, f in enumerate(files) if f[0] == jpegwin.NOISE)
    wins = np.array([(y, y + 16, 16 * c + 3, 16 * c + 9) for c in range(400 // 16) for y in (0, 16, 32)], dtype=np.int64)
    got = store.decode_windows(np.full(len(wins), ids[k]), wins, check=True)
    for i in range(len(wins)):
        _holds(got, i, full[1][k])
    assert max(f.shape[1] for f in got.frames) <= 48                     # one MCU column and its halo


def test_a_small_workspace_limit_cuts_three_groups(held):
    store, ids, files, headers, full = held
    pick = np.array([0, 5, 9])
    wins = np.array([(2, 30, 3, 40), (0, 65, 0, 97), (10, 20, 20, 45)], dtype=np.int64)
    limit = store.workspace_limit
    try:
        store.workspace_limit = 1
        assert len(plan_decode_windows(store._columns, store._row_sub, ids[pick], wins, 1)) == 3
        got = store.decode_windows(ids[pick], wins, check=True)
    finally:
        store.workspace_limit = limit
    for i, k in enumerate(pick.tolist()):
        _holds(got, i, full[1][k])


def test_an_entry_kept_as_pixels_gives_its_rectangle(held):
    store, ids, files, headers, full = held
    wins = np.array([(3, 9, 4, 30), (0, 21, 0, 35), (5, 5, 0, 3), (2, 12, 1, 20)], dtype=np.int64)
    which = np.array([len(files), len(files), len(files), 0])
    got = store.decode_windows(ids[which], wins, check=True)
    assert got.origin.tolist()[:3] == [[3, 4], [0, 0], [0, 0]] and tuple(got.frames[0].shape) == (6, 26, 3)
    for i, k in enumerate(which.tolist()):
        _holds(got, i, full[1][k])
    assert got.frames[1].data_ptr() != store._pixels[int(ids[-1])].data_ptr()        # a copy, never an alias
    with pytest.raises(UnsupportedJPEG):
        store.decode_windows(ids[which], wins, scale=2)
    store.check()


def test_argument_checks_come_before_any_launch(held):
    store, ids, files, headers, full = held
    with pytest.raises(ValueError):
        store.decode_windows(ids[:2], np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        store.decode_windows(ids[:2], np.zeros((2, 4), dtype=np.float64))
    with pytest.raises(IndexError):
        store.decode_windows([len(store)], np.zeros((1, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        store.decode_windows(ids[:1], np.zeros((1, 4), dtype=np.int64), scale=3)
    empty = store.decode_windows([], np.zeros((0, 4), dtype=np.int64), check=True)
    assert len(empty) == 0 and empty.origin.shape == (0, 2) and empty.window.shape == (0, 4)


def test_the_entry_point_refuses_without_a_launch():
    """fear_jpeg_huffman_indexed_windows' own checks: the codes the header states, and a status buffer that stays as it was."""
    lib = abi.load_train_library()
    P = ctypes.c_void_p
    scratch = torch.zeros(4096, dtype=torch.uint8, device="cuda")        # stands for every device buffer: no accepted call reads it
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    images = (abi.FearJpegIndexed * 1)()
    im = images[0]
    im.scan = im.index = im.sub_start = scratch.data_ptr()
    im.n_sub, im.sub0, im.sub_count, im.mcu_row0, im.mcu_rows = 4, 0, 4, 0, 1

    def call(n=1, records=images, table=scratch.data_ptr(), coef=scratch.data_ptr(), st=status.data_ptr(), sb=128):
        return lib.fear_jpeg_huffman_indexed_windows(records, n, P(table), P(coef), P(st), sb, None)

    im.reserved = 0 | 0 << 16                                            # no columns
    assert call() == ERR_SHAPE
    im.reserved = 1020 | 5 << 16                                         # past FEAR_JPEG_MAX_SIDE / 8 = 1024 columns
    assert call() == ERR_SHAPE
    im.reserved = 1025 | 1 << 16
    assert call() == ERR_SHAPE
    im.reserved = 0 | 2 << 16
    im.sub0, im.sub_count = 2, 3                                         # the rows form's checks: lanes past the index
    assert call() == ERR_SHAPE
    im.sub0, im.sub_count = 0, 4
    im.mcu_row0, im.mcu_rows = 1020, 5
    assert call() == ERR_SHAPE
    im.mcu_row0, im.mcu_rows = 0, 1
    assert call(sb=6) == ERR_SHAPE and call(n=-1) == ERR_SHAPE and call(n=65536) == ERR_SHAPE
    im.index = scratch.data_ptr() + 8                                    # an index not 16-byte aligned
    assert call() == ERR_SHAPE
    im.index = scratch.data_ptr()
    assert call(records=None) == ERR_NULL and call(table=None) == ERR_NULL and call(coef=None) == ERR_NULL and call(st=None) == ERR_NULL
    im.scan = 0
    assert call() == ERR_NULL
    assert call(n=0, records=None) == OK                                 # nothing to do
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [77] * 4                             # nothing was launched
