"""JpegEncoder(optimize=True) on the GPU: per-file Huffman tables built on the device ("Per-file Huffman tables"),
held to Pillow's optimize=True files (tests/golden/jpeg_encode_optimize.npz) and to jpeg_encode.jpeg_encode_host byte for byte."""
import ctypes

import numpy as np
import pytest
import torch

from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import JpegDecoder
from test_jpeg_encode_modes_host import load_cases as load_plain_cases
from test_jpeg_encode_optimize_host import MODES, load_cases, table_histograms

pytestmark = pytest.mark.gpu

OPT = train_abi.FEAR_JPEG_ENC_OPTIMIZE


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def _cuda(frame):
    return torch.from_numpy(np.ascontiguousarray(frame)).cuda()


def test_every_fixture_case_in_one_call(cases):
    """All layouts, sizes and qualities, with and without restart markers, and the case that forces the length limit, in ONE call."""
    assert {c["mode"] for c in cases} == set(MODES) and any(c["restart_rows"] for c in cases) and any(c["name"] == "gray_limit" for c in cases)
    enc = E.JpegEncoder(0, optimize=True)
    frames = [_cuda(c["frame"]) for c in cases]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # encode never waits
    try:
        pending = enc.encode(frames, [c["quality"] for c in cases], [c["mode"] for c in cases],
                             restart_rows=[c["restart_rows"] for c in cases])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = pending.result()
    for c, data in zip(cases, got):
        assert data == c["file"], c["name"]
    assert pending.lengths.cpu().tolist() == [len(c["file"]) for c in cases] and not pending.status.any()
    # the argument of the call, per frame, and the bound as the slot
    some = cases[:6]
    flags = [k % 2 == 0 for k in range(len(some))]
    got = E.JpegEncoder(0, slot_bytes="bound").encode([_cuda(c["frame"]) for c in some], [c["quality"] for c in some], [c["mode"] for c in some],
                                                      optimize=flags, restart_rows=[c["restart_rows"] for c in some]).result()
    for c, on, data in zip(some, flags, got):
        assert data == (c["file"] if on else E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling=c["mode"])), c["name"]


def test_plain_frames_between_optimised_neighbours(golden_dir, cases):
    """Every case of the jpeg_encode_modes fixture, the restart cases included, as a plain frame behind an optimised frame, in one call:
    byte-equal to today's files."""
    plain = load_plain_cases(golden_dir)
    assert len(plain) == 170 and sum(c["restart_rows"] > 0 for c in plain) == 9
    small = [c for c in cases if c["name"] != "gray_limit"]
    mixed, flags = [], []
    for k, c in enumerate(plain):
        mixed += [small[k % len(small)], c]
        flags += [True, False]
    got = E.JpegEncoder(0).encode([_cuda(c["frame"]) for c in mixed], [c["quality"] for c in mixed], [c["mode"] for c in mixed],
                                  optimize=flags, restart_rows=[c["restart_rows"] for c in mixed]).result()
    for c, data in zip(mixed, got):
        assert data == c["file"], c["name"]


def test_the_table_stage_on_chosen_histograms():
    """fear_jpeg_huff_optimal against jpeg_optimal_table_host on histograms no small image gives, the refused one among them; nothing
    outside the outputs is written."""
    hists = table_histograms()
    names = list(hists)
    n, guard = len(names), 64
    freq = torch.from_numpy(np.stack([hists[k] for k in names]).astype(np.uint32).view(np.int32)).cuda()
    sizes = dict(counts=n * 16, values=n * 256, nvalues=n * 4, codes=n * 1024, status=n * 4)
    bufs = {k: torch.full((guard + v + guard,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    lib = train_abi.load_train_library()
    ptr = {k: ctypes.c_void_p(b.data_ptr() + guard) for k, b in bufs.items()}
    rc = lib.fear_jpeg_huff_optimal(ctypes.c_void_p(freq.data_ptr()), n, ptr["counts"], ptr["values"], ptr["nvalues"], ptr["codes"],
                                    ptr["status"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, v in sizes.items():
        assert (host[k][:guard] == 0xA5).all() and (host[k][guard + v:] == 0xA5).all(), k
    counts = host["counts"][guard:-guard].reshape(n, 16)
    values = host["values"][guard:-guard].reshape(n, 256)
    nvalues = host["nvalues"][guard:-guard].view(np.int32)
    codes = host["codes"][guard:-guard].view(np.uint32).reshape(n, 256)
    status = host["status"][guard:-guard].view(np.int32)
    for i, name in enumerate(names):
        if name == "deep":
            assert status[i] == train_abi.FEAR_JPEG_ENC_HUFF_DEPTH and nvalues[i] == 0 and not counts[i].any() and not codes[i].any()
            continue
        want_counts, want_values, _ = E.jpeg_optimal_table_host(hists[name])
        assert status[i] == 0 and tuple(counts[i]) == want_counts and nvalues[i] == len(want_values), name
        assert values[i, :nvalues[i]].tobytes() == want_values and (values[i, nvalues[i]:] == 0xA5).all(), name
        table = E._codes(want_counts, want_values)
        want_codes = np.zeros(256, dtype=np.uint32)
        for sym, (code, length) in table.items():
            want_codes[sym] = length << 16 | code
        assert np.array_equal(codes[i], want_codes), name
    assert lib.fear_jpeg_huff_optimal(None, 1, ptr["counts"], ptr["values"], ptr["nvalues"], ptr["codes"], ptr["status"], None) == -1
    assert lib.fear_jpeg_huff_optimal(None, 0, None, None, None, None, None, None) == 0


def test_an_optimised_image_that_spans_workgroups_chunks_and_segments():
    rgb = np.random.default_rng(21).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    rgb[:, :320] //= 16                                        # half of it quiet, so that the statistics are not flat
    want = E.jpeg_encode_host(rgb, 90, 1, optimize=True)
    assert len(want) > 8 * train_abi.FEAR_JPEG_ENC_CHUNK_BYTES and 40 * 30 * 6 > 8 * train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS
    enc = E.JpegEncoder(0, quality=90, restart_rows=1, optimize=True)
    frame = _cuda(rgb)
    first, second = enc.encode([frame]), enc.encode(frame[None])
    (a,), (b,) = first.result(), second.result()
    assert a == want and b == want
    n = len(want)
    assert torch.equal(first.buffer[:n], second.buffer[:n]) and torch.equal(first.lengths, second.lengths)
    assert len(want) < len(E.jpeg_encode_host(rgb, 90, 1))


def test_overflow_leaves_the_neighbours_and_the_guards_alone(cases):
    by_name = {c["name"]: c for c in cases}
    left, big, right = by_name["444_8x8"], by_name["444_noise_q100"], by_name["gray_13x17"]
    slot, guard = len(big["file"]) - 1, 48                     # one byte short of the largest file
    three = (left, big, right)
    enc = E.JpegEncoder(0, slot_bytes=slot, guard_bytes=guard, optimize=True)
    pending = enc.encode([_cuda(c["frame"]) for c in three], [c["quality"] for c in three], [c["mode"] for c in three])
    with pytest.raises(E.JpegOverflow) as err:
        pending.result()
    assert err.value.items == [1]
    lengths, status, offsets = pending.lengths.cpu().tolist(), pending.status.cpu().tolist(), pending.offsets.cpu().tolist()
    assert lengths == [len(left["file"]), 0, len(right["file"])] and status == [0, E.ENC_OVERFLOW, 0]
    buf = pending.buffer.cpu().numpy()
    for k, c in ((0, left), (2, right)):
        assert buf[offsets[k]:offsets[k] + lengths[k]].tobytes() == c["file"]
        assert (buf[offsets[k] + lengths[k]:offsets[k] + slot] == 0xA5).all()
    assert (buf[offsets[1]:offsets[1] + slot] == 0xA5).all()
    for k in range(3):
        end = offsets[k + 1] if k < 2 else len(buf)
        assert end - offsets[k] >= slot + guard and (buf[offsets[k] + slot:end] == 0xA5).all()
    for fits in (slot + 1, "bound"):
        (data,) = E.JpegEncoder(0, slot_bytes=fits, optimize=True).encode([_cuda(big["frame"])], 100, "4:4:4").result()
        assert data == big["file"]


def test_optimised_files_decode_to_the_plain_files_pixels(cases):
    from feartracker_amd.jpeg_store import JpegStore
    picture = next(c for c in cases if c["name"] == "420_picture_q90")["frame"]
    frame = _cuda(picture)
    enc = E.JpegEncoder(0, quality=90)
    files = enc.encode([frame] * 8, subsampling=list(MODES) * 2, optimize=[True] * 4 + [False] * 4).result()
    dec = JpegDecoder(device=0)
    pixels = [p.cpu().numpy() for p in dec.decode(files)]
    dec.close()
    for k, mode in enumerate(MODES):
        assert len(files[k]) < len(files[k + 4]) and np.array_equal(pixels[k], pixels[k + 4]), mode
    store = JpegStore(device=0, threads=2)
    ids = store.add(files[:3])                                 # (the store's layouts: three components)
    for k, p in enumerate(store.decode(ids, check=True)):
        assert np.array_equal(p.cpu().numpy(), pixels[k])
    store.close()


def test_refusals():
    enc = E.JpegEncoder(0)
    rgb = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    for bad in (1, "yes", [1], [True, "no"]):
        with pytest.raises(TypeError):
            enc.encode([rgb], optimize=bad)
    with pytest.raises(ValueError):
        enc.encode([rgb], optimize=[True, False])
    with pytest.raises(TypeError):
        E.JpegEncoder(0, optimize=1)
    with pytest.raises(ValueError):
        enc.encode([rgb], restart_rows=[0, 1])
    # the C ABI: unknown flag bits, and a flag changed after planning, with real device buffers
    lib = train_abi.load_train_library()
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    header = torch.zeros(640, dtype=torch.uint8, device="cuda")
    rec = (train_abi.FearJpegEncImage * 1)()
    rec[0].src, rec[0].out, rec[0].header = rgb.data_ptr(), out.data_ptr(), header.data_ptr()
    rec[0].width, rec[0].height, rec[0].quality, rec[0].out_cap, rec[0].header_bytes = 8, 8, 75, 4096, 191
    rec[0].flags = 2
    assert lib.fear_jpeg_encode_plan(rec, 1) == -2
    rec[0].flags = OPT
    assert lib.fear_jpeg_encode_plan(rec, 1) == 0
    ws = torch.zeros(int(lib.fear_jpeg_encode_workspace_bytes(rec, 1)), dtype=torch.uint8, device="cuda")
    verdict = torch.zeros(2, dtype=torch.int32, device="cuda")
    rec[0].flags = 0
    args = (ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(verdict[0:].data_ptr()), ctypes.c_void_p(verdict[1:].data_ptr()), None)
    assert lib.fear_jpeg_encode_u8(rec, 1, *args) == -2
    torch.cuda.synchronize()
    assert not out.any() and not verdict.any()
