"""fear_jpeg_encode_u8's 4:2:2, 4:4:4 and gray layouts through JpegEncoder on the GPU, held to Pillow's files
(tests/golden/jpeg_encode_modes.npz) and to jpeg_encode.jpeg_encode_host byte for byte ("Writing JPEG files")."""
import numpy as np
import pytest
import torch

from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import JpegDecoder, _parse, jpeg_decode_host
from test_jpeg_encode_modes_host import MCU, MODES, load_cases

pytestmark = pytest.mark.gpu

BLOCKS = {"4:2:0": 6, "4:2:2": 4, "4:4:4": 3, "gray": 1}                   # per MCU; 24 blocks per workgroup of the transform
NEW = ("4:2:2", "4:4:4", "gray")


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def _cuda(frame):
    return torch.from_numpy(np.ascontiguousarray(frame)).cuda()


def test_every_fixture_case_in_one_call(cases):
    """All four layouts, mixed sizes and per-image qualities in ONE call: Pillow's bytes."""
    plain = [c for c in cases if c["restart_rows"] == 0]
    assert {c["mode"] for c in plain} == set(MODES) and len(plain) >= 160
    assert any(c["mode"] == "gray" and c["frame"].ndim == 3 for c in plain) and any(c["frame"].ndim == 2 for c in plain)
    enc = E.JpegEncoder(0)
    frames = [_cuda(c["frame"]) for c in plain]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # encode never waits
    try:
        pending = enc.encode(frames, [c["quality"] for c in plain], [c["mode"] for c in plain])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = pending.result()
    for c, data in zip(plain, got):
        assert data == c["file"], c["name"]
    assert pending.lengths.cpu().tolist() == [len(c["file"]) for c in plain]
    # the restart cases: the interval is the encoder's, so each distinct restart_rows is a call of its own, again of mixed layouts
    for rows in sorted({c["restart_rows"] for c in cases} - {0}):
        some = [c for c in cases if c["restart_rows"] == rows]
        assert {c["mode"] for c in some} == set(MODES)
        got = E.JpegEncoder(0, restart_rows=rows).encode([_cuda(c["frame"]) for c in some], [c["quality"] for c in some],
                                                         [c["mode"] for c in some]).result()
        for c, data in zip(some, got):
            assert data == c["file"], c["name"]
    # the constructor's layout, and a batch tensor of gray frames
    c = next(c for c in plain if c["name"] == "gray_40x23_q90")
    (a,) = E.JpegEncoder(0, quality=90, subsampling="gray").encode(_cuda(c["frame"])[None]).result()
    (b,) = E.JpegEncoder(0, quality=90).encode(_cuda(c["frame"])[None], subsampling="gray").result()
    assert a == b == c["file"]


def test_the_old_fixture_between_neighbours_of_other_layouts(golden_dir, cases):
    """The 60 cases of jpeg_encode.npz, each followed by a case of another layout, in one call: the 4:2:0 files are still theirs, so a
    neighbour's geometry does not leak through start[]."""
    d = np.load(f"{golden_dir}/jpeg_encode.npz")
    old = [dict(frame=d[f"in_{f}"], quality=int(q), file=d[f"file_{n}"].tobytes(), name=str(n), mode=None)
           for n, f, q, r in zip(d["names"], d["frames"], d["quality"], d["restart_rows"]) if int(r) == 0]
    assert len(old) >= 58
    others = [c for c in cases if c["restart_rows"] == 0 and c["mode"] != "4:2:0"]
    mixed = []
    for k, c in enumerate(old):
        mixed += [c, others[(k * 7) % len(others)]]
    assert {c["mode"] for c in mixed} == {None, "4:2:2", "4:4:4", "gray"}
    got = E.JpegEncoder(0).encode([_cuda(c["frame"]) for c in mixed], [c["quality"] for c in mixed],
                                  [c["mode"] or "4:2:0" for c in mixed]).result()
    for c, data in zip(mixed, got):
        assert data == c["file"], c["name"]


# (H, W), restart_rows: 137 x 201 has 234 MCUs in 4:2:2, a multiple of the six of a transform workgroup, so that layout takes 145 x 201
WIDE = {"4:2:0": ((137, 201), 1), "4:2:2": ((145, 201), 2), "4:4:4": ((137, 201), 2), "gray": ((201, 233), 2)}


@pytest.mark.parametrize("mode", MODES)
def test_an_image_that_spans_workgroups_chunks_and_segments(mode):
    (H, W), rows = WIDE[mode]
    rgb = np.random.default_rng(11).integers(0, 256, (H, W) if mode == "gray" else (H, W, 3), dtype=np.uint8)
    want = E.jpeg_encode_host(rgb, 100, rows, subsampling=mode)
    mcus = -(-W // MCU[mode][0]) * -(-H // MCU[mode][1])
    blocks = mcus * BLOCKS[mode]
    assert blocks > 2 * train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS and blocks % train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS
    assert mcus % (24 // BLOCKS[mode]) and 24 // BLOCKS["4:2:0"] == train_abi.FEAR_JPEG_ENC_MCUS
    hd = _parse(want)
    stuffed = want[hd.scan:].count(b"\xFF\x00")
    markers = -(-mcus // hd.restart) - 1
    assert len(want) - hd.scan - 2 - stuffed - 2 * markers > 3 * train_abi.FEAR_JPEG_ENC_CHUNK_BYTES and markers + 1 >= 9 and stuffed >= 3
    enc = E.JpegEncoder(0, quality=100, restart_rows=rows, subsampling=mode)
    frame = _cuda(rgb)
    first = enc.encode([frame])
    second = enc.encode(frame[None])                           # the same call twice, as one batch tensor
    (a,), (b,) = first.result(), second.result()
    assert a == want and b == want
    n = len(want)
    assert torch.equal(first.buffer[:n], second.buffer[:n]) and torch.equal(first.lengths, second.lengths)
    dec = JpegDecoder(device=0, entropy="device")
    (px,) = dec.decode([a], check=True)
    np.testing.assert_array_equal(px.cpu().numpy(), jpeg_decode_host(a))
    dec.close()


@pytest.mark.parametrize("mode", NEW)
def test_257_segments_of_one_mcu(mode):
    """The scan over an image's segments takes two rounds of 256, and a marker stands in front of all but one."""
    tall = np.random.default_rng(12).integers(0, 256, (2050, 8) if mode == "gray" else (2050, 8, 3), dtype=np.uint8)
    want = E.jpeg_encode_host(tall, 60, 1, subsampling=mode)
    hd = _parse(want)
    assert hd.restart == 1 and hd.mcus_x * hd.mcus_y == 257
    (d,) = E.JpegEncoder(0, quality=60, restart_rows=1).encode([_cuda(tall)], subsampling=mode).result()
    assert d == want


def test_the_smallest_and_the_tallest_frame():
    rng = np.random.default_rng(13)
    for H, W in ((1, 1), (8192, 1)):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        frames = [_cuda(rgb)] * 4 + [_cuda(rgb[..., 0])]
        modes = list(MODES) + ["gray"]
        got = E.JpegEncoder(0, quality=85).encode(frames, subsampling=modes).result()
        for k, mode in enumerate(modes):
            assert got[k] == E.jpeg_encode_host(rgb if k < 4 else rgb[..., 0], 85, subsampling=mode), (H, W, mode, k)


@pytest.mark.parametrize("mode", NEW)
def test_overflow_leaves_the_neighbours_and_the_guards_alone(cases, mode):
    by_name = {c["name"]: c for c in cases}
    tag = mode.replace(":", "")
    checker, left, right = by_name[f"{tag}_checker_q100"], by_name[f"{tag}_8x8_q50"], by_name[f"{tag}_5x7_q90"]
    slot, guard = len(checker["file"]) - 1, 48                 # one byte short of the checkerboard's file
    assert len(left["file"]) <= slot and len(right["file"]) <= slot
    enc = E.JpegEncoder(0, slot_bytes=slot, guard_bytes=guard, subsampling=mode)
    pending = enc.encode([_cuda(left["frame"]), _cuda(checker["frame"]), _cuda(right["frame"])], [50, 100, 90])
    with pytest.raises(E.JpegOverflow) as err:
        pending.result()
    assert err.value.items == [1]
    lengths, status, offsets = pending.lengths.cpu().tolist(), pending.status.cpu().tolist(), pending.offsets.cpu().tolist()
    assert lengths == [len(left["file"]), 0, len(right["file"])] and status == [0, E.ENC_OVERFLOW, 0]
    buf = pending.buffer.cpu().numpy()
    for k, c in ((0, left), (2, right)):
        assert buf[offsets[k]:offsets[k] + lengths[k]].tobytes() == c["file"]
        assert (buf[offsets[k] + lengths[k]:offsets[k] + slot] == 0xA5).all()          # nothing behind the file's end
    assert (buf[offsets[1]:offsets[1] + slot] == 0xA5).all()                           # nothing of the file that does not fit
    for k in range(3):
        end = offsets[k + 1] if k < 2 else len(buf)
        assert end - offsets[k] >= slot + guard and (buf[offsets[k] + slot:end] == 0xA5).all()
    # the exact length fits, and so does the bound of the layout
    for fits in (slot + 1, "bound"):
        (data,) = E.JpegEncoder(0, slot_bytes=fits, subsampling=mode).encode([_cuda(checker["frame"])], 100).result()
        assert data == checker["file"]


def test_refusals():
    enc = E.JpegEncoder(0)
    rgb = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    plane = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    for bad in ("4:1:1", "Gray", 2):
        with pytest.raises(ValueError):
            enc.encode([rgb], subsampling=bad)
    with pytest.raises(ValueError):
        enc.encode([rgb], subsampling=["4:4:4", "nope"])
    with pytest.raises(ValueError):
        E.JpegEncoder(0, subsampling="4:1:1")
    with pytest.raises(ValueError):
        enc.encode([rgb, rgb], subsampling=["4:4:4"])          # one name per frame
    with pytest.raises(ValueError):
        enc.encode([rgb], subsampling=["4:4:4", "gray"])
    for mode in (None, "4:2:0", "4:2:2", "4:4:4"):
        with pytest.raises(ValueError):
            enc.encode([plane], subsampling=mode)              # (H, W) only with "gray"
        with pytest.raises(ValueError):
            enc.encode(plane[None], subsampling=mode)          # and so is a batch (n, H, W)
    with pytest.raises(ValueError):
        enc.encode(torch.stack([plane, plane]), subsampling=["gray", "4:4:4"])
    with pytest.raises(ValueError):
        enc.encode([torch.zeros((8, 8, 2), dtype=torch.uint8, device="cuda")], subsampling="gray")
    with pytest.raises(ValueError):
        enc.encode([torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")], subsampling="gray")
    with pytest.raises(TypeError):
        enc.encode([plane.float()], subsampling="gray")
    with pytest.raises(ValueError):
        enc.encode([torch.zeros((8, 16), dtype=torch.uint8, device="cuda")[:, ::2]], subsampling="gray")
    with pytest.raises(ValueError):
        enc.encode([plane.cpu()], subsampling="gray")
    assert enc.encode([], subsampling="gray").result() == [] and enc.encode([], subsampling=[]).result() == []


def test_track_draw_encode_444_keeps_the_outline():
    """Track, draw, encode and decode: on the outline's pixels the 4:4:4 file is closer to the drawn frame than the 4:2:0 file is."""
    from conftest import WEIGHTS
    from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARNetHIP
    rng = np.random.RandomState(4)
    clip = [rng.randint(112, 144, size=(120, 200, 3)).astype(np.uint8) for _ in range(2)]
    net = FEARNetHIP(WEIGHTS, device=0, max_batch=8)
    mt = FEARMultiTracker(net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    mt.add(_cuda(clip[0]), np.array([(150, 80, 60, 50)]), stream=0)
    frame = _cuda(clip[1])
    mt.submit([frame])
    mt.draw([frame], thickness=1)
    drawn = frame.cpu().numpy()
    outline = (drawn != clip[1]).any(axis=-1)
    assert outline.sum() >= 16
    files = E.JpegEncoder(0, quality=90).encode([frame, frame], subsampling=["4:4:4", "4:2:0"]).result()
    assert files[0] == E.jpeg_encode_host(drawn, 90, subsampling="4:4:4") and files[1] == E.jpeg_encode_host(drawn, 90)
    dec = JpegDecoder(device=0)
    back = [b.cpu().numpy() for b in dec.decode(files)]
    dec.close()
    np.testing.assert_array_equal(back[0], jpeg_decode_host(files[0]))
    err = [np.abs(b[outline].astype(np.int64) - drawn[outline].astype(np.int64)).mean() for b in back]
    print("mean absolute error on the outline: 4:4:4", err[0], "4:2:0", err[1])
    assert err[0] < err[1]
