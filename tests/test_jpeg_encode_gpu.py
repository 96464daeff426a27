"""fear_jpeg_encode_u8 through JpegEncoder on the GPU, held to Pillow's files (tests/golden/jpeg_encode.npz) and to
jpeg_encode.jpeg_encode_host byte for byte ("Writing JPEG files")."""
import numpy as np
import pytest
import torch

from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import JpegDecoder, jpeg_decode_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden_dir):
    d = np.load(f"{golden_dir}/jpeg_encode.npz")
    return [dict(name=str(n), rgb=d[f"in_{f}"], quality=int(q), restart_rows=int(r), file=d[f"file_{n}"].tobytes())
            for n, f, q, r in zip(d["names"], d["frames"], d["quality"], d["restart_rows"])]


def _cuda(rgb):
    return torch.from_numpy(np.ascontiguousarray(rgb)).cuda()


def test_every_fixture_case_in_one_call(cases):
    """Mixed sizes and per-image qualities in one call: Pillow's bytes, which are jpeg_encode_host's (tests/test_jpeg_encode_host.py)."""
    plain = [c for c in cases if c["restart_rows"] == 0]
    assert len(plain) >= 58
    enc = E.JpegEncoder(0)
    frames = [_cuda(c["rgb"]) for c in plain]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # encode never waits
    try:
        pending = enc.encode(frames, [c["quality"] for c in plain])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = pending.result()
    for c, data in zip(plain, got):
        assert data == c["file"], c["name"]
    assert pending.lengths.cpu().tolist() == [len(c["file"]) for c in plain]
    assert pending.buffer.dtype == torch.uint8 and pending.offsets.dtype == torch.int64 and pending.offsets.is_cuda
    # the restart cases: the interval is the encoder's, so each distinct restart_rows is a call of its own
    for rows in sorted({c["restart_rows"] for c in cases} - {0}):
        some = [c for c in cases if c["restart_rows"] == rows]
        got = E.JpegEncoder(0, restart_rows=rows).encode([_cuda(c["rgb"]) for c in some], [c["quality"] for c in some]).result()
        for c, data in zip(some, got):
            assert data == c["file"] == E.jpeg_encode_host(c["rgb"], c["quality"], rows), c["name"]


@pytest.fixture(scope="module")
def wide():
    """Noise at quality 95, sized from the operator's constants: 9 x 13 MCUs are 702 blocks — three workgroups of the sizes and write
    passes, the last one partly filled; 30 transform workgroups, the last with one MCU; about 33 KB of stream — nine chunks, every
    chunk border inside some block's codes; a restart interval of two MCU rows, so five segments of which the last is short."""
    rgb = np.random.default_rng(11).integers(0, 256, (137, 201, 3), dtype=np.uint8)
    data = E.jpeg_encode_host(rgb, 95, 2)
    blocks = 9 * 13 * 6
    assert 2 * train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS < blocks and blocks % train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS
    assert len(data) > 3 * train_abi.FEAR_JPEG_ENC_CHUNK_BYTES + 629 and (9 * 13) % train_abi.FEAR_JPEG_ENC_MCUS
    assert sum(data.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) >= 4 and data.count(b"\xFF\x00") >= 3
    return rgb, data


def test_an_image_that_spans_workgroups_chunks_and_segments(wide):
    rgb, want = wide
    enc = E.JpegEncoder(0, quality=95, restart_rows=2)
    frame = _cuda(rgb)
    first = enc.encode([frame])
    second = enc.encode(frame[None])                           # the same call twice, as one (n, H, W, 3) tensor
    (a,), (b,) = first.result(), second.result()
    assert a == want and b == want
    n = len(want)
    assert torch.equal(first.buffer[:n], second.buffer[:n]) and torch.equal(first.lengths, second.lengths)
    # and the device's own decoder reads the file as the host statement does
    dec = JpegDecoder(device=0, entropy="device")
    (px,) = dec.decode([a], check=True)
    np.testing.assert_array_equal(px.cpu().numpy(), jpeg_decode_host(a))
    dec.close()
    # without an interval the whole scan is one segment, scanned by one workgroup in three rounds
    (c,) = E.JpegEncoder(0, quality=95).encode([frame]).result()
    assert c == E.jpeg_encode_host(rgb, 95)
    # 257 segments of one MCU each: the scan over an image's segments takes two rounds of 256, and a marker stands in front of all but one
    tall = np.random.default_rng(12).integers(0, 256, (4100, 8, 3), dtype=np.uint8)
    (d,) = E.JpegEncoder(0, quality=60, restart_rows=1).encode([_cuda(tall)]).result()
    assert d == E.jpeg_encode_host(tall, 60, 1)


def test_overflow_leaves_the_neighbours_and_the_guards_alone(cases):
    by_name = {c["name"]: c for c in cases}
    checker, left, right = by_name["checker_q100"], by_name["8x8_q50"], by_name["5x7_q90"]
    slot, guard = 800, 48
    assert len(left["file"]) <= slot and len(right["file"]) <= slot < len(checker["file"])
    enc = E.JpegEncoder(0, slot_bytes=slot, guard_bytes=guard)
    pending = enc.encode([_cuda(left["rgb"]), _cuda(checker["rgb"]), _cuda(right["rgb"])], [50, 100, 90])
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
    # the bound is a slot that always fits
    (data,) = E.JpegEncoder(0, slot_bytes="bound").encode([_cuda(checker["rgb"])], 100).result()
    assert data == checker["file"]
    # a slot one byte short of the file, and one that fits exactly
    with pytest.raises(E.JpegOverflow):
        E.JpegEncoder(0, slot_bytes=len(checker["file"]) - 1).encode([_cuda(checker["rgb"])], 100).result()
    (data,) = E.JpegEncoder(0, slot_bytes=len(checker["file"])).encode([_cuda(checker["rgb"])], 100).result()
    assert data == checker["file"]


def test_empty_calls_and_refusals():
    enc = E.JpegEncoder(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        empty = enc.encode([])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert empty.result() == [] and len(empty) == 0 and empty.lengths.numel() == 0
    assert enc.encode(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda")).result() == []
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        enc.encode([good.float()])
    with pytest.raises(TypeError):
        enc.encode([np.zeros((8, 8, 3), dtype=np.uint8)])
    with pytest.raises(ValueError):
        enc.encode([torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError):
        enc.encode([torch.zeros((8, 16, 3), dtype=torch.uint8, device="cuda")[:, ::2]])
    with pytest.raises(ValueError):
        enc.encode([good.cpu()])
    with pytest.raises(ValueError):
        enc.encode(good)                                       # one tensor is a batch (n, H, W, 3)
    for q in (0, 101):
        with pytest.raises(ValueError):
            enc.encode([good], q)
    with pytest.raises(ValueError):
        enc.encode([good], [75, 75])
    with pytest.raises(TypeError):
        enc.encode([good], 75.0)


def test_track_draw_encode_decode():
    """The demo loop's last stage: frames marked by FEARMultiTracker.draw are encoded, and what JpegDecoder reads back from the files is
    what the host statements say of the drawn frames."""
    from conftest import WEIGHTS
    from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARNetHIP
    rng = np.random.RandomState(4)
    clip = [[rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8) for _ in range(2)] for _ in range(2)]
    net = FEARNetHIP(WEIGHTS, device=0, max_batch=8)
    mt = FEARMultiTracker(net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    mt.add(_cuda(clip[0][0]), np.array([(150, 80, 60, 50)]), stream=0)
    mt.add(_cuda(clip[1][0]), np.array([(40, 30, 50, 40)]), stream=1)
    frames = [_cuda(clip[0][1]), _cuda(clip[1][1])]
    mt.submit(frames)
    mt.draw(frames, thickness=3)
    files = E.JpegEncoder(0, quality=80).encode(frames).result()
    drawn = [f.cpu().numpy() for f in frames]
    assert (drawn[0] != clip[0][1]).any() and (drawn[1] != clip[1][1]).any()
    dec = JpegDecoder(device=0)
    back = dec.decode(files)
    for k in range(2):
        assert files[k] == E.jpeg_encode_host(drawn[k], 80)
        np.testing.assert_array_equal(back[k].cpu().numpy(), jpeg_decode_host(files[k]))
    dec.close()
