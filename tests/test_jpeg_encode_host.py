"""The JPEG encoder's statement on the host (feartracker_amd/jpeg_encode.py; DESIGN.md section 14, "Writing JPEG files"), held to the
files Pillow's libjpeg-turbo wrote into tests/golden/jpeg_encode.npz (tools/make_jpeg_encode_golden.py).  No GPU, and no Pillow except
in the one live comparison, which is skipped without it."""
import ctypes
import struct

import numpy as np
import pytest

import feartracker_amd
from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import _parse, jpeg_coefficients_host, jpeg_decode_host
from feartracker_amd.train_data.jpeg import jpeg_roundtrip_u8_host


@pytest.fixture(scope="module")
def fixture(golden_dir):
    d = np.load(f"{golden_dir}/jpeg_encode.npz")
    return [dict(name=str(n), rgb=d[f"in_{f}"], quality=int(q), restart_rows=int(r), file=d[f"file_{n}"].tobytes())
            for n, f, q, r in zip(d["names"], d["frames"], d["quality"], d["restart_rows"])], d


def _scan_facts(data):
    """What the entropy-coded part of a file exhibits: stuffed bytes, restart markers, ZRL symbols, blocks without an EOB, the largest DC
    category and the largest AC magnitude.  A plain walk over the scan with the parser's tables (T.81 F.2), counting symbols."""
    from feartracker_amd.jpeg_frames import _Bits, _extend
    hd = _parse(data)
    scan = data[hd.scan:]
    facts = dict(stuffed=scan.count(b"\xFF\x00"), markers=sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8)), zrl=0, no_eob=0,
                 dc_category=0, ac_max=0)
    bits = _Bits(data, hd.scan)
    for mcu in range(hd.mcus_x * hd.mcus_y):
        if hd.restart and mcu and mcu % hd.restart == 0:
            bits.restart((mcu // hd.restart - 1) & 7)
        for c in range(3):
            for _ in range(hd.h[c] * hd.v[c]):
                t = bits.symbol(hd.dc[hd.td[c]])
                facts["dc_category"] = max(facts["dc_category"], t)
                bits.bits(t)
                k = 1
                while k < 64:
                    rs = bits.symbol(hd.ac[hd.ta[c]])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        facts["zrl"] += 1
                        k += 16
                        continue
                    k += r
                    facts["ac_max"] = max(facts["ac_max"], abs(_extend(bits.bits(s), s)))
                    k += 1
                else:
                    facts["no_eob"] += 1
    return facts


def test_the_fixture_exhibits_every_rule(fixture):
    """A regenerated fixture cannot silently lose a case: each property the cases were chosen for is asserted on Pillow's own files."""
    cases, d = fixture
    by_name = {c["name"]: c for c in cases}
    sizes = {c["rgb"].shape[:2] for c in cases}
    assert {(1, 1), (5, 7), (8, 8), (16, 16), (9, 17), (40, 23), (23, 40), (31, 33), (70, 50)} <= sizes
    assert {c["quality"] for c in cases} >= {1, 10, 50, 75, 90, 100}
    assert any(1 <= h % 16 <= 8 for h, _ in sizes), "a height whose last MCU row has one block row: the downsampled-row rule"
    assert any(-(-w // 8) % 2 for _, w in sizes) and any(-(-h // 8) % 2 for h, _ in sizes), "dummy blocks on both axes"
    f = _scan_facts(by_name["noise_q100"]["file"])
    assert f["stuffed"] >= 10 and f["no_eob"] >= 10
    assert _scan_facts(by_name["noise_q10"]["file"])["zrl"] >= 1
    f = _scan_facts(by_name["columns_q100"]["file"])
    assert f["dc_category"] == 11 and f["stuffed"] >= 1
    c = by_name["checker_q100"]
    assert _scan_facts(c["file"])["ac_max"] >= 512 and len(c["file"]) > c["rgb"].size
    for name, rows in (("restart1_31x33", 1), ("restart2_70x50", 2)):
        c = by_name[name]
        hd = _parse(c["file"])
        assert c["restart_rows"] == rows and hd.restart == rows * hd.mcus_x
        assert _scan_facts(c["file"])["markers"] >= -(-hd.mcus_y // rows) - 1 >= 1
    # the four standard tables, as every file carries them, are the module's
    for (tc, th), (counts, values) in E.STD_HUFFMAN.items():
        assert bytes(d[f"dht_{tc}{th}_counts"]) == bytes(counts) and bytes(d[f"dht_{tc}{th}_values"]) == values


def test_encode_host_equals_pillow_byte_for_byte(fixture):
    for c in fixture[0]:
        got = E.jpeg_encode_host(c["rgb"], c["quality"], c["restart_rows"])
        assert got == c["file"], c["name"]


def test_the_parts_equal_the_files_parts(fixture):
    """Header, coefficients and scan each on their own: the coefficients read back from Pillow's file are the forward transform's on the
    real blocks, and the rest follow the dummy rule."""
    for c in fixture[0]:
        data = c["file"]
        hd, want = jpeg_coefficients_host(data)
        H, W = c["rgb"].shape[:2]
        assert E.jpeg_header_host(W, H, c["quality"], hd.restart) == data[:hd.scan], c["name"]
        got = E.jpeg_forward_coefficients_host(c["rgb"], c["quality"])
        for k in range(3):
            assert got[k].dtype == np.int16 and got[k].shape == want[k].shape == (hd.blocks_h[k], hd.blocks_w[k], 64)
            assert np.array_equal(got[k], want[k]), (c["name"], k)
        by, bx = -(-H // 8), -(-W // 8)
        luma = got[0]
        for j in range(luma.shape[0]):
            for i in range(luma.shape[1]):
                if j >= by or i >= bx:
                    order = [(j & ~1, i & ~1), (j & ~1, i | 1), (j | 1, i & ~1), (j | 1, i | 1)]
                    before = order[order.index((j, i)) - 1]
                    assert not luma[j, i, 1:].any() and luma[j, i, 0] == luma[before][0], (c["name"], j, i)
        assert E.jpeg_entropy_encode_host(want, hd.mcus_x, hd.mcus_y, hd.restart) + b"\xFF\xD9" == data[hd.scan:], c["name"]


def test_encode_then_decode_is_the_image_compression_round_trip():
    """Ties the encoder to the ImageCompression contract already held to Pillow (which reads channel 0 as B)."""
    x = np.random.default_rng(5).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    for q in (35, 90):
        assert np.array_equal(jpeg_decode_host(E.jpeg_encode_host(x, q)), jpeg_roundtrip_u8_host(x[..., ::-1], q)[..., ::-1])


def test_live_comparison_with_pillow():
    Image = pytest.importorskip("PIL.Image")
    import io
    x = np.random.default_rng().integers(0, 256, (29, 37, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "JPEG", quality=83, restart_marker_rows=1)
    assert E.jpeg_encode_host(x, 83, 1) == buf.getvalue()


def test_argument_errors():
    x = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(TypeError):
        E.jpeg_encode_host(x.astype(np.float32))
    with pytest.raises(ValueError):
        E.jpeg_encode_host(x[..., :2])
    with pytest.raises(ValueError):
        E.jpeg_encode_host(np.zeros((0, 8, 3), dtype=np.uint8))
    for q in (0, 101):
        with pytest.raises(ValueError):
            E.jpeg_encode_host(x, q)
        with pytest.raises(ValueError):
            E.jpeg_header_host(8, 8, q)
    with pytest.raises(TypeError):
        E.jpeg_encode_host(x, 75.0)
    with pytest.raises(ValueError):
        E.jpeg_encode_host(x, 75, -1)
    with pytest.raises(ValueError):
        E.jpeg_header_host(0, 8)
    with pytest.raises(ValueError):
        E.jpeg_header_host(8, 8, 75, 65536)


def _record(lib, w=16, h=16, q=75, interval=0, cap=4096):
    rec = (train_abi.FearJpegEncImage * 1)()
    rec[0].src, rec[0].out, rec[0].header = 1 << 20, 1 << 24, 1 << 28
    rec[0].width, rec[0].height, rec[0].quality, rec[0].restart_interval, rec[0].out_cap, rec[0].header_bytes = w, h, q, interval, cap, 623
    return rec


def test_symbols_and_statuses_that_need_no_gpu(fixture):
    names = {"fear_jpeg_encode_header", "fear_jpeg_encode_bound", "fear_jpeg_encode_plan", "fear_jpeg_encode_workspace_bytes", "fear_jpeg_encode_u8"}
    assert names <= set(train_abi.TRAIN_SYMBOLS)
    for name in ("JpegEncoder", "JpegOverflow", "PendingJpegs", "jpeg_encode_host"):
        assert name in feartracker_amd.__all__ and hasattr(feartracker_amd, name)
    assert issubclass(feartracker_amd.JpegOverflow, ValueError)
    assert (train_abi.FEAR_JPEG_ENC_GROUP_BLOCKS, train_abi.FEAR_JPEG_ENC_CHUNK_BYTES) == (256, 4096)
    lib = train_abi.load_train_library()
    OK, NULL, SHAPE, WORKSPACE = 0, -1, -2, -7
    fake = ctypes.c_void_p(4096)
    enc = lib.fear_jpeg_encode_u8
    assert enc(None, 0, None, 0, None, None, None) == OK
    assert enc(None, -1, None, 0, None, None, None) == SHAPE and enc(None, 65536, None, 0, None, None, None) == SHAPE
    rec = _record(lib)
    assert lib.fear_jpeg_encode_plan(rec, 1) == OK and lib.fear_jpeg_encode_plan(None, 1) == NULL and lib.fear_jpeg_encode_plan(None, 0) == OK
    need = lib.fear_jpeg_encode_workspace_bytes(rec, 1)
    assert need >= 96 + 6 * 128 + rec[0].stream_cap and rec[0].stream_offset == 96 and rec[0].work_offset == 96 + rec[0].stream_cap
    assert enc(None, 1, fake, need, fake, fake, None) == NULL and enc(rec, 1, fake, need, None, fake, None) == NULL
    assert enc(rec, 1, fake, need, fake, None, None) == NULL
    assert enc(rec, 1, None, need, fake, fake, None) == WORKSPACE and enc(rec, 1, fake, need - 1, fake, fake, None) == WORKSPACE
    for field in ("src", "out", "header"):
        bad = _record(lib)
        lib.fear_jpeg_encode_plan(bad, 1)
        setattr(bad[0], field, 0)
        assert enc(bad, 1, fake, need, fake, fake, None) == NULL
    for change in (dict(w=0), dict(w=8193), dict(h=0), dict(h=8193), dict(q=0), dict(q=101), dict(interval=-1), dict(interval=65536)):
        bad = _record(lib, **change)
        assert lib.fear_jpeg_encode_plan(bad, 1) == SHAPE and lib.fear_jpeg_encode_workspace_bytes(bad, 1) == 0
        assert enc(bad, 1, fake, 1 << 30, fake, fake, None) == SHAPE
    bad = _record(lib)                                        # a record that was not planned
    assert enc(bad, 1, fake, need, fake, fake, None) == SHAPE
    bad = _record(lib)                                        # a source inside the slot
    lib.fear_jpeg_encode_plan(bad, 1)
    bad[0].src = bad[0].out + 100
    assert enc(bad, 1, fake, need, fake, fake, None) == SHAPE
    # the header builder equals the Python statement; the bound covers every fixture file
    out, used = (ctypes.c_uint8 * train_abi.FEAR_JPEG_ENC_HEADER_MAX)(), ctypes.c_size_t(0)
    for w, h, q, interval in ((1, 1, 1, 0), (640, 480, 75, 0), (8192, 8192, 100, 65535), (33, 31, 50, 3)):
        assert lib.fear_jpeg_encode_header(w, h, q, interval, out, len(out), ctypes.byref(used)) == OK
        assert bytes(out[:used.value]) == E.jpeg_header_host(w, h, q, interval)
    assert lib.fear_jpeg_encode_header(16, 16, 75, 0, out, 100, ctypes.byref(used)) == WORKSPACE
    assert lib.fear_jpeg_encode_header(16, 16, 0, 0, out, len(out), ctypes.byref(used)) == SHAPE
    assert lib.fear_jpeg_encode_header(16, 16, 75, 0, None, len(out), ctypes.byref(used)) == NULL
    assert lib.fear_jpeg_encode_bound(0, 16, 0) == 0 and lib.fear_jpeg_encode_bound(16, 16, 65536) == 0
    for c in fixture[0]:
        H, W = c["rgb"].shape[:2]
        assert lib.fear_jpeg_encode_bound(W, H, c["restart_rows"] * -(-W // 16)) >= len(c["file"]), c["name"]


def test_front_end_refusals_that_need_no_gpu():
    with pytest.raises(ValueError):
        E.JpegEncoder("cpu", quality=0)
    with pytest.raises(ValueError):
        E.JpegEncoder("cpu", restart_rows=-1)
    with pytest.raises(TypeError):
        E.JpegEncoder("cpu", slot_bytes="raw")
    with pytest.raises(ValueError):
        E.JpegEncoder("cpu", slot_bytes=0)
    err = E.JpegOverflow([1, 4])
    assert err.items == [1, 4] and "1" in str(err)


def _chunks(data, at, end):
    out = []
    while at < end:
        tag, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        out.append((tag, at, size))
        at += 8 + size + (size & 1)
    assert at == end
    return out


def test_write_mjpeg_avi(tmp_path, fixture):
    rng = np.random.default_rng(3)
    made = [E.jpeg_encode_host(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), q) for q in range(30, 50)]
    files = [f for f in made if len(f) & 1][:2] + [f for f in made if not len(f) & 1][:2]         # two odd payloads, then two even ones
    assert len(files) == 4
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files), "both an odd and an even payload"
    path = tmp_path / "clip.avi"
    E.write_mjpeg_avi(path, files, 25)
    data = path.read_bytes()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hdrl_at, hdrl_size), (_, movi_at, movi_size), (_, idx_at, idx_size) = top
    assert data[hdrl_at + 8:hdrl_at + 12] == b"hdrl" and data[movi_at + 8:movi_at + 12] == b"movi"
    inner = _chunks(data, hdrl_at + 12, hdrl_at + 8 + hdrl_size)
    assert [t for t, _, _ in inner] == [b"avih", b"LIST"] and inner[0][2] == 56
    avih = struct.unpack("<14I", data[inner[0][1] + 8:inner[0][1] + 64])
    assert (avih[0], avih[4], avih[6], avih[8], avih[9]) == (40000, 4, 1, 40, 24) and avih[3] & 0x10
    strl_at, strl_size = inner[1][1], inner[1][2]
    assert data[strl_at + 8:strl_at + 12] == b"strl"
    strl = _chunks(data, strl_at + 12, strl_at + 8 + strl_size)
    assert [(t, s) for t, _, s in strl] == [(b"strh", 56), (b"strf", 40)]
    strh = data[strl[0][1] + 8:strl[0][1] + 64]
    assert strh[:8] == b"vidsMJPG" and struct.unpack("<II", strh[20:28]) == (1, 25) and struct.unpack("<I", strh[32:36])[0] == 4
    strf = data[strl[1][1] + 8:strl[1][1] + 48]
    assert struct.unpack("<Iii", strf[:12]) == (40, 40, 24) and strf[16:20] == b"MJPG"
    frames = _chunks(data, movi_at + 12, movi_at + 8 + movi_size)
    assert [t for t, _, _ in frames] == [b"00dc"] * 4
    assert idx_size == 16 * 4
    for k, f in enumerate(files):
        tag, flags, offset, size = struct.unpack("<4sIII", data[idx_at + 8 + 16 * k:idx_at + 24 + 16 * k])
        at = movi_at + 8 + offset                             # offsets count from the 'movi' tag
        assert tag == b"00dc" and flags == 0x10 and size == len(f)
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == len(f) and data[at + 8:at + 8 + size] == f
        assert at % 2 == 0
    with pytest.raises(ValueError):
        E.write_mjpeg_avi(path, [], 25)
    with pytest.raises(ValueError):
        E.write_mjpeg_avi(path, [files[0], fixture[0][0]["file"]], 25)
    with pytest.raises(ValueError):
        E.write_mjpeg_avi(path, files, 0)
