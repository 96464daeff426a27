"""The JPEG encoder's other layouts on the host — 4:2:2, 4:4:4 and gray beside 4:2:0 (feartracker_amd/jpeg_encode.py; DESIGN.md
section 14, "Writing JPEG files") — held to the files Pillow's libjpeg-turbo wrote into tests/golden/jpeg_encode_modes.npz
(tools/make_jpeg_encode_modes_golden.py).  No GPU, and no Pillow except in the one live comparison, which is skipped without it."""
import ctypes
import os

import numpy as np
import pytest

import feartracker_amd
from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import _Bits, _extend, _parse, jpeg_coefficients_host, jpeg_decode_host

MODES = ("4:2:0", "4:2:2", "4:4:4", "gray")
MODE_ID = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "gray": 3}
MCU = {"4:2:0": (16, 16), "4:2:2": (16, 8), "4:4:4": (8, 8), "gray": (8, 8)}          # (width, height)
SLOT_FACTOR = {"4:2:0": 3, "4:2:2": 4, "4:4:4": 6, "gray": 3}
OK, NULL, SHAPE, WORKSPACE = 0, -1, -2, -7


def load_cases(golden_dir):
    d = np.load(f"{golden_dir}/jpeg_encode_modes.npz")
    out = []
    for k, name in enumerate(d["names"]):
        frame, plane = d[f"in_{d['frames'][k]}"], int(d["plane"][k])
        out.append(dict(name=str(name), mode=str(d["modes"][k]), frame=frame if plane < 0 else np.ascontiguousarray(frame[..., plane]),
                        quality=int(d["quality"][k]), restart_rows=int(d["restart_rows"][k]),
                        file=d["files"][int(d["file_at"][k]):int(d["file_at"][k + 1])].tobytes()))
    return out


@pytest.fixture(scope="module")
def cases(golden_dir):
    assert os.path.getsize(f"{golden_dir}/jpeg_encode_modes.npz") < 256 * 1024
    return load_cases(golden_dir)


def _scan_facts(data):
    """What the entropy-coded part of a file of any layout exhibits: a walk over the scan with the parser's tables (T.81 F.2)."""
    hd = _parse(data)
    scan = data[hd.scan:]
    n = len(hd.h)
    facts = dict(stuffed=scan.count(b"\xFF\x00"), markers=sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8)), zrl=0, no_eob=0,
                 dc_category=0, ac_max=0, components=n, blocks_per_mcu=sum(hd.h[c] * hd.v[c] for c in range(n)) if n > 1 else 1)
    bits = _Bits(data, hd.scan)
    for mcu in range(hd.mcus_x * hd.mcus_y):
        if hd.restart and mcu and mcu % hd.restart == 0:
            bits.restart((mcu // hd.restart - 1) & 7)
        for c in range(n):
            for _ in range(hd.h[c] * hd.v[c] if n > 1 else 1):
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


def _sof_sampling(data):
    at = data.index(b"\xFF\xC0")
    n = data[at + 9]
    return n, [data[at + 11 + 3 * c] for c in range(n)]


def test_the_fixture_exhibits_every_rule(cases):
    """A regenerated fixture cannot silently lose a case: each property the cases were chosen for is asserted on Pillow's own files."""
    for mode in MODES:
        mine = [c for c in cases if c["mode"] == mode]
        by_name = {c["name"].split("_", 1)[1]: c for c in mine}
        sizes = {c["frame"].shape[:2] for c in mine}
        assert {(1, 1), (5, 7), (8, 8), (16, 16), (9, 17), (40, 23), (23, 40), (31, 33), (70, 50)} <= sizes
        assert {c["quality"] for c in mine} >= {1, 10, 50, 90, 100}
        f = _scan_facts(by_name["noise_q100"]["file"])
        assert f["stuffed"] >= 10 and f["no_eob"] >= 10
        assert (f["components"], f["blocks_per_mcu"]) == {"4:2:0": (3, 6), "4:2:2": (3, 4), "4:4:4": (3, 3), "gray": (1, 1)}[mode]
        assert _scan_facts(by_name["noise_q10"]["file"])["zrl"] >= 1
        f = _scan_facts(by_name["columns_q100"]["file"])
        assert f["dc_category"] == 11 and f["stuffed"] >= 1
        c = by_name["checker_q100"]
        assert _scan_facts(c["file"])["ac_max"] >= 512 and len(c["file"]) > c["frame"].size // (1 if mode == "gray" else 3)
        for name, rows in (("restart1_31x33", 1), ("restart2_70x50", 2)):
            c = by_name[name]
            hd = _parse(c["file"])
            H, W = c["frame"].shape[:2]
            mcus_x, mcus_y = -(-W // MCU[mode][0]), -(-H // MCU[mode][1])
            assert c["restart_rows"] == rows and hd.restart == rows * mcus_x
            assert _scan_facts(c["file"])["markers"] >= -(-mcus_y // rows) - 1 >= 1
        # the DRI value on 31 x 33 and the header lengths, with and without DRI
        assert _parse(by_name["restart1_31x33"]["file"]).restart == {"4:2:0": 3, "4:2:2": 3, "4:4:4": 5, "gray": 5}[mode]
        plain, dri = (623, 629) if mode != "gray" else (328, 334)
        for c in mine:
            assert _parse(c["file"]).scan == (dri if c["restart_rows"] else plain), c["name"]
            n, sampling = _sof_sampling(c["file"])
            assert (n, sampling[0]) == {"4:2:0": (3, 0x22), "4:2:2": (3, 0x21), "4:4:4": (3, 0x11), "gray": (1, 0x11)}[mode]
            assert c["file"].count(b"\xFF\xDB") >= (1 if mode == "gray" else 2) and all(s == 0x11 for s in sampling[1:])
        if mode == "gray":
            assert all(c["file"][:328].count(b"\xFF\xC4\x00") == 2 for c in mine if not c["restart_rows"])
            rgb = [c for c in mine if c["frame"].ndim == 3]
            assert len(rgb) >= 2 and any(c["restart_rows"] for c in rgb) and sum(c["frame"].ndim == 2 for c in mine) >= 40
        else:
            assert all(c["frame"].ndim == 3 for c in mine)
        if mode == "4:2:2":
            widths, heights = {w for _, w in sizes}, {h for h, _ in sizes}
            assert any(-(-w // 8) % 2 for w in widths), "a dummy Y1 in the last MCU column"
            assert any(-(-w // 8) % 2 == 0 for w in widths) and any(w % 2 for w in widths) and any(h % 8 for h in heights)


def test_encode_host_equals_pillow_byte_for_byte(cases):
    for c in cases:
        got = E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling=c["mode"])
        assert got == c["file"], c["name"]


def test_the_parts_equal_the_files_parts(cases):
    """Header, coefficients and scan each on their own."""
    for c in cases:
        data, mode = c["file"], c["mode"]
        hd, want = jpeg_coefficients_host(data)
        H, W = c["frame"].shape[:2]
        assert E.jpeg_header_host(W, H, c["quality"], hd.restart, subsampling=mode) == data[:hd.scan], c["name"]
        got = E.jpeg_forward_coefficients_host(c["frame"], c["quality"], subsampling=mode)
        assert len(got) == len(want) == (1 if mode == "gray" else 3)
        for k in range(len(want)):
            assert got[k].dtype == np.int16 and got[k].shape == want[k].shape == (hd.blocks_h[k], hd.blocks_w[k], 64)
            assert np.array_equal(got[k], want[k]), (c["name"], k)
        by, bx = -(-H // 8), -(-W // 8)
        luma = got[0]
        if mode == "4:2:2":                                   # the dummy rule: Y1 of the last MCU column when ceil(W / 8) is odd
            assert luma.shape[:2] == (by, 2 * -(-W // 16))
            if bx & 1:
                assert not luma[:, bx, 1:].any() and np.array_equal(luma[:, bx, 0], luma[:, bx - 1, 0]), c["name"]
        elif mode in ("4:4:4", "gray"):                       # no dummy blocks
            assert all(g.shape[:2] == (by, bx) for g in got)
        mcus_x, mcus_y = -(-W // MCU[mode][0]), -(-H // MCU[mode][1])
        assert (hd.mcus_x, hd.mcus_y) == (mcus_x, mcus_y)
        assert E.jpeg_entropy_encode_host(want, mcus_x, mcus_y, hd.restart, subsampling=mode) + b"\xFF\xD9" == data[hd.scan:], c["name"]


def test_every_mode_decodes():
    """The files are files the decoder's host statement reads, whole: every MCU of the scan and the EOI behind it."""
    x = np.random.default_rng(5).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    for mode in MODES:
        for rows in (0, 1):
            data = E.jpeg_encode_host(x, 85, rows, subsampling=mode)
            px = jpeg_decode_host(data)
            assert px.dtype == np.uint8 and px.shape[:2] == (29, 37), mode
            hd, coef = jpeg_coefficients_host(data)
            assert len(coef) == (1 if mode == "gray" else 3)


def test_gray_decodes_as_pillows_file_does(cases):
    for c in cases:
        if c["mode"] == "gray" and c["frame"].ndim == 2 and c["quality"] in (50, 100):
            got = jpeg_decode_host(E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling="gray"))
            assert np.array_equal(got, jpeg_decode_host(c["file"])), c["name"]


def test_the_default_is_todays_bytes(golden_dir):
    d = np.load(f"{golden_dir}/jpeg_encode.npz")
    for n, f, q, r in zip(d["names"], d["frames"], d["quality"], d["restart_rows"]):
        want = d[f"file_{n}"].tobytes()
        assert E.jpeg_encode_host(d[f"in_{f}"], int(q), int(r)) == want, n
        assert E.jpeg_encode_host(d[f"in_{f}"], int(q), int(r), subsampling="4:2:0") == want, n
        hd = _parse(want)
        assert E.jpeg_header_host(hd.width, hd.height, int(q), hd.restart) == want[:hd.scan]


@pytest.mark.parametrize("mode", MODES)
def test_live_comparison_with_pillow(mode):
    Image = pytest.importorskip("PIL.Image")
    import io
    x = np.random.default_rng().integers(0, 256, (29, 37, 3), dtype=np.uint8)
    buf = io.BytesIO()
    if mode == "gray":
        Image.fromarray(x).convert("L").save(buf, "JPEG", quality=83, restart_marker_rows=1)
    else:
        Image.fromarray(x).save(buf, "JPEG", quality=83, restart_marker_rows=1, subsampling={"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}[mode])
    assert E.jpeg_encode_host(x, 83, 1, subsampling=mode) == buf.getvalue()
    if mode == "gray":
        buf = io.BytesIO()
        Image.fromarray(x[..., 2].copy()).save(buf, "JPEG", quality=83, restart_marker_rows=1)
        assert E.jpeg_encode_host(x[..., 2].copy(), 83, 1, subsampling="gray") == buf.getvalue()


def test_argument_errors():
    x = np.zeros((8, 8, 3), dtype=np.uint8)
    for bad in ("4:1:1", "GRAY", 2, None):
        with pytest.raises(ValueError):
            E.jpeg_encode_host(x, 75, 0, subsampling=bad)
        with pytest.raises(ValueError):
            E.jpeg_header_host(8, 8, subsampling=bad)
    for mode in ("4:2:0", "4:2:2", "4:4:4"):
        with pytest.raises(ValueError):
            E.jpeg_encode_host(x[..., 0], subsampling=mode)   # (H, W) only with "gray"
    with pytest.raises(ValueError):
        E.jpeg_encode_host(x[..., :2], subsampling="gray")
    with pytest.raises(ValueError):
        E.JpegEncoder("cpu", subsampling="4:1:1")
    assert "SUBSAMPLINGS" in feartracker_amd.__all__ and feartracker_amd.SUBSAMPLINGS == MODES


def _record(mode, w=16, h=16, q=75, interval=0, cap=4096, header=623):
    rec = (train_abi.FearJpegEncImage * 1)()
    rec[0].src, rec[0].out, rec[0].header = 1 << 20, 1 << 24, 1 << 28
    rec[0].width, rec[0].height, rec[0].quality, rec[0].restart_interval, rec[0].out_cap, rec[0].header_bytes = w, h, q, interval, cap, header
    rec[0].sampling = mode
    return rec


def test_the_abi_without_a_gpu(cases):
    assert {"fear_jpeg_encode_header_mode", "fear_jpeg_encode_bound_mode"} <= set(train_abi.TRAIN_SYMBOLS)
    assert (train_abi.FEAR_JPEG_ENC_420, train_abi.FEAR_JPEG_ENC_422, train_abi.FEAR_JPEG_ENC_444, train_abi.FEAR_JPEG_ENC_GRAY) == (0, 1, 2, 3)
    assert ctypes.sizeof(train_abi.FearJpegEncImage) == 96
    lib = train_abi.load_train_library()
    out, used = (ctypes.c_uint8 * train_abi.FEAR_JPEG_ENC_HEADER_MAX)(), ctypes.c_size_t(0)
    old, old_used = (ctypes.c_uint8 * train_abi.FEAR_JPEG_ENC_HEADER_MAX)(), ctypes.c_size_t(0)
    for mode in MODES:
        for w, h, q, interval in ((1, 1, 1, 0), (640, 480, 75, 0), (8192, 8192, 100, 65535), (33, 31, 50, 3)):
            assert lib.fear_jpeg_encode_header_mode(w, h, q, interval, MODE_ID[mode], out, len(out), ctypes.byref(used)) == OK
            assert bytes(out[:used.value]) == E.jpeg_header_host(w, h, q, interval, subsampling=mode), (mode, w, h)
            if mode == "4:2:0":
                assert lib.fear_jpeg_encode_header(w, h, q, interval, old, len(old), ctypes.byref(old_used)) == OK
                assert bytes(old[:old_used.value]) == bytes(out[:used.value])
    for bad in (-1, 4, 0x103):
        assert lib.fear_jpeg_encode_header_mode(16, 16, 75, 0, bad, out, len(out), ctypes.byref(used)) == SHAPE
        assert lib.fear_jpeg_encode_bound_mode(16, 16, 0, bad) == 0
    assert lib.fear_jpeg_encode_header_mode(16, 16, 75, 0, 3, out, 100, ctypes.byref(used)) == WORKSPACE
    assert lib.fear_jpeg_encode_header_mode(16, 16, 75, 0, 3, None, len(out), ctypes.byref(used)) == NULL
    for c in cases:
        H, W = c["frame"].shape[:2]
        interval = c["restart_rows"] * -(-W // MCU[c["mode"]][0])
        assert lib.fear_jpeg_encode_bound_mode(W, H, interval, MODE_ID[c["mode"]]) >= len(c["file"]), c["name"]
    for w, h, interval in ((1, 1, 0), (33, 31, 3), (640, 480, 40), (8192, 8192, 65535)):
        assert lib.fear_jpeg_encode_bound_mode(w, h, interval, 0) == lib.fear_jpeg_encode_bound(w, h, interval)
    # the longest MCU per mode: 9952, 6636, 4978 and 1658 bits, and a byte of padding for the one segment
    for mode, bits, header in (("4:2:0", 9952, 623), ("4:2:2", 6636, 623), ("4:4:4", 4978, 623), ("gray", 1658, 328)):
        assert lib.fear_jpeg_encode_bound_mode(1, 1, 0, MODE_ID[mode]) == header + 2 * ((bits + 7) // 8 + 1) + 2


def test_plan_and_encode_refusals_without_a_gpu():
    lib = train_abi.load_train_library()
    fake = ctypes.c_void_p(4096)
    enc = lib.fear_jpeg_encode_u8
    GRAY_RGB = train_abi.FEAR_JPEG_ENC_GRAY_RGB
    work = {}
    for mode in (0, 1, 2, 3, 3 | GRAY_RGB):
        rec = _record(mode, w=40, h=24)
        assert lib.fear_jpeg_encode_plan(rec, 1) == OK and rec[0].sampling == mode          # a planned record keeps its mode
        need = lib.fear_jpeg_encode_workspace_bytes(rec, 1)
        blocks = {0: 3 * 2 * 6, 1: 3 * 3 * 4, 2: 5 * 3 * 3, 3: 5 * 3}[mode & 255]
        assert need >= 96 + blocks * 128 + rec[0].stream_cap and rec[0].work_offset == 96 + rec[0].stream_cap
        work[mode] = need
        changed = _record(mode, w=40, h=24)
        lib.fear_jpeg_encode_plan(changed, 1)
        changed[0].sampling = (mode + 1) & 3                                                # changed after planning
        assert enc(changed, 1, fake, 1 << 30, fake, fake, None) == SHAPE
    assert work[0] == work[1] < work[2] and work[3] < work[0] and work[3 | GRAY_RGB] == work[3]      # 36, 36, 45 and 15 blocks
    for bad in (4, 255, GRAY_RGB, 1 | GRAY_RGB, 0x203, 1 << 31):                            # an unknown mode
        rec = _record(bad)
        assert lib.fear_jpeg_encode_plan(rec, 1) == SHAPE and lib.fear_jpeg_encode_workspace_bytes(rec, 1) == 0
        assert enc(rec, 1, fake, 1 << 30, fake, fake, None) == SHAPE
    # an all-zero sampling is today's record: the same plan as a record that never heard of the field
    a, b = _record(0, w=70, h=50, interval=5), _record(0, w=70, h=50, interval=5)
    lib.fear_jpeg_encode_plan(a, 1)
    lib.fear_jpeg_encode_plan(b, 1)
    assert bytes(a) == bytes(b) and a[0].stream_cap == ((min(5 * 4 * 1244 + 4, 4096) + 4 + 15) & ~15)
    # the overlap check knows a plain gray source is W H bytes: a slot right behind it is fine, one inside it is not
    for mode, size in ((3, 40 * 24), (3 | GRAY_RGB, 40 * 24 * 3), (2, 40 * 24 * 3)):
        rec = _record(mode, w=40, h=24)
        rec[0].out = rec[0].src + size
        lib.fear_jpeg_encode_plan(rec, 1)
        assert enc(rec, 1, None, 0, fake, fake, None) == WORKSPACE                          # past the shape checks
        rec[0].out = rec[0].src + size - 1
        assert enc(rec, 1, None, 0, fake, fake, None) == SHAPE


def test_the_default_slot_holds_noise_at_quality_100():
    rng = np.random.default_rng(17)
    for H, W in ((64, 64), (137, 201)):
        for mode in MODES:
            mcu_w, mcu_h = MCU[mode]
            slot = 1024 + SLOT_FACTOR[mode] * (mcu_w * -(-W // mcu_w)) * (mcu_h * -(-H // mcu_h))
            shape = (H, W) if mode == "gray" else (H, W, 3)
            for frame in (rng.integers(0, 256, shape, dtype=np.uint8), (rng.integers(0, 2, shape) * 255).astype(np.uint8)):
                assert len(E.jpeg_encode_host(frame, 100, subsampling=mode)) < slot, (mode, H, W)
