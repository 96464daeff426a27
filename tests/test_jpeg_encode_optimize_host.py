"""Per-file Huffman tables ("Per-file Huffman tables") without a GPU: jpeg_encode.jpeg_encode_host(optimize=True)
and its stages against the files Pillow's libjpeg-turbo writes with optimize=True (tests/golden/jpeg_encode_optimize.npz, written by
tools/make_jpeg_encode_optimize_golden.py), and the host half of the C ABI against the statement."""
import ctypes
import io
import os

import numpy as np
import pytest

import feartracker_amd
from feartracker_amd import jpeg_encode as E
from feartracker_amd import train_abi
from feartracker_amd.jpeg_frames import _parse, jpeg_coefficients_host, jpeg_decode_host

MODES = ("4:2:0", "4:2:2", "4:4:4", "gray")
MODE_ID = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "gray": 3}
MCU = {"4:2:0": (16, 16), "4:2:2": (16, 8), "4:4:4": (8, 8), "gray": (8, 8)}
OK, NULL, SHAPE = 0, -1, -2
OPT = train_abi.FEAR_JPEG_ENC_OPTIMIZE
# the limit case's block counts: each exceeds the sum of all before it, so the unlimited tree is a chain
LIMIT_COUNTS = (1, 3, 3, 6, 9, 15, 24, 39, 63, 102, 165, 267, 432, 699, 1131, 1830, 2961, 4791, 7752, 12543)
LIMIT_AC_COUNTS = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 2, 0, 7)          # what Pillow's AC table of that file has


def load_cases(golden_dir):
    d = np.load(f"{golden_dir}/jpeg_encode_optimize.npz")
    out = []
    for k, name in enumerate(d["names"]):
        out.append(dict(name=str(name), mode=str(d["modes"][k]), frame=d[f"in_{d['frames'][k]}"], quality=int(d["quality"][k]),
                        restart_rows=int(d["restart_rows"][k]), file=d["files"][int(d["file_at"][k]):int(d["file_at"][k + 1])].tobytes()))
    return out


def limit_histogram():
    """The AC histogram of the limit case: EOB in every one of the 128 x 257 blocks and the 20 symbols of LIMIT_COUNTS."""
    freq = np.zeros(256, dtype=np.int64)
    freq[0] = 128 * 257
    symbols = [(k - 1) << 4 | size for size in (1, 2, 3) for k in range(1, 17)][:len(LIMIT_COUNTS)]
    freq[symbols] = LIMIT_COUNTS
    return freq


def deep_histogram():
    """Fibonacci-like counts on 40 symbols: a chain of depth 40, which libjpeg refuses."""
    freq, a, b = np.zeros(256, dtype=np.int64), 1, 2
    for s in range(40):
        freq[3 * s + 1] = a
        a, b = b, a + b
    return freq


def table_histograms():
    """The five histograms the table rule is held to, by name."""
    one = np.zeros(256, dtype=np.int64)
    one[7] = 5
    two = np.zeros(256, dtype=np.int64)
    two[[3, 200]] = 9
    return {"one": one, "two_equal": two, "all_ones": np.ones(256, dtype=np.int64), "limit": limit_histogram(), "deep": deep_histogram()}


def table_of_file(data, tc, th):
    """(counts, values) of a file's DHT segment of class tc and id th."""
    at = 2
    while data[at + 1] != 0xDA:
        size = data[at + 2] << 8 | data[at + 3]
        if data[at + 1] == 0xC4 and data[at + 4] == (tc << 4 | th):
            counts = tuple(data[at + 5:at + 21])
            return counts, data[at + 21:at + 21 + sum(counts)]
        at += 2 + size
    raise KeyError((tc, th))


@pytest.fixture(scope="module")
def cases(golden_dir):
    assert os.path.getsize(f"{golden_dir}/jpeg_encode_optimize.npz") < 256 * 1024
    return load_cases(golden_dir)


def test_the_fixture_has_every_case(cases):
    for mode in MODES:
        mine = {c["name"].split("_", 1)[1]: c for c in cases if c["mode"] == mode}
        assert {"1x1", "8x8", "13x17", "flat16", "restart1_31x33", "noise_q100", "noise_q1", "picture_q90"} <= set(mine)
        assert mine["restart1_31x33"]["restart_rows"] == 1 and mine["noise_q100"]["quality"] == 100 and mine["noise_q1"]["quality"] == 1
        assert mine["picture_q90"]["frame"].shape == (96, 128, 3) and mine["noise_q100"]["frame"].shape == (50, 70, 3)
        flat = mine["flat16"]["file"]                                       # one DC symbol and EOB only: two tables of one code
        for th in range(1 if mode == "gray" else 2):
            assert table_of_file(flat, 0, th)[0][0] == 1 and table_of_file(flat, 1, th) == ((1,) + (0,) * 15, b"\x00")
        for c in mine.values():
            data, std = c["file"], (328 if mode == "gray" else 623) + (6 if c["restart_rows"] else 0)
            assert data.count(b"\xFF\xC4") >= (2 if mode == "gray" else 4) and _parse(data).scan <= std, c["name"]
            if c["restart_rows"]:                                           # DRI follows the DHT segments
                assert data.index(b"\xFF\xDD\x00\x04") > data.rindex(b"\xFF\xC4", 0, _parse(data).scan)
    limit = next(c for c in cases if c["name"] == "gray_limit")
    assert limit["frame"].shape == (2056, 1024) and table_of_file(limit["file"], 1, 0)[0] == LIMIT_AC_COUNTS


def test_encode_host_equals_pillow_byte_for_byte(cases):
    for c in cases:
        got = E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling=c["mode"], optimize=True)
        assert got == c["file"], c["name"]
        if c["name"] != "gray_limit":                                       # and the plain file is what it was
            plain = E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling=c["mode"])
            assert plain == E.jpeg_encode_host(c["frame"], c["quality"], c["restart_rows"], subsampling=c["mode"], optimize=False)
            assert np.array_equal(jpeg_decode_host(got), jpeg_decode_host(plain)), c["name"]


def test_the_stages_equal_the_files_parts(cases):
    for c in cases:
        data, mode = c["file"], c["mode"]
        hd, coef = jpeg_coefficients_host(data)
        hist = E.jpeg_symbol_histograms_host(coef, hd.mcus_x, hd.mcus_y, hd.restart, subsampling=mode)
        assert hist.shape == (4, 256) and hist.dtype == np.int64
        blocks = sum(int(np.prod(p.shape[:2])) for p in coef) if mode in ("4:4:4", "gray") else None
        if blocks is not None:                                              # one DC symbol per block
            assert hist[0].sum() + hist[2].sum() == blocks
        tables = {}
        for tc, th in ((0, 0), (1, 0)) if mode == "gray" else ((0, 0), (1, 0), (0, 1), (1, 1)):
            counts, values, depth = E.jpeg_optimal_table_host(hist[2 * th + tc])
            assert (tuple(counts), bytes(values)) == table_of_file(data, tc, th), (c["name"], tc, th)
            assert set(values) == set(np.flatnonzero(hist[2 * th + tc]).tolist())
            tables[(tc, th)] = (counts, values)
            if c["name"] == "gray_limit" and tc == 1:
                assert depth == 21 > 16, "the case that forces the length limit"
        if mode == "gray":
            assert not hist[2:].any()
        H, W = c["frame"].shape[:2]
        assert E.jpeg_header_host(W, H, c["quality"], hd.restart, subsampling=mode, tables=tables) == data[:hd.scan], c["name"]
        assert E.jpeg_entropy_encode_host(coef, hd.mcus_x, hd.mcus_y, hd.restart, mode, tables) + b"\xFF\xD9" == data[hd.scan:]


def test_histograms_restart_the_dc_prediction():
    """With a restart interval the DC differences begin at 0 again, which changes the DC counts and nothing else."""
    x = np.random.default_rng(3).integers(0, 256, (40, 24), dtype=np.uint8)
    coef = E.jpeg_forward_coefficients_host(x, 75, "gray")
    whole = E.jpeg_symbol_histograms_host(coef, 3, 5, 0, "gray")
    rows = E.jpeg_symbol_histograms_host(coef, 3, 5, 3, "gray")
    assert np.array_equal(whole[1], rows[1]) and whole[0].sum() == rows[0].sum() == 15 and not np.array_equal(whole[0], rows[0])


def test_optimal_table_on_chosen_histograms():
    h = table_histograms()
    assert E.jpeg_optimal_table_host(h["one"]) == ((1,) + (0,) * 15, b"\x07", 1)
    # two equal symbols and the reserved one: the reserved symbol is merged first with the LARGER symbol, which gets the longer code
    assert E.jpeg_optimal_table_host(h["two_equal"]) == ((1, 1) + (0,) * 14, bytes([3, 200]), 2)
    counts, values, depth = E.jpeg_optimal_table_host(h["all_ones"])
    assert depth == 9 and counts == (0,) * 6 + (0, 255, 1) + (0,) * 7 and values == bytes(range(256))
    counts, values, depth = E.jpeg_optimal_table_host(h["limit"])
    assert depth == 21 and counts == LIMIT_AC_COUNTS and len(values) == 21 and values[0] == 0
    with pytest.raises(E.JpegHuffmanDepth):
        E.jpeg_optimal_table_host(h["deep"])
    assert E.jpeg_optimal_table_host(np.zeros(256, dtype=np.int64)) == ((0,) * 16, b"", 0)
    for bad in (np.zeros(255), -np.ones(256)):
        with pytest.raises(ValueError):
            E.jpeg_optimal_table_host(bad)
    # any table the rule gives is a prefix code that leaves the all-ones code unused
    rng = np.random.default_rng(8)
    for _ in range(20):
        freq = rng.integers(0, 1 << rng.integers(1, 20), 256) * (rng.random(256) < rng.random())
        counts, values, depth = E.jpeg_optimal_table_host(freq)
        assert sum(counts) == len(values) == np.count_nonzero(freq)
        assert sum(c * 2 ** (16 - n) for n, c in enumerate(counts, 1)) < 2 ** 16 or not len(values)


def test_live_comparison_with_pillow():
    Image = pytest.importorskip("PIL.Image")
    x = np.random.default_rng().integers(0, 256, (29, 37, 3), dtype=np.uint8)
    for mode in MODES:
        buf = io.BytesIO()
        if mode == "gray":
            Image.fromarray(x).convert("L").save(buf, "JPEG", quality=83, restart_marker_rows=1, optimize=True)
        else:
            Image.fromarray(x).save(buf, "JPEG", quality=83, restart_marker_rows=1, optimize=True,
                                    subsampling={"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}[mode])
        assert E.jpeg_encode_host(x, 83, 1, subsampling=mode, optimize=True) == buf.getvalue(), mode


def test_result_names_both_kinds_of_refused_item():
    """`result()` on a verdict with a refused tree and an overflow: `JpegHuffmanDepth` wins and carries the overflowing items too."""
    import torch
    buffer = torch.zeros(64, dtype=torch.uint8)
    for status, kind, items, overflow in (([0, 2, 1, 0], E.JpegHuffmanDepth, [1], [2]), ([2, 0], E.JpegHuffmanDepth, [0], []),
                                          ([0, 1], E.JpegOverflow, [1], None)):
        n = len(status)
        pending = E.PendingJpegs(buffer, torch.arange(n) * 16, torch.zeros(n, dtype=torch.int32), torch.tensor(status, dtype=torch.int32),
                                 [16 * k for k in range(n)])
        with pytest.raises(kind) as err:
            pending.result()
        assert err.value.items == items and getattr(err.value, "overflow", None) == overflow
        assert not overflow or str(overflow) in str(err.value)


def _record(mode, flags=0, w=16, h=16, q=75, interval=0, cap=4096, header=623):
    rec = (train_abi.FearJpegEncImage * 1)()
    rec[0].src, rec[0].out, rec[0].header = 1 << 20, 1 << 24, 1 << 28
    rec[0].width, rec[0].height, rec[0].quality, rec[0].restart_interval, rec[0].out_cap, rec[0].header_bytes = w, h, q, interval, cap, header
    rec[0].sampling, rec[0].flags = mode, flags
    return rec


def test_the_abi_without_a_gpu(cases):
    names = {"fear_jpeg_encode_header_flags", "fear_jpeg_encode_bound_flags", "fear_jpeg_huff_optimal"}
    assert names <= set(train_abi.TRAIN_SYMBOLS)
    assert ctypes.sizeof(train_abi.FearJpegEncImage) == 96 and train_abi.FearJpegEncImage.flags.offset == 92 and OPT == 1
    for name in ("JpegHuffmanDepth", "jpeg_symbol_histograms_host", "jpeg_optimal_table_host"):
        assert name in feartracker_amd.__all__ and hasattr(feartracker_amd, name)
    lib = train_abi.load_train_library()
    out, used = (ctypes.c_uint8 * train_abi.FEAR_JPEG_ENC_HEADER_MAX)(), ctypes.c_size_t(0)
    for mode in MODES:
        split = 102 if mode == "gray" else 177
        for w, h, q, interval in ((1, 1, 1, 0), (640, 480, 75, 0), (8192, 8192, 100, 65535), (33, 31, 50, 3)):
            whole = E.jpeg_header_host(w, h, q, interval, subsampling=mode)
            assert lib.fear_jpeg_encode_header_flags(w, h, q, interval, MODE_ID[mode], 0, out, len(out), ctypes.byref(used)) == OK
            assert bytes(out[:used.value]) == whole
            # an optimised record's header: the same bytes without the DHT segments, which stood at `split`
            assert lib.fear_jpeg_encode_header_flags(w, h, q, interval, MODE_ID[mode], OPT, out, len(out), ctypes.byref(used)) == OK
            bare = bytes(out[:used.value])
            dht = 216 if mode == "gray" else 432                                # the standard tables' segments
            assert bare == whole[:split] + whole[split + dht:] and whole[split:split + 2] == b"\xFF\xC4"
            assert bare[split:split + 2] == (b"\xFF\xDD" if interval else b"\xFF\xDA")
        assert lib.fear_jpeg_encode_header_flags(16, 16, 75, 0, MODE_ID[mode], 2, out, len(out), ctypes.byref(used)) == SHAPE
        assert lib.fear_jpeg_encode_bound_flags(16, 16, 0, MODE_ID[mode], 2) == 0
    # the bound: every block at 16 + 11 + 63 * 26 bits, a byte of padding for the one segment, every byte stuffed, the standard header
    # and the EOI; it is at least the plain bound, and at least every fixture file
    for mode, mcu_bits, header in (("4:2:0", 6 * 1665, 623), ("4:2:2", 4 * 1665, 623), ("4:4:4", 3 * 1665, 623), ("gray", 1665, 328)):
        assert lib.fear_jpeg_encode_bound_flags(8, 8, 0, MODE_ID[mode], OPT) == header + 2 * (-(-mcu_bits // 8) + 1) + 2
        for w, h, interval in ((1, 1, 0), (33, 31, 3), (640, 480, 40), (8192, 8192, 65535)):
            assert lib.fear_jpeg_encode_bound_flags(w, h, interval, MODE_ID[mode], 0) == lib.fear_jpeg_encode_bound_mode(w, h, interval, MODE_ID[mode])
            assert lib.fear_jpeg_encode_bound_flags(w, h, interval, MODE_ID[mode], OPT) > lib.fear_jpeg_encode_bound_mode(w, h, interval, MODE_ID[mode])
    for c in cases:
        H, W = c["frame"].shape[:2]
        interval = c["restart_rows"] * -(-W // MCU[c["mode"]][0])
        assert lib.fear_jpeg_encode_bound_flags(W, H, interval, MODE_ID[c["mode"]], OPT) >= len(c["file"]), c["name"]


def test_the_plan_without_a_gpu():
    lib = train_abi.load_train_library()
    for mode in MODES:
        header = 328 if mode == "gray" else 623
        plain = _record(MODE_ID[mode], 0, w=70, h=50, header=header)
        assert lib.fear_jpeg_encode_plan(plain, 1) == OK
        # a plain record's plan is what it was: its scratch directly behind its stream
        assert plain[0].flags == 0 and plain[0].work_offset == 96 + plain[0].stream_cap and plain[0].stream_offset == 96
        assert plain[0].plan_sampling == MODE_ID[mode] and list(plain[0].start) == [0, 0, 0, 0]
        opt = _record(MODE_ID[mode], OPT, w=70, h=50, header=header - (216 if mode == "gray" else 432))
        assert lib.fear_jpeg_encode_plan(opt, 1) == OK
        # the flags are kept; the counts stand in front of the stream, the tables behind the plain scratch
        assert opt[0].flags == OPT and opt[0].sampling == MODE_ID[mode] and opt[0].plan_sampling == (MODE_ID[mode] | OPT << 16)
        assert opt[0].stream_offset == 96 + 4096 and opt[0].work_offset == opt[0].stream_offset + opt[0].stream_cap
        assert opt[0].stream_cap == plain[0].stream_cap == (4096 + 4 + 15) & ~15          # (both are cut to the slot here)
        extra = lib.fear_jpeg_encode_workspace_bytes(opt, 1) - lib.fear_jpeg_encode_workspace_bytes(plain, 1)
        assert extra == 4096 + 4096 + 4 * 288 + 32
        # unknown bits, and flags changed after planning (fear_jpeg_encode_u8 refuses before it touches the device)
        for bad in (2, 3, 1 << 31):
            assert lib.fear_jpeg_encode_plan(_record(MODE_ID[mode], bad, header=header), 1) == SHAPE
            assert lib.fear_jpeg_encode_workspace_bytes(_record(MODE_ID[mode], bad, header=header), 1) == 0
        length, status = (ctypes.c_int32 * 1)(), (ctypes.c_int32 * 1)()
        for rec, new in ((plain, OPT), (opt, 0)):
            rec[0].flags = new
            assert lib.fear_jpeg_encode_u8(rec, 1, ctypes.c_void_p(1 << 30), 1 << 30, length, status, None) == SHAPE
        # an optimised record's header has to reach past the place of the DHT segments
        short = _record(MODE_ID[mode], OPT, header=102 if mode == "gray" else 177)
        assert lib.fear_jpeg_encode_plan(short, 1) == SHAPE
    # a plain record next to an optimised one keeps its grids: start[] counts workgroups, which the flag does not change
    pair = (train_abi.FearJpegEncImage * 2)()
    for k, flags in enumerate((OPT, 0)):
        src = _record(0, flags, w=70, h=50, header=623 - 432 * flags)[0]
        ctypes.memmove(ctypes.byref(pair[k]), ctypes.byref(src), 96)
    assert lib.fear_jpeg_encode_plan(pair, 2) == OK
    assert list(pair[1].start) == [-(-20 // 4), 1, 1, -(-pair[0].stream_cap // 4096)]
    assert pair[1].stream_offset == pair[0].stream_offset + pair[0].stream_cap     # no counts in front of a plain stream
