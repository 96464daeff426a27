"""Plumbing shared by the JPEG frame decoder's tests (test_jpeg_decode_host, test_jpeg_decode_gpu): the fixture
tests/golden/jpeg_decode.npz (tools/make_jpeg_decode_golden.py), the library's host decoder through ctypes, and the layout of one
fear_jpeg_decode_u8 call.  A plain module, imported by name as dataops and headref are."""
import ctypes
import os

import numpy as np

from feartracker_amd import train_abi as abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_decode.npz")
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_FORMAT, ERR_UNSUPPORTED = 0, -1, -2, -7, -9, -10
_cases = None


def cases():
    """[(name, the file's bytes, Pillow's (H, W, 3) pixels)], loaded once and shared."""
    global _cases
    if _cases is None:
        with np.load(GOLDEN) as d:
            _cases = [(str(name), d[f"jpg_{i}"].tobytes(), d[f"px_{i}"]) for i, name in enumerate(d["names"])]
        for _, _, px in _cases:
            px.setflags(write=False)
    return _cases


def supported():
    return [c for c in cases() if "progressive" not in c[0]]


def case(prefix):
    found = [c for c in cases() if c[0].startswith(prefix)]
    assert len(found) == 1, prefix
    return found[0]


def c_decode(lib, data, slack=0):
    """fear_jpeg_parse and fear_jpeg_entropy_decode on one file: the failing status, or (FearJpegInfo, packed int16 values, block_start).
    The buffers are exactly as long as the calls are told, with a sentinel behind them."""
    info = abi.FearJpegInfo()
    rc = lib.fear_jpeg_parse(data, len(data), ctypes.byref(info))
    if rc != OK:
        return rc
    cap = lib.fear_jpeg_packed_bound(ctypes.byref(info))
    assert cap == 64 * info.total_blocks
    coef = np.full(cap + 8, 0x5A5A, dtype=np.int16)
    start = np.full(info.total_blocks + 1 + 8, 0xA5A5A5A5, dtype=np.uint32)
    used = ctypes.c_size_t(0)
    rc = lib.fear_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, cap, start.ctypes.data, ctypes.byref(used))
    assert np.all(coef[cap:] == 0x5A5A) and np.all(start[info.total_blocks + 1:] == 0xA5A5A5A5), "written past the capacity"
    if rc != OK:
        return rc
    return info, coef[:used.value].copy(), start[:info.total_blocks + 1].copy()


def unpack(info, coef, start):
    """The packed stream as one (blocks_h, blocks_w, 64) int16 array per component, zigzag order."""
    out, b = [], 0
    for c in range(info.components):
        bh, bw = info.blocks_h[c], info.blocks_w[c]
        plane = np.zeros((bh * bw, 64), dtype=np.int16)
        for k in range(bh * bw):
            plane[k, :start[b + 1] - start[b]] = coef[start[b]:start[b + 1]]
            b += 1
        out.append(plane.reshape(bh, bw, 64))
    return out


def call_layout(decoded):
    """The host side of one fear_jpeg_decode_u8 call over [(info, coef, start)]: the record array (device pointers still zero), the byte
    offsets of every image's plane, coefficients, block_start and output, and the sizes of the buffers they index."""
    n = len(decoded)
    records = (abi.FearJpegImage * n)()
    infos = (abi.FearJpegInfo * n)()
    prefix = np.zeros((2, n + 1), dtype=np.uint32)
    at = dict(coef=[], start=[], out=[])
    up_bytes = out_bytes = plane_at = 0
    for k, (info, coef, start) in enumerate(decoded):
        infos[k] = info
        r = records[k]
        r.width, r.height, r.components, r.h, r.v = info.width, info.height, info.components, info.h[0], info.v[0]
        ctypes.memmove(r.qt, info.qt, ctypes.sizeof(r.qt))
        r.plane_offset = plane_at
        plane_at += info.total_blocks * 64
        prefix[0, k + 1] = prefix[0, k] + -(-info.total_blocks // abi.FEAR_JPEG_GROUP_BLOCKS)
        prefix[1, k + 1] = prefix[1, k] + -(-info.width * info.height // abi.FEAR_JPEG_GROUP_PIXELS)
        at["coef"].append(up_bytes)
        up_bytes += -(-coef.nbytes // 16) * 16
        at["start"].append(up_bytes)
        up_bytes += -(-start.nbytes // 16) * 16
        at["out"].append(out_bytes)
        out_bytes += info.width * info.height * 3 + 64                  # a gap between frames: the guard band of each
    return records, infos, prefix, at, up_bytes, out_bytes


def table_bytes(prefix, records):
    """The device table of a call: the two prefix tables, padding to 16 bytes, the records."""
    table = np.zeros(-(-prefix.nbytes // 16) * 16 + ctypes.sizeof(records), dtype=np.uint8)
    table[:prefix.nbytes] = prefix.reshape(-1).view(np.uint8)
    table[-ctypes.sizeof(records):] = np.frombuffer(records, dtype=np.uint8)
    return table
