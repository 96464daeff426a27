"""Plumbing shared by the tests of the device's Huffman stage (test_jpeg_huffman_host, test_jpeg_huffman_gpu): the second fixture
tests/golden/jpeg_entropy.npz (tools/make_jpeg_entropy_golden.py), fear_jpeg_scan_prepare through ctypes with exact-size buffers, the
hostile corpus of the 16 x 16 4:2:0 file, and the layout of one fear_jpeg_huffman call.  A plain module, imported by name as jpegdec is."""
import ctypes
import os
import struct

import numpy as np

import jpegdec
from jpegdec import OK
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi

GOLDEN = os.path.join(jpegdec.HERE, "golden", "jpeg_entropy.npz")
_cases = _reference = None


def entropy_cases():
    """[(name, the file's bytes, Pillow's (H, W, 3) pixels)] of jpeg_entropy.npz, loaded once and shared."""
    global _cases
    if _cases is None:
        with np.load(GOLDEN) as d:
            _cases = [(str(name), d[f"jpg_{i}"].tobytes(), d[f"px_{i}"]) for i, name in enumerate(d["names"])]
        for _, _, px in _cases:
            px.setflags(write=False)
    return _cases


def supported():
    """Every supported file of both fixtures."""
    return jpegdec.supported() + entropy_cases()


def reference():
    """{name: jpeg_coefficients_host's coefficients per component} for `supported()`, computed once, shared and left unchanged."""
    global _reference
    if _reference is None:
        _reference = {}
        for name, data, _ in supported():
            coef = jf.jpeg_coefficients_host(data)[1]
            for c in coef:
                c.setflags(write=False)
            _reference[name] = coef
    return _reference


def corpus():
    """The hostile files: every single flipped byte of the 16 x 16 4:2:0 fixture's entropy segment (the corpus of
    test_every_flipped_entropy_byte_gets_the_same_verdict) and every prefix of that file.  [(what, bytes)]"""
    F = jpegdec.case("16x16_420")[1]
    scan = F.index(b"\xff\xda")
    first = scan + 2 + struct.unpack(">H", F[scan + 2:scan + 4])[0]
    out = []
    for k in range(first, len(F) - 2):
        bad = bytearray(F)
        bad[k] ^= 0xFF
        out.append((f"byte {k} flipped", bytes(bad)))
    return out + [(f"prefix {k}", F[:k]) for k in range(len(F) + 1)]


def segments(info):
    n_mcu = info.mcus_x * info.mcus_y
    return -(-n_mcu // info.restart_interval) if info.restart_interval else 1


def c_prepare(lib, data, bytes_cap=None, seg_cap=None):
    """fear_jpeg_parse and fear_jpeg_scan_prepare on one file: the failing status, or (FearJpegInfo, bytes, seg_start, FearJpegScan).  The
    buffers are exactly as long as the call is told, with a sentinel behind them."""
    info = abi.FearJpegInfo()
    rc = lib.fear_jpeg_parse(data, len(data), ctypes.byref(info))
    if rc != OK:
        return rc
    bytes_cap = len(data) if bytes_cap is None else bytes_cap
    seg_cap = segments(info) + 1 if seg_cap is None else seg_cap
    out = np.full(bytes_cap + 8, 0x5A, dtype=np.uint8)
    start = np.full(seg_cap + 8, 0xA5A5A5A5, dtype=np.uint32)
    scan = abi.FearJpegScan()
    rc = lib.fear_jpeg_scan_prepare(data, len(data), ctypes.byref(info), out.ctypes.data, bytes_cap, start.ctypes.data, seg_cap, ctypes.byref(scan))
    assert np.all(out[bytes_cap:] == 0x5A) and np.all(start[seg_cap:] == 0xA5A5A5A5), "written past the capacity"
    if rc != OK:
        return rc
    return info, out[:scan.n_bytes].copy(), start[:scan.n_seg + 1].copy(), scan


def dense(info, flat):
    """Dense coefficients (64 total_blocks values) as one (blocks_h, blocks_w, 64) array per component."""
    out, at = [], 0
    for c in range(info.components):
        size = info.blocks_w[c] * info.blocks_h[c]
        out.append(flat[64 * at:64 * (at + size)].reshape(info.blocks_h[c], info.blocks_w[c], 64))
        at += size
    return out


def huffman_layout(prepared):
    """The host side of one fear_jpeg_huffman call over [(info, bytes, seg_start, scan)]: the record array (device addresses still zero),
    the upload buffer (bytes and seg_start of every image at 16-byte boundaries), their offsets, the offset of the table, and the number
    of coefficients."""
    n = len(prepared)
    records = (abi.FearJpegScan * n)()
    prefix = np.zeros(n + 1, dtype=np.uint32)
    at, parts, up_bytes, values = dict(bytes=[], seg=[]), [], 0, 0
    for k, (info, data, start, scan) in enumerate(prepared):
        ctypes.memmove(ctypes.byref(records[k]), ctypes.byref(scan), ctypes.sizeof(scan))
        records[k].coef_offset = values
        values += 64 * info.total_blocks
        prefix[k + 1] = prefix[k] + scan.n_seg
        for key, arr in (("bytes", data), ("seg", start)):
            at[key].append(up_bytes)
            parts.append((up_bytes, arr.view(np.uint8)))
            up_bytes += -(-max(arr.nbytes, 1) // 16) * 16
    table_at = up_bytes
    records_at = (4 * n + 4 + 15) & ~15
    host = np.zeros(table_at + records_at + ctypes.sizeof(records), dtype=np.uint8)
    for where, raw in parts:
        host[where:where + raw.size] = raw
    host[table_at:table_at + prefix.nbytes] = prefix.view(np.uint8)
    return records, host, at, table_at, records_at, values


def finish_layout(records, host, at, table_at, records_at, base):
    """Set the device addresses once the upload buffer's address is known, and copy the records into the table."""
    for k in range(len(records)):
        records[k].bytes = base + at["bytes"][k]
        records[k].seg_start = base + at["seg"][k]
    host[table_at + records_at:] = np.frombuffer(records, dtype=np.uint8)
