"""Plumbing shared by the progressive JPEG tests (test_jpeg_progressive_host, test_jpeg_progressive_gpu): the fixture
tests/golden/jpeg_progressive.npz (tools/make_jpeg_progressive_golden.py), the library's three progressive entry points through ctypes with
sentinels behind every buffer, the scans of a file, and a hand-made file of any scan script.  A plain module, imported by name as jpegdec
is."""
import ctypes
import os
import struct

import numpy as np

from feartracker_amd import MalformedJPEG, UnsupportedJPEG
from feartracker_amd import train_abi as abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_progressive.npz")
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_FORMAT, ERR_UNSUPPORTED = 0, -1, -2, -7, -9, -10
N_CASES = 24
_cases = None


def cases():
    """[(name, the progressive file, Pillow's (H, W, 3) pixels, the baseline twin)], loaded once and shared."""
    global _cases
    if _cases is None:
        with np.load(GOLDEN) as d:
            _cases = [(str(name), d[f"jpg_{i}"].tobytes(), d[f"px_{i}"], d[f"base_{i}"].tobytes()) for i, name in enumerate(d["names"])]
        for _, _, px, _ in _cases:
            px.setflags(write=False)
    return _cases


def pillow_made():
    return [c for c in cases() if not c[0].startswith("written_")]


def case(prefix):
    found = [c for c in cases() if c[0].startswith(prefix)]
    assert len(found) == 1, prefix
    return found[0]


def smallest(count=2):
    return sorted(cases(), key=lambda c: len(c[1]))[:count]


def status_of(call, *args):
    """A Python decoder's verdict in the library's codes: (status, result or None)."""
    try:
        return OK, call(*args)
    except MalformedJPEG:
        return ERR_FORMAT, None
    except UnsupportedJPEG:
        return ERR_UNSUPPORTED, None


def c_parse(lib, data):
    info = abi.FearJpegInfo()
    rc = lib.fear_jpeg_progressive_parse(data, len(data), ctypes.byref(info))
    return rc if rc != OK else info


def c_decode(lib, data):
    """fear_jpeg_progressive_parse and fear_jpeg_progressive_decode on one file: the failing status, or (FearJpegInfo, packed int16
    values, block_start).  The buffers are exactly as long as the calls are told, with a sentinel behind them."""
    info = c_parse(lib, data)
    if isinstance(info, int):
        return info
    cap = lib.fear_jpeg_packed_bound(ctypes.byref(info))
    coef = np.full(cap + 8, 0x5A5A, dtype=np.int16)
    start = np.full(info.total_blocks + 1 + 8, 0xA5A5A5A5, dtype=np.uint32)
    used = ctypes.c_size_t(0)
    rc = lib.fear_jpeg_progressive_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, cap, start.ctypes.data, ctypes.byref(used))
    assert np.all(coef[cap:] == 0x5A5A) and np.all(start[info.total_blocks + 1:] == 0xA5A5A5A5), "written past the capacity"
    if rc != OK:
        return rc
    return info, coef[:used.value].copy(), start[:info.total_blocks + 1].copy()


def c_to_baseline(lib, data, cap=None):
    """fear_jpeg_progressive_to_baseline on one file: the failing status, or the baseline file's bytes.  `cap` (by default
    fear_jpeg_baseline_bound of the file's header) is what the call is told; a sentinel lies behind it."""
    if cap is None:
        info = c_parse(lib, data)
        if isinstance(info, int):
            return info
        cap = lib.fear_jpeg_baseline_bound(ctypes.byref(info))
    out = np.full(cap + 16, 0xA5, dtype=np.uint8)
    used = ctypes.c_size_t(0)
    rc = lib.fear_jpeg_progressive_to_baseline(data, len(data), out.ctypes.data, cap, ctypes.byref(used))
    assert np.all(out[cap:] == 0xA5), "written past the capacity"
    if rc != OK:
        return rc
    assert used.value <= cap
    return out[:used.value].tobytes()


def scans(F):
    """[(offset of the SOS marker, offset behind its entropy data, Ah)] of a well-formed file."""
    out, p = [], 2
    while F[p + 1] != 0xD9:
        L = struct.unpack(">H", F[p + 2:p + 4])[0]
        if F[p + 1] != 0xDA:
            p += L + 2
            continue
        q = p + 2 + L
        while not (F[q] == 0xFF and F[q + 1] != 0 and not 0xD0 <= F[q + 1] <= 0xD7):
            q += 1
        out.append((p, q, F[p + 1 + L] >> 4))
        p = q
    return out


def segment(F, marker):
    """(offset, length with the marker) of the first segment `marker` in front of the first scan."""
    p = 2
    while F[p + 1] != 0xDA:
        L = struct.unpack(">H", F[p + 2:p + 4])[0]
        if F[p + 1] == marker:
            return p, L + 2
        p += L + 2
    raise KeyError(marker)


def tiny(script, frame=0xC2):
    """An 8 x 8 gray file whose coefficients are all zero, under any scan script [(Ss, Se, Ah, Al)]: both Huffman tables hold the one
    symbol 0 with the code '0', so a DC difference of 0, a DC refinement bit of 0 and an end of block are each the bit 0, and every
    scan's data is the byte 7F.  It decodes to the flat colour 128."""
    out = b"\xff\xd8\xff\xdb\x00\x43\x00" + bytes([1] * 64) + bytes([0xFF, frame]) + b"\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00"
    for tc in (0, 1):
        out += b"\xff\xc4\x00\x14" + bytes([tc << 4, 1] + [0] * 15 + [0])
    for Ss, Se, Ah, Al in script:
        out += b"\xff\xda\x00\x08\x01\x01\x00" + bytes([Ss, Se, Ah << 4 | Al]) + b"\x7f"
    return out + b"\xff\xd9"


def tiny_script(n_scans):
    """A complete progression of an 8 x 8 gray block in exactly `n_scans` scans, 64 <= n_scans <= 127: the DC term at once, the AC terms one
    by one, the first n_scans - 64 of them in two steps (Al = 1, then the refinement)."""
    twice = n_scans - 64
    assert 0 <= twice <= 63
    script = [(0, 0, 0, 0)]
    for k in range(1, 64):
        script += [(k, k, 0, 1), (k, k, 1, 0)] if k <= twice else [(k, k, 0, 0)]
    assert len(script) == n_scans
    return script
