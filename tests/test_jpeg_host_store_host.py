"""JpegStore(residence="host"), the host side ("Bytes on the host"): the byte range a workgroup of the staged
kernels copies into LDS — `fear_jpeg_stage_range` through the library, `jpeg_huffman.stage_range_host` and a brute-force union of the
lanes' byte intervals, all three equal on prepared scans of the fixture files — the argument checks of the two new host functions, the
constructor's, and the prototypes."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpeghuff
from jpegdec import ERR_NULL, ERR_SHAPE, OK
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_huffman import scan_sub_start, stage_range_host
from feartracker_amd.jpeg_store import LANES, JpegStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_HIP = -4
SIZES = (32, 128, 1024)


def _union(seg, sub, first, count, sb):
    """The union of the lanes' [seg_start[s] + k sb, min(that + sb, seg_start[s + 1])): (byte0, byte1), asserted to be one range."""
    owner = np.repeat(np.arange(seg.size - 1), np.diff(sub.astype(np.int64)))     # the segment that owns each subsequence
    pieces = []
    for lane in range(first, first + count):
        s = int(owner[lane])
        assert sub[s] <= lane < sub[s + 1]
        lo = int(seg[s]) + (lane - int(sub[s])) * sb
        pieces.append((lo, min(lo + sb, int(seg[s + 1]))))
    if not pieces:
        return 0, 0
    assert all(a < b for a, b in pieces) and all(p[1] == q[0] for p, q in zip(pieces, pieces[1:])), "the lanes' bytes are one range"
    return pieces[0][0], pieces[-1][1]


def _call(lib, seg, sub, n_seg, n_bytes, first, count, sb):
    b0, b1 = ctypes.c_uint32(0xDEAD), ctypes.c_uint32(0xBEEF)
    rc = lib.fear_jpeg_stage_range(seg.ctypes.data, sub.ctypes.data, n_seg, n_bytes, first, count, sb, ctypes.byref(b0), ctypes.byref(b1))
    return rc, b0.value, b1.value


@pytest.fixture(scope="module")
def prepared():
    lib = abi.load_train_library()
    return lib, [(name,) + jpeghuff.c_prepare(lib, data)[1:] for name, data, _ in jpeghuff.supported()]


@pytest.mark.parametrize("sb", SIZES)
def test_stage_range_equals_its_model_and_the_union_of_the_lanes(prepared, sb):
    lib, files = prepared
    seen = dict(inside=0, spans=0, last_partial=0, empty=0)
    for name, data, seg, scan in files:
        sub = scan_sub_start(seg, sb)
        n_sub, n_seg = int(sub[-1]), int(scan.n_seg)
        assert lib.fear_jpeg_sub_start(seg.ctypes.data, n_seg, scan.n_bytes, sb, None, 0, ctypes.byref(ctypes.c_uint32())) == OK
        lanes = [(lane0, min(LANES, n_sub - lane0)) for lane0 in range(0, n_sub, LANES)]        # the workgroups of a full decode
        # a band's workgroups (they begin anywhere), single lanes at both ends, short runs across segment boundaries, no lane at all
        lanes += [(f, min(c, n_sub - f)) for f in {0, 1, n_sub // 3, n_sub // 2, n_sub - 1} if 0 <= f < n_sub for c in (1, 2, 7, LANES)]
        lanes += [(f, 0) for f in (0, n_sub // 2, n_sub)]
        for first, count in lanes:
            want = _union(seg, sub, first, count, sb)
            assert stage_range_host(seg, sub, first, count, sb) == want, (name, first, count)
            assert _call(lib, seg, sub, n_seg, scan.n_bytes, first, count, sb) == (OK,) + want, (name, first, count)
            assert 0 <= want[0] <= want[1] <= scan.n_bytes and want[1] - want[0] <= count * sb
            if count == 0:
                seen["empty"] += 1
                continue
            owners = {int(np.searchsorted(sub, lane, side="right")) - 1 for lane in (first, first + count - 1)}
            spanned = range(min(owners), max(owners) + 1)
            if len(spanned) == 1 and count > 1:
                seen["inside"] += 1
            if len(spanned) >= 3 and all((int(seg[s + 1]) - int(seg[s])) % sb for s in spanned):
                seen["spans"] += 1
            if first > 0 and first % LANES == 0 and first + count == n_sub and count < LANES:
                seen["last_partial"] += 1
    # (at 1024 bytes no fixture has more than 256 subsequences: its last workgroup is its only one)
    assert seen["inside"] and seen["spans"] and seen["empty"] and (seen["last_partial"] or sb == 1024), seen


def test_a_partial_last_workgroup_at_every_size(prepared):
    """The image's last workgroup, a partial one, with workgroups of a few lanes in place of 256 where the fixtures are too short."""
    lib, files = prepared
    name, data, seg, scan = next(f for f in files if f[0] == "256x192_gray_noise_q90_rst8")
    for sb in SIZES:
        sub = scan_sub_start(seg, sb)
        n_sub = int(sub[-1])
        group = next(g for g in (8, 7, 5) if n_sub % g)
        assert n_sub > group
        first = n_sub - n_sub % group
        want = _union(seg, sub, first, n_sub - first, sb)
        assert want[1] == scan.n_bytes and stage_range_host(seg, sub, first, n_sub - first, sb) == want
        assert _call(lib, seg, sub, scan.n_seg, scan.n_bytes, first, n_sub - first, sb) == (OK,) + want


def test_argument_errors_of_stage_range(prepared):
    lib, files = prepared
    name, data, seg, scan = next(f for f in files if f[0] == "40x24_444_random_q30_rst3")
    sub, n = scan_sub_start(seg, 32), int(scan.n_seg)
    n_sub = int(sub[-1])
    assert _call(lib, seg, sub, n, scan.n_bytes, 0, n_sub, 32)[0] == OK
    b = ctypes.c_uint32()
    for args in ((None, sub.ctypes.data, ctypes.byref(b), ctypes.byref(b)), (seg.ctypes.data, None, ctypes.byref(b), ctypes.byref(b)),
                 (seg.ctypes.data, sub.ctypes.data, None, ctypes.byref(b)), (seg.ctypes.data, sub.ctypes.data, ctypes.byref(b), None)):
        assert lib.fear_jpeg_stage_range(args[0], args[1], n, scan.n_bytes, 0, 1, 32, args[2], args[3]) == ERR_NULL
    for size in (0, 2, 30, 1028, -32):
        assert _call(lib, seg, sub, n, scan.n_bytes, 0, 1, size)[0] == ERR_SHAPE, size
    assert _call(lib, seg, sub, n, scan.n_bytes + 1, 0, 1, 32)[0] == ERR_SHAPE               # a seg_start that is not the scan's
    assert _call(lib, seg[1:].copy(), sub, n - 1, scan.n_bytes, 0, 1, 32)[0] == ERR_SHAPE
    bad = seg.copy()
    bad[1] = bad[2] + 1
    assert _call(lib, bad, sub, n, scan.n_bytes, 0, 1, 32)[0] == ERR_SHAPE
    assert _call(lib, seg, sub, 0, scan.n_bytes, 0, 1, 32)[0] == ERR_SHAPE
    assert _call(lib, seg, scan_sub_start(seg, 128), n, scan.n_bytes, 0, 1, 32)[0] == ERR_SHAPE   # another size's sub_start
    assert _call(lib, seg, sub, n, scan.n_bytes, n_sub, 1, 32)[0] == ERR_SHAPE               # lanes the scan does not have
    assert _call(lib, seg, sub, n, scan.n_bytes, 1, n_sub, 32)[0] == ERR_SHAPE
    assert _call(lib, seg, sub, n, scan.n_bytes, n_sub, 0, 32) == (OK, 0, 0)


def test_argument_errors_of_host_mapped_pointer():
    lib = abi.load_train_library()
    out = ctypes.c_void_p(0x1234)
    pageable = np.zeros(4096, dtype=np.uint8)
    assert lib.fear_host_mapped_pointer(ctypes.c_void_p(pageable.ctypes.data), None) == ERR_NULL
    assert lib.fear_host_mapped_pointer(None, ctypes.byref(out)) == ERR_SHAPE and not out.value
    rc = lib.fear_host_mapped_pointer(ctypes.c_void_p(pageable.ctypes.data), ctypes.byref(out))
    if rc == ERR_HIP:
        pytest.skip("no device: the library cannot ask the runtime about a pointer")
    assert rc == ERR_SHAPE and not out.value


def test_constructor_validation():
    with pytest.raises(ValueError, match="residence"):
        JpegStore(residence="disk")
    with pytest.raises(ValueError, match="residence"):
        JpegStore(residence=None)
    with pytest.raises(ValueError, match="host_capacity_bytes"):
        JpegStore(host_capacity_bytes=1 << 20)
    with pytest.raises(ValueError, match="host_capacity_bytes"):
        JpegStore(residence="device", host_capacity_bytes=0)


def test_train_abi_mirrors_the_prototypes():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fear_train.h")).read())
    P, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    plain = "(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev, int subsequence_bytes, void* stream);"
    rows_dev = ("(const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev, int16_t* coef, int32_t* status_dev, "
                "int subsequence_bytes, void* stream);")
    want = {"fear_jpeg_huffman_indexed_host": (plain, [P, i, P, P, P, i, P]),
            "fear_jpeg_huffman_indexed_rows_host": (plain, [P, i, P, P, P, i, P]),
            "fear_jpeg_huffman_indexed_windows_host": (plain, [P, i, P, P, P, i, P]),
            "fear_jpeg_huffman_indexed_rows_dev_host": (rows_dev, [P, i, P, P, P, P, i, P]),
            "fear_host_mapped_pointer": ("(const void* host, void** device);", [P, P]),
            "fear_jpeg_stage_range": ("(const uint32_t* seg_start, const uint32_t* sub_start, uint32_t n_seg, uint32_t n_bytes, uint32_t sub_first, "
                                      "uint32_t sub_count, int subsequence_bytes, uint32_t* byte0, uint32_t* byte1);", [P, P, u, u, u, u, i, P, P])}
    lib = abi.load_train_library()
    for name, (prototype, args) in want.items():
        assert f"int {name}{prototype}" in header, name
        assert abi.TRAIN_SYMBOLS[name] == (args, ctypes.c_int), name
        assert getattr(lib, name).argtypes == args
    # the staged calls take what the direct ones take: the existing prototypes are as they were
    for name in ("fear_jpeg_huffman_indexed", "fear_jpeg_huffman_indexed_rows", "fear_jpeg_huffman_indexed_windows", "fear_jpeg_huffman_indexed_rows_dev"):
        assert abi.TRAIN_SYMBOLS[name] == abi.TRAIN_SYMBOLS[name + "_host"] and f"int {name}{want[name + '_host'][0]}" in header
