"""The JPEG frame decoder on the host: `jpeg_decode_host` against Pillow's libjpeg-turbo — the recorded fixture
tests/golden/jpeg_decode.npz (tools/make_jpeg_decode_golden.py) and, where Pillow is installed, a live decode — byte for byte; the
library's parser and Huffman stage (fear_jpeg_parse, fear_jpeg_entropy_decode) against the Python decoder: the same headers, the same
coefficients, a well-formed packed stream, and the same verdict on every prefix, every flipped byte and every header fault of a file.
No GPU."""
import io
import struct

import numpy as np
import pytest

import jpegdec
from jpegdec import ERR_FORMAT, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, OK
from feartracker_amd import JpegDecoder, MalformedJPEG, UnsupportedJPEG, jpeg_decode_host, jpeg_info
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


def _python_verdict(data):
    """(status, coefficients per component or None) of the Python decoder, in the library's codes."""
    try:
        return OK, jf.jpeg_coefficients_host(data)[1]
    except MalformedJPEG:
        return ERR_FORMAT, None
    except UnsupportedJPEG:
        return ERR_UNSUPPORTED, None


def _c_verdict(lib, data):
    res = jpegdec.c_decode(lib, data)
    return (res, None) if isinstance(res, int) else (OK, jpegdec.unpack(*res))


def _same(lib, data, what):
    """Both decoders on one file: the same status, and the same coefficients where they accept.  Returns the status."""
    rc_py, coef_py = _python_verdict(data)
    rc_c, coef_c = _c_verdict(lib, data)
    assert rc_py == rc_c, f"{what}: Python {rc_py}, library {rc_c}"
    if rc_py == OK:
        assert len(coef_py) == len(coef_c)
        for a, b in zip(coef_py, coef_c):
            assert a.shape == b.shape and np.array_equal(a, b), f"{what}: coefficients differ"
    return rc_py


def test_host_decoder_equals_pillow_on_every_case():
    seen = 0
    for name, data, px in jpegdec.supported():
        got = jpeg_decode_host(data)
        assert got.dtype == np.uint8 and got.shape == px.shape, name
        bad = np.argwhere(got != px)
        assert bad.size == 0, f"{name}: {len(bad)} bytes differ, first at {bad[:3].tolist()}"
        seen += 1
    assert seen == 43
    modes = {name.split("_")[1] for name, _, _ in jpegdec.supported()}
    assert modes == {"444", "422", "420", "gray"}


def test_progressive_file_is_unsupported(lib):
    _, data, _ = jpegdec.case("33x31_420_smooth_q75_progressive")
    with pytest.raises(UnsupportedJPEG, match="progressive"):
        jpeg_decode_host(data)
    with pytest.raises(UnsupportedJPEG):
        jpeg_info(data)
    assert jpegdec.c_decode(lib, data) == ERR_UNSUPPORTED


def test_library_headers_and_coefficients_equal_the_python_decoder(lib):
    for name, data, px in jpegdec.supported():
        info, coef, start = jpegdec.c_decode(lib, data)
        want = jpeg_info(data)
        assert (info.height, info.width) == px.shape[:2] == (want["height"], want["width"]), name
        n = want["components"]
        assert info.components == n and info.restart_interval == want["restart_interval"], name
        assert (info.mcus_x, info.mcus_y) == (want["mcus_x"], want["mcus_y"]), name
        for field in ("h", "v", "blocks_w", "blocks_h"):
            assert list(getattr(info, field))[:n] == want[field], (name, field)
        assert info.total_blocks == sum(w * h for w, h in zip(want["blocks_w"], want["blocks_h"])), name
        assert np.array_equal(np.ctypeslib.as_array(info.qt)[:n], want["qt"]), name
        # geometry of the contract: mcus = ceil(side / (8 max sampling)), blocks = mcus x the component's own sampling
        assert info.mcus_x == -(-info.width // (8 * info.h[0])) and info.mcus_y == -(-info.height // (8 * info.v[0])), name
        hd, coef_py = jf.jpeg_coefficients_host(data)
        for a, b in zip(coef_py, jpegdec.unpack(info, coef, start)):
            assert a.shape == b.shape and np.array_equal(a, b), name
    assert {"rst3" in name or "rstrows" in name for name, _, _ in jpegdec.supported()} == {True, False}


def test_packed_stream_is_well_formed(lib):
    for name, data, _ in jpegdec.supported():
        info, coef, start = jpegdec.c_decode(lib, data)
        lengths = np.diff(start.astype(np.int64))
        assert start[0] == 0 and start[-1] == coef.size and len(start) == info.total_blocks + 1, name
        assert np.all(lengths >= 1) and np.all(lengths <= 64), name                    # monotone, 1..64 values per block
        last = coef[start[1:] - 1]
        assert np.all((last != 0) | (lengths == 1)), name                             # the last stored value is non-zero unless it is the DC term
        assert coef.size <= 64 * info.total_blocks, name


def test_capacity_and_argument_checks(lib):
    import ctypes
    _, data, _ = jpegdec.case("16x16_420")
    info, coef, start = jpegdec.c_decode(lib, data)
    used, out = ctypes.c_size_t(0), np.zeros(coef.size, dtype=np.int16)
    args = (data, len(data), ctypes.byref(info))
    assert lib.fear_jpeg_entropy_decode(*args, out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == OK and used.value == coef.size
    assert np.array_equal(out, coef)
    out[:] = 0x5A5A
    assert lib.fear_jpeg_entropy_decode(*args, out.ctypes.data, coef.size - 1, start.ctypes.data, ctypes.byref(used)) == ERR_WORKSPACE
    assert np.all(out[coef.size - 1:] == 0x5A5A)
    assert lib.fear_jpeg_entropy_decode(*args, None, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_entropy_decode(None, len(data), ctypes.byref(info), out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_parse(None, 10, ctypes.byref(info)) == ERR_NULL and lib.fear_jpeg_parse(data, len(data), None) == ERR_NULL
    assert lib.fear_jpeg_packed_bound(None) == 0
    other = abi.FearJpegInfo()
    assert lib.fear_jpeg_parse(jpegdec.case("8x8_420")[1], len(jpegdec.case("8x8_420")[1]), ctypes.byref(other)) == OK
    assert lib.fear_jpeg_entropy_decode(data, len(data), ctypes.byref(other), out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_SHAPE
    infos = (abi.FearJpegInfo * 2)(info, other)
    assert lib.fear_jpeg_decode_workspace_bytes(infos, 2) == 64 * (info.total_blocks + other.total_blocks) + 16
    assert lib.fear_jpeg_decode_workspace_bytes(None, 2) == 0 and lib.fear_jpeg_decode_workspace_bytes(infos, 65536) == 0
    # the device call's checks that come before any launch
    assert lib.fear_jpeg_decode_u8(None, 0, None, None, 0, None) == OK
    assert lib.fear_jpeg_decode_u8(None, -1, None, None, 0, None) == ERR_SHAPE
    assert lib.fear_jpeg_decode_u8(None, 65536, None, None, 0, None) == ERR_SHAPE
    assert lib.fear_jpeg_decode_u8(None, 1, None, None, 0, None) == ERR_NULL


def test_every_prefix_is_an_error_in_both_decoders(lib):
    _, F, px = jpegdec.case("16x16_420")
    assert "plain" in jpegdec.case("16x16_420")[0] and F[-2:] == b"\xff\xd9"
    for k in range(len(F) - 2):
        rc = _same(lib, F[:k], f"prefix {k}")
        assert rc == ERR_FORMAT, f"prefix {k} of {len(F)}: status {rc}"
    assert _same(lib, F[:-2], "the file without its EOI") == OK
    assert np.array_equal(jpeg_decode_host(F[:-2]), px)
    assert _same(lib, F[:-1], "the file without its last byte") == OK
    assert _same(lib, F + b"trailing bytes", "bytes behind EOI") == OK


def test_every_flipped_entropy_byte_gets_the_same_verdict(lib):
    _, F, _ = jpegdec.case("16x16_420")
    scan = F.index(b"\xff\xda")
    first = scan + 2 + struct.unpack(">H", F[scan + 2:scan + 4])[0]
    verdicts = {OK: 0, ERR_FORMAT: 0}
    for k in range(first, len(F) - 2):
        bad = bytearray(F)
        bad[k] ^= 0xFF
        verdicts[_same(lib, bytes(bad), f"byte {k} flipped")] += 1
    assert verdicts[OK] > 0 and verdicts[ERR_FORMAT] > 0, verdicts


def test_restart_marker_faults(lib):
    def markers(F):
        scan = F.index(b"\xff\xda")
        return [i for i in range(scan, len(F) - 1) if F[i] == 0xFF and 0xD0 <= F[i + 1] <= 0xD7]

    F = next(data for name, data, _ in jpegdec.supported() if "rst3" in name and len(markers(data)) >= 2)
    at = markers(F)
    swapped = bytearray(F)
    swapped[at[0] + 1], swapped[at[1] + 1] = F[at[1] + 1], F[at[0] + 1]
    assert _same(lib, F, "as it is") == OK
    assert _same(lib, bytes(swapped), "restart markers out of order") == ERR_FORMAT
    _, F, _ = jpegdec.case("40x24_420_random_q75_rstrows1")
    at = markers(F)
    assert len(at) == 1 and _same(lib, F, "as it is") == OK
    assert _same(lib, F[:at[0]] + F[at[0] + 2:], "a restart marker missing") == ERR_FORMAT
    assert _same(lib, F[:at[0]] + b"\x00" + F[at[0]:], "a byte in front of a restart marker") == ERR_FORMAT


def _segments(F):
    """{marker: (offset of its FF, length with the marker)} of the segments in front of the scan (the first of each kind)."""
    out, p = {}, 2
    while F[p + 1] != 0xDA:
        L = struct.unpack(">H", F[p + 2:p + 4])[0]
        out.setdefault(F[p + 1], (p, L + 2))
        p += L + 2
    out[0xDA] = (p, struct.unpack(">H", F[p + 2:p + 4])[0] + 2)
    return out


def _header_faults():
    _, F, _ = jpegdec.case("16x16_420")
    seg = _segments(F)
    sof, sof_len = seg[0xC0]
    dht, dht_len = seg[0xC4]

    def patch(at, value):
        bad = bytearray(F)
        bad[at:at + len(value)] = value
        return bytes(bad)

    def frame(components):
        body = bytes([8, 0, 16, 0, 16, len(components)]) + b"".join(bytes(c) for c in components)
        return F[:sof] + b"\xff\xc0" + struct.pack(">H", len(body) + 2) + body + F[sof + sof_len:]

    def huffman(counts, symbols):
        body = bytes([0x00]) + bytes(counts) + bytes(symbols)
        return F[:dht] + b"\xff\xc4" + struct.pack(">H", len(body) + 2) + body + F[dht:]

    return {
        "zero width": (patch(sof + 7, b"\x00\x00"), ERR_FORMAT),
        "zero height": (patch(sof + 5, b"\x00\x00"), ERR_UNSUPPORTED),
        "sampling factor 3": (patch(sof + 11, b"\x31"), ERR_UNSUPPORTED),
        "sampling factor 0": (patch(sof + 11, b"\x02"), ERR_FORMAT),
        "2 components": (frame([(1, 0x22, 0), (2, 0x11, 1)]), ERR_UNSUPPORTED),
        "4 components": (frame([(1, 0x11, 0), (2, 0x11, 1), (3, 0x11, 1), (4, 0x11, 0)]), ERR_UNSUPPORTED),
        "a Tq with no table": (patch(sof + 12, b"\x03"), ERR_FORMAT),
        "a DHT with more than 256 symbols": (huffman([17] * 16, range(256)), ERR_FORMAT),
        "an over-subscribed code length": (huffman([3] + [0] * 15, [0, 1, 2]), ERR_FORMAT),
        "a segment length past the end": (patch(seg[0xE0][0] + 2, b"\xff\xff"), ERR_FORMAT),
        "SOS before SOF": (F[:sof] + F[sof + sof_len:], ERR_FORMAT),
        "12-bit precision": (patch(sof + 4, b"\x0c"), ERR_UNSUPPORTED),
        "SOF2": (patch(sof + 1, b"\xc2"), ERR_UNSUPPORTED),
        "SOF9": (patch(sof + 1, b"\xc9"), ERR_UNSUPPORTED),
        "16-bit DQT": (patch(seg[0xDB][0] + 4, b"\x10"), ERR_UNSUPPORTED),
        "DNL": (F[:sof] + b"\xff\xdc\x00\x04\x00\x10" + F[sof:], ERR_UNSUPPORTED),
        "Adobe transform 0": (F[:sof] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + F[sof:], ERR_UNSUPPORTED),
        "a scan with one component": (patch(seg[0xDA][0] + 4, b"\x01"), ERR_UNSUPPORTED),
        "no SOI": (b"\x00" + F[1:], ERR_FORMAT),
    }


def test_header_faults_get_their_status(lib):
    import ctypes
    for what, (data, want) in _header_faults().items():
        info = abi.FearJpegInfo()
        assert lib.fear_jpeg_parse(data, len(data), ctypes.byref(info)) == want, what
        assert _same(lib, data, what) == want, what
        with pytest.raises(MalformedJPEG if want == ERR_FORMAT else UnsupportedJPEG):
            jpeg_decode_host(data)


def test_fill_bytes_and_skipped_segments(lib):
    name, F, px = jpegdec.case("33x31_422_smooth_q75_com_app1")
    assert b"\xff\xfe" in F and b"\xff\xe1" in F                     # COM and APP1 are in the file
    sof = _segments(F)[0xC0][0]
    padded = F[:sof] + b"\xff\xff\xff" + F[sof:]                      # fill bytes in front of a marker
    assert _same(lib, padded, "fill bytes") == OK
    assert np.array_equal(jpeg_decode_host(padded), px)


def test_decoder_threads_follow_the_affinity_mask(monkeypatch):
    import os
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(3)))
    monkeypatch.setattr(os, "cpu_count", lambda: 512)
    d = JpegDecoder(device=0)
    assert d.threads == 3
    d.close()
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(64)))
    d = JpegDecoder(device=0)
    assert d.threads == 8
    d.close()
    d = JpegDecoder(device=0, threads=100)
    assert d.threads == 16
    # the host stage of the product is the library's: the same packed stream as through the C ABI
    _, data, _ = jpegdec.case("17x23_420")
    info, coef, start = d.entropy_decode(data)
    want = jpegdec.c_decode(abi.load_train_library(), data)
    assert np.array_equal(coef, want[1]) and np.array_equal(start, want[2]) and bytes(info) == bytes(want[0])
    assert d.entropy_decode(data[:200]) == ERR_FORMAT
    d.close()


def test_fixture_pixels_are_pillows():
    Image = pytest.importorskip("PIL.Image")
    for name, data, px in jpegdec.cases():
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert got.shape == px.shape and np.array_equal(got, px), name
