"""Progressive JPEG files on the host ("Progressive files"): `jpeg_decode_host(data, progressive=True)` against
Pillow's libjpeg-turbo on the recorded fixture tests/golden/jpeg_progressive.npz (tools/make_jpeg_progressive_golden.py), the progressive
coefficients against the pinned baseline decoder on each file's baseline twin, the library's three entry points
(fear_jpeg_progressive_parse, _decode, _to_baseline) against the Python statement — headers, coefficients, the transcode byte for byte,
and the same verdict on every prefix and every flipped byte of the two smallest files — and the files each rule declines.  No GPU."""
import ctypes
import io

import numpy as np
import pytest

import jpegdec
import jpegprog
from jpegprog import ERR_FORMAT, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, OK
from feartracker_amd import (JpegDecoder, JpegStore, MalformedJPEG, UnsupportedJPEG, jpeg_decode_host, jpeg_info, jpeg_to_baseline_host)
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import jpeg_progressive as jp
from feartracker_amd import train_abi as abi


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


@pytest.fixture(scope="module")
def python_coefficients():
    """{name: (header, coefficients)} of the Python decoder for every fixture case, computed once and shared."""
    return {name: jf.jpeg_coefficients_host(data, progressive=True) for name, data, _, _ in jpegprog.cases()}


def _same_verdicts(lib, data, what):
    """The three entry points in both decoders on one file: the same statuses, and the same results where they accept.  Returns the
    status of the decode."""
    rc_info, _ = jpegprog.status_of(jp.progressive_info, data)
    rc_py, res_py = jpegprog.status_of(jp.progressive_coefficients_host, data)
    rc_tb, tb_py = jpegprog.status_of(jpeg_to_baseline_host, data)
    info_c, res_c, tb_c = jpegprog.c_parse(lib, data), jpegprog.c_decode(lib, data), jpegprog.c_to_baseline(lib, data)
    assert (rc_info if rc_info else OK) == (info_c if isinstance(info_c, int) else OK), f"{what}: parse, Python {rc_info}, library {info_c}"
    assert rc_py == (res_c if isinstance(res_c, int) else OK), f"{what}: decode, Python {rc_py}, library {res_c}"
    assert rc_tb == (tb_c if isinstance(tb_c, int) else OK), f"{what}: to_baseline, Python {rc_tb}, library {tb_c}"
    assert rc_py == rc_tb, f"{what}: the decode says {rc_py}, the transcode {rc_tb}"
    if rc_py == OK:
        for a, b in zip(res_py[1], jpegdec.unpack(*res_c)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{what}: coefficients differ"
        assert tb_py == tb_c, f"{what}: the transcodes differ"
    return rc_py


def _markers(F):
    """The markers of the segments up to and including the first SOS."""
    out, p = [], 2
    while not out or out[-1] != 0xDA:
        out.append(F[p + 1])
        p += 2 + ((F[p + 2] << 8) | F[p + 3])
    return out


def test_host_decoder_equals_pillow_on_every_case(python_coefficients):
    seen = 0
    for name, data, px, _ in jpegprog.cases():
        got = jf.jpeg_pixels_host(*python_coefficients[name])
        assert got.dtype == np.uint8 and got.shape == px.shape, name
        bad = np.argwhere(got != px)
        assert bad.size == 0, f"{name}: {len(bad)} bytes differ, first at {bad[:3].tolist()}"
        seen += 1
    assert seen == jpegprog.N_CASES == 24
    names = [name for name, _, _, _ in jpegprog.cases()]
    assert {n.split("_")[1] for n in names if not n.startswith("written_")} == {"444", "422", "420", "gray"}
    assert sum(n.startswith("written_") for n in names) == 3
    assert any("rst3" in n for n in names) and any("rstrows1" in n for n in names) and any(n.startswith("512x512_gray") for n in names)
    # the one progressive file of the baseline fixture, through the public entry point
    _, data, px = jpegdec.case("33x31_420_smooth_q75_progressive")
    assert np.array_equal(jpeg_decode_host(data, progressive=True), px)


def test_the_option_is_off_by_default_and_leaves_baseline_files_alone():
    _, data, _, base = jpegprog.case("17x9_420")
    with pytest.raises(UnsupportedJPEG, match="progressive"):
        jpeg_decode_host(data)
    with pytest.raises(UnsupportedJPEG, match="progressive"):
        jpeg_info(data)
    assert np.array_equal(jpeg_decode_host(base, progressive=True), jpeg_decode_host(base))
    assert jpeg_info(base, progressive=True)["restart_interval"] == jpeg_info(base)["restart_interval"]
    with pytest.raises(UnsupportedJPEG, match="baseline"):
        jp.progressive_coefficients_host(base)
    with pytest.raises(UnsupportedJPEG, match="baseline"):
        jpeg_to_baseline_host(base)
    # a file neither decoder takes keeps the baseline decoder's verdict and message
    sof9 = bytearray(base)
    sof9[jpegprog.segment(base, 0xC0)[0] + 1] = 0xC9
    with pytest.raises(UnsupportedJPEG, match="SOF9"):
        jpeg_decode_host(bytes(sof9), progressive=True)


def test_coefficients_equal_the_baseline_twins(python_coefficients):
    seen = 0
    for name, _, _, base in jpegprog.pillow_made():
        hd, coef = python_coefficients[name]
        hb, want = jf.jpeg_coefficients_host(base)
        assert (hd.height, hd.width, hd.h, hd.v, hd.ids, hd.tq) == (hb.height, hb.width, hb.h, hb.v, hb.ids, hb.tq), name
        assert all(np.array_equal(hd.q[t], hb.q[t]) for t in hd.tq), name
        for c, (a, b) in enumerate(zip(coef, want)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: component {c}"
        seen += 1
    assert seen == 21


def test_library_headers_and_coefficients_equal_the_python_decoder(lib, python_coefficients):
    for name, data, px, base in jpegprog.cases():
        info, coef, start = jpegprog.c_decode(lib, data)
        want = jpeg_info(data, progressive=True)
        n = want["components"]
        assert (info.height, info.width) == px.shape[:2] == (want["height"], want["width"]), name
        assert info.components == n and info.restart_interval == 0 == want["restart_interval"], name
        assert (info.mcus_x, info.mcus_y) == (want["mcus_x"], want["mcus_y"]), name
        for field in ("h", "v", "blocks_w", "blocks_h"):
            assert list(getattr(info, field))[:n] == want[field], (name, field)
        assert info.total_blocks == sum(w * h for w, h in zip(want["blocks_w"], want["blocks_h"])), name
        assert np.array_equal(np.ctypeslib.as_array(info.qt)[:n], want["qt"]), name
        # but for the restart interval, the header of the baseline twin
        twin = abi.FearJpegInfo()
        assert lib.fear_jpeg_parse(base, len(base), ctypes.byref(twin)) == OK
        twin.restart_interval = 0
        assert bytes(twin) == bytes(info), name
        for a, b in zip(python_coefficients[name][1], jpegdec.unpack(info, coef, start)):
            assert a.shape == b.shape and np.array_equal(a, b), name
        # the packed stream is well formed
        lengths = np.diff(start.astype(np.int64))
        assert start[0] == 0 and start[-1] == coef.size and len(start) == info.total_blocks + 1, name
        assert np.all(lengths >= 1) and np.all(lengths <= 64), name
        last = coef[start[1:] - 1]
        assert np.all((last != 0) | (lengths == 1)), name
        # a baseline file is not this entry point's
        assert jpegprog.c_parse(lib, base) == ERR_UNSUPPORTED and jpegprog.c_to_baseline(lib, base, cap=1 << 16) == ERR_UNSUPPORTED, name
        assert jpegdec.c_decode(lib, data) == ERR_UNSUPPORTED, name                     # and fear_jpeg_parse keeps declining SOF2


def test_transcode_is_the_python_one_and_a_baseline_file_of_the_same_coefficients(lib, python_coefficients):
    d = JpegDecoder(device=0, progressive=True)
    for name, data, px, _ in jpegprog.cases():
        out = jpegprog.c_to_baseline(lib, data)
        assert out == jpeg_to_baseline_host(data), name
        assert d.to_baseline(data) == out, name
        info, coef, start = jpegdec.c_decode(lib, out)                                   # the existing baseline decoder
        assert info.restart_interval == info.mcus_x, name
        for a, b in zip(python_coefficients[name][1], jpegdec.unpack(info, coef, start)):
            assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(jpeg_decode_host(out), px), name
        _, _, seg, scan = d.scan_prepare(out)
        assert scan.n_seg == info.mcus_y == seg.size - 1 and scan.restart_interval == info.mcus_x, name
        assert scan.max_seg_bytes <= 512 * info.mcus_x * 6 < jf.DEVICE_SCAN_MAX // 64, name
        assert out[:2] == b"\xff\xd8" and out[-2:] == b"\xff\xd9", name
        tables = [0xDB] * len(set(python_coefficients[name][0].tq)) + [0xC0] + [0xC4] * (4 if info.components == 3 else 2)
        assert _markers(out) == ([0xE0] if b"JFIF\x00" in data[:24] else []) + tables + [0xDD, 0xDA], name
        assert (b"JFIF\x00" in out[:24]) == (b"JFIF\x00" in data[:24]), name
    d.close()


def test_transcode_keeps_jfif_and_adobe_and_drops_the_rest(lib):
    _, F, px, _ = jpegprog.case("17x9_422")
    sof = jpegprog.segment(F, 0xC2)[0]
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    extra = b"\xff\xe1\x00\x08Exif\x00\x00" + b"\xff\xfe\x00\x05abc"
    G = F[:sof] + extra + adobe + F[sof:]
    plain, out = jpegprog.c_to_baseline(lib, F), jpegprog.c_to_baseline(lib, G)
    assert out == jpeg_to_baseline_host(G)
    jfif = F[2:2 + jpegprog.segment(F, 0xE0)[1]]
    assert out[2:].startswith(jfif + adobe) and _markers(out) == [0xE0, 0xEE, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert out == plain[:2 + len(jfif)] + adobe + plain[2 + len(jfif):]
    assert np.array_equal(jpeg_decode_host(out), px)
    rgb = F[:sof] + adobe[:-1] + b"\x00" + F[sof:]                                       # Adobe transform 0: RGB samples
    assert _same_verdicts(lib, rgb, "Adobe transform 0") == ERR_UNSUPPORTED


def test_every_prefix_and_every_flipped_byte_gets_the_same_verdict(lib):
    verdicts = {OK: 0, ERR_FORMAT: 0, ERR_UNSUPPORTED: 0}
    for name, F, _, _ in jpegprog.smallest(2):
        assert F[-2:] == b"\xff\xd9" and len(F) < 600, name
        assert _same_verdicts(lib, F, name) == OK
        for k in range(len(F)):
            rc = _same_verdicts(lib, F[:k], f"{name}: prefix {k}")
            assert rc == ERR_FORMAT, f"{name}: prefix {k} of {len(F)}: status {rc}"     # a file without its EOI included
        assert _same_verdicts(lib, F + b"trailing bytes", "bytes behind EOI") == OK
        for k in range(len(F)):
            bad = bytearray(F)
            bad[k] ^= 0xFF
            verdicts[_same_verdicts(lib, bytes(bad), f"{name}: byte {k} flipped")] += 1
    assert all(v > 0 for v in verdicts.values()), verdicts


def test_every_low_bit_flip_of_a_file_with_refinements_gets_the_same_verdict(lib):
    """Bytes of the hand-written file with three approximation steps and restart markers in its AC scans, one bit each: the refinement
    paths of both decoders on damaged data."""
    _, F, _, _ = jpegprog.case("written_33x31_444_noise_q75_approx210_rst")
    first = jpegprog.scans(F)[0][0]
    seen = set()
    for k in range(first, len(F), 23):
        bad = bytearray(F)
        bad[k] ^= 0x10
        seen.add(_same_verdicts(lib, bytes(bad), f"byte {k}"))
    assert OK in seen and ERR_FORMAT in seen


def test_declined_progressions(lib):
    _, F, _, _ = jpegprog.case("17x9_420")
    spans = jpegprog.scans(F)
    assert len(spans) >= 6 and any(ah for _, _, ah in spans)

    def declined(data, what, message, status=ERR_UNSUPPORTED):
        assert _same_verdicts(lib, data, what) == status, what
        with pytest.raises(UnsupportedJPEG if status == ERR_UNSUPPORTED else MalformedJPEG, match=message):
            jpeg_decode_host(data, progressive=True)

    a, b, _ = spans[-1]
    declined(F[:a] + F[b:], "the last scan removed", "incomplete progression")
    a, b, _ = next(s for s in spans if s[2])
    declined(F[:b] + F[a:b] + F[b:], "a refinement scan twice", "inconsistent progression")
    a, b, _ = spans[1]
    declined(F[:b] + F[a:b] + F[b:], "a first scan twice", "inconsistent progression")
    a, b = spans[0][1], spans[1][1]                                                       # the second scan, an AC one, with its DHT
    assert F[spans[1][0] + 7] > 0
    declined(F[:spans[0][0]] + F[a:b] + F[spans[0][0]:], "an AC scan in front of the DC scan", "inconsistent progression")
    dqt, length = jpegprog.segment(F, 0xDB)
    at = spans[0][1]
    declined(F[:at] + F[dqt:dqt + length] + F[at:], "a DQT after the first SOS", "after the first scan")
    # the scan count, on a hand-made file whose every scan is one byte
    px = np.full((8, 8, 3), 128, dtype=np.uint8)
    for n_scans in (64, 100):
        T = jpegprog.tiny(jpegprog.tiny_script(n_scans))
        assert T.count(b"\xff\xda") == n_scans and _same_verdicts(lib, T, f"{n_scans} scans") == OK
        assert np.array_equal(jpeg_decode_host(T, progressive=True), px)
    declined(jpegprog.tiny(jpegprog.tiny_script(101)), "101 scans", "more than 100 scans")
    # the scan header's rules
    declined(jpegprog.tiny([(0, 1, 0, 0)]), "a DC scan with Se = 1", "spectral selection", ERR_FORMAT)
    declined(jpegprog.tiny([(0, 0, 0, 0), (5, 4, 0, 0)]), "Se below Ss", "spectral selection", ERR_FORMAT)
    declined(jpegprog.tiny([(0, 0, 0, 0), (1, 64, 0, 0)]), "Se above 63", "spectral selection", ERR_FORMAT)
    declined(jpegprog.tiny([(0, 0, 0, 14)]), "Al above 13", "successive approximation", ERR_FORMAT)
    declined(jpegprog.tiny([(0, 0, 3, 1)]), "Ah that is not Al + 1", "successive approximation", ERR_FORMAT)
    declined(jpegprog.tiny([(0, 0, 0, 0)]), "a file of the DC scan alone", "incomplete progression")
    assert _same_verdicts(lib, jpegprog.tiny([(0, 0, 0, 0), (1, 63, 0, 0)], frame=0xC0), "SOF0") == ERR_UNSUPPORTED


def test_coefficients_beyond_the_baseline_alphabet_are_declined_by_both_calls(lib):
    """A DC term of 1 << 11 after the point transform: every scan is valid T.81, the value has no baseline code."""
    T = bytearray(jpegprog.tiny([(0, 0, 0, 12), (0, 0, 12, 11)] + [(0, 0, al + 1, al) for al in range(10, -1, -1)] + [(1, 63, 0, 0)]))
    assert _same_verdicts(lib, bytes(T), "thirteen DC scans of zeros") == OK
    at = jpegprog.scans(bytes(T))[1][1] - 1
    assert T[at] == 0x7F
    T[at] = 0xFF                                                                          # the refinement bit at Al = 11, then padding
    T[at + 1:at + 1] = b"\x00"
    assert _same_verdicts(lib, bytes(T), "a DC term of 2048") == ERR_UNSUPPORTED
    with pytest.raises(UnsupportedJPEG, match="beyond the baseline alphabet"):
        jpeg_decode_host(bytes(T), progressive=True)


def test_capacity_and_argument_checks(lib):
    _, data, _, _ = jpegprog.case("17x9_444")
    _, other, _, _ = jpegprog.case("8x8_444")
    info, coef, start = jpegprog.c_decode(lib, data)
    used, out = ctypes.c_size_t(0), np.full(coef.size + 8, 0x5A5A, dtype=np.int16)
    args = (data, len(data), ctypes.byref(info))
    assert lib.fear_jpeg_progressive_decode(*args, out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == OK
    assert used.value == coef.size and np.array_equal(out[:coef.size], coef) and np.all(out[coef.size:] == 0x5A5A)
    out[:] = 0x5A5A
    assert lib.fear_jpeg_progressive_decode(*args, out.ctypes.data, coef.size - 1, start.ctypes.data, ctypes.byref(used)) == ERR_WORKSPACE
    assert np.all(out[coef.size - 1:] == 0x5A5A)
    assert lib.fear_jpeg_progressive_decode(*args, None, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_progressive_decode(*args, out.ctypes.data, coef.size, None, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_progressive_decode(*args, out.ctypes.data, coef.size, start.ctypes.data, None) == ERR_NULL
    assert lib.fear_jpeg_progressive_decode(None, len(data), ctypes.byref(info), out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_progressive_decode(data, len(data), None, out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_NULL
    foreign = jpegprog.c_parse(lib, other)
    assert lib.fear_jpeg_progressive_decode(data, len(data), ctypes.byref(foreign), out.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used)) == ERR_SHAPE
    assert lib.fear_jpeg_progressive_parse(None, 10, ctypes.byref(info)) == ERR_NULL
    assert lib.fear_jpeg_progressive_parse(data, len(data), None) == ERR_NULL
    assert lib.fear_jpeg_baseline_bound(None) == 0
    whole = jpegprog.c_to_baseline(lib, data)
    assert len(whole) <= lib.fear_jpeg_baseline_bound(ctypes.byref(info))
    assert jpegprog.c_to_baseline(lib, data, cap=len(whole)) == whole                    # the exact capacity, a sentinel behind it
    for cap in (len(whole) - 1, len(whole) // 2, 3, 0):
        assert jpegprog.c_to_baseline(lib, data, cap=cap) == ERR_WORKSPACE, cap
    buf = np.zeros(len(whole), dtype=np.uint8)
    assert lib.fear_jpeg_progressive_to_baseline(None, len(data), buf.ctypes.data, buf.size, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_progressive_to_baseline(data, len(data), None, buf.size, ctypes.byref(used)) == ERR_NULL
    assert lib.fear_jpeg_progressive_to_baseline(data, len(data), buf.ctypes.data, buf.size, None) == ERR_NULL


def test_decoder_and_store_take_the_option_and_decline_without_it(lib):
    _, data, _, base = jpegprog.case("33x31_420")
    plain, d = JpegDecoder(device=0), JpegDecoder(device=0, progressive=True)
    assert plain.progressive is False and d.progressive is True
    assert plain.entropy_decode(data) == ERR_UNSUPPORTED and plain._prepare(data) == ERR_UNSUPPORTED
    want = jpegprog.c_decode(lib, data)
    for got in (d.entropy_decode(data), d._prepare(data), d.progressive_decode(data)):
        assert len(got) == 3 and bytes(got[0]) == bytes(want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert len(d._prepare(base)) == 4 and len(d.entropy_decode(base)) == 3                # baseline files go the way they went
    assert d.entropy_decode(data[:-2]) == ERR_FORMAT and d.to_baseline(data[:-2]) == ERR_FORMAT
    assert d.progressive_decode(base) == ERR_UNSUPPORTED
    with pytest.raises(MalformedJPEG, match="truncated"):
        jf._raise_as_python(data[:-2], ERR_FORMAT, True)
    with pytest.raises(UnsupportedJPEG, match="progressive frame"):
        jf._raise_as_python(data, ERR_UNSUPPORTED)
    plain.close()
    d.close()
    store = JpegStore(device=0, progressive=True)
    assert store.progressive and store._host.progressive and not JpegStore(device=0).progressive
    assert store._transcode(base) is None and store._transcode(data) == jpeg_to_baseline_host(data)
    assert store._transcode(data[:-2]) == ERR_FORMAT
    assert "progressive files" not in JpegStore.__doc__.split("Out of scope")[1]
    store.close()


def test_fixture_pixels_are_pillows():
    Image = pytest.importorskip("PIL.Image")
    for name, data, px, base in jpegprog.cases():
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert got.shape == px.shape and np.array_equal(got, px), name
        if not name.startswith("written_"):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(base)).convert("RGB")), px), name
