"""The Huffman stage of the JPEG frame decoder as the device runs it, on the host: the Python statement of the
self-synchronising parallel decode, `jpeg_entropy_parallel_host`, against the sequential decoder `jpeg_coefficients_host` — the same
coefficients on every file of both fixtures at every subsequence length and lane count, the worst case of 256 rounds really run, the same
verdict on every flipped byte and every prefix of a file — and the library's `fear_jpeg_scan_prepare` against its Python restatement.
No GPU."""
import ctypes

import numpy as np
import pytest

import jpegdec
import jpeghuff
from jpegdec import ERR_FORMAT, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, OK
from feartracker_amd import MalformedJPEG, UnsupportedJPEG
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import jpeg_huffman as jh
from feartracker_amd import train_abi as abi


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


def _model(data, subsequence_bytes, lanes):
    """(status, coefficients or None, rounds) of the parallel model, a header or marker fault in the library's codes."""
    try:
        _, coef, status, rounds = jh.jpeg_entropy_parallel_host(data, subsequence_bytes, lanes)
    except MalformedJPEG:
        return ERR_FORMAT, None, []
    except UnsupportedJPEG:
        return ERR_UNSUPPORTED, None, []
    return status, coef, rounds


def _sequential(data):
    try:
        return OK, jf.jpeg_coefficients_host(data)[1]
    except MalformedJPEG:
        return ERR_FORMAT, None
    except UnsupportedJPEG:
        return ERR_UNSUPPORTED, None


@pytest.mark.parametrize("lanes", [4, 256])
@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_model_equals_the_sequential_decoder(subsequence_bytes, lanes):
    """Four lanes force many sequences even on a 300-byte file: the carry of state, block ordinal and DC predictor between them."""
    want = jpeghuff.reference()
    sequences = 0
    for name, data, _ in jpeghuff.supported():
        status, coef, rounds = _model(data, subsequence_bytes, lanes)
        assert status == OK, name
        assert len(coef) == len(want[name]), name
        for c, (a, b) in enumerate(zip(coef, want[name])):
            assert a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all()), f"{name}: component {c} differs"
        assert all(1 <= r <= lanes for r in rounds), name
        sequences = max(sequences, len(rounds))
    assert sequences > (1 if subsequence_bytes == 128 and lanes == 256 else 4)


def test_the_worst_case_runs_every_round():
    """At 16-byte subsequences the 64 x 48 4:4:4 random file spans 783 subsequences in 4 sequences and needs every round of the first:
    no lane but lane 0 ever holds the true state.  The cap of lanes - 1 rounds behind the first leaves nothing out."""
    name, data, _ = jpegdec.case("64x48_444_random_q100_plain2")
    status, coef, rounds = _model(data, 16, 256)
    assert status == OK and len(rounds) == 4
    print(f"{name}: rounds per sequence {rounds}")
    assert max(rounds) >= 128
    for a, b in zip(coef, jpeghuff.reference()[name]):
        assert bool((a == b).all())
    status, _, rounds128 = _model(data, 128, 256)
    assert status == OK and max(rounds128) < max(rounds)


def test_model_gives_the_sequential_verdict_on_the_hostile_corpus():
    """Every flipped entropy byte and every prefix of the 16 x 16 4:2:0 file: OK exactly where the sequential decoder accepts, and there
    the same coefficients.  Four lanes of 4 bytes: the verdict is gathered across many sequences."""
    verdicts = {OK: 0, ERR_FORMAT: 0}
    for what, data in jpeghuff.corpus():
        want, coef = _sequential(data)
        got, mine, _ = _model(data, 4, 4)
        assert got == want, f"{what}: model {got}, sequential {want}"
        verdicts[want] += 1
        if want == OK:
            for a, b in zip(mine, coef):
                assert bool((a == b).all()), what
    assert verdicts[OK] > 100 and verdicts[ERR_FORMAT] > 1000, verdicts
    # one pass with the kernel's shape as well, on the files the flips accept and a share of the others
    for what, data in jpeghuff.corpus()[::7]:
        assert _model(data, 16, 256)[0] == _sequential(data)[0], what


def test_model_refuses_a_bad_subsequence_length():
    data = jpegdec.case("8x8_420")[1]
    for bad in (0, 2, 6, 1028):
        with pytest.raises(ValueError):
            jh.jpeg_entropy_parallel_host(data, bad)


# ------------------------------------------------------------------------------------------------------------ fear_jpeg_scan_prepare
def _python_prepare(data):
    try:
        return jh.jpeg_scan_prepare_host(data)
    except MalformedJPEG:
        return ERR_FORMAT
    except UnsupportedJPEG:
        return ERR_UNSUPPORTED


def _same_prepare(lib, data, what):
    want, got = _python_prepare(data), jpeghuff.c_prepare(lib, data)
    if isinstance(want, int):
        assert got == want, f"{what}: Python {want}, library {got if isinstance(got, int) else OK}"
        return want
    assert not isinstance(got, int), f"{what}: library {got}, Python accepts"
    info, out, start, scan = got
    assert out.tobytes() == want[0] and start.tolist() == want[1], what
    assert scan.n_bytes == len(want[0]) and scan.n_seg == len(want[1]) - 1 == jpeghuff.segments(info), what
    assert scan.max_seg_bytes == int(np.diff(start.astype(np.int64)).max()), what
    return OK


def test_scan_prepare_equals_the_python_restatement(lib):
    seen_ff = seen_segments = 0
    for name, data, _ in jpeghuff.supported():
        assert _same_prepare(lib, data, name) == OK
        info, out, start, scan = jpeghuff.c_prepare(lib, data)
        seen_ff += int((out == 0xFF).sum())
        seen_segments = max(seen_segments, scan.n_seg)
        assert (scan.components, scan.h, scan.v, scan.mcus_x, scan.mcus_y) == (info.components, info.h[0], info.v[0], info.mcus_x, info.mcus_y)
        assert scan.total_blocks == info.total_blocks and scan.restart_interval == info.restart_interval, name
        assert scan.bytes == 0 and scan.seg_start == 0 and scan.coef_offset == 0                 # the caller's to set
    assert seen_ff > 0 and seen_segments > 8                                                    # stuffing and restarts are in the fixtures


def test_scan_tables_are_the_headers(lib):
    """The tables of the record against `_Huffman` of the Python parser: the slow path's arrays and the 9-bit look-up."""
    for name in ("80x72_420", "33x31_444", "64x48_gray", "256x192_422"):
        _, data, _ = next(c for c in jpeghuff.supported() if c[0].startswith(name))
        hd = jf._parse(data)
        scan = jpeghuff.c_prepare(lib, data)[3]
        for c in range(len(hd.ids)):
            for got, want in ((scan.dc[c], hd.dc[hd.td[c]]), (scan.ac[c], hd.ac[hd.ta[c]])):
                assert list(got.counts) == want.counts and list(got.first)[1:] == want.first[1:] and list(got.index)[1:] == want.index[1:]
                assert bytes(got.values)[:len(want.values)] == bytes(want.values)
                look = jh._look16(want)
                for prefix in range(512):
                    e = look[prefix << 7]
                    assert got.look[prefix] == (e if (e >> 8) <= 9 else 0), (name, c, prefix)
        for c in range(len(hd.ids), 3):
            assert not any(bytes(scan.dc[c])) and not any(bytes(scan.ac[c])), name


def _markers(F):
    scan = F.index(b"\xff\xda")
    return [i for i in range(scan, len(F) - 1) if F[i] == 0xFF and 0xD0 <= F[i + 1] <= 0xD7]


def test_scan_prepare_restart_marker_faults(lib):
    F = next(data for name, data, _ in jpegdec.supported() if "rst3" in name and len(_markers(data)) >= 3)
    at = _markers(F)
    assert _same_prepare(lib, F, "as it is") == OK
    swapped = bytearray(F)
    swapped[at[0] + 1], swapped[at[1] + 1] = F[at[1] + 1], F[at[0] + 1]
    faults = {
        "out of order": bytes(swapped),
        "missing": F[:at[1]] + F[at[1] + 2:],
        "surplus": F[:at[1]] + F[at[1]:at[1] + 2] + F[at[1]:],
        "surplus, another number": F[:at[0] + 2] + b"\xff\xd5" + F[at[0] + 2:],
        "cut inside a marker": F[:at[1] + 1],
        "cut in front of a marker": F[:at[1]],
        "EOI in place of a marker": F[:at[1]] + b"\xff\xd9",
    }
    for what, data in faults.items():
        assert _same_prepare(lib, data, what) == ERR_FORMAT, what
        assert _sequential(data)[0] == ERR_FORMAT, what                                         # and the sequential decoder agrees
    # the last segment ends at any marker or with the file, as the sequential reader ends the data: what is missing there is the
    # decoder's to find, and a marker behind complete data is accepted by both
    last = at[-1] + 2
    for what, data, verdict in (("a surplus marker inside the last segment", F[:last + 1] + b"\xff\xd0" + F[last + 1:], ERR_FORMAT),
                                ("a surplus marker behind the last segment", F[:-2] + b"\xff\xd3" + F[-2:], OK),
                                ("the file ends inside the last segment", F[:last + 1], ERR_FORMAT)):
        assert _same_prepare(lib, data, what) == OK, what
        assert _sequential(data)[0] == verdict and _model(data, 4, 4)[0] == verdict, what


def test_scan_prepare_on_the_hostile_corpus(lib):
    """Every flipped byte and every prefix: the library's preparation and the Python one agree in verdict and bytes."""
    seen = {OK: 0, ERR_FORMAT: 0}
    for what, data in jpeghuff.corpus():
        seen[_same_prepare(lib, data, what)] += 1
    assert seen[OK] > 0 and seen[ERR_FORMAT] > 0


def test_scan_prepare_capacity_and_argument_checks(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    info, out, start, scan = jpeghuff.c_prepare(lib, data)
    assert scan.n_seg > 1 and 0xFF in out
    exact = jpeghuff.c_prepare(lib, data, bytes_cap=out.size, seg_cap=start.size)                # at the exact capacities
    assert not isinstance(exact, int) and np.array_equal(exact[1], out) and np.array_equal(exact[2], start)
    assert jpeghuff.c_prepare(lib, data, bytes_cap=out.size - 1) == ERR_WORKSPACE                  # one byte short
    assert jpeghuff.c_prepare(lib, data, seg_cap=start.size - 1) == ERR_WORKSPACE                  # one entry short
    assert jpeghuff.c_prepare(lib, data, bytes_cap=0) == ERR_WORKSPACE
    # a file whose last data byte is a stuffed FF: the byte written behind a copied run is checked on its own
    _, plain, _ = jpegdec.case("16x16_420")
    stuffed = plain[:-2] + b"\xff\x00" + plain[-2:]
    full = jpeghuff.c_prepare(lib, stuffed)
    assert full[1][-1] == 0xFF and jpeghuff.c_prepare(lib, stuffed, bytes_cap=full[1].size - 1) == ERR_WORKSPACE
    assert not isinstance(jpeghuff.c_prepare(lib, stuffed, bytes_cap=full[1].size), int)
    buf, seg, rec = np.zeros(len(data), np.uint8), np.zeros(start.size, np.uint32), abi.FearJpegScan()
    args = [data, len(data), ctypes.byref(info), buf.ctypes.data, buf.size, seg.ctypes.data, seg.size, ctypes.byref(rec)]
    assert lib.fear_jpeg_scan_prepare(*args) == OK
    for k in (0, 2, 3, 5, 7):
        bad = list(args)
        bad[k] = None
        assert lib.fear_jpeg_scan_prepare(*bad) == ERR_NULL, k
    other = abi.FearJpegInfo()
    assert lib.fear_jpeg_parse(plain, len(plain), ctypes.byref(other)) == OK
    args[2] = ctypes.byref(other)
    assert lib.fear_jpeg_scan_prepare(*args) == ERR_SHAPE
    # the device call's checks that come before any launch
    assert lib.fear_jpeg_huffman(None, 0, None, None, None, 128, None) == OK
    assert lib.fear_jpeg_huffman(None, 1, None, None, None, 128, None) == ERR_NULL
    for n, sb in ((-1, 128), (65536, 128), (1, 0), (1, 2), (1, 6), (1, 1028), (1, -4)):
        assert lib.fear_jpeg_huffman(None, n, None, None, None, sb, None) == ERR_SHAPE, (n, sb)
    assert lib.fear_jpeg_dense_block_start(None, 4, None) == ERR_NULL
