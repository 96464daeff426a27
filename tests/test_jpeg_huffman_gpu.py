"""The Huffman stage of the JPEG frame decoder on the GPU (include/fear_train.h: fear_jpeg_huffman): the operator
through the C ABI against the host library's fear_jpeg_entropy_decode — the same coefficients with `==` on every file of both fixtures, in
one ragged call and one by one, at three subsequence lengths, and through the unchanged fear_jpeg_decode_u8 Pillow's recorded pixels byte
for byte; the host library's verdict on every flipped byte and every prefix of a file; its argument checks; and
`JpegDecoder(entropy="device")` against `entropy="host"`."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec
import jpeghuff
from dataops import GUARD, P, SENTINEL_U8, equal as _equal, guarded, inner, inside
from jpegdec import ERR_FORMAT, ERR_NULL, ERR_SHAPE, OK
from feartracker_amd import JpegDecoder, MalformedJPEG, UnsupportedJPEG
from feartracker_amd import train_abi as abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


@pytest.fixture(scope="module")
def sequential(lib):
    """{name: the unpacked output of fear_jpeg_entropy_decode} for every supported file, computed once and shared."""
    return {name: jpegdec.unpack(*jpegdec.c_decode(lib, data)) for name, data, _ in jpeghuff.supported()}


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _huffman(lib, files, subsequence_bytes):
    """fear_jpeg_huffman on the files in one call: the host's preparation through the C ABI, one upload, guard bands around the
    coefficients.  Returns (statuses, [FearJpegInfo], [flat dense coefficients], the device buffers that hold them)."""
    prepared = [jpeghuff.c_prepare(lib, data) for data in files]
    assert not any(isinstance(p, int) for p in prepared)
    n = len(prepared)
    records, host, at, table_at, records_at, values = jpeghuff.huffman_layout(prepared)
    up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
    jpeghuff.finish_layout(records, host, at, table_at, records_at, up.data_ptr())
    up.copy_(torch.from_numpy(host))
    coef = guarded(2 * values)
    status = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
    rc = lib.fear_jpeg_huffman(records, n, P(up.data_ptr() + table_at), inner(coef), P(status.data_ptr()), subsequence_bytes, _stream())
    assert rc == OK
    torch.cuda.synchronize()
    flat = inside(coef, 2 * values, "coefficients").view(np.int16)
    st = status.cpu().numpy()
    assert st[n] == 77 and st[n + 1] == 77, "a status behind the last image written"
    infos = [p[0] for p in prepared]
    dense = [flat[records[k].coef_offset:records[k].coef_offset + 64 * infos[k].total_blocks] for k in range(n)]
    return st[:n], infos, dense, (coef, records, up)


def _pixels(lib, infos, keep):
    """The unchanged fear_jpeg_decode_u8 on the dense coefficients still on the device: every image's record points at its own
    coefficients and at the one shared block_start table 0, 64, 128, ..."""
    coef, scans, _ = keep
    n = len(infos)
    dummy = (np.zeros(1, np.int16), np.zeros(1, np.uint32))
    records, jinfos, prefix, at, _, out_bytes = jpegdec.call_layout([(info,) + dummy for info in infos])
    most = max(info.total_blocks for info in infos)
    start = torch.full((most + 1 + 16,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    assert lib.fear_jpeg_dense_block_start(P(start.data_ptr()), most, _stream()) == OK
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(jinfos, n)
    ws = guarded(ws_bytes)
    for k in range(n):
        records[k].coef = coef.data_ptr() + GUARD + 2 * scans[k].coef_offset
        records[k].block_start = start.data_ptr()
        records[k].out = out.data_ptr() + GUARD + at["out"][k]
    table = torch.from_numpy(jpegdec.table_bytes(prefix, records)).cuda()
    assert lib.fear_jpeg_decode_u8(records, n, P(table.data_ptr()), inner(ws), ws_bytes, _stream()) == OK
    torch.cuda.synchronize()
    got = start.cpu().numpy()
    assert np.array_equal(got[:most + 1], 64 * np.arange(most + 1)) and np.all(got[most + 1:] == 0x7FFFFFFF)
    inside(ws, ws_bytes, "workspace")
    flat = inside(out, out_bytes)
    return [flat[at["out"][k]:at["out"][k] + info.height * info.width * 3].reshape(info.height, info.width, 3) for k, info in enumerate(infos)]


def _check_coefficients(cases, infos, dense, sequential, what):
    for (name, _, _), info, flat in zip(cases, infos, dense):
        for c, (a, b) in enumerate(zip(jpeghuff.dense(info, flat), sequential[name])):
            assert a.shape == b.shape and bool((a == b).all()), f"{what} {name}: component {c}: {int((a != b).sum())} values differ"


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_every_file_in_one_ragged_call(lib, sequential, subsequence_bytes):
    """Both fixtures in one call.  At 4 bytes the 13 kB file has about 3 500 subsequences in 14 sequences; the random files run every
    round; the restart files have one workgroup per segment."""
    cases = jpeghuff.supported()
    status, infos, dense, keep = _huffman(lib, [data for _, data, _ in cases], subsequence_bytes)
    assert not status.any(), [(cases[k][0], int(status[k])) for k in np.flatnonzero(status)]
    _check_coefficients(cases, infos, dense, sequential, f"{subsequence_bytes} bytes")
    for got, (name, _, px) in zip(_pixels(lib, infos, keep), cases):
        assert got.shape == px.shape and np.array_equal(got, px), f"{name}: pixels differ from Pillow's"


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_every_file_on_its_own(lib, sequential, subsequence_bytes):
    for case in jpeghuff.supported():
        status, infos, dense, keep = _huffman(lib, [case[1]], subsequence_bytes)
        assert status[0] == OK, case[0]
        _check_coefficients([case], infos, dense, sequential, f"{subsequence_bytes} bytes, alone:")
    got = _pixels(lib, infos, keep)[0]                                                 # (the last file through the pixel stage alone)
    assert np.array_equal(got, case[2])


def test_hostile_corpus_gets_the_host_librarys_verdict(lib):
    """Every flipped entropy byte and every prefix of the 16 x 16 4:2:0 file that gets as far as the device — the header and marker
    faults are the host's — in one ragged call: the status fear_jpeg_entropy_decode returns, and its coefficients where it accepts."""
    files, want = [], []
    for what, data in jpeghuff.corpus():
        if isinstance(jpeghuff.c_prepare(lib, data), int):
            assert isinstance(jpegdec.c_decode(lib, data), int), what                 # refused before any launch, and the host agrees
            continue
        files.append((what, data))
        want.append(jpegdec.c_decode(lib, data))
    assert len(files) > 1000
    for subsequence_bytes in (4, 128):
        status, infos, dense, _ = _huffman(lib, [data for _, data in files], subsequence_bytes)   # the call returns and the stream synchronises
        accepted = 0
        for k, ((what, _), ref) in enumerate(zip(files, want)):
            assert status[k] == (ref if isinstance(ref, int) else OK), f"{what}: device {status[k]}, host {ref if isinstance(ref, int) else OK}"
            if not isinstance(ref, int):
                accepted += 1
                for a, b in zip(jpeghuff.dense(infos[k], dense[k]), jpegdec.unpack(*ref)):
                    assert bool((a == b).all()), what
        assert 100 < accepted < len(files) - 100
        assert set(np.unique(status)) == {OK, ERR_FORMAT}


def test_huffman_argument_checks(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    prepared = [jpeghuff.c_prepare(lib, data)]
    records, host, at, table_at, records_at, values = jpeghuff.huffman_layout(prepared)
    up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
    coef = guarded(2 * values)
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    table = P(up.data_ptr() + table_at)

    def call(n=1, scans=records, table=table, out=inner(coef), st=P(status.data_ptr()), sb=128):
        return lib.fear_jpeg_huffman(scans, n, table, out, st, sb, _stream())

    def with_field(**fields):
        saved = {k: getattr(records[0], k) for k in fields}
        for k, v in fields.items():
            setattr(records[0], k, v)
        rc = call()
        for k, v in saved.items():
            setattr(records[0], k, v)
        return rc

    assert call() == ERR_NULL                                                        # the record's addresses are still null
    jpeghuff.finish_layout(records, host, at, table_at, records_at, up.data_ptr())
    up.copy_(torch.from_numpy(host))
    assert call(n=0, scans=None, table=None, out=None, st=None) == OK
    assert call(n=-1) == ERR_SHAPE and call(n=65536) == ERR_SHAPE
    for sb in (0, 2, 6, 130, 1028, -128):
        assert call(sb=sb) == ERR_SHAPE, sb
    assert call(scans=None) == ERR_NULL and call(table=None) == ERR_NULL and call(out=None) == ERR_NULL and call(st=None) == ERR_NULL
    assert with_field(bytes=0) == ERR_NULL and with_field(seg_start=0) == ERR_NULL
    for bad in (dict(components=2), dict(h=3), dict(h=1, v=2), dict(mcus_x=0), dict(mcus_y=1025), dict(restart_interval=-1),
                dict(restart_interval=65536), dict(n_seg=records[0].n_seg + 1), dict(total_blocks=records[0].total_blocks - 1),
                dict(bytes=records[0].bytes + 1), dict(max_seg_bytes=abi.FEAR_JPEG_DEVICE_SCAN_MAX + 1), dict(max_seg_bytes=records[0].n_bytes + 1)):
        assert with_field(**bad) == ERR_SHAPE, bad
    assert lib.fear_jpeg_dense_block_start(None, 4, _stream()) == ERR_NULL
    assert lib.fear_jpeg_dense_block_start(P(up.data_ptr()), 3 * 1024 * 1024 + 1, _stream()) == ERR_SHAPE
    torch.cuda.synchronize()
    inside(coef, 2 * values, "coefficients")
    assert bool((inside(coef, 2 * values) == SENTINEL_U8).all()) and int(status[0]) == 77    # none of the refused calls launched anything
    assert call() == OK
    torch.cuda.synchronize()
    assert int(status[0]) == OK and not bool((inside(coef, 2 * values) == SENTINEL_U8).all())


# --------------------------------------------------------------------------------------------------------- JpegDecoder(entropy="device")
@pytest.fixture(scope="module")
def decoders():
    host, device = JpegDecoder(device=0, threads=4), JpegDecoder(device=0, threads=4, entropy="device")
    yield host, device
    host.close()
    device.close()


def test_device_frames_equal_host_frames(decoders):
    host, device = decoders
    cases = jpeghuff.supported()
    files = [data for _, data, _ in cases]
    a, b = host.decode(files), device.decode(files, check=True)
    for (name, _, px), x, y in zip(cases, a, b):
        assert y.is_cuda and y.dtype == torch.uint8 and y.is_contiguous() and torch.equal(x, y), name
        assert np.array_equal(y.cpu().numpy(), px), name
    assert device.decode([]) == []
    device.check()                                                                    # nothing pending: returns


def test_device_decoder_never_waits_for_the_gpu(decoders):
    _, device = decoders
    cases = jpeghuff.supported()
    files = [data for _, data, _ in cases]
    device.decode(files[:3], check=True)                                              # (the allocators warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = device.decode(files)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    device.check()
    for f, (name, _, px) in zip(frames, cases):
        assert np.array_equal(f.cpu().numpy(), px), name


def test_truncated_entropy_passes_decode_and_fails_check(decoders):
    host, device = decoders
    good = jpegdec.case("16x16_420")[1]
    cut = good[:len(good) - 40]                                                       # the headers are whole, the entropy data is not
    with pytest.raises(MalformedJPEG):
        host.decode([good, cut])
    frames = device.decode([good, cut, good])                                         # no wait, so no verdict yet
    assert len(frames) == 3 and torch.equal(frames[0], frames[2])
    with pytest.raises(MalformedJPEG, match="item 1"):
        device.check()
    device.check()                                                                    # the failed call is checked and done with
    with pytest.raises(MalformedJPEG, match="item 0"):
        device.decode([cut, good], check=True)
    assert np.array_equal(device.decode([good], check=True)[0].cpu().numpy(), jpegdec.case("16x16_420")[2])


def test_header_fault_raises_and_launches_nothing(decoders, monkeypatch):
    _, device = decoders
    good = jpegdec.case("16x16_420")[1]
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    with pytest.raises(MalformedJPEG):
        device.decode([good, good[:400]], fallback=lambda data: np.zeros((16, 16, 3), np.uint8))
    rst = next(data for name, data, _ in jpegdec.supported() if "rst3" in name and data.count(b"\xff\xd1") == 1)
    with pytest.raises(MalformedJPEG, match="restart marker"):
        device.decode([good, rst.replace(b"\xff\xd1", b"\xff\xd2")])                   # a marker fault is the host's to find
    assert launched == []
    device.decode([good], check=True)
    assert launched == ["fear_jpeg_dense_block_start", "fear_jpeg_huffman", "fear_jpeg_decode_u8"]


def test_progressive_file_reaches_the_fallback_in_device_mode(decoders):
    _, device = decoders
    prog = jpegdec.case("33x31_420_smooth_q75_progressive")
    plain = next(c for c in jpegdec.supported() if c[0].startswith("33x31_420"))
    with pytest.raises(UnsupportedJPEG, match="progressive"):
        device.decode([plain[1], prog[1]])
    seen = []

    def fallback(data):
        seen.append(data)
        return prog[2]

    frames = device.decode([plain[1], prog[1], plain[1]], fallback=fallback, check=True)
    assert seen == [prog[1]]
    for f, c in zip(frames, (plain, prog, plain)):
        assert np.array_equal(f.cpu().numpy(), c[2])
    only = device.decode([prog[1]], fallback=fallback, check=True)
    assert np.array_equal(only[0].cpu().numpy(), prog[2])


def test_a_tiny_workspace_limit_splits_the_call(decoders, monkeypatch):
    _, device = decoders
    cases = jpeghuff.entropy_cases() + jpegdec.supported()[::5]
    files = [data for _, data, _ in cases]
    whole = device.decode(files, check=True)
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    small = JpegDecoder(device=0, threads=2, entropy="device", workspace_limit=300_000)   # a 256 x 192 4:4:4 file needs 294 912 bytes dense
    try:
        parts = small.decode(files, check=True)
        one = JpegDecoder(device=0, threads=2, entropy="device", workspace_limit=1)        # every image is its own group
        alone = one.decode(files[:4], check=True)
        one.close()
    finally:
        small.close()
    assert launched.count("fear_jpeg_huffman") >= 4 + 4 and launched.count("fear_jpeg_huffman") == launched.count("fear_jpeg_decode_u8")
    for x, y in zip(whole, parts):
        assert torch.equal(x, y)
    for x, y in zip(whole, alone):
        assert torch.equal(x, y)


def test_an_oversize_scan_goes_through_the_host_stage(decoders, monkeypatch):
    """A file above the device's limit rides along through fear_jpeg_entropy_decode in the same call (the limit lowered for the test)."""
    from feartracker_amd import jpeg_frames
    cases = jpeghuff.entropy_cases()[:4]
    files = [data for _, data, _ in cases]
    monkeypatch.setattr(jpeg_frames, "DEVICE_SCAN_MAX", 10_000)                          # two of the four files are longer
    mixed = JpegDecoder(device=0, threads=2, entropy="device")
    try:
        frames = mixed.decode(files, check=True)
        assert sorted(mixed.last_paths) == ["device", "device", "host", "host"]
    finally:
        mixed.close()
    for f, (name, _, px) in zip(frames, cases):
        assert np.array_equal(f.cpu().numpy(), px), name


def test_train_pairs_from_device_decoded_frames(decoders):
    from feartracker_amd.train_data import TrainPairBuilder
    _, device = decoders
    cases = [jpegdec.case("64x48_444_random_q100_plain2"), jpegdec.case("80x72_420"), jpegdec.case("64x48_gray"), jpegdec.case("80x72_422")]
    B = 4
    rng = np.random.default_rng(3)
    pairs = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % 4), (5, (k + 1) % 4)):
            h, w = cases[f][2].shape[:2]
            bw, bh = rng.integers(8, w // 2), rng.integers(8, h // 2)
            pairs[k, col:col + 5] = [f, rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1), bw, bh]
        pairs[k, 10] = 1
    builder = TrainPairBuilder(device=0)
    params = builder.draw(pairs, [c[2].shape[:2] for c in cases], np.random.default_rng(7))
    frames = device.decode([c[1] for c in cases], check=True)
    dev = builder.build(frames, pairs, params)
    ref = builder.build([np.ascontiguousarray(c[2]) for c in cases], pairs, params)
    torch.cuda.synchronize()
    _equal(dev, ref)
