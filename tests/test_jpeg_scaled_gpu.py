"""Reduced-size JPEG decoding on the GPU (include/fear_train.h: fear_jpeg_decode_scaled_u8; DESIGN.md section 14, "Reduced-size
decoding"): the operator through the C ABI against Pillow's recorded `draft` pixels (tests/golden/jpeg_scaled.npz) — or the host model
for the 16 pairs `draft` cannot take — byte for byte, per scale every file in one ragged call, in reverse order and one by one, with a
guard band around the workspace and every frame; its argument checks; `JpegDecoder.decode(scale=)` in both entropy modes and with a
fallback; `JpegStore.decode(ids, scale=)` and `decode_rows(ids, rows, scale=)`; and `TrainPairBuilder.build` on scaled frames."""
import numpy as np
import pytest
import torch

import jpegdec
import jpegscaled
from dataops import GUARD, P, SENTINEL_U8, equal as _equal, guarded, inner, inside
from jpegdec import ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, OK
from jpegscaled import SCALES
from feartracker_amd import JpegDecoder, JpegStore, UnsupportedJPEG, jpeg_scaled_shape
from feartracker_amd import train_abi as abi
from feartracker_amd.train_data import TrainPairBuilder, scale_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


_decoded = {}


def _c_decode(lib, name, data):
    if name not in _decoded:
        _decoded[name] = jpegdec.c_decode(lib, data)
    return _decoded[name]


def _layout(decoded, scale):
    """jpegdec.call_layout with the second prefix table counting scaled pixels; the frames keep the full-size gaps between them."""
    records, infos, prefix, at, up_bytes, out_bytes = jpegdec.call_layout(decoded)
    for k, (info, _, _) in enumerate(decoded):
        h, w, _ = jpeg_scaled_shape(info.height, info.width, scale)
        prefix[1, k + 1] = prefix[1, k] + -(-h * w // abi.FEAR_JPEG_GROUP_PIXELS)
    return records, infos, prefix, at, up_bytes, out_bytes


def _run(lib, files, scale):
    """fear_jpeg_decode_scaled_u8 on the files in one call, the guard bands around the workspace and around every scaled frame
    checked.  Returns the frames."""
    decoded = [_c_decode(lib, name, data) for name, data in files]
    n = len(decoded)
    records, infos, prefix, at, up_bytes, out_bytes = _layout(decoded, scale)
    table_at = up_bytes
    host = np.zeros(up_bytes + jpegdec.table_bytes(prefix, records).nbytes, dtype=np.uint8)
    up = torch.empty(host.nbytes, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, n)
    ws = guarded(ws_bytes)
    for k, (info, coef, start) in enumerate(decoded):
        records[k].coef = up.data_ptr() + at["coef"][k]
        records[k].block_start = up.data_ptr() + at["start"][k]
        records[k].out = out.data_ptr() + GUARD + at["out"][k]
        host[at["coef"][k]:at["coef"][k] + coef.nbytes] = coef.view(np.uint8)
        host[at["start"][k]:at["start"][k] + start.nbytes] = start.view(np.uint8)
    host[table_at:] = jpegdec.table_bytes(prefix, records)
    up.copy_(torch.from_numpy(host))
    rc = lib.fear_jpeg_decode_scaled_u8(records, n, P(up.data_ptr() + table_at), scale, inner(ws), ws_bytes,
                                        P(torch.cuda.current_stream().cuda_stream))
    assert rc == OK
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    flat = inside(out, out_bytes)
    frames, covered = [], np.zeros(out_bytes, dtype=bool)
    for k, (info, _, _) in enumerate(decoded):
        h, w, _ = jpeg_scaled_shape(info.height, info.width, scale)
        frames.append(flat[at["out"][k]:at["out"][k] + h * w * 3].reshape(h, w, 3))
        covered[at["out"][k]:at["out"][k] + h * w * 3] = True
    assert np.all(flat[~covered] == SENTINEL_U8), "bytes behind a scaled frame written"
    return frames, prefix


def _check(frames, files, scale):
    for got, (name, data) in zip(frames, files):
        want, _ = jpegscaled.expected(name, data, scale)
        assert got.shape == want.shape, (name, scale)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name} at 1/{scale}: {len(bad)} of {want.size} bytes differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("scale", SCALES)
def test_every_file_in_one_ragged_call_and_in_reverse(lib, scale):
    files = jpegscaled.files()
    assert len(files) == 47
    frames, prefix = _run(lib, files, scale)
    _check(frames, files, scale)
    groups = np.diff(prefix.astype(np.int64), axis=1)
    assert groups[0].max() >= 5 and groups[0].min() == 1                               # several workgroups of blocks, and one
    if scale == 2:
        assert groups[1].max() >= 5                                                    # several workgroups of scaled pixels
    back = files[::-1]
    _check(_run(lib, back, scale)[0], back, scale)


@pytest.mark.parametrize("scale", SCALES)
def test_every_file_on_its_own(lib, scale):
    for one in jpegscaled.files():
        _check(_run(lib, [one], scale)[0], [one], scale)


def test_argument_checks(lib):
    name, data, _ = jpegdec.case("17x23_420")
    decoded = [_c_decode(lib, name, data)]
    records, infos, prefix, at, up_bytes, out_bytes = _layout(decoded, 2)
    st = P(torch.cuda.current_stream().cuda_stream)
    up = torch.zeros(up_bytes + 1024, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, 1)
    ws = guarded(ws_bytes)
    table = P(up.data_ptr())

    def call(n=1, images=records, table=table, scale=2, workspace=inner(ws), nbytes=ws_bytes):
        return lib.fear_jpeg_decode_scaled_u8(images, n, table, scale, workspace, nbytes, st)

    def with_field(**fields):
        saved = {k: getattr(records[0], k) for k in fields}
        for k, v in fields.items():
            setattr(records[0], k, v)
        rc = call()
        for k, v in saved.items():
            setattr(records[0], k, v)
        return rc

    assert call() == ERR_NULL                                                        # the record's pointers are still null
    records[0].coef, records[0].block_start, records[0].out = up.data_ptr(), up.data_ptr(), out.data_ptr() + GUARD
    for bad in (1, 0, 3, 5, 16, -2, 256 + 2):
        assert call(scale=bad) == ERR_SHAPE, bad
        assert call(n=0, images=None, table=None, scale=bad, workspace=None, nbytes=0) == ERR_SHAPE, bad
    for scale in SCALES:
        assert call(n=0, images=None, table=None, scale=scale, workspace=None, nbytes=0) == OK
    assert call(n=-1) == ERR_SHAPE and call(n=65536) == ERR_SHAPE
    assert call(images=None) == ERR_NULL and call(table=None) == ERR_NULL
    assert with_field(out=0) == ERR_NULL and with_field(coef=0) == ERR_NULL and with_field(block_start=0) == ERR_NULL
    assert call(workspace=None) == ERR_WORKSPACE and call(nbytes=ws_bytes - 1) == ERR_WORKSPACE and call(nbytes=0) == ERR_WORKSPACE
    assert with_field(plane_offset=16) == ERR_WORKSPACE and with_field(plane_offset=8) == ERR_SHAPE
    for bad in (dict(width=0), dict(height=0), dict(width=8193), dict(components=2), dict(components=4), dict(h=3), dict(h=1, v=2),
                dict(components=1, h=2, v=2)):
        assert with_field(**bad) == ERR_SHAPE, bad
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    inside(out, out_bytes)                                                           # none of the refused calls launched anything


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_decoder_at_a_scale(entropy, monkeypatch):
    files = jpegscaled.files(progressive=True)
    decoder = JpegDecoder(device=0, threads=4, entropy=entropy, progressive=True)
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    try:
        for scale in SCALES:
            del launched[:]
            frames = decoder.decode([data for _, data in files], check=True, scale=scale)
            assert launched.count("fear_jpeg_decode_scaled_u8") == 1 and "fear_jpeg_decode_u8" not in launched
            for f in frames:
                assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous()
            _check([f.cpu().numpy() for f in frames], files, scale)
        del launched[:]
        name, data, px = jpegdec.case("33x31_444")
        assert np.array_equal(decoder.decode([data], scale=1)[0].cpu().numpy(), px)
        assert launched[-1] == "fear_jpeg_decode_u8" and "fear_jpeg_decode_scaled_u8" not in launched
        del launched[:]
        for bad in (0, 3, 16, "2", 2.0):
            with pytest.raises(ValueError, match="scale"):
                decoder.decode([b"not parsed at all"], scale=bad)
        assert launched == []
    finally:
        decoder.close()


def test_decoder_fallback_at_a_scale():
    prog_name, prog = jpegscaled.new_files()[-1]
    assert "progressive" in prog_name
    plain = jpegscaled.files()[20]
    want, pinned = jpegscaled.expected(prog_name, prog, 4)
    assert pinned
    decoder = JpegDecoder(device=0, threads=2)                                       # progressive files are unsupported here
    try:
        with pytest.raises(UnsupportedJPEG, match="progressive"):
            decoder.decode([plain[1], prog], scale=4)
        frames = decoder.decode([plain[1], prog, plain[1]], fallback=lambda data: np.array(want), scale=4)
        _check([f.cpu().numpy() for f in frames], [plain, (prog_name, prog), plain], 4)
        full, _ = jpegscaled.expected(prog_name, prog, 2)
        with pytest.raises(ValueError, match="item 1"):
            decoder.decode([plain[1], prog], fallback=lambda data: np.array(full), scale=4)   # the shape of another scale
    finally:
        decoder.close()


@pytest.fixture(scope="module")
def store():
    files = jpegscaled.files(progressive=True)
    s = JpegStore(device=0, threads=4, progressive=True)
    ids = s.add([data for _, data in files])
    assert (s.kinds[ids] == "scan").all()                                            # the progressive twin is a transcoded scan entry
    yield s, files, ids
    s.close()


@pytest.mark.parametrize("scale", SCALES)
def test_store_decode_at_a_scale(store, scale):
    s, files, ids = store
    rng = np.random.default_rng(scale)
    order = np.concatenate([rng.permutation(len(files)), rng.integers(0, len(files), 9), [len(files) - 1]])      # shuffled, with repeats
    frames = s.decode(ids[order], check=True, scale=scale)
    _check([f.cpu().numpy() for f in frames], [files[i] for i in order], scale)
    shapes = s.shape(ids[order], scale=scale)
    assert shapes.dtype == np.int32 and [tuple(x) for x in shapes] == [tuple(f.shape[:2]) for f in frames]
    assert np.array_equal(s.shape(ids), s.shape(ids, scale=1))
    small = JpegStore(device=0, threads=2, workspace_limit=128 * 40)                 # several groups per call
    try:
        few = small.add([data for _, data in files[30:40]])
        _check([f.cpu().numpy() for f in small.decode(few[::-1], check=True, scale=scale)], files[30:40][::-1], scale)
    finally:
        small.close()


def test_store_refuses_pixel_entries_and_other_scales():
    prog_name, prog = jpegscaled.new_files()[-1]
    plain = jpegscaled.files()[20]
    s = JpegStore(device=0, threads=2)
    try:
        ids = s.add([plain[1], prog], fallback=lambda data: np.zeros((16, 48, 3), np.uint8))
        assert s.kinds.tolist() == ["scan", "pixels"]
        assert len(s.decode(ids)) == 2                                               # full size: copied as before
        for call in (lambda: s.decode(ids, scale=2), lambda: s.decode_rows(ids, [[0, 1], [0, 1]], scale=2)):
            with pytest.raises(UnsupportedJPEG, match=f"id {int(ids[1])}"):
                call()
        _check([s.decode(ids[:1], scale=2)[0].cpu().numpy()], [plain], 2)
        for bad in (0, 3, 16, 2.0):
            with pytest.raises(ValueError, match="scale"):
                s.decode(ids[:1], scale=bad)
            with pytest.raises(ValueError, match="scale"):
                s.decode_rows(ids[:1], [[0, 1]], scale=bad)
            with pytest.raises(ValueError, match="scale"):
                s.shape(ids[:1], scale=bad)
        rows = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="scale"):
            s.decode_rows(ids[:1], rows, scale=2)
    finally:
        s.close()


@pytest.mark.parametrize("scale", SCALES)
def test_store_decode_rows_at_a_scale(store, scale):
    """Bands at the first row, at the last row, interior rows and the empty band: the rows asked for are `decode(scale=)`'s."""
    s, files, ids = store
    full = [f.cpu().numpy() for f in s.decode(ids, check=True, scale=scale)]
    rng = np.random.default_rng(10 + scale)
    asked, which = [], []
    for k, frame in enumerate(full):
        H = frame.shape[0]
        mid = H // 2
        for y0, y1 in {(0, 1), (H - 1, H), (0, H), (mid, min(mid + 2, H)), (mid, mid), (H, H + 5), (-3, 1),
                       tuple(sorted(rng.integers(0, H + 1, 2).tolist()))}:
            which.append(k)
            asked.append((y0, y1))
    order = rng.permutation(len(which))
    which, asked = np.array(which)[order], np.array(asked)[order]
    frames = s.decode_rows(ids[which], asked, check=True, scale=scale)
    seen_empty = seen_inner = 0
    for k, (y0, y1), f in zip(which, asked, frames):
        want = full[k]
        assert tuple(f.shape) == want.shape, files[k][0]
        y0, y1 = min(max(y0, 0), want.shape[0]), min(max(y1, 0), want.shape[0])
        seen_empty += y0 >= y1
        seen_inner += 0 < y0 < y1 < want.shape[0]
        got = f.cpu().numpy()[y0:y1]
        bad = np.argwhere(got != want[y0:y1])
        assert bad.size == 0, f"{files[k][0]} at 1/{scale}, rows {y0}..{y1}: {len(bad)} bytes differ, first at {bad[:3].tolist()}"
    assert seen_empty > 40 and (seen_inner > 20 or scale == 8)


def test_train_pairs_from_scaled_frames(store):
    """`scale_pairs`, `frame_rows`, `decode_rows(scale=)` and `build(borders=)` on frames of half the size, against `build_host` on the
    same frames decoded whole."""
    s, files, ids = store
    names = [name for name, _ in files]
    picks = [names.index(jpegdec.case(p)[0]) for p in ("64x48_444_random_q100_plain2", "80x72_420", "64x48_gray", "80x72_422")]
    scale, B = 2, 4
    rng = np.random.default_rng(3)
    pairs = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % 4), (5, (k + 1) % 4)):
            w, h = (64, 48) if f in (0, 2) else (80, 72)
            bw, bh = rng.integers(16, w // 2), rng.integers(16, h // 2)
            pairs[k, col:col + 5] = [f, rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1), bw, bh]
        pairs[k, 10] = 1
    small = scale_pairs(pairs, scale)
    shapes = [tuple(x) for x in s.shape(ids[picks], scale=scale)]
    assert shapes == [(24, 32), (36, 40), (24, 32), (36, 40)]
    builder = TrainPairBuilder(device=0)
    params = builder.draw(small, shapes, np.random.default_rng(7))
    rows = builder.frame_rows(small, params, shapes)
    borders = s.borders(ids[picks])
    whole = s.decode(ids[picks], scale=scale)
    bands = s.decode_rows(ids[picks], rows, check=True, scale=scale)
    dev = builder.build(bands, small, params, borders=borders)
    ref = builder.build_host([f.cpu().numpy() for f in whole], small, params, borders=borders.cpu().numpy())
    torch.cuda.synchronize()
    _equal(dev, ref)
