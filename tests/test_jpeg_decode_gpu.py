"""The JPEG frame decoder on the GPU (include/fear_train.h: fear_jpeg_decode_u8): the operator through the C ABI
against Pillow's recorded pixels (tests/golden/jpeg_decode.npz), byte for byte — every case in one ragged call and one by one, with a
guard band around every frame and the workspace; its argument checks; `JpegDecoder.decode` from bytes and paths, its fallback and its
errors; and `TrainPairBuilder.build` on decoded frames."""
import numpy as np
import pytest
import torch

import jpegdec
from dataops import GUARD, P, SENTINEL_U8, equal as _equal, guarded, inner, inside
from jpegdec import ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, OK
from feartracker_amd import JpegDecoder, MalformedJPEG, UnsupportedJPEG
from feartracker_amd import train_abi as abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


def _run(lib, files):
    """fear_jpeg_decode_u8 on the files in one call: the host stage through the C ABI, one upload, the guard bands around the workspace
    and around every output frame checked.  Returns the frames."""
    decoded = [jpegdec.c_decode(lib, data) for data in files]
    n = len(decoded)
    records, infos, prefix, at, up_bytes, out_bytes = jpegdec.call_layout(decoded)
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
    rc = lib.fear_jpeg_decode_u8(records, n, P(up.data_ptr() + table_at), inner(ws), ws_bytes, P(torch.cuda.current_stream().cuda_stream))
    assert rc == OK
    torch.cuda.synchronize()
    inside(ws, ws_bytes, "workspace")
    flat = inside(out, out_bytes)
    frames, covered = [], np.zeros(out_bytes, dtype=bool)
    for k, (info, _, _) in enumerate(decoded):
        size = info.height * info.width * 3
        frames.append(flat[at["out"][k]:at["out"][k] + size].reshape(info.height, info.width, 3))
        covered[at["out"][k]:at["out"][k] + size] = True
    assert np.all(flat[~covered] == SENTINEL_U8), "the gap between two frames written"
    return frames


def _check(frames, cases):
    for got, (name, _, px) in zip(frames, cases):
        assert got.shape == px.shape, name
        bad = np.argwhere(got != px)
        assert bad.size == 0, f"{name}: {len(bad)} of {px.size} bytes differ, first at {bad[:3].tolist()}"


def test_every_case_in_one_ragged_call(lib):
    cases = jpegdec.supported()
    assert len(cases) == 43
    _check(_run(lib, [data for _, data, _ in cases]), cases)
    _check(_run(lib, [data for _, data, _ in reversed(cases)]), list(reversed(cases)))


def test_every_case_on_its_own(lib):
    for case in jpegdec.supported():
        _check(_run(lib, [case[1]]), [case])


def test_argument_checks(lib):
    name, data, px = jpegdec.case("17x23_420")
    decoded = [jpegdec.c_decode(lib, data)]
    records, infos, prefix, at, up_bytes, out_bytes = jpegdec.call_layout(decoded)
    st = P(torch.cuda.current_stream().cuda_stream)
    up = torch.zeros(up_bytes + 1024, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, 1)
    ws = guarded(ws_bytes)
    table = P(up.data_ptr())

    def call(n=1, images=records, table=table, workspace=inner(ws), nbytes=ws_bytes):
        return lib.fear_jpeg_decode_u8(images, n, table, workspace, nbytes, st)

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
    assert call(n=0, images=None, table=None, workspace=None, nbytes=0) == OK
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


@pytest.fixture(scope="module")
def decoder():
    d = JpegDecoder(device=0, threads=4)
    yield d
    d.close()


def test_decoder_never_waits_for_the_gpu(decoder):
    cases = jpegdec.supported()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = decoder.decode([data for _, data, _ in cases])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(frames) == len(cases)
    for f in frames:
        assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and f.dim() == 3 and f.shape[2] == 3
    _check([f.cpu().numpy() for f in frames], cases)
    assert decoder.decode([]) == []


def test_decoder_reads_paths(decoder, tmp_path):
    cases = jpegdec.supported()[5:12]
    items = []
    for i, (name, data, _) in enumerate(cases):
        if i % 2:
            items.append(data)
        else:
            path = tmp_path / f"{name}.jpg"
            path.write_bytes(data)
            items.append(path if i % 4 else str(path))
    _check([f.cpu().numpy() for f in decoder.decode(items)], cases)


def test_progressive_file_reaches_the_fallback(decoder):
    prog = jpegdec.case("33x31_420_smooth_q75_progressive")
    plain = next(c for c in jpegdec.supported() if c[0].startswith("33x31_420"))
    with pytest.raises(UnsupportedJPEG, match="progressive"):
        decoder.decode([plain[1], prog[1]])
    seen = []

    def fallback(data):
        seen.append(data)
        return prog[2]

    frames = decoder.decode([plain[1], prog[1], plain[1]], fallback=fallback)
    assert seen == [prog[1]]
    _check([f.cpu().numpy() for f in frames], [plain, prog, plain])
    only = decoder.decode([prog[1]], fallback=fallback)                              # a call with nothing for the kernels
    _check([only[0].cpu().numpy()], [prog])


def test_truncated_file_raises_and_launches_nothing(decoder, monkeypatch):
    good, cut = jpegdec.case("16x16_420")[1], jpegdec.case("16x16_420")[1][:400]
    launched = []
    real = decoder._lib.fear_jpeg_decode_u8
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(*args))
    with pytest.raises(MalformedJPEG):
        decoder.decode([good, cut], fallback=lambda data: np.zeros((16, 16, 3), np.uint8))
    assert launched == []
    decoder.decode([good])
    assert launched == ["fear_jpeg_decode_u8"]                                      # (the probe sees a call that does launch)


def test_train_pairs_from_decoded_frames(decoder):
    from feartracker_amd.train_data import TrainPairBuilder
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
    frames = decoder.decode([c[1] for c in cases])
    dev = builder.build(frames, pairs, params)
    ref = builder.build([np.ascontiguousarray(c[2]) for c in cases], pairs, params)
    torch.cuda.synchronize()
    _equal(dev, ref)
