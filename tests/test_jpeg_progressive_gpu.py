"""Progressive JPEG files through the product on the device ("Progressive files"): `JpegDecoder(progressive=True)`
in both entropy modes and `JpegStore(progressive=True)` — `add`, `decode`, `decode_rows`, `borders` — on every case of
tests/golden/jpeg_progressive.npz, byte for byte Pillow's pixels, mixed with baseline files; the launches of a store decode; a truncated
file in `add`."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec
import jpegprog
from jpegrows import windows
from feartracker_amd import JpegDecoder, JpegStore, MalformedJPEG, UnsupportedJPEG, jpeg_to_baseline_host
from feartracker_amd import train_abi as abi

pytestmark = pytest.mark.gpu


def _mixed():
    """Every progressive case with a baseline file after every third: [(name, file, pixels)]."""
    base = jpegdec.supported()
    out = []
    for k, (name, data, px, _) in enumerate(jpegprog.cases()):
        out.append((name, data, px))
        if k % 3 == 0:
            out.append(base[k % len(base)])
    return out


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_decoder_decodes_every_case_mixed_with_baseline_files(entropy):
    mixed = _mixed()
    files = [data for _, data, _ in mixed]
    dec = JpegDecoder(device=0, threads=4, entropy=entropy, progressive=True)
    try:
        dec.decode(files[:2], check=True)                                              # (the allocators warm)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                        # it never waits
        try:
            frames = dec.decode(files)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        dec.check()
        assert len(frames) == len(mixed) == jpegprog.N_CASES + 8
        for f, (name, _, px) in zip(frames, mixed):
            assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and np.array_equal(f.cpu().numpy(), px), name
        if entropy == "device":
            progressive = [data in {c[1] for c in jpegprog.cases()} for data in files]
            assert dec.last_paths == ["host" if p else "device" for p in progressive]
        # a declined progressive file still reaches the fallback; without one it raises
        _, F, px, _ = jpegprog.case("17x9_420")
        a, b, _ = jpegprog.scans(F)[-1]
        seen = []

        def fallback(data):
            seen.append(data)
            return px

        got = dec.decode([files[1], F[:a] + F[b:], F], fallback=fallback, check=True)
        assert seen == [F[:a] + F[b:]] and all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, (mixed[1][2], px, px)))
        with pytest.raises(UnsupportedJPEG, match="incomplete progression"):
            dec.decode([F[:a] + F[b:]])
        with pytest.raises(MalformedJPEG, match="truncated"):
            dec.decode([F, F[:-2]], fallback=fallback)
    finally:
        dec.close()
    plain = JpegDecoder(device=0, threads=2, entropy=entropy)
    try:
        with pytest.raises(UnsupportedJPEG, match="progressive"):
            plain.decode(files[:1])
    finally:
        plain.close()


@pytest.fixture(scope="module")
def resident():
    """A store with every progressive case and some baseline files, and the full decode of each entry, made once and left unchanged."""
    mixed = _mixed()
    store = JpegStore(device=0, threads=4, initial_rows=8, progressive=True)
    ids = store.add([data for _, data, _ in mixed])
    full = store.decode(ids, check=True)
    torch.cuda.synchronize()
    yield store, ids, full, mixed
    store.close()


def test_store_keeps_progressive_files_as_scans_and_decodes_them(resident, monkeypatch):
    store, ids, full, mixed = resident
    assert store.kinds[ids].tolist() == ["scan"] * len(mixed) and store._pixels == {} and store.resident["pixels"] == 0
    assert store.shape(ids).tolist() == [list(px.shape[:2]) for _, _, px in mixed]
    for f, (name, _, px) in zip(full, mixed):
        assert np.array_equal(f.cpu().numpy(), px), name
    # what is resident is the transcode: one restart segment per MCU row
    where = [k for k, (name, _, _) in enumerate(mixed) if name.startswith("130x70_420")][0]
    col = store._columns[int(ids[where])]
    assert col["n_seg"] == col["mcus_y"] == 5 and col["mcus_x"] == 9
    rng = np.random.default_rng(5)
    order = np.concatenate([rng.permutation(ids), ids[:5], ids[:5]])                    # shuffled, with repeats
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = store.decode(order)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    assert launched == ["fear_jpeg_huffman_indexed", "fear_jpeg_decode_u8"]            # the block-start table is from the fixture's decode
    for f, i in zip(frames, order):
        assert torch.equal(f, full[int(i)]), mixed[int(i)][0]
    fresh = JpegStore(device=0, threads=2, progressive=True)
    try:
        del launched[:]
        one = fresh.add([mixed[0][1]])
        del launched[:]
        first = fresh.decode(one, check=True)
        assert launched == ["fear_jpeg_dense_block_start", "fear_jpeg_huffman_indexed", "fear_jpeg_decode_u8"]
        assert np.array_equal(first[0].cpu().numpy(), mixed[0][2])
    finally:
        fresh.close()


def test_decode_rows_equals_decode_on_every_window(resident):
    store, ids, full, mixed = resident
    positions = []
    ours = {c[1] for c in jpegprog.cases()}
    for k, (name, data, px) in enumerate(mixed):
        if data in ours and name.startswith(("130x70_", "33x31_", "written_33x31_")):
            mcu_h = int(store._columns[int(ids[k])]["mcu_h"])
            positions += [(int(ids[k]), y0, y1) for y0, y1 in windows(px.shape[0], mcu_h)]
    assert len(positions) > 300 and len({p[0] for p in positions}) == 10
    rng = np.random.default_rng(7)
    positions = [positions[k] for k in rng.permutation(len(positions))]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = store.decode_rows([p[0] for p in positions], np.array([p[1:] for p in positions]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    for f, (i, y0, y1) in zip(frames, positions):
        assert f.shape == full[i].shape and torch.equal(f[y0:y1], full[i][y0:y1]), f"{mixed[i][0]}: rows {y0}..{y1}"


def test_borders_are_the_border_colours_of_the_full_decode(resident):
    store, ids, full, mixed = resident
    table = np.zeros(len(full), dtype=np.dtype(abi.FearFrame))
    for k, f in enumerate(full):
        table[k] = (f.data_ptr(), f.shape[0], f.shape[1])
    dev = torch.from_numpy(table.view(np.uint8)).cuda()
    want = torch.empty((len(full), 3), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert store._lib.fear_frame_border_u8(ctypes.c_void_p(dev.data_ptr()), len(full), ctypes.c_void_p(want.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(store.borders(ids), want) and torch.equal(store.borders(ids[::-1][:5]), want.flip(0)[:5])


def test_store_faults_commit_nothing_and_name_the_item():
    _, F, px, _ = jpegprog.case("33x31_422_noise")
    _, G, _, _ = jpegprog.case("8x8_420")
    good = jpegdec.case("16x16_420")[1]
    store = JpegStore(device=0, threads=2, slab_bytes=40_000, progressive=True)
    try:
        store.add([good, F])
        before = (len(store), store.nbytes, len(store._slabs), store._cursor, dict(store.resident))
        a, b, _ = jpegprog.scans(F)[-1]
        data_at = a + 2 + ((F[a + 2] << 8) | F[a + 3])
        assert b - data_at >= 4
        with pytest.raises(MalformedJPEG, match="item 2: truncated entropy data"):
            store.add([good, G, F[:(data_at + b) // 2], G])                             # cut inside the last scan's entropy data
        with pytest.raises(UnsupportedJPEG, match="item 1: incomplete progression"):
            store.add([G, F[:a] + F[b:]])
        with pytest.raises(MalformedJPEG, match="item 0"):                              # a fallback does not take a malformed file
            store.add([F[:-2]], fallback=lambda data: px)
        assert (len(store), store.nbytes, len(store._slabs), store._cursor, dict(store.resident)) == before
        seen = []

        def fallback(data):
            seen.append(data)
            return px

        more = store.add([F[:a] + F[b:], F], fallback=fallback)                         # declined: the original goes to the fallback
        assert seen == [F[:a] + F[b:]] and store.kinds[more].tolist() == ["pixels", "scan"]
        for f in store.decode(more, check=True):
            assert np.array_equal(f.cpu().numpy(), px)
        # capacity is counted on the transcode
        tb = jpeg_to_baseline_host(G)
        probe = JpegStore(device=0, threads=1, progressive=True)
        probe.add([tb])
        need = probe.nbytes
        probe.close()
        small = JpegStore(device=0, threads=1, progressive=True, capacity_bytes=need)
        try:
            small.add([G])
            assert small.nbytes == need
        finally:
            small.close()
    finally:
        store.close()
    plain = JpegStore(device=0, threads=1)
    try:
        with pytest.raises(UnsupportedJPEG, match="item 0: progressive"):
            plain.add([F])
    finally:
        plain.close()
