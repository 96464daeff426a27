"""JpegStore(residence="host") on the GPU (include/fear_train.h: the fear_jpeg_huffman_indexed*_host calls; DESIGN.md section 14,
"Bytes on the host"): a store whose scan bytes lie in pinned host memory against a store of the same files on the device — every call,
frame by frame with torch.equal — and, for the plain decode, against jpeg_decode_host.  The files are every fixture the store keeps as
a scan and five written here with Pillow from seeded noise.  Every test runs under a watchdog of its own, which ends the process."""
import ctypes
import faulthandler
import io

import numpy as np
import pytest
import torch

import jpeghuff
from feartracker_amd import JpegStore
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_frames import jpeg_decode_host
from feartracker_amd.jpeg_huffman import scan_sub_start, stage_range_host
from feartracker_amd.jpeg_store import LANES, StoreFull, _up

pytestmark = pytest.mark.gpu
STAGE_CAP = 64 << 10                                                     # csrc/fear_jpeg_store.h: kJiStageCap
_made = None


@pytest.fixture(autouse=True)
def watchdog():
    """A time limit for each test: a hung GPU step ends the process with the stacks, nothing more starts on the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _noise(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def _write(pixels, **kw):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(pixels).save(out, "JPEG", **kw)
    return out.getvalue()


def made():
    """[(name, bytes)] written once: a scan shorter than one subsequence, one longer than a workgroup's 256 subsequences, two with a
    restart marker after every MCU row (many short, unaligned segments) and a progressive one."""
    global _made
    if _made is None:
        _made = [("16x16_q30", _write(_noise(16, 16, 1), quality=30, subsampling="4:2:0")),
                 ("256x256_noise_q95_420", _write(_noise(256, 256, 2), quality=95, subsampling="4:2:0")),
                 ("136x120_420_restart", _write(_noise(136, 120, 3), quality=90, subsampling="4:2:0", restart_marker_rows=1)),
                 ("136x120_422_restart", _write(_noise(136, 120, 4), quality=90, subsampling="4:2:2", restart_marker_rows=1)),
                 ("97x65_420_progressive", _write(_noise(97, 65, 5), quality=90, subsampling="4:2:0", progressive=True))]
    return _made


@pytest.fixture(scope="module")
def files():
    """(names, the files' bytes, jpeg_decode_host's frames): computed once, shared and left unchanged."""
    cases = [(name, data) for name, data, _ in jpeghuff.supported()] + made()
    reference = [jpeg_decode_host(data, progressive=name.endswith("progressive")) for name, data in cases]
    for px in reference:
        px.setflags(write=False)
    return [name for name, _ in cases], [data for _, data in cases], reference


def _pair(files, **kw):
    stores = [JpegStore(device=0, threads=4, progressive=True, residence=r, **kw) for r in ("device", "host")]
    ids = [s.add(files[1]) for s in stores]
    assert ids[0].tolist() == ids[1].tolist() == list(range(len(files[1]))) and set(stores[0].kinds) == set(stores[1].kinds) == {"scan"}
    return stores[0], stores[1], ids[0]


@pytest.fixture(scope="module")
def pair(files):
    dev, host, ids = _pair(files, subsequence_bytes=128, slab_bytes=1 << 20)
    yield dev, host, ids
    dev.close()
    host.close()


def _equal(a, b, names, ids):
    assert len(a) == len(b) == len(ids)
    for x, y, i in zip(a, b, ids):
        assert x.is_cuda and x.dtype == torch.uint8 and x.shape == y.shape and torch.equal(x, y), names[int(i)]


def _slab_bytes(slabs, address, count):
    """`count` bytes of the store's memory at `address`: slabs are (tensor, address of its first byte)."""
    for slab, base in slabs:
        if base <= address and address + count <= base + slab.numel():
            return slab[address - base:address - base + count].cpu().numpy()
    raise AssertionError("an address outside every slab")


def _entry(store, i):
    """What the store keeps of entry i, read back: the record, the unstuffed bytes, seg_start, sub_start and the index's bytes."""
    device = [(s, s.data_ptr()) for s in store._slabs]
    row = store._indexed[i]
    record = abi.FearJpegScan.from_buffer_copy(_slab_bytes(device, int(row["scan"]), ctypes.sizeof(abi.FearJpegScan)).tobytes())
    where = store._host_slabs if store.residence == "host" else device
    data = _slab_bytes(where, record.bytes, record.n_bytes)
    seg = _slab_bytes(device, record.seg_start, 4 * (record.n_seg + 1)).view(np.uint32)
    sub = _slab_bytes(device, int(row["sub_start"]), 4 * (record.n_seg + 1)).view(np.uint32)
    index = _slab_bytes(device, int(row["index"]), 16 * int(row["n_sub"]))
    return record, data, seg, sub, index


def test_what_is_resident_equals_the_device_stores(pair, files):
    dev, host, ids = pair
    names = files[0]
    assert dev.residence == "device" and host.residence == "host" and len(host._host_slabs) >= 1 and dev._host_slabs == []
    n_sub = {}
    for i in ids:
        a, b = _entry(dev, int(i)), _entry(host, int(i))
        for x, y in zip(a[1:], b[1:]):                                    # bytes, seg_start, sub_start and the index, byte for byte
            assert np.array_equal(x, y), names[i]
        head = abi.FearJpegScan.bytes.size + abi.FearJpegScan.seg_start.size
        assert bytes(a[0])[head:] == bytes(b[0])[head:], names[i]                # the records but their two addresses
        n_sub[names[i]] = int(a[3][-1])
    assert n_sub["256x256_noise_q95_420"] > LANES and n_sub["16x16_q30"] == 1    # a workgroup boundary inside | less than a subsequence
    assert np.array_equal(dev._row_sub[:dev._row_used], host._row_sub[:host._row_used]) and dev._row_used > 0
    assert np.array_equal(dev._columns[:len(ids)], host._columns[:len(ids)])
    assert torch.equal(dev.borders(ids), host.borders(ids))
    # the accounts: nbytes is the device's, host_nbytes the pinned bytes, and together they are the device store's
    assert set(dev.resident) == set(host.resident) == {"bytes", "index", "records", "pixels", "rows", "border", "host_bytes"}
    assert dev.resident["host_bytes"] == dev.host_nbytes == 0 and dev.nbytes == sum(dev.resident.values())
    assert host.host_nbytes == host.resident["host_bytes"] == sum(_up(max(_entry(dev, int(i))[0].n_bytes, 1), 16) for i in ids)
    assert host.nbytes == sum(host.resident.values()) - host.host_nbytes
    assert host.resident["bytes"] + host.resident["host_bytes"] == dev.resident["bytes"] and host.nbytes + host.host_nbytes == dev.nbytes
    for key in ("index", "records", "pixels", "rows", "border"):
        assert host.resident[key] == dev.resident[key], key


def test_decode_in_a_permuted_order_with_a_repeat(pair, files):
    dev, host, ids = pair
    names, _, reference = files
    order = np.random.default_rng(7).permutation(ids)
    order = np.concatenate([order, order[:3], order[:1]])
    frames = host.decode(order, check=True)
    _equal(frames, dev.decode(order, check=True), names, order)
    for f, i in zip(frames, order):
        assert np.array_equal(f.cpu().numpy(), reference[int(i)]), names[int(i)]
    assert torch.equal(host.decode([int(order[0])])[0], frames[0]) and [f.shape for f in frames] == [reference[int(i)].shape for i in order]
    assert host.shape(order).tolist() == dev.shape(order).tolist()
    host.check()


def _bands(shape):
    """(n, 4, 2): per frame a band inside, one at each edge and an empty one."""
    H = shape[:, 0].astype(np.int64)
    inside = np.stack([H // 3, np.maximum(H // 3 + 1, 2 * H // 3)], axis=1)
    return np.stack([inside, np.stack([0 * H, np.minimum(H, 9)], axis=1), np.stack([np.maximum(H - 9, 0), H], axis=1),
                     np.stack([0 * H + 5, 0 * H + 5], axis=1)], axis=1)


def test_decode_rows_with_rows_on_the_host_and_on_the_device(pair, files):
    dev, host, ids = pair
    names = files[0]
    full = dev.decode(ids, check=True)
    bands = _bands(dev.shape(ids))
    for k in range(bands.shape[1]):
        rows = bands[:, k]
        on_device = torch.from_numpy(rows.astype(np.int32)).cuda()
        for got, want in ((host.decode_rows(ids, rows, check=True), dev.decode_rows(ids, rows, check=True)),
                          (host.decode_rows(ids, on_device, check=True), dev.decode_rows(ids, on_device, check=True))):
            for g, w, f, (y0, y1), i in zip(got, want, full, rows.tolist(), ids):
                assert g.shape == f.shape and torch.equal(g[y0:y1], w[y0:y1]) and torch.equal(g[y0:y1], f[y0:y1]), (names[i], k)
    host.check()


def _holds(got, want, full, names, ids):
    assert np.array_equal(got.origin, want.origin) and np.array_equal(got.window, want.window) and np.array_equal(got.shape, want.shape)
    for g, w, f, (oy, ox), (y0, y1, x0, x1), i in zip(got.frames, want.frames, full, got.origin.tolist(), got.window.tolist(), ids):
        assert g.shape == w.shape, names[i]
        mine = g[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        assert torch.equal(mine, w[y0 - oy:y1 - oy, x0 - ox:x1 - ox]) and torch.equal(mine, f[y0:y1, x0:x1]), names[i]


def _windows(shape):
    """(n, 3, 4): per frame a window inside, one that touches the right edge and one of a single MCU."""
    H, W = shape[:, 0].astype(np.int64), shape[:, 1].astype(np.int64)
    inside = np.stack([H // 4, np.maximum(H // 4 + 1, 3 * H // 4), W // 4, np.maximum(W // 4 + 1, 3 * W // 4)], axis=1)
    right = np.stack([H // 5, H, np.maximum(W - 9, 0), W], axis=1)
    one = np.stack([H // 2, H // 2 + 1, W // 2, W // 2 + 1], axis=1)
    return np.stack([inside, right, one], axis=1)


def test_decode_windows(pair, files):
    dev, host, ids = pair
    full = dev.decode(ids, check=True)
    windows = _windows(dev.shape(ids))
    for k in range(windows.shape[1]):
        _holds(host.decode_windows(ids, windows[:, k], check=True), dev.decode_windows(ids, windows[:, k], check=True), full, files[0], ids)


def test_every_scale_form(pair, files):
    dev, host, ids = pair
    names = files[0]
    mix = np.array([1, 2, 4, 8])[np.arange(ids.size) % 4]
    for scale in (2, 8, mix):
        full = dev.decode(ids, check=True, scale=scale)
        _equal(host.decode(ids, check=True, scale=scale), full, names, ids)
        shape = dev.shape(ids, scale)
        assert host.shape(ids, scale).tolist() == shape.tolist()
        rows = _bands(shape)[:, 0]
        for g, f, (y0, y1), i in zip(host.decode_rows(ids, rows, check=True, scale=scale), full, rows.tolist(), ids):
            assert g.shape == f.shape and torch.equal(g[y0:y1], f[y0:y1]), names[i]
        windows = _windows(shape)[:, 1]
        _holds(host.decode_windows(ids, windows, check=True, scale=scale), dev.decode_windows(ids, windows, check=True, scale=scale), full,
               names, ids)


@pytest.mark.parametrize("subsequence_bytes", [32, 1024])
def test_the_plain_decode_at_other_subsequence_sizes(files, subsequence_bytes):
    """At 1024 bytes a workgroup of the noise file covers more than the 64 KiB a workgroup stages: the tail is fetched directly."""
    names, data, reference = files
    dev, host, ids = _pair(files, subsequence_bytes=subsequence_bytes, slab_bytes=1 << 20)
    try:
        record, _, seg, sub, _ = _entry(host, names.index("256x256_noise_q95_420"))
        ranges = [stage_range_host(seg, sub, lane0, min(LANES, int(sub[-1]) - lane0), subsequence_bytes) for lane0 in range(0, int(sub[-1]), LANES)]
        assert np.array_equal(sub, scan_sub_start(seg, subsequence_bytes))
        assert (max(b - a for a, b in ranges) > STAGE_CAP) == (subsequence_bytes == 1024) and (len(ranges) > 1) == (subsequence_bytes == 32)
        frames = host.decode(ids[::-1], check=True)
        _equal(frames, dev.decode(ids[::-1], check=True), names, ids[::-1])
        for f, i in zip(frames, ids[::-1]):
            assert np.array_equal(f.cpu().numpy(), reference[int(i)]), names[int(i)]
        for i in ids:
            assert np.array_equal(_entry(dev, int(i))[4], _entry(host, int(i))[4]), names[i]
    finally:
        dev.close()
        host.close()


def test_a_scan_that_ends_at_its_slabs_last_word(files):
    """One file alone in a store whose slabs are as long as its entry: the pinned slab ends where the scan's last 16 bytes end, and the
    last lane's window reads no word behind it."""
    names, data, reference = files
    for name in ("256x256_noise_q95_420", "16x16_q30", "136x120_422_restart"):
        k = names.index(name)
        lib = abi.load_train_library()
        n_bytes = jpeghuff.c_prepare(lib, data[k])[3].n_bytes
        size = _up(n_bytes, 16)
        host = JpegStore(device=0, threads=1, residence="host", slab_bytes=size)
        dev = JpegStore(device=0, threads=1, slab_bytes=size)
        try:
            i, j = host.add([data[k]]), dev.add([data[k]])
            assert len(host._host_slabs) == 1 and host._host_slabs[0][0].numel() == size == host.host_nbytes and size - n_bytes < 16
            frame = host.decode(i, check=True)[0]
            assert torch.equal(frame, dev.decode(j, check=True)[0]) and np.array_equal(frame.cpu().numpy(), reference[k]), name
            H = frame.shape[0]
            rows = np.array([[H - 1, H]])
            assert torch.equal(host.decode_rows(i, rows, check=True)[0][H - 1:], frame[H - 1:]), name
        finally:
            host.close()
            dev.close()


def test_store_full_at_the_host_capacity_commits_nothing_on_either_side(files):
    names, data, reference = files
    small, large = data[names.index("16x16_q30")], data[names.index("256x256_noise_q95_420")]
    host = JpegStore(device=0, threads=2, residence="host", host_capacity_bytes=4096, slab_bytes=1 << 16)
    try:
        ids = host.add([small])
        before = (len(host), host.nbytes, host.host_nbytes, dict(host.resident), len(host._slabs), host._cursor, len(host._host_slabs),
                  host._host_cursor, host._row_used)
        with pytest.raises(StoreFull, match="host"):
            host.add([small, large])
        assert (len(host), host.nbytes, host.host_nbytes, dict(host.resident), len(host._slabs), host._cursor, len(host._host_slabs),
                host._host_cursor, host._row_used) == before
        tight = JpegStore(device=0, threads=2, residence="host", capacity_bytes=host.nbytes, slab_bytes=1 << 16)
        try:
            tight.add([small])
            with pytest.raises(StoreFull) as refused:                    # the device's limit, named as such
                tight.add([small])
            assert "host" not in str(refused.value) and len(tight) == 1 and tight.host_nbytes == host.host_nbytes
        finally:
            tight.close()
        more = host.add([small])                                         # and the store goes on
        assert more.tolist() == [1] and host.host_nbytes == 2 * before[2]
        frames = host.decode(np.concatenate([ids, more]), check=True)
        assert torch.equal(frames[0], frames[1]) and np.array_equal(frames[0].cpu().numpy(), reference[names.index("16x16_q30")])
    finally:
        host.close()


def test_decode_never_waits_for_the_gpu(pair, files):
    dev, host, ids = pair
    host.decode(ids[:3], check=True)                                     # (the allocators warm)
    want = dev.decode(ids[::-1], check=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = host.decode(ids[::-1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host.check()
    _equal(frames, want, files[0], ids[::-1])
    assert host.last_upload_bytes < 1024 * ids.size                      # records alone go up: no file bytes
