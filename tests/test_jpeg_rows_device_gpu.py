"""Rows from the device on the GPU (include/fear_train.h: fear_jpeg_huffman_indexed_rows_dev, fear_jpeg_decode_u8_rows_dev; DESIGN.md
section 14, "Rows from the device"): `JpegStore.decode_rows(ids, rows)` with `rows` a device tensor against `decode` on the rows asked
for — every file of jpeg_decode.npz in one store, the progressive one as its baseline transcode — next to the host-planned form with
the same rows; the positions `fear_jpeg_huffman_indexed_rows_dev` writes, through the C ABI into a buffer of sentinels; and the argument
checks of the two entry points and of the store."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec
from dataops import GUARD, P, SENTINEL_U8, guarded, inner, inside
from jpegdec import ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, OK
from test_jpeg_store_gpu import RECORD, _Built, _Indexed, _stream, without_lanes
from feartracker_amd import JpegStore, scan_row_sub
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_huffman import rows_band

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


def _windows(H, rng, extra=6):
    """The rows of one file: nothing at either end, rows clipped at either end, a reversed window, the whole, and seeded ones."""
    out = [(0, 0), (H, H), (-5, 3), (H - 1, H + 9), (H // 2 + 1, H // 2), (0, H), (-(1 << 30), 1 << 30)]
    for _ in range(extra):
        y0 = int(rng.integers(-3, H + 3))
        out.append((y0, int(rng.integers(y0 - 2, H + 6))))
    return out


def _positions(store, ids, seed):
    """(id, y0, y1) for the windows of every entry, shuffled: ids of mixed sizes, permuted and repeated."""
    rng = np.random.default_rng(seed)
    out = [(int(i), y0, y1) for i in ids for y0, y1 in _windows(int(store.shape([i])[0, 0]), rng)]
    return [out[k] for k in rng.permutation(len(out))]


def _on_device(positions):
    """The rows as decode_rows takes them from a device: (n, 2) int32, staged in pinned memory and sent without waiting."""
    pinned = torch.tensor([p[1:] for p in positions], dtype=torch.int32).reshape(-1, 2).pin_memory()
    return pinned.to("cuda", non_blocking=True), pinned


def _check_rows(frames, positions, full, ids):
    where = {int(i): k for k, i in enumerate(ids)}
    for f, (i, y0, y1) in zip(frames, positions):
        ref = full[where[i]]
        lo, hi = min(max(y0, 0), ref.shape[0]), min(max(y1, 0), ref.shape[0])
        assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and f.shape == ref.shape
        assert torch.equal(f[lo:hi], ref[lo:hi]), f"id {i}: rows {y0}..{y1}"


@pytest.fixture(scope="module", params=[128, 16], ids=["sb128", "sb16"])
def resident(request):
    """Every file of jpeg_decode.npz in one store, the progressive one as its transcode; the full decode of each, made once."""
    cases = jpegdec.cases()
    store = JpegStore(device=0, threads=4, initial_rows=8, subsequence_bytes=request.param, progressive=True)
    ids = store.add([data for _, data, _ in cases])
    assert store.kinds[ids].tolist() == ["scan"] * len(cases)
    if request.param == 16:                                                              # several workgroups per image
        assert int(store._columns["n_sub"][ids].max()) > 256
    full = store.decode(ids, check=True)
    torch.cuda.synchronize()
    yield store, ids, full
    store.close()


def test_rows_on_the_device_equal_decode_on_the_rows_asked_for(resident):
    store, ids, full = resident
    positions = _positions(store, ids, 41)
    assert len(positions) > 500
    pids = [p[0] for p in positions]
    rows, keep = _on_device(positions)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                              # it never waits
    try:
        frames = store.decode_rows(pids, rows)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    _check_rows(frames, positions, full, ids)
    assert len({f.data_ptr() for f in frames}) == len(frames)                           # private frames, repeated ids included
    # the host-planned form with the same rows
    hosted = store.decode_rows(pids, np.array([p[1:] for p in positions]), check=True)
    _check_rows(hosted, positions, full, ids)
    # a CPU tensor is host rows, as before
    _check_rows(store.decode_rows(pids[:9], keep[:9], check=True), positions[:9], full, ids)
    assert store.decode_rows([], torch.zeros((0, 2), dtype=torch.int32, device="cuda")) == []


def test_rows_a_kernel_has_just_written(resident):
    """`rows` produced on the current stream right in front of the call, the whole of it under sync debug mode "error"."""
    store, ids, full = resident
    positions = _positions(store, ids, 43)[:200]
    staged, keep = _on_device(positions)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rows = (staged * 3 - staged - staged).contiguous()                               # kernels on this stream write the values
        frames = store.decode_rows([p[0] for p in positions], rows)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    _check_rows(frames, positions, full, ids)


def test_a_small_workspace_limit_splits_the_device_form(resident, monkeypatch):
    store, ids, full = resident
    positions = _positions(store, ids, 47)[:120]
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    monkeypatch.setattr(store, "workspace_limit", 60_000)
    rows, keep = _on_device(positions)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = store.decode_rows([p[0] for p in positions], rows)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    n = launched.count("fear_jpeg_huffman_indexed_rows_dev")
    assert 3 <= n < 120 and n == launched.count("fear_jpeg_decode_u8_rows_dev")
    assert not {"fear_jpeg_huffman_indexed", "fear_jpeg_huffman_indexed_rows", "fear_jpeg_decode_u8"} & set(launched)
    _check_rows(frames, positions, full, ids)


def test_a_pixels_entry_is_copied_whole_and_gathers_the_groups_rows():
    """A file sent through the fallback, between "scan" entries: its frame is the whole copy, and the group's rows are gathered on the
    device for the "scan" positions around it."""
    prog = jpegdec.case("33x31_420_smooth_q75_progressive")
    scans = [jpegdec.case(n) for n in ("15x50_420_random_q100_rst3", "64x48_444_random_q100_plain2", "80x72_gray_smooth_q100_rst3")]
    store = JpegStore(device=0, threads=2)
    try:
        ids = store.add([scans[0][1], prog[1], scans[1][1], scans[2][1]], fallback=lambda data: prog[2])
        assert store.kinds[ids].tolist() == ["scan", "pixels", "scan", "scan"]
        full = store.decode(ids, check=True)
        positions = [(0, 17, 33), (1, 3, 4), (2, 40, 48), (1, 0, 0), (3, -2, 9), (0, 0, 50)]
        rows, keep = _on_device(positions)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            frames = store.decode_rows([p[0] for p in positions], rows)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        store.check()
        _check_rows(frames, positions, full, ids)
        for k in (1, 3):
            assert torch.equal(frames[k], full[1]) and frames[k].data_ptr() != full[1].data_ptr()
    finally:
        store.close()


def test_argument_errors_of_the_store_come_before_any_launch(resident, monkeypatch):
    store, ids, full = resident
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    good = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
    for bad in (good[:2], torch.zeros((3, 3), dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda"),
                good.to(torch.int64), good.to(torch.float32)):
        with pytest.raises(ValueError):
            store.decode_rows(ids[:3], bad)
    if torch.cuda.device_count() > 1:                                                   # another device
        with pytest.raises(ValueError):
            store.decode_rows(ids[:3], good.to("cuda:1"))
    with pytest.raises(IndexError):
        store.decode_rows([0, len(store), 1], good)
    assert launched == []
    store.decode_rows(ids[:3], good, check=True)
    assert launched == ["fear_jpeg_huffman_indexed_rows_dev", "fear_jpeg_decode_u8_rows_dev"]


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
class _RowsDev(_Indexed):
    """One fear_jpeg_huffman_indexed_rows_dev call over the images `which` of a built index: fear_jpeg_huffman_indexed's records and
    table, the row tables and the rows on the device, and the coefficients in a buffer of sentinels."""

    def __init__(self, built, which, row_sub, rows, run=True):
        super().__init__(built, which, run=False)
        flat = np.concatenate([np.asarray(row_sub[k], dtype=np.uint32) for k in self.which])
        self.row_dev = torch.from_numpy(flat.view(np.int32)).cuda()
        at = 0
        for j, k in enumerate(self.which):
            self.images[j].row_sub = self.row_dev.data_ptr() + 4 * at
            at += len(row_sub[k])
        records_at = (4 * self.m + 4 + 15) & ~15
        table = self.table.cpu().numpy()
        table[records_at:] = np.frombuffer(self.images, dtype=np.uint8)
        self.table = torch.from_numpy(table).cuda()
        self.rows = torch.tensor(rows, dtype=torch.int32, device="cuda").reshape(-1, 2)
        if run:
            assert self.call() == OK
            torch.cuda.synchronize()

    def call(self, n=None, **kw):
        a = dict(images=self.images, table=P(self.table.data_ptr()), rows=P(self.rows.data_ptr()), out=inner(self.coef),
                 st=P(self.status.data_ptr()), sb=self.built.sb)
        a.update(kw)
        return self.built.lib.fear_jpeg_huffman_indexed_rows_dev(a["images"], self.m if n is None else n, a["table"], a["rows"], a["out"],
                                                                 a["st"], a["sb"], _stream())


FILES = ("1x1_444", "1x1_gray", "15x50_420_random_q100_rst3", "40x24_420_random_q75_rstrows1", "80x72_444_random_q95_rst3",
         "64x48_444_random_q100_plain2", "80x72_gray", "80x72_422", "15x50_422", "80x72_420")


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_the_written_positions_are_the_bands_blocks(lib, subsequence_bytes):
    """Several windows of each file in one ragged call into sentinels: the band's blocks hold fear_jpeg_huffman_indexed's values, every
    other position of the image still holds the sentinel, and so do the guards."""
    cases = [jpegdec.case(n) for n in FILES]
    built = _Built(lib, [data for _, data, _ in cases], subsequence_bytes)
    assert not built.statuses().any()
    row_sub = [scan_row_sub(jf._parse(data), sub, entries) for (_, data, _), sub, entries in zip(cases, built.sub, built.entries())]
    whole = _Indexed(built, range(len(cases))).dense()
    rng = np.random.default_rng(subsequence_bytes)
    which, rows = [], []
    for k, info in enumerate(built.infos):
        for y0, y1 in _windows(info.height, rng, extra=4):
            which.append(k)
            rows.append((y0, y1))
    order = rng.permutation(len(which))
    which, rows = [which[i] for i in order], [rows[i] for i in order]
    run = _RowsDev(built, which, row_sub, rows)
    assert not run.statuses().any()
    if subsequence_bytes == 4:
        assert np.diff(run.groups).max() > 10                                           # images of many workgroups
    sentinel = np.array([SENTINEL_U8 * 0x0101], dtype=np.uint16).view(np.int16)[0]
    partial = 0
    for j, (k, (y0, y1), got) in enumerate(zip(which, rows, run.dense())):
        info = built.infos[k]
        mcu_h = 8 * info.v[0]
        band = rows_band(y0, y1, mcu_h * info.mcus_y, mcu_h, info.mcus_y, info.v[0] == 2)
        want = np.full(got.shape, sentinel, dtype=np.int16)
        if band is not None:
            at = 0
            for c in range(info.components):
                wide, v = 64 * info.blocks_w[c], (info.v[0] if c == 0 else 1)
                lo, hi = at + band[0] * v * wide, at + band[1] * v * wide
                want[lo:hi] = whole[k][lo:hi]
                at += wide * info.blocks_h[c]
            partial += band[1] - band[0] < info.mcus_y
        assert bool((got == want).all()), f"{cases[k][0]}: rows {y0}..{y1}: {int((got != want).sum())} of {want.size} values differ"
    assert partial > 20


def test_an_image_without_a_subsequence_has_no_lane_and_fails(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    built = _Built(lib, [data], 128)
    row_sub = [scan_row_sub(jf._parse(data), built.sub[0], built.entries()[0])]
    assert without_lanes(_RowsDev(built, [0], row_sub, [(10, 30)], run=False), n_sub=0) == jpegdec.ERR_FORMAT


def test_argument_checks_of_the_two_entry_points(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    built = _Built(lib, [data], 128)
    row_sub = [scan_row_sub(jf._parse(data), built.sub[0], built.entries()[0])]
    run = _RowsDev(built, [0], row_sub, [(10, 30)], run=False)
    im = run.images[0]

    def with_field(call, **fields):
        saved = {k: getattr(im, k) for k in fields}
        for k, v in fields.items():
            setattr(im, k, v)
        rc = call()
        for k, v in saved.items():
            setattr(im, k, v)
        return rc

    assert run.call(n=0, images=None, table=None, rows=None, out=None, st=None) == OK
    assert run.call(n=-1) == ERR_SHAPE and run.call(n=65536) == ERR_SHAPE
    for sb in (0, 2, 6, 130, 1028, -128):
        assert run.call(sb=sb) == ERR_SHAPE, sb
    for name in ("images", "table", "rows", "out", "st"):
        assert run.call(**{name: None}) == ERR_NULL, name
    for null in ("scan", "index", "sub_start", "row_sub"):
        assert with_field(run.call, **{null: 0}) == ERR_NULL, null
    assert with_field(run.call, index=im.index + 8) == ERR_SHAPE and with_field(run.call, sub_start=im.sub_start + 2) == ERR_SHAPE
    assert with_field(run.call, scan=im.scan + 4) == ERR_SHAPE and with_field(run.call, row_sub=im.row_sub + 2) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((inside(run.coef, 2 * run.values) == SENTINEL_U8).all()) and int(run.status[0]) == 77   # nothing was launched

    # fear_jpeg_decode_u8_rows_dev: fear_jpeg_decode_u8's checks, and the rows
    decoded = jpegdec.c_decode(lib, data)
    records, infos, prefix, at, up_bytes, out_bytes = jpegdec.call_layout([decoded])
    up = torch.zeros(up_bytes + jpegdec.table_bytes(prefix, records).nbytes, dtype=torch.uint8, device="cuda")
    out = guarded(out_bytes)
    records[0].coef, records[0].block_start, records[0].out = up.data_ptr() + at["coef"][0], up.data_ptr() + at["start"][0], out.data_ptr() + GUARD
    ws_bytes = lib.fear_jpeg_decode_workspace_bytes(infos, 1)
    ws = guarded(ws_bytes)
    rows = torch.tensor([[3, 9]], dtype=torch.int32, device="cuda")
    table = P(up.data_ptr() + up_bytes)

    def call(n=1, images=records, table=table, rows=P(rows.data_ptr()), workspace=inner(ws), nbytes=ws_bytes):
        return lib.fear_jpeg_decode_u8_rows_dev(images, n, table, rows, workspace, nbytes, _stream())

    def with_record(**fields):
        saved = {k: getattr(records[0], k) for k in fields}
        for k, v in fields.items():
            setattr(records[0], k, v)
        rc = call()
        for k, v in saved.items():
            setattr(records[0], k, v)
        return rc

    assert call(n=0, images=None, table=None, rows=None, workspace=None, nbytes=0) == OK
    assert call(n=-1) == ERR_SHAPE and call(n=65536) == ERR_SHAPE
    assert call(images=None) == ERR_NULL and call(table=None) == ERR_NULL and call(rows=None) == ERR_NULL
    for null in ("coef", "block_start", "out"):
        assert with_record(**{null: 0}) == ERR_NULL, null
    assert with_record(width=0) == ERR_SHAPE and with_record(height=8193) == ERR_SHAPE and with_record(components=2) == ERR_SHAPE
    assert with_record(h=1, v=2) == ERR_SHAPE and with_record(plane_offset=8) == ERR_SHAPE
    assert call(workspace=None) == ERR_WORKSPACE and call(nbytes=ws_bytes - 1) == ERR_WORKSPACE and call(nbytes=0) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((inside(out, out_bytes) == SENTINEL_U8).all()) and bool((inside(ws, ws_bytes) == SENTINEL_U8).all())   # nothing was launched
