"""Bands of rows from the resident JPEG store on the GPU (include/fear_train.h: fear_jpeg_huffman_indexed_rows; DESIGN.md section 14,
"Bands of rows"): the band's coefficients through the C ABI against the slices of fear_jpeg_huffman_indexed's, every MCU-row band of
every supported file in one ragged call; `JpegStore.decode_rows` against `decode` on the rows asked for, `borders` against
fear_frame_border_u8 of the full decode and the host's means, and `TrainPairBuilder.build(..., borders=)` on band-decoded frames
against `build` on whole ones; the argument checks of the call and of the store."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec
import jpeghuff
from dataops import P, SENTINEL_U8, equal as _equal, guarded, inner, inside
from jpegdec import ERR_NULL, ERR_SHAPE, OK
from jpegrows import all_bands, windows
from test_jpeg_store_gpu import RECORD, _Built, _Indexed, _stream
from feartracker_amd import JpegStore, scan_row_sub
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi
from feartracker_amd.geometry import border_color_u8
from feartracker_amd.train_data import TrainPairBuilder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_train_library()


class _Rows:
    """One fear_jpeg_huffman_indexed_rows call over (image of a built index, MCU rows a .. b)) records, in that order."""

    def __init__(self, built, which, row_sub, run=True):
        self.built, self.which, m = built, list(which), len(which)
        self.m = m
        self.images = (abi.FearJpegIndexed * m)()
        prefix, self.values, self.sizes = np.zeros(m + 1, dtype=np.uint32), 0, []
        for j, (k, a, b) in enumerate(self.which):
            im, ix, info = self.images[j], built.indexes[k], built.infos[k]
            im.scan = built.up.data_ptr() + built.table_at + built.records_at + RECORD * k
            im.index, im.sub_start, im.n_sub, im.coef_offset = ix.index, ix.sub_start, ix.n_sub, self.values
            table = row_sub[k]
            im.mcu_row0, im.mcu_rows = a, b - a
            im.sub0 = int(table[a])
            im.sub_count = min(int(table[b]), ix.n_sub - 1) - int(table[a]) + 1 if b > a else 0
            per_mcu = info.h[0] * info.v[0] + 2 if info.components == 3 else 1
            self.sizes.append(64 * (b - a) * info.mcus_x * per_mcu)
            self.values += self.sizes[-1]
            prefix[j + 1] = prefix[j] + -(-im.sub_count // 256)
        self.groups = prefix
        records_at = (4 * m + 4 + 15) & ~15
        table = np.zeros(records_at + ctypes.sizeof(self.images), dtype=np.uint8)
        table[:prefix.nbytes] = prefix.view(np.uint8)
        table[records_at:] = np.frombuffer(self.images, dtype=np.uint8)
        self.table = torch.from_numpy(table).cuda()
        self.coef = guarded(2 * self.values)
        self.status = torch.full((m + 2,), 77, dtype=torch.int32, device="cuda")
        if run:
            assert self.call() == OK
            torch.cuda.synchronize()

    def call(self, n=None, **kw):
        a = dict(images=self.images, table=P(self.table.data_ptr()), out=inner(self.coef), st=P(self.status.data_ptr()), sb=self.built.sb)
        a.update(kw)
        return self.built.lib.fear_jpeg_huffman_indexed_rows(a["images"], self.m if n is None else n, a["table"], a["out"], a["st"], a["sb"],
                                                             _stream())

    def statuses(self):
        st = self.status.cpu().numpy()
        assert st[self.m] == 77 and st[self.m + 1] == 77, "a status behind the last image written"
        return st[:self.m]

    def dense(self):
        flat = inside(self.coef, 2 * self.values, "band coefficients").view(np.int16)
        return [flat[self.images[j].coef_offset:self.images[j].coef_offset + self.sizes[j]] for j in range(self.m)]


def _band_of(info, flat, a, b):
    """The values of the MCU rows a .. b) of an image's dense coefficients, in the band's own layout."""
    return np.concatenate([plane[a * (info.v[0] if c == 0 else 1):b * (info.v[0] if c == 0 else 1)].reshape(-1)
                           for c, plane in enumerate(jpeghuff.dense(info, flat))])


def _row_tables(cases, built):
    """scan_row_sub per file from the index the device built."""
    return [scan_row_sub(jf._parse(data), sub, entries) for (_, data, _), sub, entries in zip(cases, built.sub, built.entries())]


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_every_band_of_every_file_in_one_ragged_call(lib, subsequence_bytes):
    """1956 records: every MCU-row band [a, b) of every supported file, shuffled, each against the slices of the same file's full
    indexed decode.  The bands lie back to back in one guarded buffer: a value stored outside its band spoils a neighbour or a guard."""
    cases = jpeghuff.supported()
    built = _Built(lib, [data for _, data, _ in cases], subsequence_bytes)
    assert not built.statuses().any()
    full = _Indexed(built, range(len(cases)))
    assert not full.statuses().any()
    whole = full.dense()
    row_sub = _row_tables(cases, built)
    which = [(k, a, b) for k, info in enumerate(built.infos) for a, b in all_bands(info.mcus_y)]
    assert len(which) == 1956
    rng = np.random.default_rng(subsequence_bytes)
    which = [which[i] for i in rng.permutation(len(which))]
    run = _Rows(built, which, row_sub)
    status = run.statuses()
    assert not status.any(), [(cases[which[j][0]][0], which[j][1:], int(status[j])) for j in np.flatnonzero(status)[:5]]
    if subsequence_bytes == 4:
        assert np.diff(run.groups).max() > 40 and np.diff(run.groups).min() == 1       # bands of many workgroups and of one
    for (k, a, b), got in zip(which, run.dense()):
        want = _band_of(built.infos[k], whole[k], a, b)
        assert got.shape == want.shape and bool((got == want).all()), \
            f"{cases[k][0]}: MCU rows {a}..{b}: {int((got != want).sum())} of {want.size} values differ"


def test_bands_without_rows_or_lanes_and_the_argument_checks(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    cases = [("rst3", data, None)]
    built = _Built(lib, [data], 128)
    row_sub = _row_tables(cases, built)
    R = built.infos[0].mcus_y
    run = _Rows(built, [(0, 1, 1), (0, 0, R), (0, R, R)], row_sub)                       # an empty band, the image, an empty band at its end
    assert run.statuses().tolist() == [OK, OK, OK] and run.sizes[0] == 0 and run.sizes[2] == 0
    full = _Indexed(built, [0])
    assert bool((run.dense()[1] == full.dense()[0]).all())                              # the whole image as a band is the dense image

    run = _Rows(built, [(0, 1, 3)], row_sub, run=False)
    im = run.images[0]

    def with_field(call, **fields):
        saved = {k: getattr(im, k) for k in fields}
        for k, v in fields.items():
            setattr(im, k, v)
        rc = call()
        for k, v in saved.items():
            setattr(im, k, v)
        return rc

    assert run.call(n=0, images=None, table=None, out=None, st=None) == OK
    assert run.call(n=-1) == ERR_SHAPE and run.call(n=65536) == ERR_SHAPE
    for sb in (0, 2, 6, 130, 1028, -128):
        assert run.call(sb=sb) == ERR_SHAPE, sb
    for name in ("images", "table", "out", "st"):
        assert run.call(**{name: None}) == ERR_NULL, name
    for null in ("scan", "index", "sub_start"):
        assert with_field(run.call, **{null: 0}) == ERR_NULL, null
    assert with_field(run.call, index=im.index + 8) == ERR_SHAPE and with_field(run.call, sub_start=im.sub_start + 2) == ERR_SHAPE
    assert with_field(run.call, scan=im.scan + 4) == ERR_SHAPE
    assert with_field(run.call, sub0=im.n_sub) == ERR_SHAPE and with_field(run.call, sub_count=im.n_sub - im.sub0 + 1) == ERR_SHAPE
    assert with_field(run.call, mcu_row0=1025) == ERR_SHAPE and with_field(run.call, mcu_row0=1000, mcu_rows=25) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((inside(run.coef, 2 * run.values) == SENTINEL_U8).all()) and int(run.status[0]) == 77   # nothing was launched
    assert run.call() == OK
    torch.cuda.synchronize()
    assert run.statuses()[0] == OK
    assert bool((run.dense()[0] == _band_of(built.infos[0], full.dense()[0], 1, 3)).all())


def test_a_call_of_empty_bands_alone_launches_no_lane(lib):
    _, data, _ = jpegdec.case("15x50_420_random_q100_rst3")
    built = _Built(lib, [data], 128)
    R = built.infos[0].mcus_y
    run = _Rows(built, [(0, 1, 1), (0, R, R)], _row_tables([("rst3", data, None)], built))
    assert run.groups.tolist() == [0, 0, 0] and run.statuses().tolist() == [OK, OK] and run.values == 0
    inside(run.coef, 0, "band coefficients")


# ------------------------------------------------------------------------------------------------------------------------- JpegStore
@pytest.fixture(scope="module")
def resident():
    """A store with every supported file and, last, a progressive file kept as pixels; the full decode of each entry, made once and
    left unchanged."""
    cases = jpeghuff.supported()
    prog = jpegdec.case("33x31_420_smooth_q75_progressive")
    store = JpegStore(device=0, threads=4, initial_rows=8)
    ids = store.add([data for _, data, _ in cases] + [prog[1]], fallback=lambda data: prog[2])
    assert store.kinds[ids].tolist() == ["scan"] * len(cases) + ["pixels"]
    full = store.decode(ids, check=True)
    torch.cuda.synchronize()
    yield store, ids, full, cases + [prog]
    store.close()


def _positions(store, ids):
    """(id, y0, y1) for every window of every entry — every MCU-aligned window, each moved by a row at either end, the first row, the
    last, the whole — plus an empty and a reversed window per entry, shuffled: ids of mixed sizes, permuted and repeated."""
    out = []
    for i in ids:
        H = int(store.shape([i])[0, 0])
        col = store._columns[int(i)]
        out += [(int(i), y0, y1) for y0, y1 in windows(H, max(int(col["mcu_h"]), 8))]
        out += [(int(i), H // 2, H // 2), (int(i), H, 0)]
    rng = np.random.default_rng(23)
    return [out[k] for k in rng.permutation(len(out))]


def _check_rows(frames, positions, full, ids):
    where = {int(i): k for k, i in enumerate(ids)}
    for f, (i, y0, y1) in zip(frames, positions):
        ref = full[where[i]]
        assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and f.shape == ref.shape
        assert torch.equal(f[y0:y1], ref[y0:y1]), f"id {i}: rows {y0}..{y1}"


def test_decode_rows_equals_decode_on_the_rows_asked_for(resident):
    store, ids, full, cases = resident
    positions = _positions(store, ids)
    assert len(positions) > 3000
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                          # it never waits
    try:
        chunks = [positions[at:at + 600] for at in range(0, len(positions), 600)]
        results = [store.decode_rows([p[0] for p in chunk], np.array([p[1:] for p in chunk])) for chunk in chunks]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    for chunk, frames in zip(chunks, results):
        _check_rows(frames, chunk, full, ids)
    frames = store.decode_rows(ids, None, check=True)                                # rows=None is decode
    assert all(torch.equal(f, ref) for f, ref in zip(frames, full))
    pix = store.decode_rows(ids[-1:], np.array([[3, 4]]), check=True)[0]             # a "pixels" entry is copied whole
    assert torch.equal(pix, full[-1]) and pix.data_ptr() != full[-1].data_ptr()
    assert store.decode_rows([], np.zeros((0, 2), np.int64)) == []
    store.decode_rows(ids[:4], np.array([[-5, 3], [0, 10 ** 6], [7, 7], [-9, -2]]), check=True)   # clipped to [0, H]


def test_a_small_workspace_limit_splits_decode_rows(resident, monkeypatch):
    store, ids, full, cases = resident
    positions = _positions(store, ids)[:300]
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    monkeypatch.setattr(store, "workspace_limit", 40_000)
    frames = store.decode_rows([p[0] for p in positions], np.array([p[1:] for p in positions]), check=True)
    n = launched.count("fear_jpeg_huffman_indexed_rows")
    assert 10 < n < 300 and n == launched.count("fear_jpeg_decode_u8") and "fear_jpeg_huffman_indexed" not in launched
    _check_rows(frames, positions, full, ids)


def test_borders_are_the_border_colours_of_the_full_decode(resident, lib):
    store, ids, full, cases = resident
    table = np.zeros(len(full), dtype=np.dtype(abi.FearFrame))
    for k, f in enumerate(full):
        table[k] = (f.data_ptr(), f.shape[0], f.shape[1])
    dev = torch.from_numpy(table.view(np.uint8)).cuda()
    want = torch.empty((len(full), 3), dtype=torch.uint8, device="cuda")
    assert lib.fear_frame_border_u8(P(dev.data_ptr()), len(full), P(want.data_ptr()), _stream()) == OK
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = store.borders(ids)
        again = store.borders(ids[::-1][:7])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got.dtype == torch.uint8 and got.shape == (len(ids), 3) and torch.equal(got, want)
    assert torch.equal(again, want.flip(0)[:7])
    means = np.stack([border_color_u8(np.mean(f.cpu().numpy().astype(np.float64), axis=(0, 1))) for f in full])
    assert np.array_equal(got.cpu().numpy(), means)
    assert store.borders([]).shape == (0, 3)
    assert store.nbytes == sum(store.resident.values()) and store.resident["border"] == 3 * len(ids) and store.resident["rows"] > 4 * len(ids)


def test_argument_errors_come_before_any_launch(resident, monkeypatch):
    store, ids, full, cases = resident
    launched = []
    real = abi.launch
    monkeypatch.setattr(abi, "launch", lambda lib, name, *args: launched.append(name) or real(lib, name, *args))
    with pytest.raises(ValueError):
        store.decode_rows(ids[:3], np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        store.decode_rows(ids[:3], np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        store.decode_rows(ids[:3], np.zeros((3, 2), np.float64))
    with pytest.raises(IndexError):
        store.decode_rows([0, len(store)], np.zeros((2, 2), np.int64))
    with pytest.raises(IndexError):
        store.decode_rows([-1], np.zeros((1, 2), np.int64))
    with pytest.raises(IndexError):
        store.borders([len(store)])
    assert launched == []
    store.decode_rows(ids[:2], np.array([[0, 1], [0, 1]]), check=True)
    assert launched == ["fear_jpeg_huffman_indexed_rows", "fear_jpeg_decode_u8"]


@pytest.mark.parametrize("config", [None, dict(photometric=True, colour_members="all", noise_members="all")], ids=["defaults", "all"])
def test_build_on_band_frames_with_the_stores_borders(config):
    """The intended use, on the 256 x 192 files: draw, frame_rows, decode_rows, build(borders=) against decode and build."""
    cases = [c for c in jpeghuff.supported() if c[0].startswith("256x192")]
    assert len(cases) == 7
    B, F = 12, len(cases)
    rng = np.random.default_rng(31)
    pairs = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % (F - 1)), (5, (k + 2) % (F - 1))):                    # the last frame is used by no pair
            bw, bh = rng.integers(6, 40), rng.integers(4, 14)
            pairs[k, col:col + 5] = [f, rng.integers(-10, 256 - bw + 10), rng.integers(-6, 192 - bh + 6), bw, bh]
        pairs[k, 10] = k != 3
    builder = TrainPairBuilder(config=config, device=0)
    store = JpegStore(device=0, threads=2)
    try:
        ids = store.add([c[1] for c in cases])
        shapes = store.shape(ids)
        params = builder.draw(pairs, shapes, np.random.default_rng(7))
        rows = builder.frame_rows(pairs, params, shapes)
        assert rows[-1].tolist() == [0, 0] and int(((rows[:-1, 1] - rows[:-1, 0]) < 160).sum()) >= 3
        whole = builder.build(store.decode(ids), pairs, params)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            bands = builder.build(store.decode_rows(ids, rows), pairs, params, borders=store.borders(ids))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        store.check()
        torch.cuda.synchronize()
        for name in ("template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox"):
            assert torch.equal(getattr(bands, name), getattr(whole, name)), name
        _equal(builder.build(store.decode(ids), pairs, params, borders=store.borders(ids).cpu().numpy()), whole)
    finally:
        store.close()
