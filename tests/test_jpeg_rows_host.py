"""Bands of rows from the resident JPEG store, the host side ("Bands of rows"): the row table
`jpeg_huffman.scan_row_sub` against a sequential walk of the scan; the band write pass stated in Python (`jpeg_entropy_bands_host`, and
lane by lane `jpeg_entropy_indexed_host(band=)`) against the matching slices of `jpeg_coefficients_host`, every MCU-row band of every
supported file; the pixel rule — a band's coefficients through the pixel model as an image of their own, with the halo of one MCU row
where chroma is subsampled vertically — against `jpeg_decode_host`'s rows; `plan_decode_rows` against a per-file loop; and
`TrainPairBuilder.frame_rows` and `borders=` through `build_host`."""
import numpy as np
import pytest

import jpeghuff
from jpegrows import all_bands, frames_and_pairs, slices, windows
from feartracker_amd import (jpeg_decode_host, jpeg_entropy_indexed_host, jpeg_pixels_host, jpeg_scan_index_host, jpeg_scan_prepare_host,
                             plan_decode_rows, scan_row_sub)
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi
from feartracker_amd.geometry import border_color_u8
from feartracker_amd.jpeg_huffman import _DC, _ERR, _Geometry, _decode, jpeg_entropy_bands_host
from feartracker_amd.jpeg_store import COLUMNS, KIND_PIXELS, KIND_SCAN, scan_columns
from feartracker_amd.train_data import TrainPairBuilder

_indexes: dict = {}


def _index(name, data, subsequence_bytes):
    """jpeg_scan_index_host of a file, computed once per length and shared."""
    key = (name, subsequence_bytes)
    if key not in _indexes:
        _indexes[key] = jpeg_scan_index_host(data, subsequence_bytes)
    return _indexes[key]


def _same(coef, ref):
    return len(coef) == len(ref) and all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(coef, ref))


# ---------------------------------------------------------------------------------------------------------------------- the row table
def _walked_row_sub(data, subsequence_bytes):
    """The subsequence in which the first block of every MCU row begins, by decoding every segment from its start: a block begins at the
    bit where its DC code does, and the lane that decodes a symbol is the one whose subsequence holds the symbol's first bit."""
    hd = jf._parse(data)
    stream, seg_start = jpeg_scan_prepare_host(data, hd)
    g = _Geometry(hd)
    SB = 8 * subsequence_bytes
    per_segment = hd.restart if hd.restart else g.n_mcu
    out, first_sub = {}, 0
    for s in range(len(seg_start) - 1):
        L = 8 * (seg_start[s + 1] - seg_start[s])
        ev = []
        _decode(stream[seg_start[s]:seg_start[s + 1]] + bytes(8), L, (0, 0, 0), L, g, ev)
        expected = min(per_segment, g.n_mcu - s * per_segment) * g.nslots
        at, ordinal = 0, 0                                                           # the position behind the last symbol
        for e in ev:
            if ordinal == expected and e[0] in (_ERR, _DC):                           # the padding behind the segment's last block
                break
            assert e[0] != _ERR
            if e[0] == _DC:
                mcu, slot = s * per_segment + ordinal // g.nslots, ordinal % g.nslots
                if slot == 0 and mcu % hd.mcus_x == 0:
                    out[mcu // hd.mcus_x] = first_sub + at // SB
                ordinal += 1
            at = e[-1]
        first_sub += -(-L // SB)
    return [out[r] for r in range(hd.mcus_y)] + [first_sub]


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_row_sub_equals_a_sequential_walk(subsequence_bytes):
    several = 0
    for name, data, _ in jpeghuff.supported():
        hd, sub_start, index, status = _index(name, data, subsequence_bytes)
        got = scan_row_sub(hd, sub_start, index)
        assert got.dtype == np.uint32 and got.shape == (hd.mcus_y + 1,) and got[-1] == len(index), name
        assert got.tolist() == _walked_row_sub(data, subsequence_bytes), name
        assert bool((np.diff(got.astype(np.int64)) >= 0).all()), name
        several += len(set(got.tolist())) > 2
    assert several > 20                                                              # rows that begin in different subsequences


# ------------------------------------------------------------------------------------------------------------------ the band write pass
@pytest.mark.parametrize("subsequence_bytes", [4, 128])
def test_band_write_pass_equals_the_slices_of_the_full_decode(subsequence_bytes):
    """Every MCU-row band [a, b) of every supported file: 1 to 300 bands per file (24 MCU rows).  jpeg_entropy_bands_host asserts
    that every position of a band is written exactly once."""
    reference, bands_seen = jpeghuff.reference(), 0
    for name, data, _ in jpeghuff.supported():
        hd, sub_start, index, status = _index(name, data, subsequence_bytes)
        bands = all_bands(hd.mcus_y)
        got = jpeg_entropy_bands_host(data, sub_start, index, subsequence_bytes, bands)
        for (a, b), (coef, status) in zip(bands, got):
            assert status == 0 and _same(coef, slices(hd, reference[name], a, b)), f"{name}: MCU rows {a}..{b}"
        bands_seen += len(bands)
    assert bands_seen == 1956


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_band_lanes_one_by_one(subsequence_bytes):
    """The lane-by-lane statement, as the kernel runs it: only the band's subsequences, in shuffled order, stores by the explicit range
    test.  The first row, the last, an inner band and the whole image of every file; the empty band and bands past the image."""
    reference = jpeghuff.reference()
    rng = np.random.default_rng(subsequence_bytes)
    for name, data, _ in jpeghuff.supported():
        hd, sub_start, index, status = _index(name, data, subsequence_bytes)
        R = hd.mcus_y
        row_sub = scan_row_sub(hd, sub_start, index)
        for a, b in sorted({(0, 1), (R - 1, R), (R // 3, max(R // 3 + 1, 2 * R // 3)), (0, R)}):
            lanes = min(int(row_sub[b]), len(index) - 1) - int(row_sub[a]) + 1
            for order in (None, rng.permutation(lanes)):
                coef, status = jpeg_entropy_indexed_host(data, sub_start, index, subsequence_bytes, order=order, band=(a, b), row_sub=row_sub)
                assert status == 0 and _same(coef, slices(hd, reference[name], a, b)), f"{name}: MCU rows {a}..{b}"
        coef, status = jpeg_entropy_indexed_host(data, sub_start, index, subsequence_bytes, band=(1, 1))
        assert status == 0 and all(c.shape[0] == 0 for c in coef), name                  # no rows: no lanes, nothing judged
        coef, status = jpeg_entropy_indexed_host(data, sub_start, index, subsequence_bytes, band=(R - 1, R + 5))   # clipped to the image
        assert status == 0 and _same(coef, slices(hd, reference[name], R - 1, R)), name


def test_a_band_runs_fewer_lanes_than_the_image():
    name, data, _ = next(c for c in jpeghuff.supported() if c[0] == "256x192_444_noisygradient_q95")
    hd, sub_start, index, _ = _index(name, data, 128)
    row_sub = scan_row_sub(hd, sub_start, index).astype(np.int64)
    quarter = row_sub[12] - row_sub[6] + 1
    assert len(index) > 300 and quarter < 0.3 * len(index)


# ---------------------------------------------------------------------------------------------------------------------- the planner
def _columns_of(lib, cases, subsequence_bytes=128):
    """The mirror's columns and the ragged row table of `cases`, as JpegStore.add fills them, without a device."""
    columns, tables, used = np.zeros(len(cases), dtype=COLUMNS), [], 0
    for k, (name, data, _) in enumerate(cases):
        info, _, seg, scan = jpeghuff.c_prepare(lib, data)
        hd, sub_start, index, _ = _index(name, data, subsequence_bytes)
        scan_columns(columns[k], info, scan.n_seg, len(index), used)
        tables.append(scan_row_sub(hd, sub_start, index))
        used += tables[-1].size
    return columns, np.concatenate(tables)


def test_the_pixel_rule_of_a_band_with_its_halo():
    """A window's band, as plan_decode_rows cuts it, through the pixel model as an image of its own: the window's rows are
    jpeg_decode_host's, whatever the model makes of the band's outermost rows."""
    lib = abi.load_train_library()
    cases, reference = jpeghuff.supported(), jpeghuff.reference()
    columns, row_sub = _columns_of(lib, cases)
    halos = windows_seen = 0
    for k, (name, data, _) in enumerate(cases):
        hd = jf._parse(data)
        full = jpeg_decode_host(data)
        wins = windows(hd.height, 8 * hd.v[0])
        plans = plan_decode_rows(columns, row_sub, np.full(len(wins), k), np.array(wins), 1 << 40)
        assert len(plans) == 1 and plans[0]["scan"].size == len(wins)
        plan, bands = plans[0], {}
        for j, (y0, y1) in enumerate(wins):
            a, n, high, top = int(plan["mcu_row0"][j]), int(plan["mcu_rows"][j]), int(plan["band_height"][j]), int(plan["band_y0"][j])
            assert top == a * 8 * hd.v[0] and top <= y0 and y1 <= top + high <= hd.height and plan["band_out"][j] == 3 * hd.width * top
            if (a, n) not in bands:
                bands[a, n] = jpeg_pixels_host(hd, slices(hd, reference[name], a, a + n), height=high)
            assert bands[a, n].shape == (high, hd.width, 3)
            assert np.array_equal(bands[a, n][y0 - top:y1 - top], full[y0:y1]), f"{name}: rows {y0}..{y1}"
            if hd.v[0] == 2 and 0 < a and a + n < hd.mcus_y:                           # an inner band's outermost rows are wrong: the halo
                halos += not np.array_equal(bands[a, n], full[top:top + high])
        windows_seen += len(wins)
    assert halos > 20 and windows_seen > 3000


def _naive_rows_plan(columns, row_sub, ids, rows, limit):
    """plan_decode_rows one file at a time, by the band geometry as DESIGN.md states it."""
    groups, cur, dense = [], None, 0
    for pos, (i, (y0, y1)) in enumerate(zip(ids, rows)):
        col = columns[i]
        H, W, mcu_h = int(col["H"]), int(col["W"]), int(col["mcu_h"])
        y0, y1 = min(max(int(y0), 0), H), min(max(int(y1), 0), H)
        band = None
        if col["kind"] == KIND_SCAN and y0 < y1:
            a, b = y0 // mcu_h, -(-y1 // mcu_h)
            if col["halo"]:
                a, b = max(a - 1, 0), min(b + 1, int(col["mcus_y"]))
            table = row_sub[int(col["row_at"]):int(col["row_at"]) + int(col["mcus_y"]) + 1]
            first, last = int(table[a]), min(int(table[b]), int(col["n_sub"]) - 1)
            high = (b - a) * mcu_h if b < int(col["mcus_y"]) else H - a * mcu_h
            band = (a, b - a, first, max(last - first + 1, 0), high, (b - a) * int(col["mcus_x"]) * int(col["nslots"]))
        need = 128 * band[5] if band else 0
        if cur is None or dense + need > limit:
            cur = dict(lo=pos, scan=[], sub=[0], blk=[0], pix=[0], coef=[], out=[], values=0, out_bytes=0, most=0, bands=[], band_out=[])
            groups.append(cur)
            dense = 0
        dense += need
        cur["hi"] = pos + 1
        cur["out"].append(cur["out_bytes"])
        cur["out_bytes"] += -(-H * W * 3 // 16) * 16
        if band:
            cur["scan"].append(pos - cur["lo"])
            cur["bands"].append(band[:5])
            cur["band_out"].append(3 * W * band[0] * mcu_h)
            cur["sub"].append(cur["sub"][-1] + -(-band[3] // 256))
            cur["blk"].append(cur["blk"][-1] + -(-band[5] // 32))
            cur["pix"].append(cur["pix"][-1] + -(-band[4] * W // 256))
            cur["coef"].append(cur["values"])
            cur["values"] += 64 * band[5]
            cur["most"] = max(cur["most"], band[5])
    return groups


@pytest.mark.parametrize("limit", [1 << 30, 60_000, 1])
def test_rows_planner_against_a_per_file_loop(limit):
    """Real files' columns and row tables with a "pixels" row among them; ids in any order with repeats, windows of every kind — whole,
    empty, reversed, past the image — and a workspace_limit that forces several groups."""
    lib = abi.load_train_library()
    cases = jpeghuff.supported()
    columns, row_sub = _columns_of(lib, cases)
    columns = np.concatenate([columns, np.zeros(1, dtype=COLUMNS)])
    columns[-1]["H"], columns[-1]["W"], columns[-1]["kind"] = 31, 33, KIND_PIXELS
    rng = np.random.default_rng(13)
    ids = np.concatenate([rng.permutation(len(columns)), rng.integers(0, len(columns), 150)])
    H = columns["H"][ids].astype(np.int64)
    y0 = rng.integers(-3, H + 3)
    y1 = np.where(rng.random(ids.size) < 0.15, y0 - rng.integers(0, 3, ids.size), rng.integers(-3, H + 6))
    whole = rng.random(ids.size) < 0.1
    rows = np.stack([np.where(whole, 0, y0), np.where(whole, H, y1)], axis=1)
    got, want = plan_decode_rows(columns, row_sub, ids, rows, limit), _naive_rows_plan(columns, row_sub, ids, rows, limit)
    assert len(got) == len(want) and (len(got) == 1) == (limit == 1 << 30) and (limit > 1 or len(got) > 100)
    empty = 0
    for g, w in zip(got, want):
        assert (g["lo"], g["hi"], g["values"], g["out_bytes"], g["most"]) == (w["lo"], w["hi"], w["values"], w["out_bytes"], w["most"])
        assert g["scan"].tolist() == w["scan"]
        bands = list(zip(g["mcu_row0"].tolist(), g["mcu_rows"].tolist(), g["sub0"].tolist(), g["sub_count"].tolist(), g["band_height"].tolist()))
        assert bands == w["bands"] and g["band_out"].tolist() == w["band_out"]
        assert g["sub_prefix"].dtype == np.uint32 and g["sub_prefix"].tolist() == w["sub"]
        assert g["block_prefix"].tolist() == w["blk"] and g["pixel_prefix"].tolist() == w["pix"]
        assert g["coef_offset"].tolist() == w["coef"] and g["plane_offset"].tolist() == w["coef"] and g["out_offset"].tolist() == w["out"]
        assert g["workspace_bytes"] == 16 + w["values"] and not (g["plane_offset"] % 16).any() and not (g["out_offset"] % 16).any()
        assert all(n >= 1 and c >= 1 and h >= 1 for _, n, _, c, h in bands)
        empty += g["hi"] - g["lo"] - g["scan"].size
    assert empty > 20                                                                # empty windows and the "pixels" row launch nothing
    assert plan_decode_rows(columns, row_sub, [], np.zeros((0, 2), np.int64), limit) == []


# ------------------------------------------------------------------------------------------------------------- the builder's two halves
@pytest.fixture(scope="module")
def built():
    """build_host on the clean frames, once; the builder, the params and the frames with it."""
    frames, pairs = frames_and_pairs()
    builder = TrainPairBuilder(device="cpu")
    params = builder.draw(pairs, [f.shape[:2] for f in frames], np.random.default_rng(5))
    return builder, frames, pairs, params, builder.build_host(frames, pairs, params)


def _equal_batches(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_frame_rows_are_the_rows_a_build_reads(built):
    builder, frames, pairs, params, clean = built
    shapes = [f.shape[:2] for f in frames]
    rows = builder.frame_rows(pairs, params, shapes)
    assert rows.dtype == np.int64 and rows.shape == (5, 2)
    assert rows[4].tolist() == [0, 0]                                               # a frame no pair uses
    assert all(0 <= a <= b <= s[0] for (a, b), s in zip(rows.tolist(), shapes))
    assert any(b - a < s[0] for (a, b), s in zip(rows.tolist(), shapes))            # and not simply everything
    tab = builder.tables(pairs, params)
    for k in range(len(pairs)):                                                     # every context row inside its frame is covered
        for f, ctx in ((int(pairs[k, 0]), tab["t_ctx"][k]), (int(pairs[k, 5]), tab["s_ctx"][k])):
            lo, hi = max(int(ctx[1]), 0), min(int(ctx[1]) + int(ctx[3]), shapes[f][0])
            assert lo >= hi or (rows[f, 0] <= lo and hi <= rows[f, 1])
    means = np.stack([border_color_u8(np.mean(f, axis=(0, 1))) for f in frames])
    rng = np.random.default_rng(17)
    dirty = []
    for f, (a, b) in zip(frames, rows.tolist()):
        d = rng.integers(0, 256, f.shape, dtype=np.uint8)
        d[a:b] = f[a:b]
        dirty.append(d)
    assert sum(not np.array_equal(d, f) for d, f in zip(dirty, frames)) >= 2 and rows[2, 1] - rows[2, 0] < 192   # rows were overwritten
    _equal_batches(builder.build_host(dirty, pairs, params, borders=means), clean)


def test_given_borders_equal_the_computed_ones(built):
    builder, frames, pairs, params, clean = built
    means = np.stack([border_color_u8(np.mean(f, axis=(0, 1))) for f in frames])
    _equal_batches(builder.build_host(frames, pairs, params, borders=means), clean)
    other = builder.build_host(frames, pairs, params, borders=(means + 90).astype(np.uint8))
    assert not np.array_equal(other.template, clean.template)                        # the colours are used: some context lies outside
    with pytest.raises(ValueError):
        builder.build_host(frames, pairs, params, borders=means[:4])
    with pytest.raises(ValueError):
        builder.build_host(frames, pairs, params, borders=means.astype(np.int32))
