"""Rows from the device, the host side ("Rows from the device"): the numpy statement of
`fear_jpeg_huffman_indexed_rows_dev` and `fear_jpeg_decode_u8_rows_dev` (`jpeg_entropy_rows_device_host`, `jpeg_rows_device_host`) on every
supported file of jpeg_decode.npz and the baseline transcodes of jpeg_progressive.npz — the lanes that run, the positions that are
written in the full-image layout, and the pixel rows that follow from them whatever the rest of the buffer holds — and the numpy
statement of `fear_tracker_rows` (`search_rows_host`) against a walk of the crop's row taps."""
import zlib

import numpy as np
import pytest

import jpegdec
import jpegprog
from jpegrows import windows
from feartracker_amd import (jpeg_decode_host, jpeg_entropy_rows_device_host, jpeg_pixels_host, jpeg_rows_device_host, jpeg_scan_index_host,
                             jpeg_to_baseline_host, scan_row_sub, search_rows_host)
from feartracker_amd import jpeg_frames as jf
from feartracker_amd.geometry import _linear_taps
from feartracker_amd.jpeg_huffman import jpeg_entropy_rows_device_many_host, rows_band

_files = _full = None
_pixels: dict = {}


def files():
    """[(name, a baseline file)]: every supported file of jpeg_decode.npz and the transcode of every file of jpeg_progressive.npz."""
    global _files
    if _files is None:
        _files = [(name, data) for name, data, _ in jpegdec.supported()]
        _files += [("transcode_" + name, jpeg_to_baseline_host(data)) for name, data, _, _ in jpegprog.cases()]
    return _files


def reference():
    """{name: (header, jpeg_coefficients_host's coefficients, jpeg_decode_host's frame)}, computed once, shared and left unchanged."""
    global _full
    if _full is None:
        _full = {}
        for name, data in files():
            hd, coef = jf.jpeg_coefficients_host(data)
            frame = jpeg_pixels_host(hd, coef)
            for c in coef + [frame]:
                c.setflags(write=False)
            _full[name] = (hd, coef, frame)
    return _full


def band_mask(hd, coef, band):
    """1 on every position of the blocks of the MCU rows a .. b), 0 elsewhere, per component in the full-image layout."""
    out = [np.zeros(c.shape, dtype=np.int64) for c in coef]
    if band is not None:
        for c, m in enumerate(out):
            v = hd.v[0] if c == 0 else 1
            m[band[0] * v:band[1] * v] = 1
    return out


def band_pixels(name, hd, coef, band):
    """jpeg_pixels_host of the reference coefficients with every position outside the band's blocks replaced by seeded random int16:
    what the pixel stage sees when the buffer held anything.  Once per band; the tests at every subsequence length share it, after
    asserting that the written positions are exactly the band's and hold the reference's values."""
    key = (name, band)
    if key not in _pixels:
        rng = np.random.default_rng([zlib.crc32(name.encode()), *band])
        held = [np.where(m > 0, c, rng.integers(-32768, 32768, c.shape).astype(np.int16)) for c, m in zip(coef, band_mask(hd, coef, band))]
        _pixels[key] = jpeg_pixels_host(hd, held)
    return _pixels[key]


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_lanes_written_positions_and_rows_of_every_window(subsequence_bytes):
    """The first row, the last row, the whole image and every MCU-aligned window moved by one row at either end, of every file."""
    ref, seen, halos, idle = reference(), 0, 0, 0
    for name, data in files():
        hd, coef, full = ref[name]
        _, sub_start, index, status = jpeg_scan_index_host(data, subsequence_bytes)
        assert status == 0, name
        row_sub = scan_row_sub(hd, sub_start, index)
        mcu_h, n_sub = 8 * hd.v[0], len(index)
        wins = windows(hd.height, mcu_h)
        bands = [rows_band(y0, y1, mcu_h * hd.mcus_y, mcu_h, hd.mcus_y, hd.v[0] == 2) for y0, y1 in wins]
        first = {}                                                                       # the first window of every band
        for w, band in zip(wins, bands):
            first.setdefault(band, w)
        got = jpeg_entropy_rows_device_many_host(data, sub_start, index, subsequence_bytes, list(first.values()), row_sub)
        for band, (lanes, dense, mask, status) in zip(first, got):                       # what is the same for every window of a band
            a, b = band
            assert status == 0, name
            # the lanes that run
            assert list(lanes) == list(range(int(row_sub[a]), min(int(row_sub[b]), n_sub - 1) + 1)), f"{name}: MCU rows {a}..{b}"
            # the written positions: exactly the widened band's blocks, each once, with the full decode's values
            for c, (m, want) in enumerate(zip(mask, band_mask(hd, coef, band))):
                assert np.array_equal(m, want), f"{name}: MCU rows {a}..{b}, component {c}"
                assert np.array_equal(dense[c][want > 0], coef[c][want > 0]), f"{name}: MCU rows {a}..{b}, component {c}"
            idle += len(lanes) < n_sub
        for (y0, y1), band in zip(wins, bands):
            a, b = band
            assert a * mcu_h <= y0 and y1 <= b * mcu_h
            # the pixel rows, whatever the unwritten positions hold
            px = band_pixels(name, hd, coef, band)
            assert np.array_equal(px[y0:y1], full[y0:y1]), f"{name}: rows {y0}..{y1}"
            if hd.v[0] == 2 and 0 < a and b < hd.mcus_y:
                halos += not np.array_equal(px[a * mcu_h:b * mcu_h], full[a * mcu_h:b * mcu_h])
        seen += len(wins)
    # many windows; an inner band's outermost rows ARE wrong where chroma is subsampled vertically; most bands leave lanes idle
    assert seen > 3000 and halos >= 1 and idle > 300


def test_the_window_the_many_form_was_given_is_the_band():
    """(The test above hands `jpeg_entropy_rows_device_many_host` one window per band: this pins that every window of a band gives the
    band's result, on one file, window by window through the one-window form.)"""
    name, data = next(f for f in files() if f[0].startswith("15x50_420_random_q100_rst3"))
    hd, coef, full = reference()[name]
    _, sub_start, index, _ = jpeg_scan_index_host(data, 16)
    row_sub = scan_row_sub(hd, sub_start, index)
    for y0, y1 in windows(hd.height, 16):
        a, b = rows_band(y0, y1, 16 * hd.mcus_y, 16, hd.mcus_y, True)
        lanes, dense, mask, status = jpeg_entropy_rows_device_host(data, sub_start, index, 16, y0, y1, row_sub)
        assert status == 0 and lanes == range(int(row_sub[a]), min(int(row_sub[b]), len(index) - 1) + 1)
        assert all(np.array_equal(m, w) for m, w in zip(mask, band_mask(hd, coef, (a, b))))


def test_empty_clipped_and_reversed_windows():
    name, data = next(f for f in files() if f[0].startswith("40x24_420_random_q75_rstrows1"))
    hd, coef, full = reference()[name]
    H = hd.height
    _, sub_start, index, _ = jpeg_scan_index_host(data, 16)
    for y0, y1 in ((0, 0), (H, H), (5, 5), (9, 3), (-7, 0), (-7, -2)):
        lanes, dense, mask, status = jpeg_entropy_rows_device_host(data, sub_start, index, 16, y0, y1)
        assert status == 0 and len(lanes) == 0 and not any(m.any() for m in mask), (y0, y1)
    for (y0, y1), same in (((-5, 3), (0, 3)), ((H - 1, H + 9), (H - 1, H)), ((-100, 10_000), (0, H))):
        got, want = (jpeg_entropy_rows_device_host(data, sub_start, index, 16, *w) for w in ((y0, y1), same))
        assert got[0] == want[0] and all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))
    # the whole statement in one call, noise where nothing was stored
    noise = np.random.default_rng(3).integers(-32768, 32768, sum(c.size for c in coef)).astype(np.int16)
    lanes, dense, mask, frame = jpeg_rows_device_host(data, 7, 20, 16, fill=noise)
    assert frame.shape == full.shape and np.array_equal(frame[7:20], full[7:20]) and not frame[:7].any() and not frame[20:].any()
    assert np.array_equal(jpeg_rows_device_host(data, -3, H + 4)[3], jpeg_decode_host(data))


def test_the_band_rule_is_the_host_planners():
    """`rows_band` with the image's height as the limit (the pixel kernels' form) gives the band `plan_decode_rows` plans, for seeded
    windows of every kind; with the rows of the MCU grid as the limit (the entropy kernel's form) it differs only for windows that begin
    in the padding rows behind the image."""
    import jpeghuff
    from feartracker_amd import plan_decode_rows
    from feartracker_amd import train_abi as abi
    from feartracker_amd.jpeg_store import COLUMNS, scan_columns
    lib = abi.load_train_library()
    cases = jpegdec.supported()
    columns, tables, used = np.zeros(len(cases), dtype=COLUMNS), [], 0
    for k, (name, data, _) in enumerate(cases):
        info, _, seg, scan = jpeghuff.c_prepare(lib, data)
        hd, sub_start, index, _ = jpeg_scan_index_host(data, 128)
        scan_columns(columns[k], info, scan.n_seg, len(index), used)
        tables.append(scan_row_sub(hd, sub_start, index))
        used += tables[-1].size
    rng = np.random.default_rng(61)
    ids = rng.integers(0, len(cases), 2000)
    H = columns["H"][ids].astype(np.int64)
    y0 = rng.integers(-20, H + 20)
    rows = np.stack([y0, y0 + rng.integers(-3, 40, ids.size)], axis=1)
    (plan,) = plan_decode_rows(columns, np.concatenate(tables), ids, rows, 1 << 40)
    planned = {int(p): (int(a), int(a + n)) for p, a, n in zip(plan["scan"], plan["mcu_row0"], plan["mcu_rows"])}
    differ = 0
    for p, (i, (a, b)) in enumerate(zip(ids, rows.tolist())):
        col = columns[i]
        mcu_h, mcus_y, halo = int(col["mcu_h"]), int(col["mcus_y"]), bool(col["halo"])
        assert rows_band(a, b, int(col["H"]), mcu_h, mcus_y, halo) == planned.get(p), (cases[i][0], a, b)
        grid = rows_band(a, b, mcu_h * mcus_y, mcu_h, mcus_y, halo)
        if grid != planned.get(p):
            assert p not in planned and a >= int(col["H"])                               # begins behind the image: nothing to store
            differ += 1
    assert len(planned) > 1000 and differ > 0


# ----------------------------------------------------------------------------------------------------------------- the tracker's rows
def _walked_rows(ctx, S):
    """Every frame row that crop_resize_normalize_kernel's `sample` is called with for one context box, over all S x S output pixels:
    the identity path (w == h == S) samples row d, the 2 x 2 path (w == h == 2 S) rows 2 d and 2 d + 1, every other box the two
    clipped taps of the bilinear row table."""
    x, y, w, h = (int(v) for v in ctx)
    if w == S and h == S:
        taps = set(range(S))
    elif w == 2 * S and h == 2 * S:
        taps = set(range(2 * S))
    else:
        with np.errstate(divide="ignore"):
            idx = _linear_taps(S, h, clamp=False)[0] if h != 0 else np.full(S, -1)       # (h == 0: scale 0, every position -0.5)
        taps = set(np.clip(idx, 0, h - 1).tolist()) | set(np.clip(idx + 1, 0, h - 1).tolist())
    return {y + t for t in taps}


def test_search_rows_host_against_a_walk_of_the_taps():
    rng = np.random.default_rng(29)
    S, H = 64, 200
    boxes = []
    for _ in range(60):                                                                  # sizes around S, 2 S and far beyond
        h = int(rng.choice([1, 2, 3, 7, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 5 * S + 3, int(rng.integers(1, 900))]))
        w = int(rng.choice([h, S, 2 * S, int(rng.integers(1, 900))]))
        boxes.append([int(rng.integers(-300, 300)), int(rng.integers(-2 * h - 50, H + 50)), w, h])
    boxes += [[10, 20, S, S], [10, 20, 2 * S, 2 * S], [10, 20, S, 2 * S], [10, 20, 2 * S, S]]    # the two exact paths and their near misses
    boxes += [[5, 50, 30, 0], [5, 0, 30, 0], [5, 50, 0, 0], [5, 50, 30, 1], [5, -1, 30, 1], [5, H, 30, 1]]   # height 0 and 1
    boxes += [[5, -500, 30, 40], [5, H + 300, 30, 40], [-900, 50, 30, 40], [5, -40, 30, 40], [5, H - 1, 30, 40]]   # wholly | partly outside
    boxes = np.array(boxes, dtype=np.int64)
    # one target per stream: the range is the walk's, end to end (the taps move monotonically: nothing but the ends is needed)
    got = search_rows_host(boxes, np.arange(len(boxes)), len(boxes), S)
    assert got.dtype == np.int32 and got.shape == (len(boxes), 2)
    for ctx, (y0, y1) in zip(boxes, got.tolist()):
        rows = _walked_rows(ctx, S)
        assert (y0, y1) == (min(rows), max(rows) + 1), ctx
        h = int(ctx[3])
        if 1 <= h <= S or (ctx[2], h) == (2 * S, 2 * S):
            assert (y0, y1) == (ctx[1], ctx[1] + h)                                      # every row of the box
        elif h >= 1:
            assert ctx[1] <= y0 < y1 <= ctx[1] + h                                       # a reduction: inside the box
        else:
            assert (y0, y1) == (ctx[1] + h - 1, ctx[1] + h)                              # degenerate: the row above the box
    # several targets per stream, streams without targets, a target on a stream that is not asked for
    stream = rng.integers(0, 9, len(boxes))
    stream[stream == 4] = 5
    got = search_rows_host(boxes, stream, 7, S)
    for s in range(7):
        mine = [_walked_rows(c, S) for c in boxes[stream == s]]
        want = [min(min(r) for r in mine), max(max(r) for r in mine) + 1] if mine else [0, 0]
        assert got[s].tolist() == want, s
    assert got[4].tolist() == [0, 0] and search_rows_host(np.zeros((0, 4)), np.zeros(0), 3, S).tolist() == [[0, 0]] * 3
    assert search_rows_host(boxes, stream, 0, S).shape == (0, 2)
