"""Windows from the resident JPEG store, the host side ("Windows"): `plan_decode_windows` against a per-file loop;
the window write pass stated in Python (`jpeg_entropy_indexed_host(band=, cols=)`) through the pixel model as an image of its own against
the rectangle of `jpeg_decode_host`, at every scale; the lane rule (`window_lanes`) held to the lanes that really hold a block of the
window; `TrainPairBuilder.frame_windows` against a brute-force union; and `build_host` on a `WindowFrames` against whole frames."""
import copy

import numpy as np
import pytest

import jpeghuff
import jpegwin
from jpegrows import frames_and_pairs
from feartracker_amd import jpeg_decode_host, jpeg_entropy_indexed_host, jpeg_pixels_host, jpeg_scan_index_host, scan_row_sub
from feartracker_amd import train_abi as abi
from feartracker_amd.geometry import border_color_u8
from feartracker_amd.jpeg_huffman import _record_lanes, window_lanes
from feartracker_amd.jpeg_store import (COLUMNS, KIND_PIXELS, KIND_SCAN, WindowFrames, plan_decode, plan_decode_rows, plan_decode_windows,
                                        scan_columns)
from feartracker_amd.train_data import TrainPairBuilder

SB = 128
_indexes: dict = {}


def _baseline():
    return [f for f in jpegwin.files() if not f[2]]


def _index(name, data):
    if name not in _indexes:
        hd, sub_start, index, status = jpeg_scan_index_host(data, SB)
        assert status == 0, name
        _indexes[name] = (hd, sub_start, index, scan_row_sub(hd, sub_start, index))
    return _indexes[name]


def _columns():
    lib = abi.load_train_library()
    cases = _baseline()
    columns, tables, used = np.zeros(len(cases) + 1, dtype=COLUMNS), [], 0
    for k, (name, data, _) in enumerate(cases):
        info, _, seg, scan = jpeghuff.c_prepare(lib, data)
        hd, sub_start, index, row_sub = _index(name, data)
        scan_columns(columns[k], info, scan.n_seg, len(index), used)
        tables.append(row_sub)
        used += row_sub.size
    columns[-1]["H"], columns[-1]["W"], columns[-1]["kind"] = 31, 33, KIND_PIXELS
    return cases, columns, np.concatenate(tables)


# ------------------------------------------------------------------------------------------------------------------------- the planner
def _geometry(hd, window, scale):
    """The window's MCUs by the rule DESIGN.md states, for one file: None for the empty window, else a dict."""
    m = 8 // scale
    H, W = -(-hd.height * m // 8), -(-hd.width * m // 8)
    y0, y1, x0, x1 = jpegwin.clipped(window, H, W)
    if y0 >= y1:
        return None
    h, v = (hd.h[0], hd.v[0])
    mcu_h, mcu_w = v * m, h * m
    a, b, c0, c1 = y0 // mcu_h, -(-y1 // mcu_h), x0 // mcu_w, -(-x1 // mcu_w)
    if v == 2 and scale == 1:
        a, b = max(a - 1, 0), min(b + 1, hd.mcus_y)
    if h == 2:
        c0, c1 = max(c0 - 1, 0), min(c1 + 1, hd.mcus_x)
    return dict(a=a, b=b, c0=c0, c1=c1, oy=a * mcu_h, ox=c0 * mcu_w, high=min(b * mcu_h, H) - a * mcu_h, wide=min(c1 * mcu_w, W) - c0 * mcu_w,
                high_full=min(b * 8 * v, hd.height) - a * 8 * v, wide_full=min(c1 * 8 * h, hd.width) - c0 * 8 * h, rect=(y0, y1, x0, x1))


@pytest.mark.parametrize("scale", [1, 2, 8])
@pytest.mark.parametrize("limit", [1 << 30, 20_000, 1])
def test_windows_planner_against_a_per_file_loop(limit, scale):
    cases, columns, row_sub = _columns()
    rng = np.random.default_rng(limit % 97 + scale)
    ids = np.concatenate([rng.permutation(len(columns)), rng.integers(0, len(columns), 60)])
    m = 8 // scale
    H, W = -(-columns["H"][ids].astype(np.int64) * m // 8), -(-columns["W"][ids].astype(np.int64) * m // 8)
    y0, x0 = rng.integers(-3, H + 3), rng.integers(-3, W + 3)
    y1 = np.where(rng.random(ids.size) < 0.15, y0 - 1, rng.integers(-3, H + 6))
    x1 = rng.integers(-3, W + 6)
    whole = rng.random(ids.size) < 0.1
    wins = np.stack([np.where(whole, 0, y0), np.where(whole, H, y1), np.where(whole, 0, x0), np.where(whole, W, x1)], axis=1)
    if scale > 1:                                                        # (a "pixels" entry cannot be decoded at a scale: the store refuses it)
        keep = columns["kind"][ids] == KIND_SCAN
        ids, wins, H, W = ids[keep], wins[keep], H[keep], W[keep]
    got = plan_decode_windows(columns, row_sub, ids, wins, limit, scale=scale)
    # the per-file loop
    want, cur, dense = [], None, 0
    for pos, (i, win) in enumerate(zip(ids.tolist(), wins)):
        col = columns[i]
        geo = None
        if col["kind"] == KIND_SCAN:
            hd = _index(*cases[i][:2])[0]
            geo = _geometry(hd, win, scale)
        blocks = (geo["b"] - geo["a"]) * (geo["c1"] - geo["c0"]) * int(col["nslots"]) if geo else 0
        if cur is None or dense + 128 * blocks > limit:
            cur = dict(lo=pos, scan=[], sub=[0], blk=[0], pix=[0], coef=[], out=[], values=0, out_bytes=0, rec=[], origin=[], shape=[], window=[])
            want.append(cur)
            dense = 0
        dense += 128 * blocks
        cur["hi"] = pos + 1
        cur["out"].append(cur["out_bytes"])
        if geo:
            table = row_sub[int(col["row_at"]):int(col["row_at"]) + int(col["mcus_y"]) + 1]
            first, last = int(table[geo["a"]]), min(int(table[geo["b"]]), int(col["n_sub"]) - 1)
            cur["scan"].append(pos - cur["lo"])
            cur["rec"].append((geo["a"], geo["b"] - geo["a"], first, last - first + 1, geo["c0"] | (geo["c1"] - geo["c0"]) << 16,
                               geo["high_full"], geo["wide_full"]))
            cur["sub"].append(cur["sub"][-1] + -(-(last - first + 1) // 256))
            cur["blk"].append(cur["blk"][-1] + -(-blocks // 32))
            cur["pix"].append(cur["pix"][-1] + -(-geo["high"] * geo["wide"] // 256))
            cur["coef"].append(cur["values"])
            cur["values"] += 64 * blocks
            cur["origin"].append((geo["oy"], geo["ox"]))
            cur["shape"].append((geo["high"], geo["wide"]))
            cur["window"].append(geo["rect"])
        else:
            rect = jpegwin.clipped(win, int(H[pos]), int(W[pos])) if col["kind"] == KIND_PIXELS else (0, 0, 0, 0)
            cur["origin"].append((rect[0], rect[2]))
            cur["shape"].append((rect[1] - rect[0], rect[3] - rect[2]))
            cur["window"].append(rect)
        cur["out_bytes"] += -(-3 * cur["shape"][-1][0] * cur["shape"][-1][1] // 16) * 16
    assert len(got) == len(want) and (len(got) == 1) == (limit == 1 << 30) and (limit > 1 or len(got) > 30)
    for g, w in zip(got, want):
        assert (g["lo"], g["hi"], g["values"], g["out_bytes"]) == (w["lo"], w["hi"], w["values"], w["out_bytes"])
        assert g["scan"].tolist() == w["scan"]
        rec = list(zip(*(g[key].tolist() for key in ("mcu_row0", "mcu_rows", "sub0", "sub_count", "cols", "band_height", "win_width"))))
        assert rec == w["rec"]
        assert g["sub_prefix"].tolist() == w["sub"] and g["block_prefix"].tolist() == w["blk"] and g["pixel_prefix"].tolist() == w["pix"]
        assert g["coef_offset"].tolist() == w["coef"] and g["out_offset"].tolist() == w["out"] and not g["band_out"].any()
        assert g["origin"].tolist() == [list(o) for o in w["origin"]] and g["window"].tolist() == [list(r) for r in w["window"]]
        assert list(zip(g["high"].tolist(), g["wide"].tolist())) == w["shape"]
        assert g["workspace_bytes"] == 16 + w["values"] and not (g["out_offset"] % 16).any()
    assert plan_decode_windows(columns, row_sub, [], np.zeros((0, 4), np.int64), limit, scale=scale) == []


@pytest.mark.parametrize("per_position", [False, True])
@pytest.mark.parametrize("scale", [1, 2, 8])
def test_the_three_plans_agree_where_their_requests_do(scale, per_position):
    """The three plans are built from the same parts: a window of a frame's whole width plans the band `plan_decode_rows` plans for its
    rows, and the rows of a whole frame plan the image `plan_decode` plans — group by group, values and dtypes."""
    cases, columns, row_sub = _columns()
    rng = np.random.default_rng(scale)
    entries = len(columns) if scale == 1 else len(cases)                 # (a "pixels" entry cannot be decoded at a scale)
    ids = np.concatenate([rng.permutation(entries), rng.integers(0, entries, 40)])
    scales = np.full(ids.size, scale) if per_position else scale
    m = 8 // scale
    H, W = -(-columns["H"][ids].astype(np.int64) * m // 8), -(-columns["W"][ids].astype(np.int64) * m // 8)
    y0 = rng.integers(-3, H + 3)
    y1 = np.where(rng.random(ids.size) < 0.15, y0 - 1, rng.integers(-3, H + 6))      # empty, to the edges and out of range among them
    zeros = np.zeros(ids.size, dtype=np.int64)

    def same(got, want, keys):
        assert len(got) == len(want) > 0
        for g, w in zip(got, want):
            assert (g["lo"], g["hi"]) == (w["lo"], w["hi"]) and np.array_equal(g["scan"], w["scan"])
            for key in keys:
                assert type(g[key]) is type(w[key]) and np.array_equal(g[key], w[key]), key
                assert not isinstance(w[key], np.ndarray) or g[key].dtype == w[key].dtype, key

    for limit in (1 << 30, 20_000):
        rows = plan_decode_rows(columns, row_sub, ids, np.stack([y0, y1], axis=1), limit, scale=scales)
        wins = plan_decode_windows(columns, row_sub, ids, np.stack([y0, y1, zeros, W], axis=1), limit, scale=scales)
        same(wins, rows, ("sub0", "sub_count", "sub_prefix", "mcu_row0", "mcu_rows", "band_height", "block_prefix", "coef_offset"))
        whole = plan_decode_rows(columns, row_sub, ids, np.stack([zeros, H], axis=1), limit, scale=scales)
        same(whole, plan_decode(columns, ids, limit, scale=scales), ("block_prefix", "pixel_prefix", "coef_offset", "values", "most"))
        assert (len(rows) == 1) == (len(whole) == 1) == (limit == 1 << 30)


# -------------------------------------------------------------------------------------------- the write pass, the pixels, the lane rule
def _held(recorded, geo):
    """The lanes that hold a block of the window, from every store every lane makes."""
    lane_of, my, mx = recorded[:3]
    inside = (my >= geo["a"]) & (my < geo["b"]) & (mx >= geo["c0"]) & (mx < geo["c1"])
    return set(lane_of[inside].tolist())


@pytest.mark.parametrize("scale", [1, 2, 8])
def test_window_write_pass_and_pixels_equal_the_rectangle_of_the_full_decode(scale):
    """Every file and every window of jpegwin: the lanes `window_lanes` names, the stores by the explicit row and column tests, the
    window's coefficients through the pixel model as an image of its own width and height."""
    halos = 0
    for name, data, _ in _baseline():
        hd, sub_start, index, row_sub = _index(name, data)
        full = jpeg_decode_host(data, scale=scale)
        m = 8 // scale
        seen = {}
        for win in jpegwin.windows(full.shape[0], full.shape[1], hd.v[0] * m, hd.h[0] * m):
            geo = _geometry(hd, win, scale)
            if geo is None:
                continue
            key = (geo["a"], geo["b"], geo["c0"], geo["c1"])
            if key not in seen:
                coef, status = jpeg_entropy_indexed_host(data, sub_start, index, SB, band=key[:2], row_sub=row_sub, cols=key[2:])
                assert status == 0, name                                 # (and every position written exactly once: asserted inside)
                image = copy.copy(hd)
                image.width = geo["wide_full"]
                seen[key] = jpeg_pixels_host(image, coef, height=geo["high_full"], scale=scale)
            px = seen[key]
            assert px.shape == (geo["high"], geo["wide"], 3), (name, win)
            y0, y1, x0, x1 = geo["rect"]
            assert np.array_equal(px[y0 - geo["oy"]:y1 - geo["oy"], x0 - geo["ox"]:x1 - geo["ox"]], full[y0:y1, x0:x1]), (name, win.tolist())
            halos += not np.array_equal(px, full[geo["oy"]:geo["oy"] + geo["high"], geo["ox"]:geo["ox"] + geo["wide"]])
    assert scale > 1 or halos > 5                                         # the halo's own pixels differ: it is needed


def test_the_lane_rule_runs_every_lane_that_holds_a_block_and_skips_others():
    skipped = 0
    for name, data, _ in _baseline():
        hd, sub_start, index, row_sub = _index(name, data)
        recorded = _record_lanes(data, sub_start, index, SB, row_sub)[5]
        for win in jpegwin.windows(hd.height, hd.width, 8 * hd.v[0], 8 * hd.h[0]):
            geo = _geometry(hd, win, 1)
            if geo is None:
                continue
            band = np.arange(int(row_sub[geo["a"]]), min(int(row_sub[geo["b"]]), len(index) - 1) + 1)
            run = set(window_lanes(hd, sub_start, index, band, (geo["c0"], geo["c1"])).tolist())
            assert run <= set(band.tolist()) and _held(recorded, geo) <= run, (name, win.tolist())
            skipped += len(band) - len(run)
    assert skipped > 0
    # a window one MCU wide in a file with at least 8 subsequences per MCU row: a strict subset of the band's lanes, and its columns
    # begin in the middle of a subsequence (the lane of its first block decodes MCUs in front of the window as well)
    name, data, _ = jpegwin.named(jpegwin.NOISE)
    hd, sub_start, index, row_sub = _index(name, data)
    assert np.diff(row_sub.astype(np.int64)).min() >= 8
    recorded = _record_lanes(data, sub_start, index, SB, row_sub)[5]
    lane_of, my, mx = recorded[:3]
    for column in (3, 11, hd.mcus_x - 1):
        for a in range(hd.mcus_y):
            geo = dict(a=a, b=a + 1, c0=column, c1=column + 1)
            band = np.arange(int(row_sub[a]), min(int(row_sub[a + 1]), len(index) - 1) + 1)
            run = set(window_lanes(hd, sub_start, index, band, (column, column + 1)).tolist())
            assert _held(recorded, geo) <= run and len(run) < len(band) / 4, (column, a)
            first = min(_held(recorded, geo))
            assert column == 0 or (mx[(lane_of == first) & (my == a)] < column).any()


# --------------------------------------------------------------------------------------------------------------------- the builder
@pytest.fixture(scope="module")
def built():
    frames, pairs = frames_and_pairs()
    pairs = np.concatenate([pairs, np.array([
        [1, -20, 10, 30, 12,           2, 250, 100, 30, 30,         1],     # leaves the frame on the left | on the right
        [2, 100, -10, 20, 30,          0, 40, 70, 30, 10,           1],     # at the top | at the bottom
    ], dtype=np.float64)])
    builder = TrainPairBuilder(device="cpu")
    params = builder.draw(pairs, [f.shape[:2] for f in frames], np.random.default_rng(5))
    means = np.stack([border_color_u8(np.mean(f, axis=(0, 1))) for f in frames])
    return builder, frames, pairs, params, means, builder.build_host(frames, pairs, params, borders=means)


def test_frame_windows_against_a_brute_force_union(built):
    builder, frames, pairs, _, means, clean = built
    shapes = [f.shape[:2] for f in frames]
    # one pair more, whose template box has neither width nor height (the numpy restatement cannot build it: the planner alone)
    pairs = np.concatenate([pairs, np.array([[3, 40, 30, 0, 0,    1, 20, 16, 18, 14,    1]], dtype=np.float64)])
    params = builder.draw(pairs, shapes, np.random.default_rng(5))
    assert builder.tables(pairs, params)["t_ctx"][-1, 2:].tolist() == [0, 0]
    got = builder.frame_windows(pairs, params, shapes)
    assert got.dtype == np.int64 and got.shape == (5, 4) and got[4].tolist() == [0, 0, 0, 0]
    tab = builder.tables(pairs, params)
    want = [None] * len(frames)
    for k in range(len(pairs)):
        for f, ctx in ((int(pairs[k, 0]), tab["t_ctx"][k]), (int(pairs[k, 5]), tab["s_ctx"][k])):
            cx, cy, cw, ch = (int(v) for v in ctx)
            ys = range(cy, cy + ch) if ch > 0 else (cy - 1, cy)           # a box without height clamps its taps to these two rows
            xs = range(cx, cx + cw) if cw > 0 else (cx - 1, cx)
            box = (min(ys), max(ys) + 1, min(xs), max(xs) + 1)
            want[f] = box if want[f] is None else (min(want[f][0], box[0]), max(want[f][1], box[1]), min(want[f][2], box[2]), max(want[f][3], box[3]))
    for f, (H, W) in enumerate(shapes):
        rect = jpegwin.clipped(want[f], H, W) if want[f] is not None else (0, 0, 0, 0)
        assert got[f].tolist() == list(rect), f
    assert np.array_equal(got[:, :2], builder.frame_rows(pairs, params, shapes))
    assert any(x1 - x0 < s[1] for (_, _, x0, x1), s in zip(got.tolist(), shapes))   # and not simply every column


def test_build_host_on_window_frames_equals_whole_frames(built):
    builder, frames, pairs, params, means, clean = built
    shapes = np.array([f.shape[:2] for f in frames], dtype=np.int32)
    wins = builder.frame_windows(pairs, params, shapes)
    rng = np.random.default_rng(23)
    compact, origin = [], []
    for f, (y0, y1, x0, x1) in zip(frames, wins.tolist()):
        if y0 >= y1:
            compact.append(np.zeros((0, 0, 3), dtype=np.uint8))
            origin.append((0, 0))
            continue
        oy, ox = max(y0 - 3, 0), max(x0 - 5, 0)                           # a margin of unspecified bytes, as a halo leaves one
        c = rng.integers(0, 256, (min(y1 + 2, f.shape[0]) - oy, min(x1 + 4, f.shape[1]) - ox, 3), dtype=np.uint8)
        c[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = f[y0:y1, x0:x1]
        compact.append(c)
        origin.append((oy, ox))
    held = WindowFrames(compact, np.array(origin, dtype=np.int32), shapes, wins)
    assert held.nbytes < sum(f.nbytes for f in frames)
    got = builder.build_host(held, pairs, params, borders=means)
    for x, y in zip(got, clean):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    with pytest.raises(ValueError):
        builder.build_host(held, pairs, params)
