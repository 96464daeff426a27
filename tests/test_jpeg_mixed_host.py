"""A scale per position in one `JpegStore` call, and `PairLoader(scale="auto")`'s rule, on the host ("A scale per
position"; section 16, "A scale per frame"): the three plans with a sequence of scales against the uniform plans position by position,
`shape`, the argument errors, `scale_pairs` with a per-frame array, `TrainPairBuilder.frame_scales` at its thresholds, `draw`'s
independence of the table, and the ABI of fear_jpeg_decode_mixed_u8."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpegdec
import jpegscaled
from feartracker_amd import UnsupportedJPEG, jpeg_scaled_shape
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_store import COLUMNS, KIND_PIXELS, JpegStore, plan_decode, plan_decode_rows, plan_decode_windows, scan_columns
from feartracker_amd.train_data import TrainPairBuilder, scale_pairs
from feartracker_amd.train_data.records import CONTEXT_SIZE, TEMPLATE_SIZE

ALL = (1, 2, 4, 8)
_mirror = None


def _columns():
    """The mirror of the fixture files (their true headers; a made-up index of four subsequences per MCU row, which the plans only
    gather) and one entry kept as pixels, the last."""
    global _mirror
    if _mirror is None:
        lib = abi.load_train_library()
        files = jpegscaled.files()
        col, tables, at = np.zeros(len(files) + 1, dtype=COLUMNS), [], 0
        for k, (name, data) in enumerate(files):
            info = abi.FearJpegInfo()
            assert lib.fear_jpeg_parse(data, len(data), ctypes.byref(info)) == 0, name
            scan_columns(col[k], info, 1, 4 * info.mcus_y, at)
            tables.append(np.arange(info.mcus_y + 1, dtype=np.uint32) * 4)
            at += info.mcus_y + 1
        col[-1]["H"], col[-1]["W"], col[-1]["kind"] = 31, 33, KIND_PIXELS
        _mirror = (col, np.concatenate(tables))
    return _mirror


def _call(seed):
    """Every entry at all four scales, shuffled, then a run in which neighbours always differ in scale, the same id four times, and
    the entry kept as pixels at scale 1."""
    col, _ = _columns()
    n = len(col) - 1
    rng = np.random.default_rng(seed)
    ids, scales = np.repeat(np.arange(n), 4), np.tile(ALL, n)
    order = rng.permutation(ids.size)
    ids, scales = ids[order], scales[order]
    ids = np.concatenate([ids, np.arange(n) % 7, [5, 5, 5, 5], [n]])
    scales = np.concatenate([scales, np.array(ALL)[np.arange(n) % 4], [8, 1, 4, 2], [1]])
    return ids.astype(np.int64), scales.astype(np.int64)


# what a plan holds per "scan" position of a group | per position of a group | as prefix sums over the "scan" positions
PER_SCAN = ("sub0", "sub_count", "mcu_row0", "mcu_rows", "band_y0", "band_height", "band_out", "cols", "win_width")
PER_POSITION = ("origin", "high", "wide", "window")
PREFIXES = ("sub_prefix", "block_prefix", "pixel_prefix")


def _by_position(plans, n):
    """{entry: one value per position of the call}, -1 where a position has none: the per-position entries as they are, the prefix
    tables and the offsets as their steps (what a position adds), so that plans whose groups differ can be compared."""
    out = {}

    def put(key, at, values):
        values = np.asarray(values).astype(np.int64)
        out.setdefault(key, np.full((n,) + values.shape[1:], -1, dtype=np.int64))[at] = values

    for p in plans:
        scan = p["lo"] + p["scan"]
        every = np.arange(p["lo"], p["hi"])
        put("scanned", scan, np.ones(scan.size))
        for key in PER_SCAN:
            if key in p:
                put(key, scan, p[key])
        for key in PER_POSITION:
            if key in p:
                put(key, every, p[key])
        for key in PREFIXES:
            put(key, scan, np.diff(p[key].astype(np.int64)))
        put("coef", scan, np.diff(np.append(p["coef_offset"].astype(np.int64), p["values"])))
        put("planes", scan, np.diff(np.append(p["plane_offset"].astype(np.int64), p["workspace_bytes"] - 16)))
        put("out", every, np.diff(np.append(p["out_offset"], p["out_bytes"])))
        assert (p["out_offset"] % 16 == 0).all() and (p["plane_offset"] % 16 == 0).all()
    return out


def _same_where(mixed, uniform, where):
    assert mixed.keys() == uniform.keys()
    for key in mixed:
        assert np.array_equal(mixed[key][where], uniform[key][where]), key


@pytest.mark.parametrize("limit", [1 << 40, 128 * 300, 0])
def test_mixed_plan_decode_is_the_uniform_plan_position_by_position(limit):
    col, _ = _columns()
    ids, scales = _call(1)
    mixed = plan_decode(col, ids, limit, scale=scales)
    assert sum(p["hi"] - p["lo"] for p in mixed) == ids.size
    got = _by_position(mixed, ids.size)
    for s in ALL:
        uniform = plan_decode(col, ids, limit, scale=s)
        assert [(p["lo"], p["hi"]) for p in uniform] == [(p["lo"], p["hi"]) for p in mixed]       # the cut does not see the scale
        for p, q in zip(mixed, uniform):
            assert np.array_equal(p["scales"], scales[p["lo"] + p["scan"]]) and "scales" not in q
            for key in ("scan", "sub_prefix", "block_prefix", "coef_offset", "values", "plane_offset", "workspace_bytes", "most"):
                assert np.array_equal(np.asarray(p[key]), np.asarray(q[key])), key            # the blocks are the file's at every scale
        _same_where(got, _by_position(uniform, ids.size), scales == s)
    if limit == 0:
        assert len(mixed) == ids.size
    # a sequence of equal values lays out what the int lays out
    for s in ALL:
        for p, q in zip(plan_decode(col, ids, limit, scale=np.full(ids.size, s)), plan_decode(col, ids, limit, scale=s)):
            for key in q:
                assert np.array_equal(np.asarray(p[key]), np.asarray(q[key])), key


def _rows_for(col, ids, scales, rng):
    """Per position a band of its own scaled frame: the whole frame, its first row, its last, an inner band, the empty band, one that
    reaches past both ends."""
    rows = np.zeros((ids.size, 2), dtype=np.int64)
    for k, (i, s) in enumerate(zip(ids.tolist(), scales.tolist())):
        H = jpeg_scaled_shape(int(col[i]["H"]), int(col[i]["W"]), s)[0]
        rows[k] = ((0, H), (0, 1), (H - 1, H), sorted(rng.integers(0, H + 1, 2).tolist()), (H // 2, H // 2), (-3, H + 9))[k % 6]
    return rows


@pytest.mark.parametrize("limit", [1 << 40, 128 * 300])
def test_mixed_plan_decode_rows_is_the_uniform_plan_position_by_position(limit):
    col, row_sub = _columns()
    ids, scales = _call(2)
    rows = _rows_for(col, ids, scales, np.random.default_rng(3))
    got = _by_position(plan_decode_rows(col, row_sub, ids, rows, limit, scale=scales), ids.size)
    for s in ALL:
        uniform = _by_position(plan_decode_rows(col, row_sub, ids, rows, limit, scale=s), ids.size)
        _same_where(got, uniform, scales == s)
    # scale-1 positions keep their halo next to scaled ones, which have none
    one = (scales == 1) & (got["scanned"] == 1) & (col["halo"][ids] == 1)
    mcu_h = np.maximum(col["mcu_h"][ids].astype(np.int64), 1)
    H = col["H"][ids].astype(np.int64)
    y0, y1 = rows[:, 0].clip(0, H), rows[:, 1].clip(0, H)
    halo = (got["mcu_rows"][one] > (-(-y1 // mcu_h) - y0 // mcu_h)[one]).sum()               # the band is more than the rows' cover
    assert halo > 3
    scaled = (scales > 1) & (got["scanned"] == 1)
    step = mcu_h[scaled] * (8 // scales[scaled]) // 8
    assert np.array_equal(got["band_y0"][scaled], rows[scaled, 0].clip(0) // step * step)


@pytest.mark.parametrize("limit", [1 << 40, 128 * 300])
def test_mixed_plan_decode_windows_is_the_uniform_plan_position_by_position(limit):
    col, row_sub = _columns()
    ids, scales = _call(4)
    rng = np.random.default_rng(5)
    rows = _rows_for(col, ids, scales, rng)
    win = np.zeros((ids.size, 4), dtype=np.int64)
    for k, (i, s) in enumerate(zip(ids.tolist(), scales.tolist())):
        W = jpeg_scaled_shape(int(col[i]["H"]), int(col[i]["W"]), s)[1]
        win[k] = (*rows[k], *((0, W), (W - 1, W), sorted(rng.integers(0, W + 1, 2).tolist()), (W // 2, W // 2))[k % 4])
    got = _by_position(plan_decode_windows(col, row_sub, ids, win, limit, scale=scales), ids.size)
    assert (got["high"] * got["wide"] == 0).sum() > 10 and (got["high"] * got["wide"] > 0).sum() > 100        # empty windows, and filled
    for s in ALL:
        _same_where(got, _by_position(plan_decode_windows(col, row_sub, ids, win, limit, scale=s), ids.size), scales == s)


def _bare_store():
    """A `JpegStore` that is its mirror alone: what `shape` and the checks in front of every launch read."""
    col, row_sub = _columns()
    s = object.__new__(JpegStore)
    s._columns, s._n, s._row_sub, s.workspace_limit = col, len(col), row_sub, 1 << 30
    return s


def test_shape_per_position():
    s = _bare_store()
    ids, scales = _call(6)
    got = s.shape(ids, scales)
    assert got.dtype == np.int32 and got.shape == (ids.size, 2)
    for sc in ALL:
        assert np.array_equal(got[scales == sc], s.shape(ids[scales == sc], sc))
    assert np.array_equal(s.shape(ids, np.full(ids.size, 4)), s.shape(ids, 4))
    assert np.array_equal(s.shape(ids, [1] * ids.size), s.shape(ids))
    assert s.shape([], []).shape == (0, 2)


def test_argument_errors_come_before_any_launch():
    """A bare store has no device: whatever does not raise in the checks would fail on a missing attribute, not on ValueError."""
    s = _bare_store()
    n = len(s._columns) - 1
    ids = np.array([0, 1, 2])
    for bad in ([1, 2], [1, 2, 4, 8], [1, 3, 2], [1, 2, 0], [1, 2, 16], [1, True, 2], np.array([True, False, True]), [1.0, 2.0, 4.0],
                [[1, 2, 4]], "124", (1, None, 2)):
        for call in (lambda: s.decode(ids, scale=bad), lambda: s.decode_rows(ids, np.zeros((3, 2), np.int64), scale=bad),
                     lambda: s.decode_windows(ids, np.zeros((3, 4), np.int64), scale=bad), lambda: s.shape(ids, bad),
                     lambda: plan_decode(s._columns, ids, 1 << 30, scale=bad),
                     lambda: plan_decode_rows(s._columns, s._row_sub, ids, np.zeros((3, 2), np.int64), 1 << 30, scale=bad),
                     lambda: plan_decode_windows(s._columns, s._row_sub, ids, np.zeros((3, 4), np.int64), 1 << 30, scale=bad)):
            with pytest.raises(ValueError, match="scale"):
                call()
    # an entry kept as pixels: fine at scale 1 (the plan takes it), UnsupportedJPEG naming the id at any other
    mixed = np.array([0, n, 1])
    assert len(plan_decode(s._columns, mixed, 1 << 30, scale=[2, 1, 4])) == 1
    assert np.array_equal(s.shape(mixed, [2, 1, 4])[1], [31, 33])
    for call in (lambda: s.decode(mixed, scale=[1, 2, 1]), lambda: s.decode_rows(mixed, np.zeros((3, 2), np.int64), scale=[1, 2, 1]),
                 lambda: s.decode_windows(mixed, np.zeros((3, 4), np.int64), scale=[1, 8, 1])):
        with pytest.raises(UnsupportedJPEG, match=f"id {n} "):
            call()
    with pytest.raises(IndexError):
        s.decode([n + 1], scale=[2])


# ---------------------------------------------------------------------------------------------------------------------------- the loader
def test_scale_pairs_with_a_scale_per_frame():
    pairs = np.array([[0, 100, 60, 41, 20, 1, 120, 80, 44, 22, 1], [2, 7, 5, 3, 1, 2, 0, 0, 9, 9, 0], [1, 8, 8, 8, 8, 0, 16, 16, 16, 16, 1]],
                     dtype=np.float64)
    keep = pairs.copy()
    for s in ALL:
        for const in (np.full(3, s), [s, s, s], np.full(3, s, dtype=np.int32)):
            got = scale_pairs(pairs, const)
            assert got.dtype == np.float64 and (got == scale_pairs(pairs, s)).all()              # bit for bit
    got = scale_pairs(pairs, np.array([2, 8, 1]))
    assert np.array_equal(pairs, keep)
    assert np.array_equal(got[:, [0, 5, 10]], pairs[:, [0, 5, 10]])
    assert np.array_equal(got[0, 1:5] * 2, pairs[0, 1:5]) and np.array_equal(got[0, 6:10] * 8, pairs[0, 6:10])   # template and search differ
    assert np.array_equal(got[1, 1:5], pairs[1, 1:5]) and np.array_equal(got[1, 6:10], pairs[1, 6:10])
    assert np.array_equal(got[2, 1:5] * 8, pairs[2, 1:5]) and np.array_equal(got[2, 6:10] * 2, pairs[2, 6:10])
    for bad in ([2, 8], [2, 3, 1], [True, True, True], [2.0, 2.0, 2.0]):
        with pytest.raises(ValueError):
            scale_pairs(pairs, bad)


def _builder():
    return TrainPairBuilder(dict(template_bbox_offset=0.5), device="cpu")                    # a context box of twice the box


def _params(builder, B, context=0.5):
    params = builder.draw(np.zeros((B, 11)), [], np.random.default_rng(0))
    params.context[:] = context                                                             # the search context: twice the box as well
    return params


def _pair(t_frame, t_side, s_frame, s_side):
    """A pair whose template context box is t_side x (t_side + 40) and whose search context box is (s_side + 64) x s_side."""
    return [t_frame, 10, 10, t_side / 2, (t_side + 40) / 2, s_frame, 20, 20, (s_side + 64) / 2, s_side / 2, 1]


def test_frame_scales_at_the_thresholds():
    builder = _builder()
    big_t, big_s = 8 * TEMPLATE_SIZE, 8 * CONTEXT_SIZE
    rows, want = [], []
    for s in (2, 4, 8):
        # a context side of exactly s * target admits s, one pixel less the next smaller scale; the other use of each pair admits 8
        rows += [_pair(len(want), s * TEMPLATE_SIZE, len(want) + 1, big_s), _pair(len(want) + 2, s * TEMPLATE_SIZE - 1, len(want) + 3, big_s)]
        want += [s, 8, s // 2, 8]
        rows += [_pair(len(want), big_t, len(want) + 1, s * CONTEXT_SIZE), _pair(len(want) + 2, big_t, len(want) + 3, s * CONTEXT_SIZE - 1)]
        want += [8, s, 8, s // 2]
    pairs = np.array(rows, dtype=np.float64)
    F = len(want) + 2                                                                        # two frames no pair uses
    params = _params(builder, len(pairs))
    tab = builder.tables(pairs, params)
    assert tab["t_ctx"][0, 2:].tolist() == [2 * TEMPLATE_SIZE, 2 * TEMPLATE_SIZE + 40]      # the boxes are what the rule is stated on
    assert tab["t_ctx"][1, 2:].tolist() == [2 * TEMPLATE_SIZE - 1, 2 * TEMPLATE_SIZE + 39]
    assert tab["s_ctx"][2, 2:].tolist() == [2 * CONTEXT_SIZE + 64, 2 * CONTEXT_SIZE]
    got = builder.frame_scales(pairs, params, [(9000, 9000)] * F)
    assert got.dtype == np.int64 and got.tolist() == want + [1, 1]
    for cap in ALL:
        assert builder.frame_scales(pairs, params, [(9000, 9000)] * F, max_scale=cap).tolist() == [min(w, cap) for w in want] + [1, 1]
    for bad in (0, 3, 16, True):
        with pytest.raises(ValueError):
            builder.frame_scales(pairs, params, [(9000, 9000)] * F, max_scale=bad)


def test_a_shared_frame_takes_its_smallest_scale():
    builder = _builder()
    pairs = np.array([_pair(0, 8 * TEMPLATE_SIZE, 1, 8 * CONTEXT_SIZE),                      # frame 0: a large template use
                      _pair(2, 8 * TEMPLATE_SIZE, 0, 2 * CONTEXT_SIZE),                      # ... and a search use that admits 2
                      _pair(1, 4 * TEMPLATE_SIZE, 1, 8 * CONTEXT_SIZE),                      # frame 1: 8, 4 and 8
                      _pair(3, TEMPLATE_SIZE - 1, 3, 8 * CONTEXT_SIZE)], dtype=np.float64)   # frame 3: a template that is enlarged already
    got = builder.frame_scales(pairs, _params(builder, 4), [(5000, 5000)] * 4)
    assert got.tolist() == [2, 4, 8, 1]


def test_no_reduction_becomes_an_enlargement():
    """For every pair, where the full-size context side was at least the target the scaled one still is — on random tables with odd
    boxes and the drawn contexts, through `scale_pairs` and `tables` as the loader runs them."""
    builder = TrainPairBuilder(device="cpu")
    rng = np.random.default_rng(11)
    B, F = 400, 37
    pairs = np.zeros((B, 11))
    pairs[:, 0], pairs[:, 5] = rng.integers(0, F, B), rng.integers(0, F, B)
    size = np.exp(rng.uniform(np.log(8), np.log(2500), F))                                  # the objects of a frame are of one size, about
    for at in (0, 5):
        mine = size[pairs[:, at].astype(np.int64)]
        pairs[:, at + 1:at + 3] = rng.uniform(0, 500, (B, 2))
        pairs[:, at + 3], pairs[:, at + 4] = mine * rng.uniform(0.8, 1.25, B), mine * rng.uniform(0.5, 2, B)
    pairs[:, 10] = 1
    params = builder.draw(pairs, [(4000, 4000)] * F, np.random.default_rng(12))
    scales = builder.frame_scales(pairs, params, [(4000, 4000)] * F)
    assert set(scales.tolist()) == {1, 2, 4, 8}
    full, small = builder.tables(pairs, params), builder.tables(scale_pairs(pairs, scales), params)
    seen = 0
    for key, col, target in (("t_ctx", 0, TEMPLATE_SIZE), ("s_ctx", 5, CONTEXT_SIZE)):
        was = full[key][:, 2:].min(axis=1) >= target
        now = small[key][:, 2:].min(axis=1) >= target
        assert (now[was]).all(), key
        seen += int(was.sum())
        # and the scale is the largest the frame's uses admit: some use of every scaled frame would be enlarged at twice the scale
        s = scales[pairs[:, col].astype(np.int64)]
        assert (full[key][:, 2:].min(axis=1)[s > 1] >= (s * target)[s > 1]).all(), key
    assert seen > 100


def test_draw_reads_of_the_pairs_their_number_alone():
    config = dict(photometric=True, noise_members=("multiplicative", "gauss", "jpeg"), iso_noise=True, weather_members=("rain", "shadow"),
                  glass_blur=True)
    builder = TrainPairBuilder(config, device="cpu", seed=3)
    rng = np.random.default_rng(1)
    one = np.concatenate([rng.integers(0, 3, (6, 1)), rng.uniform(1, 90, (6, 4)), rng.integers(0, 3, (6, 1)), rng.uniform(1, 90, (6, 4)),
                          np.ones((6, 1))], axis=1)
    two = scale_pairs(one[::-1], np.array([2, 8, 4]))
    a = builder.draw(one, [(100, 100)] * 3, np.random.default_rng(9))
    b = builder.draw(two, [(50, 50), (13, 13), (25, 25)], np.random.default_rng(9))
    assert a.photo is not None and a.jpeg_quality is not None and a.iso_key is not None and a.weather is not None   # every group drew

    def same(x, y):
        if x is None or y is None:
            return x is None and y is None
        if hasattr(x, "__dataclass_fields__"):
            return all(same(getattr(x, f), getattr(y, f)) for f in x.__dataclass_fields__)
        return np.array_equal(np.asarray(x), np.asarray(y))

    fields = [f for f in a.__dataclass_fields__ if f != "frame_shapes"]
    assert len(fields) > 10 and all(same(getattr(a, f), getattr(b, f)) for f in fields)
    assert a.frame_shapes == ((100, 100),) * 3 and b.frame_shapes == ((50, 50), (13, 13), (25, 25))


# ------------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_of_the_mixed_entry_point():
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert abi.TRAIN_SYMBOLS["fear_jpeg_decode_mixed_u8"] == ([P, i, P, P, sz, P], i)
    assert abi.TRAIN_SYMBOLS["fear_jpeg_decode_mixed_u8"] == abi.TRAIN_SYMBOLS["fear_jpeg_decode_u8"]
    lib = abi.load_train_library()
    assert lib.fear_jpeg_decode_mixed_u8.restype is i
    assert ctypes.sizeof(abi.FearJpegImage) == 448 and abi.FearJpegImage.reserved.size == 12
    header = open(os.path.join(jpegdec.HERE, "..", "include", "fear_train.h")).read()
    stated = re.search(r"scale s_i in reserved\[0\] \(byte (\d+) of the record\)", header)
    assert stated and int(stated.group(1)) == abi.FearJpegImage.reserved.offset == 52
    # the record's fields in front of the word, as the header declares them: four 8-byte fields and five int32
    body = re.search(r"typedef struct FearJpegImage \{(.*?)\} FearJpegImage;", header, re.S).group(1)
    names = re.findall(r"(?:\*|\s)(\w+)(?:\[\d+\])*(?:, (\w+))?;", body)
    flat = [n for pair in names for n in pair if n]
    assert flat == ["coef", "block_start", "out", "plane_offset", "width", "height", "components", "h", "v", "reserved", "qt"]
    assert re.search(r"int fear_jpeg_decode_mixed_u8\(const FearJpegImage\* images, int n, const uint32_t\* group_start,\s+"
                     r"void\* workspace, size_t workspace_bytes,\s+void\* stream\);", header)
    # n == 0 is OK without a launch and without a device; the null and shape checks come in the order the ABI states
    assert lib.fear_jpeg_decode_mixed_u8(None, 0, None, None, 0, None) == jpegdec.OK
    assert lib.fear_jpeg_decode_mixed_u8(None, -1, None, None, 0, None) == jpegdec.ERR_SHAPE
    assert lib.fear_jpeg_decode_mixed_u8(None, 1, None, None, 0, None) == jpegdec.ERR_NULL
    rec = (abi.FearJpegImage * 1)()
    rec[0].coef = rec[0].block_start = rec[0].out = 16                                       # (never dereferenced by a refused call)
    rec[0].width, rec[0].height, rec[0].components, rec[0].h, rec[0].v = 17, 23, 3, 2, 2
    table = (ctypes.c_uint32 * 4)()
    for bad in (3, -1, 5, 16, 256 + 2):
        rec[0].reserved[0] = bad
        assert lib.fear_jpeg_decode_mixed_u8(rec, 1, table, None, 0, None) == jpegdec.ERR_SHAPE, bad
    for fine in (0, 1, 2, 4, 8):
        rec[0].reserved[0] = fine
        assert lib.fear_jpeg_decode_mixed_u8(rec, 1, table, None, 0, None) == jpegdec.ERR_WORKSPACE, fine   # past the shape check
