"""JPEG files resident on the device ("The resident store").

A training run decodes the same files every epoch.  `JpegStore.add` prepares them once — `fear_jpeg_parse` and `fear_jpeg_scan_prepare` on
host threads, the unstuffed bytes uploaded into device slabs — and builds once the index that a baseline scan lacks
(`fear_jpeg_index_build`: the true entry of every subsequence, 16 bytes each, kept next to the bytes).  `JpegStore.decode` then runs
`fear_jpeg_huffman_indexed`, a single write pass with one lane per subsequence, and the unchanged `fear_jpeg_decode_u8`; the host's share
of a call is a few numpy gathers over the ids (`plan_decode`) and one small pinned upload.  jpeg_huffman.jpeg_scan_index_host and
jpeg_entropy_indexed_host state the two device calls in Python.

A training pair reads only the rows of its context boxes.  `add` therefore also keeps, per file, the row table `row_sub` (the
subsequence in which each MCU row begins, `jpeg_huffman.scan_row_sub`, from the index it has just built) and the frame's border colour
(`fear_frame_border_u8` of the full decode, in a device table that `borders(ids)` gathers), and `JpegStore.decode_rows` decodes a band of
rows per frame: `plan_decode_rows` on the host, `fear_jpeg_huffman_indexed_rows` with lanes for the band's subsequences alone, and the
unchanged `fear_jpeg_decode_u8` on the band as an image of its own ("Bands of rows").

A tracker knows the rows of its next search window only on the device.  `decode_rows` therefore also takes `rows` as a device tensor that
only kernels read: `plan_decode`'s full-image plan, `fear_jpeg_huffman_indexed_rows_dev` and `fear_jpeg_decode_u8_rows_dev`, whose
workgroups outside the band return early — for which `add` keeps each file's row table on the device as well ("Rows
from the device").  `StoreFrames(store, ids)` names a sequence of frames kept in a store, for `SequenceValidator`.

`decode`, `decode_rows` (rows on the host), `shape` and the plans take `scale` 2, 4 or 8: the frames at 1/2, 1/4 or 1/8 size, decoded
in the DCT domain as libjpeg's scale_denom does, with `fear_jpeg_decode_scaled_u8` in place of `fear_jpeg_decode_u8` behind the same
Huffman stage ("Reduced-size decoding").  `scale` may also be a sequence, one scale of {1, 2, 4, 8} per
position of the call: item i is then what the uniform call at its scale returns, a group whose scales differ runs
`fear_jpeg_decode_mixed_u8` — two pixel launches whatever the mix, each record's scale in its `reserved[0]` — and `decode_windows`
takes it too ("A scale per position").

A batch of training pairs reads a rectangle of a frame, not its whole rows.  `JpegStore.decode_windows` decodes per frame the MCUs that
cover one rectangle — `plan_decode_windows` on the host, `fear_jpeg_huffman_indexed_windows`, whose lanes of the band that cannot touch
the rectangle's MCU columns return early and which stores the blocks window-dense, and the unchanged pixel kernels on the window as an
image of its own — and returns COMPACT frames with their origins, a `WindowFrames` ("Windows").

The three plans are one plan over shared parts: the units that cover a request (`_cover`, for MCU rows and MCU columns alike), a band's
lanes (`_band_lanes`), what a run of units spans of the image (`_extent`), and the groups of a call (`_groups`: the cut, the layout and
what each group carries).  `add` is a sequence of stages over one `_Entry` per file, of which the last alone assigns to the store.

`JpegStore(residence="host")` keeps the scan bytes in pinned host memory, which the Huffman kernels read in place through a staged
fetch (the `fear_jpeg_huffman_indexed*_host` calls), and the index and tables on the device: every call and every frame is the
`"device"` store's ("Bytes on the host")."""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import jpeg_frames
from .jpeg_frames import (ERR_UNSUPPORTED, Item, JpegDecoder, MalformedJPEG, UnsupportedJPEG, _check_scales, _fill_header, _judge,
                          _launch_pixels, _raise_as_python, _read_items)
from .jpeg_huffman import SUBSEQ_DTYPE, _check_subsequence_bytes, scan_row_sub
from .train_data.records import WindowFrames  # noqa: F401  (what decode_windows returns; the builder takes it)

KIND_SCAN, KIND_PIXELS = 0, 1
KIND_NAMES = np.array(["scan", "pixels"])
LANES = 256                                   # csrc/fear_jpeg_store.h: subsequences per workgroup of jpeg_huffman_indexed_kernel
# one row per entry; the second line is what a band needs: the MCU grid, an MCU's height in pixels, its blocks, 1 where the fancy
# upsampling reads a chroma row above and below (v == 2), and where the entry's mcus_y + 1 values of the ragged row_sub array begin
COLUMNS = np.dtype([("n_seg", "<u4"), ("n_sub", "<u4"), ("total_blocks", "<u4"), ("H", "<i4"), ("W", "<i4"), ("kind", "u1"),
                    ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("mcu_h", "<i4"), ("nslots", "<i4"), ("halo", "u1"), ("row_at", "<i8")])


class StoreFull(MemoryError):
    """An `add` would take the store above its `capacity_bytes` or, under residence="host", its `host_capacity_bytes` — the message
    names which; nothing of the call was stored."""


def _up(x, to):
    return -(-x // to) * to


def _exclusive(a):
    out = np.zeros(a.size + 1, dtype=np.int64)
    np.cumsum(a, out=out[1:])
    return out


def plan_decode(columns: np.ndarray, ids, workspace_limit: int, max_group: int = 65535, scale=1) -> List[dict]:
    """The host's share of `JpegStore.decode` but the records: a pure function of the mirror's integer columns (COLUMNS, one row per
    entry) and the ids, any order, repeats allowed.  The call is cut into groups of consecutive positions lo..hi as JpegDecoder cuts it:
    a group takes positions while the dense coefficients of its "scan" entries (128 bytes per block) stay within `workspace_limit`, at
    least one and at most `max_group`.  Per group, over its "scan" positions `scan` (relative to lo):
        sub_prefix    uint32 [nd + 1]  prefix sums of ceil(n_sub / 256): fear_jpeg_huffman_indexed's workgroups
        block_prefix, pixel_prefix     fear_jpeg_decode_u8's two prefix tables
        coef_offset   values from the group's coefficient buffer to each image's 64 total_blocks; `values` their sum
        plane_offset  bytes from the workspace to each image's planes, multiples of 16; `workspace_bytes` what the pixel stage needs
        most          the largest total_blocks
    and over all its positions `out_offset`, multiples of 16, and `out_bytes`.  No loop over the files: gathers and prefix sums.
    At `scale` 2, 4 or 8 the frames are the scaled ones (`jpeg_scaled_shape`): `pixel_prefix` counts scaled pixels, as
    fear_jpeg_decode_scaled_u8 reads it, and `out_offset` and `out_bytes` lay out scaled frames; the blocks, the coefficients and the
    workspace are what they are at scale 1.
    `scale` may also be a sequence of len(ids) scales from {1, 2, 4, 8}, one per position (the same id may come at several): every
    per-position entry is then the uniform plan's at that position's scale, the groups are cut as ever, and a group carries `scales`,
    its "scan" positions' scales, for the records' reserved[0] and the choice of the launch (`_launch_pixels`)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    scale = _check_scales(scale, ids.size)
    rows = columns[ids]
    is_scan = rows["kind"] == KIND_SCAN
    blocks = rows["total_blocks"].astype(np.int64)
    high, wide = _scaled_sides(rows["H"], rows["W"], scale)
    pixels = high * wide
    return _groups(is_scan, np.where(is_scan, blocks, 0), rows["n_sub"].astype(np.int64), pixels, pixels, workspace_limit, max_group, scale)


def _groups(some: np.ndarray, blocks: np.ndarray, lanes: np.ndarray, pixels: np.ndarray, frame_pixels: np.ndarray, workspace_limit: int,
            max_group: int, scale, picked: dict = {}, sliced: dict = {}) -> List[dict]:   # (the defaults are only read)
    """The groups of all three plans, from per-position arrays.  Position k decodes an image of `blocks[k]` blocks (0 where it decodes
    none) and `pixels[k]` pixels with `lanes[k]` lanes, where `some[k]`, into a frame of `frame_pixels[k]` pixels.  `_cut` cuts the
    call by the dense coefficients, 128 bytes per block; a group carries lo, hi, `scan` (its positions with `some`, relative to lo),
    `sub_prefix`, `_layout`'s entries, `scales` with a scale per position, every array of `picked` (by name) over its "scan" positions
    and every array of `sliced` over lo:hi."""
    groups = []
    for lo, hi in _cut(128 * blocks, workspace_limit, max_group):
        scan = np.flatnonzero(some[lo:hi])
        pick = lo + scan
        group = dict(lo=lo, hi=hi, scan=scan, sub_prefix=_exclusive(-(-lanes[pick] // LANES)).astype(np.uint32),
                     **_layout(blocks[pick], pixels[pick], frame_pixels[lo:hi]))
        if not isinstance(scale, int):
            group["scales"] = scale[pick]
        for name, v in picked.items():
            group[name] = v[pick]
        for name, v in sliced.items():
            group[name] = v[lo:hi]
        groups.append(group)
    return groups


def _cover(lo: np.ndarray, hi: np.ndarray, size: np.ndarray, count: np.ndarray, halo: np.ndarray, some: np.ndarray):
    """The units first .. last) of `size` that cover [lo, hi), `halo` (0 or 1) more on each side, clipped to the `count` there are;
    0, 0 where not `some`.  One rule for MCU rows under pixel rows and MCU columns under pixel columns; `jpeg_huffman.rows_band` is its
    scalar statement."""
    return np.where(some, np.maximum(lo // size - halo, 0), 0), np.where(some, np.minimum(-(-hi // size) + halo, count), 0)


def _extent(begin: np.ndarray, end: np.ndarray, unit: np.ndarray, limit: np.ndarray) -> np.ndarray:
    """What the units begin .. end) of `unit` pixels span of a side of `limit` pixels: min(end unit, limit) - begin unit, the run cut
    at the image's true edge.  With the scaled or the full-size unit and side, of a band's rows or a window's columns."""
    return np.minimum(end * unit, limit) - begin * unit


def _band_lanes(row_sub: np.ndarray, row_at: np.ndarray, a: np.ndarray, b: np.ndarray, n_sub: np.ndarray, some: np.ndarray):
    """The lanes of the bands a .. b): `first` = row_sub[a] and `count` up to min(row_sub[b], n_sub - 1), of the entries whose row
    tables begin at `row_at` in the ragged `row_sub`; 0, 0 where not `some`, and everywhere while no entry has a row table."""
    if not row_sub.size:
        return np.zeros(a.size, np.int64), np.zeros(a.size, np.int64)
    at = np.where(some, row_at, 0)
    first = np.where(some, row_sub[at + a].astype(np.int64), 0)
    last = np.where(some, np.minimum(row_sub[at + b].astype(np.int64), n_sub - 1), -1)
    return first, np.maximum(last - first + 1, 0)


def _mcu_width(nslots: np.ndarray, mcu_h: np.ndarray) -> np.ndarray:
    """An MCU's width in pixels from what the mirror holds: a colour MCU has h v + 2 blocks and is `mcu_h` = 8 v rows high, a gray one
    is one block."""
    return np.where(nslots > 1, 8 * np.maximum((nslots - 2) // (mcu_h // 8).clip(1), 1), 8)


def _scaled_sides(H, W, scale):
    """`jpeg_frames.jpeg_scaled_shape` over arrays of heights and widths: int64 ceil(H m / 8) and ceil(W m / 8), m = 8 // scale; `scale`
    an int or one per height."""
    m = 8 // _check_scales(scale, np.size(H))
    return -(-np.asarray(H, dtype=np.int64) * m // 8), -(-np.asarray(W, dtype=np.int64) * m // 8)


def _cut(need_bytes: np.ndarray, workspace_limit: int, max_group: int):
    """The groups lo..hi of a call whose position k needs `need_bytes[k]` of dense coefficients: a group takes positions while their sum
    stays within `workspace_limit`, at least one and at most `max_group`.  One turn per group, none per file."""
    need, lo, n = _exclusive(need_bytes), 0, need_bytes.size
    while lo < n:
        hi = int(np.searchsorted(need, need[lo] + max(int(workspace_limit), 0), side="right")) - 1
        hi = min(max(hi, lo + 1), n, lo + max_group)
        yield lo, hi
        lo = hi


def _layout(blocks: np.ndarray, pixels: np.ndarray, frame_pixels: np.ndarray) -> dict:
    """What both plans lay out for the images the pixel stage decodes, of `blocks` blocks and `pixels` pixels each — the two prefix
    tables, the dense coefficients and the planes — and for all the group's frames, of `frame_pixels` pixels, the output."""
    dense = _exclusive(64 * blocks)
    out = _exclusive(_up(3 * frame_pixels, 16))
    return dict(block_prefix=_exclusive(-(-blocks // 32)).astype(np.uint32), pixel_prefix=_exclusive(-(-pixels // 256)).astype(np.uint32),
                coef_offset=dense[:-1].astype(np.uint64), values=int(dense[-1]),
                plane_offset=dense[:-1].astype(np.uint64), workspace_bytes=16 + int(dense[-1]),
                most=int(blocks.max()) if blocks.size else 0,
                out_offset=out[:-1], out_bytes=int(out[-1]))


def scan_columns(col, info, n_seg: int, n_sub: int, row_at: int) -> None:
    """Fill one row of the mirror (COLUMNS) for a "scan" entry from its FearJpegInfo."""
    col["n_seg"], col["n_sub"], col["total_blocks"], col["H"], col["W"], col["kind"] = n_seg, n_sub, info.total_blocks, info.height, info.width, KIND_SCAN
    col["mcus_x"], col["mcus_y"], col["mcu_h"], col["halo"] = info.mcus_x, info.mcus_y, 8 * info.v[0], info.v[0] == 2
    col["nslots"], col["row_at"] = (info.h[0] * info.v[0] + 2 if info.components == 3 else 1), row_at


def plan_decode_rows(columns: np.ndarray, row_sub: np.ndarray, ids, rows, workspace_limit: int, max_group: int = 65535,
                     scale=1) -> List[dict]:
    """The host's share of `JpegStore.decode_rows`, as `plan_decode` a pure function without a loop over the files: of the mirror's
    columns, the ragged row table (`columns["row_at"]` is where an entry's mcus_y + 1 values begin in `row_sub`), the ids and `rows`,
    (n, 2) pixel rows [y0, y1) per position, clipped to [0, H].  The band of a "scan" position is the MCU rows a .. b),
    a = y0 // mcu_h and b = ceil(y1 / mcu_h), one more on each side, clipped to the image, where `halo` is set (the fancy upsampling of
    v == 2 reads one chroma row above and below); y0 >= y1 is the empty band.  Groups are cut as `plan_decode` cuts them, by the BAND's
    dense coefficients (128 bytes per block of the band).  Per group, over its "scan" positions with a band, `scan` (relative to lo):
        sub0, sub_count       the lanes: subsequences row_sub[a] .. min(row_sub[b], n_sub - 1)
        sub_prefix            uint32 [nd + 1] prefix sums of ceil(sub_count / 256): fear_jpeg_huffman_indexed_rows' workgroups
        mcu_row0, mcu_rows    the band; `band_y0` = a mcu_h its first pixel row and `band_height` its rows: mcu_rows mcu_h, or what is left
                              of the image when the band reaches its last MCU row, so that libjpeg's edge rules apply at the true edges
        block_prefix, pixel_prefix, coef_offset, values, plane_offset, workspace_bytes, most
                              plan_decode's, of the band as an image of its own
        band_out              bytes from the position's frame to the band's first row, 3 W band_y0
    and over all its positions `out_offset` and `out_bytes`: whole frames, as plan_decode's.
    At `scale` 2, 4 or 8 (m = 8 // scale) `rows` are rows of the SCALED frame, clipped to its height ceil(H m / 8); a scaled MCU row is
    mcu_h m / 8 = v m of them, and no supported mode upsamples vertically at a scale, so there is no halo.  `band_height` stays the
    band's FULL-size height, what the record of fear_jpeg_decode_scaled_u8 holds; `band_y0`, `band_out`, `pixel_prefix`, `out_offset` and
    `out_bytes` are the scaled frame's.
    With a scale per position (`plan_decode` states the form) `rows[i]` is in rows of position i's own scaled frame, a position at
    scale 1 keeps its halo and a scaled one has none: every per-position entry is the uniform plan's at that position's scale."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    scale = _check_scales(scale, ids.size)
    m = 8 // scale
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    col = columns[ids]
    is_scan = col["kind"] == KIND_SCAN
    full_h, full_mcu_h = col["H"].astype(np.int64), np.maximum(col["mcu_h"].astype(np.int64), 1)
    (H, W), mcu_h = _scaled_sides(full_h, col["W"], scale), np.maximum(full_mcu_h * m // 8, 1)
    mcus_y = col["mcus_y"].astype(np.int64)
    y0, y1 = np.clip(rows[:, 0], 0, H), np.clip(rows[:, 1], 0, H)
    some = is_scan & (y0 < y1)
    a, b = _cover(y0, y1, mcu_h, mcus_y, col["halo"].astype(np.int64) * (m == 8), some)
    blocks = (b - a) * col["mcus_x"].astype(np.int64) * col["nslots"].astype(np.int64)
    first, count = _band_lanes(row_sub, col["row_at"], a, b, col["n_sub"].astype(np.int64), some)
    band_y0 = a * mcu_h
    picked = dict(sub0=first.astype(np.uint32), sub_count=count.astype(np.uint32), mcu_row0=a.astype(np.uint32),
                  mcu_rows=(b - a).astype(np.uint32), band_y0=band_y0, band_height=_extent(a, b, full_mcu_h, full_h).astype(np.int32),
                  band_out=3 * W * band_y0)
    return _groups(some, blocks, count, _extent(a, b, mcu_h, H) * W, H * W, workspace_limit, max_group, scale, picked)


def plan_decode_windows(columns: np.ndarray, row_sub: np.ndarray, ids, windows, workspace_limit: int, max_group: int = 65535,
                        scale=1) -> List[dict]:
    """The host's share of `JpegStore.decode_windows`, as its two siblings a pure function without a loop over the files.  `windows`
    is (n, 4) pixel rectangles [y0, y1) x [x0, x1) per position, as (y0, y1, x0, x1), clipped to the frame; one without rows or columns
    is the empty window.  The rows follow `plan_decode_rows`: the band of MCU rows a .. b) that covers [y0, y1), one more on each
    side where `halo` is set, at scale 1 alone.  The columns follow the same tap rule: the MCU columns c0 .. c1), c0 = x0 // mcu_w and
    c1 = ceil(x1 / mcu_w), one more on each side, clipped to the image, where the file subsamples horizontally (mcu_w == 16: the fancy
    upsampling reads one chroma column to the left and to the right) — at every scale, where it is conservative.  Groups are cut by the
    WINDOW's dense coefficients (128 bytes per block of its (b - a) (c1 - c0) MCUs).  Per group, over its "scan" positions with a
    window, `scan` (relative to lo):
        sub0, sub_count, sub_prefix, mcu_row0, mcu_rows     plan_decode_rows', of the band: the lanes fear_jpeg_huffman_indexed_windows gets
        cols                  uint32 c0 | (c1 - c0) << 16: the record's `reserved` word
        band_height, win_width   the FULL-size shape of the window as an image of its own: what is left of the image where the window
                              reaches its last MCU row or column, so that libjpeg's edge rules apply at the true edges
        block_prefix, pixel_prefix, coef_offset, values, plane_offset, workspace_bytes, most
                              plan_decode's, of the window as an image of its own
        band_out              zeros: a window's pixels begin where its tensor begins
    and over all its positions
        origin                int32 (hi - lo, 2): the frame coordinates (y, x) of each tensor's first pixel — (a mcu_h, c0 mcu_w) for a
                              "scan" position, (y0, x0) for one kept as pixels, (0, 0) for the empty window
        high, wide            each tensor's shape: the window's MCUs cut to the frame | the rectangle itself | 0, 0
        window                int64 (hi - lo, 4): the clipped request
        out_offset, out_bytes the compact tensors, each at a multiple of 16 bytes.
    At `scale` 2, 4 or 8 (m = 8 // scale) `windows` are rectangles of the SCALED frame; a scaled MCU is (mcu_h m / 8) x (mcu_w m / 8)
    pixels; `band_height` and `win_width` stay full-size, what the record of fear_jpeg_decode_scaled_u8 holds, and every other
    quantity is the scaled frame's.
    With a scale per position (`plan_decode` states the form) `windows[i]` is in pixels of position i's own scaled frame, and every
    per-position entry is the uniform plan's at that position's scale."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    scale = _check_scales(scale, ids.size)
    m = 8 // scale
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
    col = columns[ids]
    is_scan = col["kind"] == KIND_SCAN
    full_h, full_w = col["H"].astype(np.int64), col["W"].astype(np.int64)
    full_mcu_h = np.maximum(col["mcu_h"].astype(np.int64), 1)
    nslots = col["nslots"].astype(np.int64)
    full_mcu_w = _mcu_width(nslots, full_mcu_h)
    H, W = _scaled_sides(full_h, full_w, scale)
    mcu_h, mcu_w = np.maximum(full_mcu_h * m // 8, 1), np.maximum(full_mcu_w * m // 8, 1)
    mcus_y, mcus_x = col["mcus_y"].astype(np.int64), col["mcus_x"].astype(np.int64)
    y0, y1 = np.clip(win[:, 0], 0, H), np.clip(win[:, 1], 0, H)
    x0, x1 = np.clip(win[:, 2], 0, W), np.clip(win[:, 3], 0, W)
    filled = (y0 < y1) & (x0 < x1)
    some = is_scan & filled
    a, b = _cover(y0, y1, mcu_h, mcus_y, col["halo"].astype(np.int64) * (m == 8), some)
    c0, c1 = _cover(x0, x1, mcu_w, mcus_x, (full_mcu_w == 16).astype(np.int64), some)
    blocks = (b - a) * (c1 - c0) * nslots
    first, count = _band_lanes(row_sub, col["row_at"], a, b, col["n_sub"].astype(np.int64), some)
    kept = ~is_scan & filled                                             # an entry kept as pixels hands out the rectangle itself
    origin = np.stack([np.where(kept, y0, a * mcu_h), np.where(kept, x0, c0 * mcu_w)], axis=1).astype(np.int32)
    high, wide = np.where(kept, y1 - y0, _extent(a, b, mcu_h, H)), np.where(kept, x1 - x0, _extent(c0, c1, mcu_w, W))
    window = np.where(filled[:, None], np.stack([y0, y1, x0, x1], axis=1), 0)
    picked = dict(sub0=first.astype(np.uint32), sub_count=count.astype(np.uint32), mcu_row0=a.astype(np.uint32),
                  mcu_rows=(b - a).astype(np.uint32), cols=(c0 | (c1 - c0) << 16).astype(np.uint32),
                  band_height=_extent(a, b, full_mcu_h, full_h).astype(np.int32),
                  win_width=_extent(c0, c1, full_mcu_w, full_w).astype(np.int32), band_out=np.zeros(ids.size, dtype=np.int64))
    pixels = high * wide
    return _groups(some, blocks, count, pixels, pixels, workspace_limit, max_group, scale, picked,
                   dict(origin=origin, high=high, wide=wide, window=window))


def _place_images(images: np.ndarray, coef, coef_offset: np.ndarray, block_start, out, out_offset: np.ndarray, plane_offset: np.ndarray) -> None:
    """The addresses of a group's FearJpegImage records: each image's dense coefficients in `coef` (an int16 tensor, `coef_offset` in
    values), the dense `block_start` table they share, where its pixels go in `out` and its planes in the workspace."""
    images["coef"] = np.uint64(coef.data_ptr()) + np.uint64(2) * coef_offset
    images["block_start"] = block_start.data_ptr()
    images["out"] = np.uint64(out.data_ptr()) + out_offset.astype(np.uint64)
    images["plane_offset"] = plane_offset


def _frame_views(out, out_offset: np.ndarray, high: np.ndarray, wide: np.ndarray) -> List:
    """The frames in a group's output: frame k is `high[k]` x `wide[k]` x 3 bytes from `out_offset[k]`."""
    return [out[at:at + 3 * h * w].view(h, w, 3) for at, h, w in zip(out_offset.tolist(), high.tolist(), wide.tolist())]


@dataclasses.dataclass
class _Entry:
    """One "scan" file of an `add` on its way into the store: what `scan_prepare` made of it (info, data, seg, scan), its `sub_start`,
    its resident layout (where seg_start, sub_start, the index and the FearJpegScan record begin behind the bytes, and the `end`),
    its place (`at` in `slab`, the address `base`), its row table and the address of the table's copy on the device.  Under
    residence="host" the bytes lie apart: `host_end` of them at `host_at` in the pinned `host_slab`, which the device reads at
    `host_base`; the resident layout then begins with seg_start (`at_seg` is 0), and `build_bytes` is where the transient device copy
    of the bytes lies that `fear_jpeg_index_build` reads."""
    info: object
    data: np.ndarray
    seg: np.ndarray
    scan: object
    sub: Optional[np.ndarray] = None
    at_seg: int = 0
    at_sub: int = 0
    at_index: int = 0
    at_record: int = 0
    end: int = 0
    base: int = 0
    slab: object = None
    at: int = 0
    row_table: Optional[np.ndarray] = None
    row_dev_at: int = 0
    host_slab: object = None
    host_at: int = 0
    host_end: int = 0
    host_base: int = 0
    build_bytes: int = 0


class JpegStore:
    """Baseline JPEG files kept on the device, decoded by id: uint8 (H, W, 3) RGB device tensors, byte for byte what `JpegDecoder` and
    libjpeg decode.

        store = JpegStore(device=0)
        ids = store.add(paths_or_bytes)            # np.int64 ids, in order
        frames = store.decode(ids[perm])           # as JpegDecoder.decode returns them

    `add` is set-up and SYNCHRONISES: it parses and prepares the files on `threads` host threads, judges every file before anything is
    stored (a header or marker fault raises `JpegDecoder`'s exception, naming the item), uploads each file's unstuffed bytes, its
    `seg_start`, its `sub_start` and its `FearJpegScan` record into slabs of `slab_bytes` (uint8 tensors that are never reallocated, so
    addresses stay valid; a file never straddles a slab, a larger file gets a slab of its own), runs `fear_jpeg_index_build` over the
    call's files in groups bounded by `workspace_limit`, and waits for the verdicts: a file the device refuses raises
    `MalformedJPEG("item i: ...")`.  A call that raises commits nothing — `len(store)`, `nbytes` and every earlier id are as before; above
    `capacity_bytes` (counted as `nbytes` counts: the files' aligned resident bytes) it raises `StoreFull`.
    `store.kinds[id]` is "scan" or "pixels": an unsupported file with a `fallback` (without one: `UnsupportedJPEG`) and a file whose
    largest restart segment exceeds DEVICE_SCAN_MAX (decoded once through the host's Huffman stage) are kept as decoded pixels, which
    `decode` copies device to device.  Every returned frame is a private tensor, never an alias of the store.
    With `progressive=True` a progressive file (SOF2) is first replaced, on the pool, by its lossless baseline transcode
    (`fear_jpeg_progressive_to_baseline`: the same coefficients in one interleaved scan with a restart marker after every MCU row) and is
    from there a "scan" entry like any other — indexed, decoded by rows, judged by `check()` on the transcoded bytes; one the transcoder
    declines (an incomplete or inconsistent progression) goes to the `fallback` or raises, naming the item.

    `decode` runs on the current stream and never waits for the GPU: no file bytes go up, only about 0.5 kB of records per image in one
    pinned transfer; `fear_jpeg_dense_block_start` (only when the store's largest image grew), `fear_jpeg_huffman_indexed`,
    `fear_jpeg_decode_u8`; split by `workspace_limit` as the decoder splits.  Ids come in any order and may repeat; one out of range is
    an IndexError before any launch.  The statuses are kept and `check()` raises as `JpegDecoder.check` does — with a resident, verified
    store it should never fire.  The statuses of every group of the current call are kept, however small `workspace_limit` makes them,
    and those of the last PENDING_CALLS groups of earlier unchecked calls.  `decode` may be called on any stream (the shared block_start
    table is handed from stream to stream by an event); `add` ends with a synchronise, so what it stored is complete for all of them.
    `decode_rows(ids, rows)` decodes a band of rows per frame and `borders(ids)` gathers the frames' border colours, which `add` computed
    once: together they feed `TrainPairBuilder.build(..., borders=)` with entropy and pixel work for the rows the pairs read alone.  Per
    file the store keeps mcus_y + 1 row-table values on the host and 3 bytes of the device's border table more (`resident["rows"]`,
    `resident["border"]`, both counted in `nbytes`); the row table is also resident on the device (one tensor per `add`, the same
    4 (mcus_y + 1) bytes per file that `resident["rows"]` counts), for `decode_rows` with `rows` on the device.
    `decode_windows(ids, windows)` decodes per frame the MCUs that cover one rectangle and returns compact tensors with their origins
    (`WindowFrames`), which `TrainPairBuilder.build` takes in place of the frames.
    `residence="host"` keeps each file's unstuffed scan bytes in PINNED HOST memory and everything small — `seg_start`, `sub_start`, the
    index, the `FearJpegScan` record, the row tables, the borders — on the device: a ninth of a file's footprint, so that the store's
    capacity is the host's memory ("Bytes on the host").  The bytes lie in pinned slabs of `slab_bytes` under
    the device slabs' rules (never reallocated, a file never straddles one); a resident record's `bytes` is the slab's device-side
    address (`fear_host_mapped_pointer`), and every Huffman launch is the `_host` entry point of the same name, whose workgroups copy
    the byte range of their lanes into LDS with wide loads in front of the decode (zero copy: no file bytes are uploaded by a
    decode call).  `add` builds the index from a transient device copy of the call's bytes and drops it behind the verdicts; the
    index, the row tables and the borders are those of a `"device"` store byte for byte, and so is every frame of every call.
    `nbytes`, `capacity_bytes` and `resident["bytes"]` (then the two tables alone) count device bytes; `host_nbytes`,
    `host_capacity_bytes` and `resident["host_bytes"]` the pinned ones, and `StoreFull` names the limit that was hit.  Entries kept as
    pixels stay on the device.  `host_capacity_bytes` without `residence="host"`, or another `residence`, is a ValueError.
    Out of scope: eviction and `remove`, saving a store to disk, sharding over ranks, pageable or memory-mapped files as the backing
    of `residence="host"`, `JpegDecoder`'s default, windows given on the device."""
    PENDING_CALLS = 64

    def __init__(self, device: int = 0, capacity_bytes: Optional[int] = None, subsequence_bytes: int = 128, slab_bytes: int = 256 << 20,
                 workspace_limit: int = 1 << 30, threads: Optional[int] = None, initial_rows: int = 1024, progressive: bool = False,
                 residence: str = "device", host_capacity_bytes: Optional[int] = None):
        from .train_abi import FearJpegImage, FearJpegIndexed
        _check_subsequence_bytes(subsequence_bytes)
        if slab_bytes < 16 or initial_rows < 1:
            raise ValueError("slab_bytes is at least 16 and initial_rows at least 1")
        if residence not in ("device", "host"):
            raise ValueError(f'residence is "device" or "host", not {residence!r}')
        if host_capacity_bytes is not None and residence != "host":
            raise ValueError('host_capacity_bytes limits the pinned bytes of residence="host" alone')
        self.residence = residence
        self.host_capacity_bytes = None if host_capacity_bytes is None else int(host_capacity_bytes)
        self._staged = True                                              # (False: the direct kernels on host bytes, the bench's ablation)
        self.progressive = bool(progressive)
        self._host = JpegDecoder(device=device, threads=threads, progressive=progressive)   # the pool, sized as JpegDecoder sizes it: never by the machine's CPUs, at most 16
        self.threads, self.device, self._lib = self._host.threads, self._host.device, self._host._lib
        self.capacity_bytes = None if capacity_bytes is None else int(capacity_bytes)
        self.subsequence_bytes, self.slab_bytes, self.workspace_limit = int(subsequence_bytes), _up(int(slab_bytes), 16), int(workspace_limit)
        self._dtypes = (np.dtype(FearJpegIndexed), np.dtype(FearJpegImage), COLUMNS)
        self._initial_rows = int(initial_rows)
        self._pending: List = []
        self._pinned: List = []
        self.clear()

    # ------------------------------------------------------------------------------------------------------------------ bookkeeping
    def clear(self) -> None:
        """Forget every entry and free the slabs.  Ids start at 0 again.  (Pinned slabs are dropped behind a synchronise: a freed pinned
        block is handed out again at once, whatever kernel still reads it.)"""
        if getattr(self, "_host_slabs", None):
            import torch
            torch.cuda.synchronize(self.device)
        self._n, self.nbytes = 0, 0
        # what nbytes is made of, and `host_bytes`: the pinned bytes of residence="host", which nbytes does not count
        self.resident = dict(bytes=0, index=0, records=0, pixels=0, rows=0, border=0, host_bytes=0)
        self._host_slabs: List = []                                      # residence="host": (pinned uint8 tensor, its device-side address)
        self._host_open, self._host_cursor = None, 0
        self._row_sub, self._row_used = np.zeros(4 * self._initial_rows, dtype=np.uint32), 0   # ragged: COLUMNS["row_at"] indexes it
        self._border = None                                              # (capacity, 3) uint8 on the device, grown with the mirrors
        self._indexed, self._image, self._columns = (np.zeros(self._initial_rows, dtype=d) for d in self._dtypes)
        self._slabs: List = []
        self._row_slabs: List = []                                       # the row tables on the device, one uint32 tensor per `add`, never reallocated
        self._open, self._cursor = None, 0                               # the slab that is being filled
        self._pixels: dict = {}
        self._most, self._dense_start, self._dense_blocks, self._dense_event = 0, None, -1, None
        self._dense_retired: List = []                                   # earlier block_start tables: a decode in flight may still read one
        self._records = None                                             # the last group's host records, alive as long as the addresses are

    def close(self) -> None:
        self._host.close()
        self.clear()

    def __len__(self) -> int:
        return self._n

    @property
    def host_nbytes(self) -> int:
        """The pinned host bytes the store holds (residence="host"): `resident["host_bytes"]`, what `host_capacity_bytes` limits."""
        return self.resident["host_bytes"]

    @property
    def kinds(self) -> np.ndarray:
        return KIND_NAMES[self._columns["kind"][:self._n]]

    def borders(self, ids):
        """(len(ids), 3) uint8 on the device: `fear_frame_border_u8` of each file's full decode, computed once in `add` — what
        `TrainPairBuilder.build(..., borders=)` takes.  It stays the FULL-size decode's colour whatever `scale` the frames are decoded at.  A gather on the current stream; the ids go up non-blocking, it never waits."""
        import torch
        ids = self._checked(ids)
        with torch.cuda.device(self.device):
            if ids.size == 0 or self._border is None:
                return torch.empty((0, 3), dtype=torch.uint8, device=self.device)
            pinned = torch.empty(ids.size, dtype=torch.int64, pin_memory=True)
            np.copyto(pinned.numpy(), ids)
            index = pinned.to(self.device, non_blocking=True)
            self._pinned = self._pinned[-1:] + [pinned]
            return self._border.index_select(0, index)

    def shape(self, ids, scale=1) -> np.ndarray:
        """(len(ids), 2) int32: height and width, of the frames `decode(ids, scale=scale)` returns; `scale` an int or one per id."""
        ids = self._checked(ids)
        scale = _check_scales(scale, ids.size)
        rows = self._columns[ids]
        return np.stack(_scaled_sides(rows["H"], rows["W"], scale), axis=1).astype(np.int32)

    def _scan_only(self, ids: np.ndarray, scale) -> None:
        """At a scale every id is a "scan" entry: decoded pixels cannot be decoded again.  With a scale per position an entry kept as
        pixels is fine at a position whose scale is 1."""
        kept = np.flatnonzero((self._columns["kind"][ids] == KIND_PIXELS) & (scale > 1))
        if kept.size:
            at = scale if isinstance(scale, int) else int(scale[kept[0]])
            raise UnsupportedJPEG(f"id {int(ids[kept[0]])} is kept as decoded pixels, which scale={at} cannot decode")

    def _checked(self, ids) -> np.ndarray:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self._n):
            raise IndexError(f"an id outside 0..{self._n - 1}")
        return ids

    def _grow(self, rows: int) -> None:
        """The mirrors double until `rows` fit; old rows keep their place, so old ids stay valid."""
        have = self._columns.size
        if rows <= have:
            return
        while have < rows:
            have *= 2
        grown = []
        for old in (self._indexed, self._image, self._columns):
            new = np.zeros(have, dtype=old.dtype)
            new[:self._n] = old[:self._n]
            grown.append(new)
        self._indexed, self._image, self._columns = grown

    # -------------------------------------------------------------------------------------------------------------------------- add
    def add(self, items: Sequence[Item], fallback: Optional[Callable[[bytes], np.ndarray]] = None) -> np.ndarray:
        import torch
        blobs = _read_items(items)
        n = len(blobs)
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        # every stage in front of `_add_commit` returns values and assigns nothing on self: a call that raises commits nothing
        entries, through_host, raw = self._add_prepare(blobs, fallback)
        split = self._add_layout(entries, through_host, raw, n)
        with torch.cuda.device(self.device):
            new_slabs, open_slab, cursor, runs = self._add_place(entries)
            host_place = self._add_place_host(entries)
            transient = self._add_upload(runs)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            new_borders = torch.zeros((n, 3), dtype=torch.uint8, device=self.device)
            self._add_verdicts(self._add_index(entries, new_borders, stream), blobs)
            del transient                                                # the build's device copies of host-resident bytes
            pixels = self._add_pixels(blobs, through_host, raw, new_borders, stream)
            row_dev = self._add_row_tables(entries)
            border = self._add_border(self._n + n)
            torch.cuda.current_stream().synchronize()                    # what was stored is complete for a decode on any stream
        return self._add_commit(n, entries, pixels, split, new_slabs, open_slab, cursor, row_dev, border, new_borders, host_place)

    def _add_prepare(self, blobs: List[bytes], fallback):
        """Stage 1 of `add`: transcode (a progressive file takes its baseline transcode's place in `blobs`) and prepare on the pool, then
        judge every file before anything is stored.  The "scan" files as {item: _Entry}, the infos of those whose largest restart
        segment exceeds DEVICE_SCAN_MAX, and the fallback's pixels, by item."""
        declined = {}
        if self.progressive:
            for i, res in enumerate(self._host._pool.map(self._transcode, blobs)):
                if isinstance(res, bytes):
                    blobs[i] = res
                elif res is not None:
                    declined[i] = res                                    # the original goes to the fallback, or raises
        prepared = list(self._host._pool.map(self._host.scan_prepare, blobs))
        # (a file the transcoder declined is judged by the transcoder's status)
        jpegs, raw = _judge(blobs, [declined.get(i, res) for i, res in enumerate(prepared)], fallback, self.progressive, name_item=True)
        entries = {i: _Entry(*prepared[i]) for i in jpegs if prepared[i][3].max_seg_bytes <= jpeg_frames.DEVICE_SCAN_MAX}
        return entries, {i: prepared[i][0] for i in jpegs if i not in entries}, raw

    def _add_layout(self, entries: dict, through_host: dict, raw: dict, n: int) -> dict:
        """Stage 2: every entry's `sub_start` and resident layout from its base — bytes | seg_start | sub_start | index | FearJpegScan,
        each at 16 bytes — and what the call adds to `resident`, key by key; `StoreFull` where that exceeds the capacity.  Under
        residence="host" the bytes go to a pinned slab instead (`host_end` of them, counted as `host_bytes` against
        `host_capacity_bytes`) and the device layout begins with seg_start: `resident["bytes"]` then counts the two tables alone."""
        from . import train_abi as abi
        record = ctypes.sizeof(abi.FearJpegScan)
        split, on_host = dict(bytes=0, index=0, records=0, pixels=0, rows=0, border=3 * n, host_bytes=0), self.residence == "host"
        for e in entries.values():
            e.sub, count = np.empty(e.seg.size, dtype=np.uint32), ctypes.c_uint32(0)
            rc = self._lib.fear_jpeg_sub_start(e.seg.ctypes.data, e.scan.n_seg, e.scan.n_bytes, self.subsequence_bytes, e.sub.ctypes.data,
                                               e.sub.size, ctypes.byref(count))
            if rc != 0 or count.value != int(e.sub[-1]):
                raise abi.TrainError(f"fear_jpeg_sub_start failed with status {rc}")
            e.at_seg = _up(max(e.data.nbytes, 1), 16)
            if on_host:
                e.host_end, e.at_seg = e.at_seg, 0
                split["host_bytes"] += e.host_end
            e.at_sub = e.at_seg + _up(e.seg.nbytes, 16)
            e.at_index = e.at_sub + _up(e.sub.nbytes, 16)
            e.at_record = e.at_index + 16 * int(e.sub[-1])
            e.end = e.at_record + record
            split["bytes"] += e.at_index
            split["index"] += e.at_record - e.at_index
            split["records"] += record
            split["rows"] += 4 * (int(e.info.mcus_y) + 1)
        split["pixels"] = sum(3 * info.width * info.height for info in through_host.values()) + sum(px.nbytes for px in raw.values())
        need, host_need = sum(split.values()) - split["host_bytes"], split["host_bytes"]
        if self.capacity_bytes is not None and self.nbytes + need > self.capacity_bytes:
            raise StoreFull(f"{need} bytes more on top of {self.nbytes} exceed the capacity of {self.capacity_bytes}")
        if self.host_capacity_bytes is not None and self.host_nbytes + host_need > self.host_capacity_bytes:
            raise StoreFull(f"{host_need} pinned host bytes more on top of {self.host_nbytes} exceed the host capacity of "
                            f"{self.host_capacity_bytes}")
        return split

    def _add_place(self, entries: dict):
        """Stage 3: a place in a slab for every entry, from tentative cursors, and the runs of neighbours in a slab: the new slabs,
        the open slab and its cursor as the commit will set them, and the runs, each a list of entries."""
        import torch
        new_slabs, open_slab, cursor, runs = [], self._open, self._cursor, []
        for e in entries.values():
            if e.end > self.slab_bytes:                                  # a slab of its own; the open slab stays open
                e.slab, e.at = torch.empty(e.end, dtype=torch.uint8, device=self.device), 0
                new_slabs.append(e.slab)
            else:
                if open_slab is None or cursor + e.end > self.slab_bytes:
                    open_slab, cursor = torch.empty(self.slab_bytes, dtype=torch.uint8, device=self.device), 0
                    new_slabs.append(open_slab)
                e.slab, e.at = open_slab, cursor
                cursor += e.end
            assert e.slab.data_ptr() % 16 == 0
            e.base = e.slab.data_ptr() + e.at
            if runs and runs[-1][-1].slab is e.slab and runs[-1][-1].at + runs[-1][-1].end == e.at:
                runs[-1].append(e)
            else:
                runs.append([e])
        return new_slabs, open_slab, cursor, runs

    def _add_place_host(self, entries: dict):
        """Stage 3 for the bytes of residence="host": a place in a pinned slab for every entry's bytes, by the rule of the device
        slabs (never reallocated, a file never straddles one, a larger file gets its own), and the bytes copied there — behind the
        tentative cursor, where no entry of the store lies.  The new slabs, each with its device-side address
        (`fear_host_mapped_pointer`, once per slab), the open one and its cursor as the commit will set them; None on the device."""
        import torch
        from . import train_abi as abi
        if self.residence != "host":
            return None
        new_slabs, open_slab, cursor = [], self._host_open, self._host_cursor

        def pinned(nbytes):
            slab, mapped = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), ctypes.c_void_p(0)
            abi.launch(self._lib, "fear_host_mapped_pointer", ctypes.c_void_p(slab.data_ptr()), ctypes.byref(mapped))
            assert mapped.value % 16 == 0
            new_slabs.append((slab, mapped.value))
            return new_slabs[-1]

        for e in entries.values():
            if e.host_end > self.slab_bytes:                             # a slab of its own; the open slab stays open
                (e.host_slab, address), e.host_at = pinned(e.host_end), 0
            else:
                if open_slab is None or cursor + e.host_end > self.slab_bytes:
                    open_slab, cursor = pinned(self.slab_bytes), 0
                (e.host_slab, address), e.host_at = open_slab, cursor
                cursor += e.host_end
            e.host_base = address + e.host_at
            e.host_slab.numpy()[e.host_at:e.host_at + e.data.nbytes] = e.data
        return new_slabs, open_slab, cursor

    def _add_upload(self, runs: List[list]) -> List:
        """Stage 4: one copy per run of neighbours in a slab.  Under residence="host" the resident record points at the pinned bytes,
        and the run's bytes go up once more into a transient tensor for `fear_jpeg_index_build`, whose synchronisation passes read
        every byte several times: those tensors, which `add` drops behind the verdicts."""
        import torch
        transient = []
        for run in runs:
            host, w = np.zeros(sum(e.end for e in run), dtype=np.uint8), 0
            if self.residence == "host":
                at = _exclusive(np.array([e.host_end for e in run], dtype=np.int64))
                staged = np.zeros(int(at[-1]), dtype=np.uint8)
                for e, a in zip(run, at.tolist()):
                    staged[a:a + e.data.nbytes] = e.data
                transient.append(torch.from_numpy(staged).to(self.device))
                for e, a in zip(run, at.tolist()):
                    e.build_bytes = transient[-1].data_ptr() + a
            for e in run:
                e.scan.bytes, e.scan.seg_start, e.scan.coef_offset = e.host_base or e.base, e.base + e.at_seg, 0
                if not e.host_end:
                    host[w:w + e.data.nbytes] = e.data
                host[w + e.at_seg:w + e.at_seg + e.seg.nbytes] = e.seg.view(np.uint8)
                host[w + e.at_sub:w + e.at_sub + e.sub.nbytes] = e.sub.view(np.uint8)
                host[w + e.at_record:w + e.end] = np.frombuffer(e.scan, dtype=np.uint8)
                w += e.end
            run[0].slab[run[0].at:run[0].at + host.size].copy_(torch.from_numpy(host))
        return transient

    def _add_index(self, entries: dict, new_borders, stream) -> List[tuple]:
        """Stage 5: `fear_jpeg_index_build` over the entries in groups that `_cut` bounds by the scratch coefficients, and each group's
        border colours into `new_borders`.  Per group its items, its status tensor and what the launch reads, kept alive."""
        import torch
        from . import train_abi as abi
        items, verdicts = list(entries), []
        dense = np.array([128 * int(e.info.total_blocks) for e in entries.values()], dtype=np.int64)
        for lo, hi in _cut(dense, self.workspace_limit, 65535):
            group, m = items[lo:hi], hi - lo
            records, indexes = (abi.FearJpegScan * m)(), (abi.FearJpegIndex * m)()
            prefix, values = np.zeros(m + 1, dtype=np.uint32), 0
            for k, e in enumerate(entries[i] for i in group):
                ctypes.memmove(ctypes.byref(records[k]), ctypes.byref(e.scan), ctypes.sizeof(e.scan))
                records[k].coef_offset = values
                if e.build_bytes:
                    records[k].bytes = e.build_bytes                     # the transient device copy; the resident record keeps the host's
                values += 64 * int(e.info.total_blocks)
                prefix[k + 1] = prefix[k] + e.scan.n_seg
                ix = indexes[k]
                ix.index, ix.sub_start, ix.seg_start_host, ix.n_sub = e.base + e.at_index, e.base + e.at_sub, e.seg.ctypes.data, int(e.sub[-1])
            records_at = _up(prefix.nbytes, 16)
            index_at = records_at + ctypes.sizeof(records)
            table = np.zeros(index_at + ctypes.sizeof(indexes), dtype=np.uint8)
            table[:prefix.nbytes] = prefix.view(np.uint8)
            table[records_at:index_at] = np.frombuffer(records, dtype=np.uint8)
            table[index_at:] = np.frombuffer(indexes, dtype=np.uint8)
            dev = torch.from_numpy(table).to(self.device)
            coef = torch.empty(max(values, 8), dtype=torch.int16, device=self.device)
            status = torch.empty(m, dtype=torch.int32, device=self.device)
            abi.launch(self._lib, "fear_jpeg_index_build", records, m, ctypes.c_void_p(dev.data_ptr()), indexes,
                       ctypes.c_void_p(dev.data_ptr() + index_at), ctypes.c_void_p(coef.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                       self.subsequence_bytes, stream)
            verdicts.append((group, status, dev, coef))
            new_borders[group] = self._group_borders([entries[i].info for i in group], records, coef, stream)
        return verdicts

    def _add_verdicts(self, verdicts: List[tuple], blobs: List[bytes]) -> None:
        """Stage 6: wait for the verdicts (`add` is set-up); a file the device refuses raises, naming the item."""
        for group, status, _, _ in verdicts:
            got = status.cpu().numpy()
            for k in np.flatnonzero(got):
                i = group[int(k)]
                try:
                    _raise_as_python(blobs[i], int(got[k]))
                except MalformedJPEG as exc:
                    raise MalformedJPEG(f"item {i}: {exc}") from None

    def _add_pixels(self, blobs: List[bytes], through_host: dict, raw: dict, new_borders, stream) -> dict:
        """Stage 7: the entries kept as pixels, by item — a file with too large a restart segment once through the host's Huffman
        stage, which judges the file itself, and the fallback's arrays — and their border colours into `new_borders`."""
        import torch
        pixels = {}
        for i in through_host:
            try:
                pixels[i] = self._host.decode([blobs[i]])[0].clone()
            except (MalformedJPEG, UnsupportedJPEG) as exc:
                raise type(exc)(f"item {i}: {exc}") from None
        for i, px in raw.items():
            pixels[i] = torch.from_numpy(px.copy()).to(self.device)             # (the fallback's array may be read-only)
        if pixels:
            kept = sorted(pixels)
            new_borders[kept] = self._frame_borders([pixels[i] for i in kept], stream)
        return pixels

    def _add_row_tables(self, entries: dict):
        """Stage 8: every entry's row table, from the index the device has just written (copied back once: `add` waits anyway), and
        all of them once more on the device, for rows that only the device knows: one tensor per `add`, None without an entry."""
        import torch
        if not entries:
            return None
        for e in entries.values():
            index = e.slab[e.at + e.at_index:e.at + e.at_record].cpu().numpy().view(SUBSEQ_DTYPE)
            e.row_table = self._row_table(e.info, e.sub, index)
        tables = [e.row_table for e in entries.values()]
        row_dev = torch.from_numpy(np.concatenate(tables).astype(np.uint32).view(np.int32)).to(self.device)
        for e, at in zip(entries.values(), _exclusive(np.array([t.size for t in tables], dtype=np.int64)).tolist()):
            e.row_dev_at = row_dev.data_ptr() + 4 * at
        return row_dev

    def _add_border(self, rows: int):
        """Stage 9: the border table with room for `rows` entries: the store's, or a doubled one that holds its rows."""
        import torch
        border = self._border
        if border is None or border.shape[0] < rows:
            have = max(self._initial_rows, 1) if border is None else border.shape[0]
            while have < rows:
                have *= 2
            border = torch.zeros((have, 3), dtype=torch.uint8, device=self.device)
            if self._border is not None and self._n:
                border[:self._n] = self._border[:self._n]
        return border

    def _add_commit(self, n: int, entries: dict, pixels: dict, split: dict, new_slabs: List, open_slab, cursor: int, row_dev, border,
                    new_borders, host_place=None) -> np.ndarray:
        """Stage 10, the only one that assigns on self: the mirrors' rows, the row tables, the border colours, the slabs and the
        counts.  The ids."""
        import torch
        from . import train_abi as abi
        first = self._n
        self._grow(first + n)
        for i, e in entries.items():
            row, n_sub = self._indexed[first + i], int(e.sub[-1])
            row["scan"], row["index"], row["sub_start"], row["n_sub"] = e.base + e.at_record, e.base + e.at_index, e.base + e.at_sub, n_sub
            row["row_sub"] = e.row_dev_at
            _fill_header(abi.FearJpegImage.from_buffer(self._image, (first + i) * self._image.itemsize), e.info)
            scan_columns(self._columns[first + i], e.info, e.scan.n_seg, n_sub, self._row_used)
            used = self._row_used + e.row_table.size
            if used > self._row_sub.size:
                grown = np.zeros(max(2 * self._row_sub.size, used), dtype=np.uint32)
                grown[:self._row_used] = self._row_sub[:self._row_used]
                self._row_sub = grown
            self._row_sub[self._row_used:used] = e.row_table
            self._row_used = used
            self._most = max(self._most, int(e.info.total_blocks))
        for i, px in pixels.items():
            col = self._columns[first + i]
            col["H"], col["W"], col["kind"] = px.shape[0], px.shape[1], KIND_PIXELS
            self._pixels[first + i] = px
        with torch.cuda.device(self.device):                             # on the stream add has just waited for; a decode on another
            border[first:first + n] = new_borders                        # stream is ordered behind the synchronise below
            torch.cuda.current_stream().synchronize()
        self._border = border
        self._slabs += new_slabs
        if row_dev is not None:
            self._row_slabs.append(row_dev)
        self._open, self._cursor = open_slab, cursor
        if host_place is not None:
            self._host_slabs += host_place[0]
            self._host_open, self._host_cursor = host_place[1], host_place[2]
        self._n, self.nbytes = first + n, self.nbytes + sum(split.values()) - split["host_bytes"]
        for key, v in split.items():
            self.resident[key] += v
        return np.arange(first, first + n, dtype=np.int64)


    def _transcode(self, data: bytes):
        """None for a file the baseline parser does not decline; else the baseline transcode of a progressive file, or the status with
        which `fear_jpeg_progressive_to_baseline` declines it (FEAR_TRAIN_ERR_UNSUPPORTED also for a frame that is not SOF2)."""
        from .train_abi import FearJpegInfo
        if self._lib.fear_jpeg_parse(data, len(data), ctypes.byref(FearJpegInfo())) != ERR_UNSUPPORTED:
            return None
        return self._host.to_baseline(data)

    def _row_table(self, info, sub: np.ndarray, index: np.ndarray) -> np.ndarray:
        """`jpeg_huffman.scan_row_sub` from the library's header."""
        class Header:
            ids = list(range(info.components))
            h, v, mcus_x, mcus_y, restart = list(info.h), list(info.v), info.mcus_x, info.mcus_y, info.restart_interval
        return scan_row_sub(Header, sub, index)

    def _frame_borders(self, frames: List, stream):
        """(len(frames), 3) uint8 on the device: fear_frame_border_u8 of uint8 (H, W, 3) device frames."""
        import torch
        from . import train_abi as abi
        table = np.zeros(len(frames), dtype=np.dtype(abi.FearFrame))
        for k, f in enumerate(frames):
            table[k] = (f.data_ptr(), f.shape[0], f.shape[1])
        dev = torch.from_numpy(table.view(np.uint8)).to(self.device)
        out = torch.empty((len(frames), 3), dtype=torch.uint8, device=self.device)
        abi.launch(self._lib, "fear_frame_border_u8", ctypes.c_void_p(dev.data_ptr()), len(frames), ctypes.c_void_p(out.data_ptr()), stream)
        return out

    def _group_borders(self, infos: List, records, coef, stream):
        """The border colours of one group of `add`: the dense coefficients fear_jpeg_index_build has just left in `coef` (record k's at
        its coef_offset) through the unchanged fear_jpeg_decode_u8 and fear_frame_border_u8."""
        import torch
        from . import train_abi as abi
        m = len(infos)
        images = np.zeros(m, dtype=self._dtypes[1])
        for rec, info in zip((abi.FearJpegImage * m).from_buffer(images), infos):
            _fill_header(rec, info)
        blocks = np.array([int(i.total_blocks) for i in infos], dtype=np.int64)
        high, wide = images["height"].astype(np.int64), images["width"].astype(np.int64)
        plan = _layout(blocks, high * wide, high * wide)                 # plan_decode's, of a group that is all "scan" entries
        # a table of its own: `add` commits the store's largest image, which sizes the shared one, only at its end
        start = torch.empty(plan["most"] + 1, dtype=torch.int32, device=self.device)
        abi.launch(self._lib, "fear_jpeg_dense_block_start", ctypes.c_void_p(start.data_ptr()), plan["most"], stream)
        out = torch.empty(max(plan["out_bytes"], 16), dtype=torch.uint8, device=self.device)
        ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=self.device)
        offsets = np.array([int(r.coef_offset) for r in records], dtype=np.uint64)
        _place_images(images, coef, offsets, start, out, plan["out_offset"], plan["plane_offset"])
        dev, at = self._upload([np.concatenate([plan["block_prefix"], plan["pixel_prefix"]]), images], pinned=False)
        _launch_pixels(self._lib, ctypes.c_void_p(images.ctypes.data), m, dev.data_ptr() + at[0], ws.data_ptr(), plan["workspace_bytes"], 1,
                       stream)
        return self._frame_borders(_frame_views(out, plan["out_offset"], high, wide), stream)

    # ----------------------------------------------------------------------------------------------------------------------- decode
    def decode(self, ids, check: bool = False, scale=1) -> List:
        """`scale` 2, 4 or 8: the frames at 1/2, 1/4 or 1/8 size (`shape(ids, scale)`), byte for byte `JpegDecoder.decode(scale=)`'s and
        libjpeg's: the same plan and Huffman stage, `fear_jpeg_decode_scaled_u8` for the pixels.  An id kept as pixels is then an
        `UnsupportedJPEG` naming it, another `scale` a ValueError, both before any launch.
        `scale` may also be a sequence or array of len(ids) scales from {1, 2, 4, 8}, one per POSITION (the same id may come several
        times at different scales): frame i is `decode([ids[i]], scale=scale[i])[0]` byte for byte.  A group of the call whose scales
        differ runs `fear_jpeg_decode_mixed_u8` — still two pixel launches — and one whose scales are all equal the uniform launch; a
        sequence of equal values gives the int's bytes.  A wrong length, another value or a bool is a ValueError, and an id kept as
        pixels at a position whose scale is not 1 an `UnsupportedJPEG`, before any launch.  (`JpegDecoder.decode` takes an int alone.)"""
        ids = self._checked(ids)
        scale = _check_scales(scale, ids.size)
        self._scan_only(ids, scale)
        return self._decode_groups(ids, plan_decode(self._columns, ids, self.workspace_limit, scale=scale), check, scale=scale)

    def _decode_rows_device(self, ids: np.ndarray, rows, check: bool) -> List:
        import torch
        mine = torch.device(self.device)
        if rows.device.index != (mine.index or 0) or rows.dtype != torch.int32 or tuple(rows.shape) != (ids.size, 2):
            raise ValueError(f"rows on a device must be ({ids.size}, 2) int32 on {mine}, one [y0, y1) per id")
        return self._decode_groups(ids, plan_decode(self._columns, ids, self.workspace_limit), check, rows)

    def _decode_groups(self, ids: np.ndarray, plans: List[dict], check: bool, rows=None, scale=1) -> List:
        """The frames of one call, group by group."""
        frames: List = [None] * ids.size
        self._pending = self._pending[-self.PENDING_CALLS:]              # of earlier calls; every group of this call is kept
        for plan in plans:
            self._decode_group(ids, plan, frames, rows, scale)
        if check:
            self.check()
        return frames

    def _decode_group(self, ids: np.ndarray, plan: dict, frames: List, rows=None, scale=1) -> None:
        """One group of `decode`, of both forms of `decode_rows` and of `decode_windows`: the shared block_start table, the gathered records with the
        group's addresses, one pinned upload, the Huffman kernel, the pixel stage, the verdicts, the frames.  What the plan carries
        and `rows` select the kernels: a plan of `plan_decode_rows` carries the bands (sub0, sub_count, mcu_row0, mcu_rows, band_height,
        band_out), which go into the records for `fear_jpeg_huffman_indexed_rows`; a plan of `plan_decode_windows` carries the MCU
        columns and the window's width as well (cols, win_width) and the compact tensors' shapes (high, wide, window), for
        `fear_jpeg_huffman_indexed_windows`; `rows`, the call's device tensor, goes with
        `plan_decode`'s full-image plan to the two kernels that read the bands on the device; a plan with a scale per position
        carries `scales`, which go into the records' reserved[0] and to `_launch_pixels`, which chooses the pixel stage's entry point."""
        import torch
        from . import train_abi as abi
        P = ctypes.c_void_p
        lo, hi, scan = plan["lo"], plan["hi"], plan["scan"]
        group = ids[lo:hi]
        sids, nd, banded, windowed = group[scan], scan.size, "sub0" in plan, "cols" in plan
        huffman = ("fear_jpeg_huffman_indexed_rows_dev" if rows is not None else "fear_jpeg_huffman_indexed_windows" if windowed
                   else "fear_jpeg_huffman_indexed_rows" if banded else "fear_jpeg_huffman_indexed")
        if self.residence == "host" and self._staged:                    # the same records and grid, the staged fetch
            huffman += "_host"
        with torch.cuda.device(self.device):
            out = torch.empty(max(plan["out_bytes"], 16), dtype=torch.uint8, device=self.device)
            out_offset = plan["out_offset"]
            if nd:
                stream = P(torch.cuda.current_stream().cuda_stream)
                block_start = self._block_start(stream)
                coef = torch.empty(max(plan["values"], 8), dtype=torch.int16, device=self.device)
                ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=self.device)
                status = torch.empty(nd, dtype=torch.int32, device=self.device)
                indexed, images = self._indexed[sids], self._image[sids]  # gathers: private copies
                indexed["coef_offset"] = plan["coef_offset"]
                at_out = out_offset[scan]
                if banded:                                               # the band as an image of its own, written into its frame's rows
                    for field in ("sub0", "sub_count", "mcu_row0", "mcu_rows"):
                        indexed[field] = plan[field]
                    images["height"] = plan["band_height"]
                    at_out = at_out + plan["band_out"]
                if windowed:                                             # and the band's MCU columns: a compact image of its own
                    indexed["reserved"] = plan["cols"]
                    images["width"] = plan["win_width"]
                _place_images(images, coef, plan["coef_offset"], block_start, out, at_out, plan["plane_offset"])
                if "scales" in plan:
                    images["reserved"][:, 0] = plan["scales"]
                # one pinned upload: prefix | FearJpegIndexed records, then two prefixes | FearJpegImage records; with rows on the
                # device and a group that is no run of positions also the positions, to gather the group's rows with
                parts = [plan["sub_prefix"], indexed, np.concatenate([plan["block_prefix"], plan["pixel_prefix"]]), images]
                whole = rows is None or nd == hi - lo
                if not whole:
                    parts.append(lo + scan)
                dev, at = self._upload(parts)
                table = dev.data_ptr() + at[2]
                self._records = (indexed, images)                        # the calls below get their addresses
                self.last_upload_bytes = dev.numel()
                if rows is None:
                    abi.launch(self._lib, huffman, P(indexed.ctypes.data), nd,
                               P(dev.data_ptr()), P(coef.data_ptr()), P(status.data_ptr()), self.subsequence_bytes, stream)
                    _launch_pixels(self._lib, P(images.ctypes.data), nd, table, ws.data_ptr(), plan["workspace_bytes"],
                                   plan.get("scales", scale), stream)
                else:                                                    # the group's rows: a slice, or a gather on the device; no wait
                    mine = rows[lo:hi] if whole else rows.index_select(0, dev[at[4]:].view(torch.int64))
                    mine = mine.contiguous()
                    abi.launch(self._lib, huffman, P(indexed.ctypes.data), nd, P(dev.data_ptr()), P(mine.data_ptr()),
                               P(coef.data_ptr()), P(status.data_ptr()), self.subsequence_bytes, stream)
                    abi.launch(self._lib, "fear_jpeg_decode_u8_rows_dev", P(images.ctypes.data), nd, P(table), P(mine.data_ptr()),
                               P(ws.data_ptr()), plan["workspace_bytes"], stream)
                verdict = torch.empty(nd, dtype=torch.int32, pin_memory=True)
                verdict.copy_(status, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                self._pending.append((event, verdict, lo + scan, sids))
            high, wide = self._copy_kept(group, plan, out, scale if isinstance(scale, int) else scale[lo:hi])
        frames[lo:hi] = _frame_views(out, out_offset, high, wide)

    def _copy_kept(self, group: np.ndarray, plan: dict, out, scale):
        """The group's entries kept as pixels, copied into `out` — a whole copy, never an alias; under a plan of `plan_decode_windows`
        the rectangle itself — and the height and width of every frame of the group."""
        cols, out_offset = self._columns[group], plan["out_offset"]
        if "cols" in plan:                                               # compact tensors
            high, wide = plan["high"], plan["wide"]
            for k in np.flatnonzero((cols["kind"] == KIND_PIXELS) & (high * wide > 0)):
                y0, y1, x0, x1 = plan["window"][k].tolist()
                out[out_offset[k]:out_offset[k] + 3 * high[k] * wide[k]].view(int(high[k]), int(wide[k]), 3).copy_(
                    self._pixels[int(group[k])][y0:y1, x0:x1], non_blocking=True)
        else:
            high, wide = _scaled_sides(cols["H"], cols["W"], scale)
            for k in np.flatnonzero(cols["kind"] == KIND_PIXELS):
                out[out_offset[k]:out_offset[k] + 3 * high[k] * wide[k]].copy_(self._pixels[int(group[k])].view(-1), non_blocking=True)
        return high, wide

    def _block_start(self, stream):
        """The dense block_start table that every record of `decode` points at, long enough for the store's largest image (a band has
        no more blocks): written again when that grew, else waited for — it was written on whatever stream was current then."""
        import torch
        from . import train_abi as abi
        if self._dense_blocks < self._most:
            self._dense_retired.append(self._dense_start)
            self._dense_start = torch.empty(self._most + 1, dtype=torch.int32, device=self.device)
            abi.launch(self._lib, "fear_jpeg_dense_block_start", ctypes.c_void_p(self._dense_start.data_ptr()), self._most, stream)
            self._dense_blocks, self._dense_event = self._most, torch.cuda.Event()
            self._dense_event.record()
        else:
            torch.cuda.current_stream().wait_event(self._dense_event)
        return self._dense_start

    def _upload(self, parts: List[np.ndarray], pinned: bool = True):
        """`parts` one after the other in one transfer, each at a multiple of 16 bytes: the device tensor and where each part begins.
        Pinned and non-blocking, the staging buffer kept while the copy may run; `pinned=False` is `add`'s, which waits."""
        import torch
        at, end = [], 0
        for part in parts:
            at.append(_up(end, 16))
            end = at[-1] + part.nbytes
        staged = torch.empty(end, dtype=torch.uint8, pin_memory=pinned)
        host = staged.numpy()
        for a, part in zip(at, parts):
            host[a:a + part.nbytes] = part.view(np.uint8)
        if not pinned:
            return staged.to(self.device), at
        dev = torch.empty(end, dtype=torch.uint8, device=self.device)
        dev.copy_(staged, non_blocking=True)
        self._pinned = self._pinned[-1:] + [staged]
        return dev, at

    # ------------------------------------------------------------------------------------------------------------------ decode_rows
    def decode_rows(self, ids, rows=None, check: bool = False, scale=1) -> List:
        """`decode` for the rows a consumer reads.  `rows` is (len(ids), 2) integers, the pixel rows [y0, y1) per position, clipped to
        [0, H]; the result is what `decode` returns — private uint8 (H, W, 3) tensors of the FULL frame shape — of which only the rows
        [y0, y1) are defined: they are byte for byte `decode`'s.  ALL OTHER ROWS HOLD UNSPECIFIED BYTES (a row that is never read costs
        an allocation, no traffic).  Per "scan" position the band of MCU rows that covers [y0, y1) — one more on each side where the
        vertical chroma upsampling reads a neighbour row — is Huffman-decoded by `fear_jpeg_huffman_indexed_rows`, whose lanes are the
        band's subsequences alone, and goes through `fear_jpeg_decode_u8` as an image of its own that ends where the band ends;
        y0 >= y1 decodes nothing for the position; an entry kept as pixels is copied whole; `rows=None` is `decode`.  A `rows` of another
        shape is a ValueError and a bad id an IndexError, both before any launch.  Like `decode` it never waits, the statuses (of the
        lanes that ran; the files were judged in full by `add`) go to `check()`, and `workspace_limit` splits the call, by the bands'
        dense coefficients.

        `rows` may also be a CUDA tensor on the store's device, (len(ids), 2) int32 — `FEARMultiTracker.search_rows()` returns one.
        Its values are read ONLY BY KERNELS and may still be in flight on the current stream: the call does not synchronise and does not
        copy them to the host.  They are clipped to [0, H] on the device (a negative y0 and y1 > H included), y0 >= y1 decodes nothing
        for the position, and the result is the same list of private full-shape frames, rows [y0, y1) byte for byte `decode`'s, all
        other rows unspecified.  The host cannot know the band, so this form runs `decode`'s plan (`plan_decode`: full grids, the
        full-image layout of the dense coefficients and the planes, `workspace_limit` splitting the call by full-image coefficients,
        each group taking its slice of `rows` by device indexing with indices the host knows); the work is saved in the kernels:
        `fear_jpeg_huffman_indexed_rows_dev` runs only the lanes of the band's subsequences and `fear_jpeg_decode_u8_rows_dev` only the
        band's blocks and the window's pixels, and a workgroup outside them returns after a few loads.  A CUDA tensor of another
        shape, dtype or device is a ValueError before any launch (a CPU tensor is host rows, as any array).

        `scale` 2, 4 or 8, for rows given on the HOST: `rows` are rows of the scaled frame (`shape(ids, scale)`), the frames have that
        shape and the rows [y0, y1) are byte for byte `decode(ids, scale=scale)`'s.  The band is the MCU rows that cover them — a scaled
        MCU row is v m pixel rows, m = 8 // scale — without a halo: at a scale no supported mode upsamples vertically.  The band goes
        through `fear_jpeg_decode_scaled_u8` as an image of its own: the record's height is the band's full-size height and `out` its
        first scaled row.  An id kept as pixels is an `UnsupportedJPEG`; `rows` on the device with `scale` > 1 is a ValueError (out of
        scope).
        `scale` may also be one scale per position, as `decode` takes it, for rows on the host: `rows[i]` is then in rows of position
        i's own scaled frame, a position at scale 1 keeps its chroma halo and a scaled one has none, and an entry kept as pixels is
        fine where the scale is 1.  Rows on the device take `scale=1` alone, as an int or per position (out of scope otherwise)."""
        ids = self._checked(ids)
        scale = _check_scales(scale, ids.size)
        if rows is None:
            return self.decode(ids, check=check, scale=scale)
        if type(rows).__module__.split(".")[0] == "torch" and rows.is_cuda:         # (a CPU tensor is host rows, as before)
            if np.any(scale > 1):
                raise ValueError("decode_rows takes rows on the device at scale=1 only")
            return self._decode_rows_device(ids, rows, check)
        self._scan_only(ids, scale)
        rows = np.asarray(rows)
        if rows.shape != (ids.size, 2) or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError(f"rows must be ({ids.size}, 2) integers, one [y0, y1) per id")
        return self._decode_groups(ids, plan_decode_rows(self._columns, self._row_sub, ids, rows, self.workspace_limit, scale=scale), check,
                                   scale=scale)

    # --------------------------------------------------------------------------------------------------------------- decode_windows
    def decode_windows(self, ids, windows, check: bool = False, scale=1) -> WindowFrames:
        """`decode` for the rectangle of each frame that a consumer reads, as COMPACT tensors.  `windows` is (len(ids), 4) integers on
        the host, [y0, y1) x [x0, x1) per position as (y0, y1, x0, x1), in pixels of the frame `decode(ids, scale=scale)` returns and
        clipped to it.  The result is a `WindowFrames`: `frames[i]` is a private uint8 (wh, ww, 3) tensor (cut from one allocation per
        group) whose first pixel is the frame's pixel `origin[i]`, and
            frames[i][y0 - oy:y1 - oy, x0 - ox:x1 - ox]  equals  decode(ids, scale=scale)[i][y0:y1, x0:x1]
        byte for byte; all other bytes of the tensor are unspecified.  `shape` is `shape(ids, scale)` and `window` the clipped request.
        Per "scan" position the MCUs of the band of rows (`decode_rows`' rule, halo included) and of the MCU columns that cover
        [x0, x1) — one more on each side where the file subsamples horizontally, at every scale — are Huffman-decoded by
        `fear_jpeg_huffman_indexed_windows`: the band's lanes, of which those that cannot touch the columns return early, and the
        blocks stored window-dense.  The window then goes through `fear_jpeg_decode_u8` (at a scale `fear_jpeg_decode_scaled_u8`) as an
        image of its own that ends where the window ends, so that the edge rules apply at the frame's true right and bottom edges.
        An empty window gives a (0, 0, 3) tensor and no lanes; an entry kept as pixels gives a device-to-device copy of the rectangle
        itself at scale 1 and is an `UnsupportedJPEG` at a scale.  A `windows` of another shape is a ValueError and a bad id an
        IndexError, both before any launch.  Like `decode` it never waits, the statuses (of the lanes that ran) go to `check()`, and
        `workspace_limit` splits the call, by the windows' dense coefficients.  Windows on the device are out of scope.
        `scale` may also be one scale per position, as `decode` takes it: `windows[i]` is then in pixels of position i's own scaled
        frame, `shape` is `shape(ids, scale)` per position, and an entry kept as pixels is fine where the scale is 1."""
        ids = self._checked(ids)
        scale = _check_scales(scale, ids.size)
        self._scan_only(ids, scale)
        windows = np.asarray(windows)
        if windows.shape != (ids.size, 4) or not np.issubdtype(windows.dtype, np.integer):
            raise ValueError(f"windows must be ({ids.size}, 4) integers, one (y0, y1, x0, x1) per id")
        plans = plan_decode_windows(self._columns, self._row_sub, ids, windows, self.workspace_limit, scale=scale)
        frames = self._decode_groups(ids, plans, check, scale=scale)
        origin = np.concatenate([np.zeros((0, 2), dtype=np.int32)] + [p["origin"] for p in plans])
        window = np.concatenate([np.zeros((0, 4), dtype=np.int64)] + [p["window"] for p in plans])
        return WindowFrames(frames, origin, self.shape(ids, scale), window)

    def check(self) -> None:
        """Wait for the calls not yet checked and raise MalformedJPEG for the first image the device refused, naming the position in its
        call's ids and the id."""
        pending, self._pending = self._pending, []
        for k, (event, status, positions, sids) in enumerate(pending):
            event.synchronize()
            bad = np.flatnonzero(status.numpy())
            if bad.size:
                self._pending = pending[k + 1:]
                j = int(bad[0])
                raise MalformedJPEG(f"item {int(positions[j])}: the device refused the resident scan of id {int(sids[j])} "
                                    f"with status {int(status[j])}")


class StoreFrames:
    """The frames of one sequence kept in a `JpegStore`: `store.decode([ids[t]])[0]` is frame t.  `SequenceValidator.run` takes it in
    place of a sequence's frames and decodes, from the second frame on, only the rows the tracker's next search window reads."""

    def __init__(self, store: JpegStore, ids) -> None:
        self.store = store
        self.ids = store._checked(ids)

    def __len__(self) -> int:
        return int(self.ids.size)

    def __iter__(self):
        for i in self.ids:
            yield self.store.decode([int(i)])[0]
