"""The device's Huffman stage of the JPEG frame decoder, stated in numpy and plain Python ("The Huffman stage on the
device").  `jpeg_scan_prepare_host` restates `fear_jpeg_scan_prepare` (csrc/fear_jpeg_entropy.h): the entropy-coded bytes with the FF 00
stuffing removed, split at the restart markers.  `jpeg_entropy_parallel_host` restates `fear_jpeg_huffman` (csrc/fear_jpeg_huffman.h): the
self-synchronising parallel decode of Weissenberger and Schmidt, in the variant that is exact with bounded work — the same steps in the
same order as the kernel, lane by lane.  tests/test_jpeg_huffman_host.py holds it to `jpeg_coefficients_host`, coefficient for coefficient
and verdict for verdict."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .jpeg_frames import ERR_FORMAT, MalformedJPEG, _Header, _Huffman, _parse


def scan_segments(hd: _Header) -> int:
    """The restart segments of the scan: ceil(MCUs / restart interval), one without an interval."""
    n_mcu = hd.mcus_x * hd.mcus_y
    return -(-n_mcu // hd.restart) if hd.restart else 1


def jpeg_scan_prepare_host(data: bytes, hd: _Header = None) -> Tuple[bytes, List[int]]:
    """The scan's bytes without their stuffing and the offsets of its segments: segment s owns bytes[start[s]:start[s + 1]].  In front of
    the last segment marker k must be RST(k mod 8); the last segment ends at any marker or with the file, as Bits::fill ends the data."""
    data = bytes(data)
    if hd is None:
        hd = _parse(data)
    n, p, want = len(data), hd.scan, scan_segments(hd)
    out, start = bytearray(), [0]
    while True:
        q = data.find(b"\xff", p)
        if q < 0:
            q = n
        out += data[p:q]
        if q + 1 >= n:                              # the file ends, perhaps inside a marker
            break
        m = data[q + 1]
        if m == 0:
            out.append(0xFF)
            p = q + 2
            continue
        if len(start) == want:                      # any marker ends the last segment
            break
        if m != 0xD0 + ((len(start) - 1) & 7):
            raise MalformedJPEG("a restart marker is missing or out of order")
        start.append(len(out))
        p = q + 2
    if len(start) != want:
        raise MalformedJPEG("a restart marker is missing or out of order")
    start.append(len(out))
    return bytes(out), start


_look_cache: dict = {}


def _look16(t: _Huffman) -> list:
    """(length << 8 | symbol) for every 16-bit prefix, 0 where no code matches: the kernel's 9-bit table and slow path in one."""
    key = (tuple(t.counts), bytes(t.values))
    if key in _look_cache:
        return _look_cache[key]
    if len(_look_cache) >= 64:
        _look_cache.clear()
    look = np.zeros(1 << 16, dtype=np.int32)
    for length in range(1, 17):
        for k in range(t.counts[length]):
            base = (t.first[length] + k) << (16 - length)
            look[base:base + (1 << (16 - length))] = length << 8 | t.values[t.index[length] + k]
    _look_cache[key] = look.tolist()
    return _look_cache[key]


class _Geometry:
    """What a lane needs of the header: the slots of an MCU, their components and tables, and where a block goes."""

    def __init__(self, hd: _Header):
        nf = len(hd.ids)
        self.nf, self.h, self.v, self.mcus_x, self.n_mcu = nf, hd.h[0], hd.v[0], hd.mcus_x, hd.mcus_x * hd.mcus_y
        self.comp = [0] * (self.h * self.v) + [1, 2] if nf == 3 else [0]
        self.nslots = len(self.comp)
        cache = {}
        self.dc = [cache.setdefault(("dc", hd.td[c]), _look16(hd.dc[hd.td[c]])) for c in range(nf)]
        self.ac = [cache.setdefault(("ac", hd.ta[c]), _look16(hd.ac[hd.ta[c]])) for c in range(nf)]
        self.blocks_w = list(hd.blocks_w)
        sizes = [hd.blocks_w[c] * hd.blocks_h[c] for c in range(nf)]
        self.comp_first = [sum(sizes[:c]) for c in range(nf)]
        self.total_blocks = sum(sizes)

    def block(self, first_mcu: int, ordinal: int, slot: int) -> int:
        """The component-major, row-major index of the block with this ordinal in its segment."""
        my, mx = divmod(first_mcu + ordinal // self.nslots, self.mcus_x)
        c = self.comp[slot]
        j, i = divmod(slot, self.h) if c == 0 else (0, 0)
        hc, vc = (self.h, self.v) if c == 0 else (1, 1)
        return self.comp_first[c] + (my * vc + j) * self.blocks_w[c] + mx * hc + i


_ERR, _DC, _ZEROS, _AC, _END = range(5)


def _decode(buf: bytes, L: int, state, end: int, g: _Geometry, ev):
    """Symbols from `state` = (bit position, slot, z) until the position reaches `end` or the segment's end `L`; the exit state.  Bits
    past L read as zero.  A code in no table, a DC size above 15 or an index past 63: advance one bit, z = 0.  `ev` takes what was
    decoded: (_DC, slot, difference, position behind), (_ZEROS, z from, z to, position behind), (_AC, z, value, position behind),
    (_END, position behind) when a block is complete, (_ERR,)."""
    p, slot, z = state
    stop = min(end, L)
    comp, nslots = g.comp, g.nslots
    while p < stop:
        at = p >> 3
        w = (int.from_bytes(buf[at:at + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
        if p + 32 > L:
            w &= ~(0xFFFFFFFF >> (L - p))
        c = comp[slot]
        if z == 0:
            e = g.dc[c][w >> 16]
            n, t = e >> 8, e & 255
            if e == 0 or t > 15:
                if ev is not None:
                    ev.append((_ERR,))
                p += 1
                continue
            v = ((w << n) & 0xFFFFFFFF) >> (32 - t) if t else 0
            p += n + t
            z = 1
            if ev is not None:
                ev.append((_DC, slot, v if t == 0 or v >= 1 << (t - 1) else v - (1 << t) + 1, p))
            continue
        e = g.ac[c][w >> 16]
        n, r, s = e >> 8, (e >> 4) & 15, e & 15
        if e == 0 or z + r > (63 if s else 62 if r == 15 else 99):    # no code | an index past 63, a ZRL that runs past it included
            if ev is not None:
                ev.append((_ERR,))
            p += 1
            z = 0
            continue
        if s == 0:
            p += n
            if r == 15:                                 # ZRL: sixteen zeros, a coefficient follows
                if ev is not None:
                    ev.append((_ZEROS, z, z + 16, p))
                z += 16
                continue
            if ev is not None:                          # EOB: zeros to the end of the block
                ev.append((_ZEROS, z, 64, p))
            z = 64
        else:
            v = ((w << n) & 0xFFFFFFFF) >> (32 - s)
            p += n + s
            if ev is not None:
                if r:
                    ev.append((_ZEROS, z, z + r, p))
                ev.append((_AC, z + r, v if v >= 1 << (s - 1) else v - (1 << s) + 1, p))
            z += r + 1
        if z == 64:
            z = 0
            slot = slot + 1 if slot + 1 < nslots else 0
            if ev is not None:
                ev.append((_END, p))
    return p, slot, z


def jpeg_entropy_parallel_host(data: bytes, subsequence_bytes: int = 128, lanes: int = 256):
    """The contract of `fear_jpeg_huffman`: (header, coefficients per component as jpeg_coefficients_host returns them, status, rounds).
    `status` is 0 or ERR_FORMAT; a header or restart-marker fault raises as `_parse` and `jpeg_scan_prepare_host` do, before any decoding.
    `rounds` lists, per sequence, how many synchronisation rounds ran (the first, every lane on its own subsequence, included).  The
    coefficients of a file whose status is not 0 are unspecified."""
    if subsequence_bytes % 4 or not 4 <= subsequence_bytes <= 1024 or lanes < 1:
        raise ValueError("subsequence_bytes is a multiple of 4 in 4..1024")
    data = bytes(data)
    hd = _parse(data)
    stream, seg_start = jpeg_scan_prepare_host(data, hd)
    g = _Geometry(hd)
    dense = np.zeros(64 * g.total_blocks, dtype=np.int16)
    writes = np.zeros(64 * g.total_blocks, dtype=np.uint8)
    SB, status, rounds = 8 * subsequence_bytes, 0, []
    per_segment = (hd.restart if hd.restart else g.n_mcu)
    for s in range(len(seg_start) - 1):
        buf = stream[seg_start[s]:seg_start[s + 1]] + bytes(8)
        L = 8 * (seg_start[s + 1] - seg_start[s])
        first_mcu = s * per_segment
        expected = min(per_segment, g.n_mcu - first_mcu) * g.nslots
        last_segment = s == len(seg_start) - 2
        n_sub = -(-L // SB)
        carry, begun, pred = (0, 0, 0), 0, [0, 0, 0]
        for q in range(0, n_sub, lanes):
            m = min(lanes, n_sub - q)                                   # the lanes with a subsequence inside the segment
            # synchronisation: lane 0 holds the true state, the others guess; stored[j] is the exit of subsequence q + j
            carried = [carry] + [((q + i) * SB, 0, 0) for i in range(1, m)]
            carried = [_decode(buf, L, carried[i], (q + i + 1) * SB, g, None) for i in range(m)]
            stored, active, r = list(carried), [True] * m, 1
            while r < lanes and any(active):
                for i in range(m):
                    j = i + r
                    if not active[i]:
                        continue
                    if j >= m:
                        active[i] = False
                        continue
                    out = _decode(buf, L, carried[i], (q + j + 1) * SB, g, None)
                    if out == stored[j]:
                        active[i] = False
                    else:
                        stored[j] = carried[i] = out
                r += 1
            rounds.append(r)
            entry = [carry] + stored[:m - 1]
            # count and write.  The kernel decodes twice more: once to count the blocks that begin in each subsequence and to sum its DC
            # differences, and, after an exclusive prefix over the lanes, once to write.  Walking the lanes in order is that prefix.
            for i in range(m):
                ev = []
                out = _decode(buf, L, entry[i], (q + i + 1) * SB, g, ev)
                assert out == stored[i]
                slot, is_open = entry[i][1], entry[i][2] != 0            # a block begun in an earlier subsequence is still open
                for e in ev:
                    kind = e[0]
                    if kind == _ERR:
                        if begun - is_open < expected:                   # in the open block, or in the one that would begin here
                            status = ERR_FORMAT
                        is_open = False
                        continue
                    if kind == _END:
                        is_open = False
                        if begun == expected and not last_segment and L - e[1] >= 8:
                            status = ERR_FORMAT                          # whole bytes in front of the marker: Bits::restart
                        continue
                    if kind == _DC:
                        slot, c = e[1], g.comp[e[1]]
                        pred[c] = (pred[c] + e[2]) & 0xFFFF              # JCOEF is 16 bits wide
                        begun, is_open = begun + 1, True
                        z0, z1, value = 0, 1, pred[c] - 0x10000 if pred[c] >= 0x8000 else pred[c]
                    elif kind == _ZEROS:
                        z0, z1, value = e[1], e[2], 0
                    else:
                        z0, z1, value = e[1], e[1] + 1, e[2]
                    if 1 <= begun <= expected:                           # blocks past the segment's count are dropped
                        if e[-1] > L:                                    # the symbol or its magnitude bits run past the segment
                            status = ERR_FORMAT
                        b = g.block(first_mcu, begun - 1, slot)
                        if b < g.total_blocks:
                            dense[64 * b + z0:64 * b + z1] = value
                            writes[64 * b + z0:64 * b + z1] += 1
            carry = stored[m - 1]
        if begun - (carry[2] != 0) < expected:                           # fewer complete blocks than the segment owes
            status = ERR_FORMAT
    if status == 0:
        assert np.all(writes == 1), "every position of every block is written exactly once"
    coef, at = [], 0
    for c in range(g.nf):
        size = hd.blocks_w[c] * hd.blocks_h[c]
        coef.append(dense[64 * at:64 * (at + size)].reshape(hd.blocks_h[c], hd.blocks_w[c], 64))
        at += size
    return hd, coef, status, rounds


# ------------------------------------------------------------------------------------------------------- the index of a resident scan
# One entry per subsequence, 16 bytes: include/fear_train.h FearJpegSubseq.  `p` is the true entry bit position in the segment (it may
# lie up to 30 bits behind the subsequence's first bit: the last symbol of the subsequence in front ends there), `sz` is slot << 8 | z,
# `begun` the blocks begun in the segment in front of the subsequence, `dc` the three predictors at its entry modulo 2^16 — the JhState
# and JhLane with which the write pass of jpeg_huffman_kernel starts the lane.
SUBSEQ_DTYPE = np.dtype([("p", "<u4"), ("begun", "<u4"), ("sz", "<u2"), ("dc", "<u2", (3,))])
assert SUBSEQ_DTYPE.itemsize == 16


def scan_sub_start(seg_start, subsequence_bytes: int) -> np.ndarray:
    """uint32 [n_seg + 1]: segment s owns the subsequences sub_start[s] .. sub_start[s + 1]) of its image, ceil(bytes / subsequence_bytes)
    of them."""
    seg = np.asarray(seg_start, dtype=np.int64)
    out = np.zeros(seg.size, dtype=np.uint32)
    np.cumsum(-(-(seg[1:] - seg[:-1]) // int(subsequence_bytes)), out=out[1:])
    return out


def stage_range_host(seg_start, sub_start, sub_first: int, sub_count: int, subsequence_bytes: int) -> Tuple[int, int]:
    """The contract of `fear_jpeg_stage_range` (csrc/fear_jpeg_store.h: ji_stage_range): the bytes byte0 .. byte1) of a prepared scan
    that its subsequences sub_first .. sub_first + sub_count) cover, which a workgroup of the staged kernels copies into LDS.
    Consecutive subsequences are consecutive bytes, across segments too (an empty segment owns none), so it is one range: from the
    first subsequence's first byte to the last one's end, which is its segment's end where the segment ends inside it.  Each of the
    two lies in the last segment that starts at or in front of it.  (0, 0) for sub_count == 0."""
    seg, sub = np.asarray(seg_start, dtype=np.int64), np.asarray(sub_start, dtype=np.int64)
    if sub_count <= 0 or seg.size < 2:
        return 0, 0
    first, last = int(sub_first), int(sub_first) + int(sub_count) - 1
    s0, s1 = (min(int(np.searchsorted(sub, x, side="right")) - 1, seg.size - 2) for x in (first, last))
    lo = int(seg[s0]) + (first - int(sub[s0])) * int(subsequence_bytes)
    hi = min(int(seg[s1]) + (last - int(sub[s1]) + 1) * int(subsequence_bytes), int(seg[s1 + 1]), int(seg[-1]))
    return (lo, hi) if 0 <= lo < hi else (0, 0)


class _Segment:
    """What a lane of the write pass knows of its segment (JhSegment)."""

    def __init__(self, hd: _Header, g: _Geometry, stream: bytes, seg_start, s: int):
        per_segment = hd.restart if hd.restart else g.n_mcu
        self.buf = stream[seg_start[s]:seg_start[s + 1]] + bytes(8)
        self.L = 8 * (seg_start[s + 1] - seg_start[s])
        self.first_mcu = s * per_segment
        self.expected = min(per_segment, g.n_mcu - self.first_mcu) * g.nslots
        self.last = s == len(seg_start) - 2


def _write_pass(sg: _Segment, g: _Geometry, entry, end: int, begun: int, pred: list, dense, writes, record=None):
    """One lane of the write pass: decode from the true `entry` = (p, slot, z) to `end`, `begun` blocks of the segment begun in front
    and `pred` the predictors (updated in place).  Stores what it decodes in `dense` (the whole image's layout; None stores nothing),
    judges it, and returns (exit state, begun, failed).  `record`, a list, takes every store the lane makes, for `_place` to put in any
    layout: (MCU, slot, z from, z to, value)."""
    ev, failed = [], False
    out = _decode(sg.buf, sg.L, entry, end, g, ev)
    slot, is_open = entry[1], entry[2] != 0                              # a block begun in an earlier subsequence is still open
    for e in ev:
        kind = e[0]
        if kind == _ERR:
            if begun - is_open < sg.expected:                            # in the open block, or in the one that would begin here
                failed = True
            is_open = False
            continue
        if kind == _END:
            is_open = False
            if begun == sg.expected and not sg.last and sg.L - e[1] >= 8:
                failed = True                                            # whole bytes in front of the marker: Bits::restart
            continue
        if kind == _DC:
            slot, c = e[1], g.comp[e[1]]
            pred[c] = (pred[c] + e[2]) & 0xFFFF                          # JCOEF is 16 bits wide
            begun, is_open = begun + 1, True
            z0, z1, value = 0, 1, pred[c] - 0x10000 if pred[c] >= 0x8000 else pred[c]
        elif kind == _ZEROS:
            z0, z1, value = e[1], e[2], 0
        else:
            z0, z1, value = e[1], e[1] + 1, e[2]
        if 1 <= begun <= sg.expected:                                    # blocks past the segment's count are dropped
            if e[-1] > sg.L:                                             # the symbol or its magnitude bits run past the segment
                failed = True
            if record is not None:
                record.append((sg.first_mcu + (begun - 1) // g.nslots, slot, z0, z1, value))
            if dense is not None:
                b = g.block(sg.first_mcu, begun - 1, slot)
                if b < g.total_blocks:
                    dense[64 * b + z0:64 * b + z1] = value
                    writes[64 * b + z0:64 * b + z1] += 1
    return out, begun, failed


def _check_subsequence_bytes(subsequence_bytes: int) -> None:
    if subsequence_bytes % 4 or not 4 <= subsequence_bytes <= 1024:
        raise ValueError("subsequence_bytes is a multiple of 4 in 4..1024")


def jpeg_scan_index_host(data: bytes, subsequence_bytes: int = 128):
    """The contract of `fear_jpeg_index_build`: (header, sub_start, index, status).  Subsequences are numbered per image, segment after
    segment; `index[sub_start[s] + i]` is the true entry of subsequence i of segment s (SUBSEQ_DTYPE); `status` is
    `jpeg_entropy_parallel_host`'s verdict, judged on the way.  What the kernel finds by synchronising, counting and a prefix, the
    sequential walk here finds directly: the true chain is the same."""
    _check_subsequence_bytes(subsequence_bytes)
    data = bytes(data)
    hd = _parse(data)
    stream, seg_start = jpeg_scan_prepare_host(data, hd)
    g = _Geometry(hd)
    SB, status = 8 * subsequence_bytes, 0
    sub_start = scan_sub_start(seg_start, subsequence_bytes)
    index = np.zeros(int(sub_start[-1]), dtype=SUBSEQ_DTYPE)
    for s in range(len(seg_start) - 1):
        sg = _Segment(hd, g, stream, seg_start, s)
        state, begun, pred = (0, 0, 0), 0, [0, 0, 0]
        for i in range(-(-sg.L // SB)):
            index[int(sub_start[s]) + i] = (state[0], begun, state[1] << 8 | state[2], tuple(pred))
            state, begun, failed = _write_pass(sg, g, state, (i + 1) * SB, begun, pred, None, None)
            if failed:
                status = ERR_FORMAT
        if begun - (state[2] != 0) < sg.expected:                        # fewer complete blocks than the segment owes
            status = ERR_FORMAT
    return hd, sub_start, index, status


def scan_row_sub(header: _Header, sub_start, index) -> np.ndarray:
    """uint32 [mcus_y + 1], the row table of a resident scan: row_sub[r] is the image-numbered subsequence in which the first block of
    MCU row r begins — the last subsequence of that block's restart segment whose entry has `begun` less than or equal to the block's
    ordinal in the segment (the entries of a segment count the blocks begun in front of them, so the block begins in that subsequence
    and no later one) — and row_sub[mcus_y] = n_sub.  The blocks of the MCU rows a .. b) then lie wholly in the subsequences
    row_sub[a] .. min(row_sub[b], n_sub - 1): the last block of row b - 1 ends where the first of row b begins, or with its segment.
    From the index `fear_jpeg_index_build` wrote, `sub_start`, the restart interval, mcus_x and the slots per MCU; no loop over rows."""
    sub_start = np.asarray(sub_start, dtype=np.int64)
    n_seg, n_sub = sub_start.size - 1, int(sub_start[-1])
    assert len(index) == n_sub
    nslots = 1 if len(header.ids) == 1 else header.h[0] * header.v[0] + 2
    n_mcu = header.mcus_x * header.mcus_y
    interval = header.restart if header.restart else n_mcu
    mcu = np.arange(header.mcus_y, dtype=np.int64) * header.mcus_x
    seg = np.minimum(mcu // interval, n_seg - 1)
    ordinal = (mcu - seg * interval) * nslots
    # (segment, begun) is non-decreasing over an image's subsequences: one search for all rows
    of_sub = np.searchsorted(sub_start[1:], np.arange(n_sub), side="right")
    key = (of_sub.astype(np.int64) << 32) | np.asarray(index["begun"], dtype=np.int64)
    at = np.searchsorted(key, (seg << 32) | ordinal, side="right") - 1
    at = np.minimum(np.maximum(at, sub_start[seg]), n_sub)                     # (a segment without a subsequence: its place)
    return np.concatenate([at, [n_sub]]).astype(np.uint32)


def window_lanes(header: _Header, sub_start, index, lanes, cols) -> np.ndarray:
    """The lanes of `lanes` (image-numbered subsequences, a band's) that `fear_jpeg_huffman_indexed_windows` runs for the MCU columns
    cols = (c0, c1), clipped to mcus_x: int64, in order.  A lane knows its own entry and the next subsequence's, or its segment's block
    count where the next subsequence lies in another segment (or nowhere).  The blocks it stores have the segment ordinals lo .. hi):
    lo = begun - (1 if a block is open at its entry), hi = min(the next begun, the segment's count).  Their MCUs are the consecutive
    first_mcu + lo // nslots .. first_mcu + (hi - 1) // nslots, and the lane runs if one of them has its column in [c0, c1): `count`
    MCUs from column x_lo cover every column when count >= mcus_x, else the columns x_lo .. x_lo + count - 1, of which the part past
    mcus_x - 1 wraps to the next row's first columns.  The rows play no part: the rule may run a lane that stores nothing, never the
    reverse.  Arithmetic on loaded values alone — no loop over blocks, no bound that depends on the data."""
    sub_start = np.asarray(sub_start, dtype=np.int64)
    n_seg, n_sub = sub_start.size - 1, int(sub_start[-1])
    lanes = np.asarray(lanes, dtype=np.int64).reshape(-1)
    mcus_x = int(header.mcus_x)
    c0 = min(max(int(cols[0]), 0), mcus_x)
    c1 = min(max(int(cols[1]), c0), mcus_x)
    if lanes.size == 0 or c1 == c0:
        return np.zeros(0, dtype=np.int64)
    nslots = 1 if len(header.ids) == 1 else header.h[0] * header.v[0] + 2
    n_mcu = mcus_x * header.mcus_y
    interval = header.restart if header.restart else n_mcu
    seg = np.searchsorted(sub_start[:n_seg], lanes, side="right") - 1
    first_mcu = np.minimum(seg * interval, n_mcu)
    expected = np.minimum(interval, n_mcu - first_mcu) * nslots
    begun, z = np.asarray(index["begun"], dtype=np.int64), np.asarray(index["sz"], dtype=np.int64) & 255
    inside = (lanes + 1 < sub_start[seg + 1]) & (lanes + 1 < n_sub)
    next_begun = np.where(inside, begun[np.minimum(lanes + 1, n_sub - 1)], expected)
    lo = begun[lanes] - ((z[lanes] != 0) & (begun[lanes] > 0))
    hi = np.minimum(next_begun, expected)
    some = hi > lo
    m_lo = first_mcu + lo // nslots
    count = np.where(some, (hi - 1) // nslots - lo // nslots + 1, 0)
    x_lo = m_lo % mcus_x
    x_end = x_lo + count - 1
    touches = (count >= mcus_x) | ((x_lo < c1) & (x_end >= c0)) | ((x_end >= mcus_x) & (x_end - mcus_x >= c0))
    return lanes[some & touches]


def _record_lanes(data: bytes, sub_start, index, subsequence_bytes: int, row_sub=None, lanes=None):
    """The lanes `lanes` of the indexed decode (image-numbered subsequences, run in that order; every one by default), each once and
    whatever band is wanted (a lane's decode does not depend on it), as one lane of jpeg_huffman_indexed_kernel does it: the segment by
    a search of `sub_start`, the write pass's rules, and the verdict — the lane of a segment's last subsequence judges the segment's
    block count, the lane of its first an empty segment in front, the lane of the image's last subsequence empty segments behind.
    Returns the header, the geometry, n_sub, the row table, each subsequence's verdict (False where its lane did not run), and every
    store the lanes made, in the order they made them, one array entry per coefficient position — the lane, the MCU row and column,
    the slot, z and the value."""
    _check_subsequence_bytes(subsequence_bytes)
    data = bytes(data)
    hd = _parse(data)
    stream, seg_start = jpeg_scan_prepare_host(data, hd)
    g = _Geometry(hd)
    n_seg, n_sub, SB = len(seg_start) - 1, len(index), 8 * subsequence_bytes
    sub_start = np.asarray(sub_start, dtype=np.int64)
    assert sub_start.size == n_seg + 1 and int(sub_start[-1]) == n_sub
    if row_sub is None:
        row_sub = scan_row_sub(hd, sub_start, index)
    segs = [_Segment(hd, g, stream, seg_start, s) for s in range(n_seg)]
    lane_failed = np.zeros(n_sub, dtype=bool)
    lane_of, stores = [], []
    for sub in (range(n_sub) if lanes is None else lanes):
        sub = int(sub)
        s = int(np.searchsorted(sub_start[:n_seg], sub, side="right")) - 1   # the last segment that starts at or in front of `sub`
        sg, i, e = segs[s], sub - int(sub_start[s]), index[sub]
        slot, z = min(int(e["sz"]) >> 8, g.nslots - 1), min(int(e["sz"]) & 255, 63)
        made = []
        state, begun, failed = _write_pass(sg, g, (int(e["p"]), slot, z), (i + 1) * SB, int(e["begun"]), [int(v) for v in e["dc"]], None, None,
                                           record=made)
        if (i + 1) * SB >= sg.L and begun - (state[2] != 0) < sg.expected:    # the segment's last subsequence: its block count
            failed = True
        if i == 0 and s > 0 and sub_start[s - 1] == sub_start[s]:            # an empty segment in front owes blocks
            failed = True
        if sub == n_sub - 1 and s != n_seg - 1:                              # empty segments behind the last subsequence
            failed = True
        lane_failed[sub] = failed
        lane_of += [sub] * len(made)
        stores += made
    mcu, slot, z0, z1, value = np.array(stores, dtype=np.int64).reshape(-1, 5).T
    each = z1 - z0                                                           # a store of z0 .. z1) is one entry per position
    z_of = np.arange(int(each.sum())) - np.repeat(np.cumsum(each) - each - z0, each)
    lane_of, mcu, slot, value = (np.repeat(np.asarray(v, dtype=np.int64), each) for v in (lane_of, mcu, slot, value))
    return hd, g, n_sub, row_sub, lane_failed, (lane_of, mcu // g.mcus_x, mcu % g.mcus_x, slot, z_of, value.astype(np.int16))


def _clipped(pair, count: int):
    """(lo, hi) of `pair` clipped to 0 .. count, hi at least lo."""
    lo = min(max(int(pair[0]), 0), count)
    return lo, min(max(int(pair[1]), lo), count)


def _band_lanes(row_sub, band, n_sub: int) -> range:
    """The lanes of the MCU rows band = (a, b): the subsequences row_sub[a] .. min(row_sub[b], n_sub - 1), none for the empty band."""
    a, b = band
    return range(int(row_sub[a]), min(int(row_sub[b]), n_sub - 1) + 1) if b > a else range(0)


def _status(n_sub: int, lane_failed, lanes) -> int:
    """The verdict of the lanes that ran; an image without a subsequence fails."""
    return ERR_FORMAT if n_sub == 0 or bool(lane_failed[np.asarray(lanes, dtype=np.int64)].any()) else 0


def _place(g: _Geometry, stores, lanes=None, band=None, cols=None, own: bool = True):
    """Where every recorded store goes: (coefficients, write counts), both per component as (blocks high, blocks wide, 64), int16 and
    int64, zero where nothing was stored.  Of `stores` (`_record_lanes`') those of the range `lanes` (of every lane's stores in the
    natural order; None takes whatever lanes ran) whose MCU row passes the explicit range test of `band` = (a, b) and whose MCU
    column that of `cols` = (c0, c1) are stored (None: every row, every column).  The layout is one of three.  `own`: an image that consists of the band's rows and the columns alone, luma first —
    what jh_band_base and jh_window_base address.  Not `own`, with a band: the whole image, of which only the band's blocks are
    stored — jh_rows_base.  Not `own`, without one: the whole image in full, which is also `own` of every row and column — what
    `_Geometry.block` addresses.  A position that several stores reach holds the last one's value."""
    if lanes is not None:                                                    # (recorded in the natural order: a slice)
        first, last = np.searchsorted(stores[0], (lanes.start, lanes.stop))
        stores = [v[first:last] for v in stores]
    lane_of, my, mx, slot_of, z_of, value_of = stores
    mcus_y = g.n_mcu // g.mcus_x
    (a, b), (c0, c1) = band or (0, mcus_y), cols or (0, g.mcus_x)
    keep = (my >= a) & (my < b) & (mx >= c0) & (mx < c1)
    row0, rows, col0, wide = (a, b - a, c0, c1 - c0) if own else (0, mcus_y, 0, g.mcus_x)
    # per slot of an MCU: the block of the image's first MCU, and the blocks from an MCU to the one below it and to its right
    slots, comp, mcus = np.arange(g.nslots), np.array(g.comp, dtype=np.int64), rows * wide
    origin = np.where(comp == 0, slots // g.h * (wide * g.h) + slots % g.h, mcus * g.h * g.v + (comp - 1) * mcus)
    down, right = np.where(comp == 0, g.v * wide * g.h, wide), np.where(comp == 0, g.h, 1)
    at = (64 * (origin[slot_of] + (my - row0) * down[slot_of] + (mx - col0) * right[slot_of]) + z_of)[keep]
    dense = np.zeros(64 * mcus * g.nslots, dtype=np.int16)
    dense[at] = value_of[keep]
    writes = np.bincount(at, minlength=dense.size)
    out, first = ([], []), 0
    for c in range(g.nf):
        high, across = rows * (g.v if c == 0 else 1), wide * (g.h if c == 0 else 1)
        for flat, split in zip((dense, writes), out):
            split.append(flat[64 * first:64 * (first + high * across)].reshape(high, across, 64))
        first += high * across
    return out


def jpeg_entropy_indexed_host(data: bytes, sub_start, index, subsequence_bytes: int, order=None, band=None, row_sub=None, cols=None):
    """The contract of `fear_jpeg_huffman_indexed`: (coefficients per component, status).  Every subsequence is decoded from its index
    entry alone, in `order` (any permutation of the image's subsequences; the natural one by default), as `_record_lanes` states a lane
    of jpeg_huffman_indexed_kernel and its verdict, and an image without a subsequence fails.  Asserts that every position is written
    exactly once when the status is 0.
    With `band` = (a, b), MCU rows a .. b) clipped to the image, it is the contract of `fear_jpeg_huffman_indexed_rows`: only the
    subsequences row_sub[a] .. min(row_sub[b], n_sub - 1) are decoded (`row_sub` is `scan_row_sub`'s table, computed when None; `order`
    permutes those), only the blocks of the band's rows are stored, and the coefficients are the band's: per component the rows of an
    image that consists of those MCU rows alone.  Lanes that do not run judge nothing.
    With `band` and `cols` = (c0, c1), MCU columns c0 .. c1) clipped to the image, it is the contract of
    `fear_jpeg_huffman_indexed_windows`: of the band's lanes only those `window_lanes` names run (a lane all of whose MCUs lie outside
    the columns returns before it judges anything; `order` permutes the lanes that run), a block is stored only when its MCU row is in
    the band and its MCU column in the range, and the coefficients are the window's: per component the blocks of an image made of those
    (b - a) x (c1 - c0) MCUs alone."""
    _check_subsequence_bytes(subsequence_bytes)
    hd = _parse(bytes(data))
    if cols is not None and band is None:
        raise ValueError("cols go with a band")
    lanes = range(len(index))
    if band is not None:
        band = _clipped(band, hd.mcus_y)
        if row_sub is None:
            row_sub = scan_row_sub(hd, sub_start, index)
        lanes = _band_lanes(row_sub, band, len(index))
    if cols is not None:
        cols = _clipped(cols, hd.mcus_x)
        lanes = window_lanes(hd, sub_start, index, np.arange(lanes.start, lanes.stop), cols).tolist()
    if order is not None:
        lanes = [lanes[int(k)] for k in order]
    hd, g, n_sub, row_sub, lane_failed, stores = _record_lanes(data, sub_start, index, subsequence_bytes, row_sub, lanes)
    coef, writes = _place(g, stores, None, band, cols)
    status = _status(n_sub, lane_failed, lanes)
    if status == 0:
        assert all(np.all(w == 1) for w in writes), "every position of every block is written exactly once"
    return coef, status


def jpeg_entropy_bands_host(data: bytes, sub_start, index, subsequence_bytes: int, bands, row_sub=None):
    """`jpeg_entropy_indexed_host(..., band=(a, b))` for many bands of one file at once: [(coefficients per component, status)] in the
    order of `bands`.  Every lane decodes and judges once, whatever the band (its decode does not depend on it), and records what it
    would store; per band the stores of the lanes that run, row_sub[a] .. min(row_sub[b], n_sub - 1), whose MCU row passes the explicit
    range test a <= row < b are placed band-dense, and the lanes that do not run judge nothing.  Asserts that every position of a band
    is written exactly once when its status is 0."""
    hd, g, n_sub, row_sub, lane_failed, stores = _record_lanes(data, sub_start, index, subsequence_bytes, row_sub)
    out = []
    for band in bands:
        band = _clipped(band, hd.mcus_y)
        lanes = _band_lanes(row_sub, band, n_sub)
        coef, writes = _place(g, stores, lanes, band)
        status = _status(n_sub, lane_failed, lanes)
        if status == 0:
            assert all(np.all(w == 1) for w in writes), "every position of the band is written exactly once"
        out.append((coef, status))
    return out


# -------------------------------------------------------------------------------------------------- the band of rows taken from the device
def rows_band(y0: int, y1: int, limit: int, mcu_h: int, mcus_y: int, halo: bool):
    """The band of MCU rows (a, b) that covers the pixel rows [y0, y1) clipped to [0, limit], one MCU row more on each side with `halo`,
    clipped to mcus_y; None for the empty band y0 >= y1 (jr_band in csrc/fear_jpeg_decode.h; `jpeg_store._cover` states the same rule over arrays, for the host's plans)."""
    y0, y1 = min(max(int(y0), 0), limit), min(max(int(y1), 0), limit)
    if y0 >= y1:
        return None
    a, b = max(y0 // mcu_h - bool(halo), 0), min(-(-y1 // mcu_h) + bool(halo), mcus_y)
    return (a, b) if a < b else None


def jpeg_entropy_rows_device_many_host(data: bytes, sub_start, index, subsequence_bytes: int, windows, row_sub=None):
    """The contract of `fear_jpeg_huffman_indexed_rows_dev` for many windows [y0, y1) of one file: per window
    (lanes, coefficients, mask, status).  The band is `rows_band` with the rows of the MCU grid as the limit (the resident record does
    not hold the height) and the halo where v == 2; `lanes` is the range of subsequences that run, row_sub[a] .. min(row_sub[b],
    n_sub - 1), empty for the empty band; `coefficients` are per component in the FULL-IMAGE layout, as `jpeg_coefficients_host` returns
    them, zero where nothing was stored; `mask` has their shapes and counts the stores to each position: 1 on the band's blocks, 0
    elsewhere.  A lane that runs decodes and judges as `jpeg_entropy_indexed_host`'s, a block whose MCU row lies outside the band (an
    explicit range test) is not stored, and lanes that do not run judge nothing."""
    hd, g, n_sub, row_sub, lane_failed, stores = _record_lanes(data, sub_start, index, subsequence_bytes, row_sub)
    mcu_h, out = 8 * g.v, []
    for y0, y1 in windows:
        band = rows_band(y0, y1, mcu_h * hd.mcus_y, mcu_h, hd.mcus_y, g.v == 2) or (0, 0)
        lanes = _band_lanes(row_sub, band, n_sub)
        coef, mask = _place(g, stores, lanes, band, own=False)
        out.append((lanes, coef, mask, _status(n_sub, lane_failed, lanes)))
    return out


def jpeg_entropy_rows_device_host(data: bytes, sub_start, index, subsequence_bytes: int, y0: int, y1: int, row_sub=None):
    """`jpeg_entropy_rows_device_many_host` for one window: (lanes, coefficients, mask, status)."""
    return jpeg_entropy_rows_device_many_host(data, sub_start, index, subsequence_bytes, [(y0, y1)], row_sub)[0]


def jpeg_rows_device_host(data: bytes, y0: int, y1: int, subsequence_bytes: int = 128, fill=None):
    """The contract of `JpegStore.decode_rows(ids, rows)` with `rows` on the device, for one file and one window: (lanes, coefficients,
    mask, frame).  The index is `jpeg_scan_index_host`'s; lanes, coefficients and mask are `jpeg_entropy_rows_device_host`'s; `frame` is
    uint8 (H, W, 3) of which the rows [y0, y1) clipped to [0, H] are defined — `fear_jpeg_decode_u8_rows_dev` on those coefficients: the
    pixel stage of the whole image, in which the positions that were never stored hold `fill` (an int16 array of 64 total_blocks values:
    what the buffer held; zeros by default) — and all other rows are zero here and unspecified on the device.  Whatever `fill` holds, the
    defined rows are `jpeg_decode_host`'s: their luma lies in the band without its halo and their chroma rows in the band with it."""
    from .jpeg_frames import jpeg_pixels_host
    hd, sub_start, index, status = jpeg_scan_index_host(data, subsequence_bytes)
    if status != 0:
        raise MalformedJPEG("the scan does not decode")
    lanes, coef, mask, status = jpeg_entropy_rows_device_host(data, sub_start, index, subsequence_bytes, y0, y1)
    if fill is not None:
        fill, at = np.asarray(fill, dtype=np.int16).reshape(-1), 0
        held = []
        for c, m in zip(coef, mask):
            held.append(np.where(m > 0, c, fill[at:at + c.size].reshape(c.shape)))
            at += c.size
    else:
        held = coef
    frame = np.zeros((hd.height, hd.width, 3), dtype=np.uint8)
    lo, hi = min(max(int(y0), 0), hd.height), min(max(int(y1), 0), hd.height)
    if lo < hi:
        frame[lo:hi] = jpeg_pixels_host(hd, held)[lo:hi]
    return lanes, coef, mask, frame
