"""Baseline JPEG files written from uint8 RGB frames ("Writing JPEG files").

`jpeg_encode_host` is the contract: numpy and plain Python that produce, byte for byte, the file libjpeg writes with its defaults for a
three-component frame (`PIL.Image.fromarray(rgb).save(f, "JPEG", quality=q)`): baseline SOF0, 4:2:0, islow FDCT, the standard Huffman
tables of T.81 annex K, optionally a restart interval of whole MCU rows — and, with `subsampling=`, the 4:2:2, 4:4:4 and
single-component files Pillow writes with `subsampling=1`, `subsampling=0` and for a mode-L image.  tests/test_jpeg_encode_host.py and
tests/test_jpeg_encode_modes_host.py hold it to Pillow's libjpeg-turbo.  With `optimize=True` the file is the one Pillow writes with
`optimize=True`: per-file Huffman tables, stated by `jpeg_symbol_histograms_host` and `jpeg_optimal_table_host`
(tests/test_jpeg_encode_optimize_host.py).  `JpegEncoder` is the product: `fear_jpeg_encode_u8`
(csrc/fear_jpeg_encode.h) runs every stage on the device and `PendingJpegs.result()` downloads the files' bytes alone.  `write_mjpeg_avi` puts equal-sized files into a Motion-JPEG AVI."""
from __future__ import annotations

import ctypes
import struct
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from .jpeg_frames import MAX_SIDE, ZIGZAG
from .train_data.jpeg import jpeg_fdct_islow, jpeg_quant_tables

# T.81 tables K.3 to K.6: the code counts per length 1..16 and the symbols in code order, as (class, id) of their DHT segment
STD_HUFFMAN = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
        "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
        "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
        "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
        "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
}
ENC_OVERFLOW = 1                          # include/fear_train.h FEAR_JPEG_ENC_OVERFLOW
ENC_HUFF_DEPTH = 2                        # include/fear_train.h FEAR_JPEG_ENC_HUFF_DEPTH
HUFF_MAX_DEPTH = 32                       # libjpeg's MAX_CLEN: an unlimited Huffman depth above it is refused
# The layouts a file can have, by name: include/fear_train.h's FEAR_JPEG_ENC_420 .. _GRAY, the MCU's (width, height) in pixels, the
# (horizontal, vertical) luma sampling factors and Pillow's `subsampling=` (None: a single-component file)
SUBSAMPLINGS = ("4:2:0", "4:2:2", "4:4:4", "gray")
_MODE = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "gray": 3}
_MCU = {"4:2:0": (16, 16), "4:2:2": (16, 8), "4:4:4": (8, 8), "gray": (8, 8)}
_LUMA = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1), "gray": (1, 1)}
_SLOT_FACTOR = {"4:2:0": 3, "4:2:2": 4, "4:4:4": 6, "gray": 3}


class JpegOverflow(ValueError):
    """Some files of an `encode` call did not fit their slots; `.items` lists their indexes."""

    def __init__(self, items: Sequence[int]):
        self.items = list(items)
        super().__init__(f"the JPEG files of items {self.items} exceed their slots")


class JpegHuffmanDepth(ValueError):
    """The symbol statistics of some optimised files of an `encode` call give a Huffman tree deeper than 32 before limiting, which
    libjpeg refuses (JERR_HUFF_CLEN_OVERFLOW); `.items` lists their indexes.  It is raised in preference to `JpegOverflow`: `.overflow`
    lists the items of the same call whose files exceed their slots, so that neither kind goes unnamed."""

    def __init__(self, items: Sequence[int], overflow: Sequence[int] = ()):
        self.items, self.overflow = list(items), list(overflow)
        also = f"; the files of items {self.overflow} exceed their slots" if self.overflow else ""
        super().__init__(f"the Huffman trees of items {self.items} are deeper than {HUFF_MAX_DEPTH}{also}")


def _codes(counts: Sequence[int], values: bytes):
    """Canonical codes of T.81 annex C: symbol -> (code, length)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


_STD_CODES = {key: _codes(*tab) for key, tab in STD_HUFFMAN.items()}


def _check_subsampling(subsampling) -> str:
    if not isinstance(subsampling, str) or subsampling not in _MODE:
        raise ValueError(f"subsampling is one of {', '.join(SUBSAMPLINGS)}")
    return subsampling


def _check_rgb(rgb, subsampling: str = "4:2:0") -> np.ndarray:
    v = np.asarray(rgb)
    if v.dtype != np.uint8:
        raise TypeError("a frame is uint8")
    if subsampling == "gray":
        if v.ndim != 2 and (v.ndim != 3 or v.shape[2] != 3):
            raise ValueError('a frame is (H, W) or (H, W, 3) with "gray"')
    elif v.ndim != 3 or v.shape[2] != 3:
        raise ValueError("a frame is (H, W, 3)")
    if not (1 <= v.shape[0] <= MAX_SIDE and 1 <= v.shape[1] <= MAX_SIDE):
        raise ValueError(f"a frame's sides lie in 1..{MAX_SIDE}")
    return v


def _check_quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)):
        raise TypeError("a JPEG quality is an int")
    if not 1 <= int(quality) <= 100:
        raise ValueError("a JPEG quality lies in 1..100")
    return int(quality)


def _restart_interval(restart_rows, mcus_x: int) -> int:
    if isinstance(restart_rows, bool) or not isinstance(restart_rows, (int, np.integer)):
        raise TypeError("restart_rows is an int")
    interval = int(restart_rows) * mcus_x
    if restart_rows < 0 or interval > 65535:
        raise ValueError("restart_rows is not negative and restart_rows mcus_x fits 16 bits")
    return interval


def _edge(plane: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """Replicate the last column out to `cols` columns and the last row down to `rows` rows."""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def _quantise(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(8 bh, 8 bw) samples -> (bh, bw, 64) int64 coefficients in zigzag order."""
    h, w = plane.shape
    v = jpeg_fdct_islow((plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3))
    div = (q << 3).reshape(8, 8)
    coef = np.sign(v) * ((np.abs(v) + (div >> 1)) // div)
    return coef.reshape(h // 8, w // 8, 64)[..., ZIGZAG]


def jpeg_forward_coefficients_host(rgb: np.ndarray, quality: int = 75, subsampling: str = "4:2:0") -> List[np.ndarray]:
    """The quantised coefficients libjpeg codes for an RGB frame of any size: per component (blocks_h, blocks_w, 64) int16 in zigzag
    order, padded to whole MCUs (`jpeg_coefficients_host`'s shape), the dummy blocks of the luma component included.  `subsampling`
    is the file's layout: with "gray" the frame is (H, W), or (H, W, 3) of which the luma is coded, and there is one component."""
    v = _check_rgb(rgb, _check_subsampling(subsampling))
    q_luma, q_chroma = jpeg_quant_tables(_check_quality(quality))
    H, W = v.shape[:2]
    p = v.astype(np.int64)
    by, bx = -(-H // 8), -(-W // 8)
    if p.ndim == 2:
        return [_quantise(_edge(p, 8 * by, 8 * bx), q_luma).astype(np.int16)]
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    if subsampling == "gray":
        return [_quantise(_edge(y, 8 * by, 8 * bx), q_luma).astype(np.int16)]
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling == "4:4:4":                                               # replication right and down, no dummy blocks
        return [_quantise(_edge(c, 8 * by, 8 * bx), q).astype(np.int16) for c, q in ((y, q_luma), (cb, q_chroma), (cr, q_chroma))]
    if subsampling == "4:2:2":
        mcus_x = -(-W // 16)
        luma = np.zeros((by, 2 * mcus_x, 64), dtype=np.int64)
        luma[:, :bx] = _quantise(_edge(y, 8 * by, 8 * bx), q_luma)
        if bx & 1:                                                           # Y1 of the last MCU column: the DC term of Y0, no AC terms
            luma[:, bx, 0] = luma[:, bx - 1, 0]
        out = [luma.astype(np.int16)]
        bias = np.tile(np.array([0, 1], dtype=np.int64), 4 * mcus_x)
        for c in (cb, cr):
            full = _edge(c, 8 * by, 16 * mcus_x)                             # every row and column replicated at full size
            out.append(_quantise((full[:, 0::2] + full[:, 1::2] + bias[None, :]) >> 1, q_chroma).astype(np.int16))
        return out
    mcus_y, mcus_x = -(-H // 16), -(-W // 16)
    luma = np.zeros((2 * mcus_y, 2 * mcus_x, 64), dtype=np.int64)
    luma[:by, :bx] = _quantise(_edge(y, 8 * by, 8 * bx), q_luma)
    # dummy blocks: no AC terms, the DC term of the previous block in MCU order (Y00 Y01 Y10 Y11)
    for my in range(mcus_y):
        for mx in range(mcus_x):
            order = [(2 * my, 2 * mx), (2 * my, 2 * mx + 1), (2 * my + 1, 2 * mx), (2 * my + 1, 2 * mx + 1)]
            for k in range(1, 4):
                if order[k][0] >= by or order[k][1] >= bx:
                    luma[order[k]][0] = luma[order[k - 1]][0]
    out = [luma.astype(np.int16)]
    ch, cw = -(-H // 2), 8 * mcus_x                                          # cw = 8 ceil(ceil(W / 2) / 8)
    bias = np.tile(np.array([1, 2], dtype=np.int64), cw // 2)
    for c in (cb, cr):
        full = _edge(c, 2 * ch, 2 * cw)                                      # the last row only as far as an even height
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias[None, :]) >> 2
        out.append(_quantise(_edge(down, 8 * mcus_y, cw), q_chroma).astype(np.int16))   # then the last downsampled row
    return out


def jpeg_header_host(width: int, height: int, quality: int = 75, restart_interval: int = 0, subsampling: str = "4:2:0",
                     tables=None) -> bytes:
    """Everything in front of the scan: SOI, JFIF APP0, the two DQT, SOF0, the four standard DHT, DRI if there is an interval, SOS.
    "gray" has one DQT, one component and the two luma DHT.  `tables` are per-file tables in STD_HUFFMAN's form, {(class, id): (counts,
    values)}: they take the standard ones' place, in the same order."""
    tables = STD_HUFFMAN if tables is None else tables
    gray = _check_subsampling(subsampling) == "gray"
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"a frame's sides lie in 1..{MAX_SIDE}")
    if not 0 <= restart_interval <= 65535:
        raise ValueError("a restart interval fits 16 bits")
    out = bytearray(b"\xFF\xD8\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, q in enumerate(jpeg_quant_tables(_check_quality(quality))[:1 if gray else 2]):
        out += b"\xFF\xDB\x00\x43" + bytes([t]) + bytes(int(x) for x in q[ZIGZAG])
    if gray:
        out += b"\xFF\xC0\x00\x0B\x08" + struct.pack(">HH", height, width) + b"\x01\x01\x11\x00"
    else:
        h, v = _LUMA[subsampling]
        out += b"\xFF\xC0\x00\x11\x08" + struct.pack(">HH", height, width) + bytes([3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (tc, th) in ((0, 0), (1, 0)) if gray else ((0, 0), (1, 0), (0, 1), (1, 1)):
        counts, values = tables[(tc, th)]
        if len(counts) != 16 or sum(counts) != len(values) or len(values) > 256:
            raise ValueError("a Huffman table is 16 counts and as many values as they sum to")
        out += b"\xFF\xC4" + struct.pack(">H", 19 + len(values)) + bytes([tc << 4 | th]) + bytes(int(c) for c in counts) + bytes(values)
    if restart_interval:
        out += b"\xFF\xDD\x00\x04" + struct.pack(">H", restart_interval)
    out += b"\xFF\xDA\x00\x08\x01\x01\x00\x00\x3F\x00" if gray else b"\xFF\xDA\x00\x0C\x03\x01\x00\x02\x11\x03\x11\x00\x3F\x00"
    return bytes(out)


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.have = bytearray(), 0, 0

    def put(self, value: int, count: int) -> None:
        self.acc = (self.acc << count) | (value & ((1 << count) - 1))
        self.have += count
        while self.have >= 8:
            byte = (self.acc >> (self.have - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.have -= 8
        self.acc &= (1 << self.have) - 1

    def flush(self) -> None:
        if self.have:
            self.put((1 << (8 - self.have)) - 1, 8 - self.have)             # ones up to the byte; stuffed like any other byte


def _scan_walk(coefficients: Sequence[np.ndarray], mcus_x: int, mcus_y: int, restart_interval: int, subsampling: str, symbol, extra,
               restart) -> None:
    """T.81 F.1.2's walk over one interleaved scan, an MCU's luma blocks row by row and then Cb and Cr ("gray": one block): calls
    `symbol(class, table, value)` for every Huffman symbol, `extra(value, bits)` for the bits behind it and `restart(k)` at the k-th
    restart boundary, where the DC predictions return to 0."""
    hs, vs = _LUMA[_check_subsampling(subsampling)]
    pred = [0, 0, 0]
    for mcu in range(mcus_x * mcus_y):
        if restart_interval and mcu and mcu % restart_interval == 0:
            restart(mcu // restart_interval - 1)
            pred = [0, 0, 0]
        my, mx = divmod(mcu, mcus_x)
        blocks = [(0, vs * my + j, hs * mx + i) for j in range(vs) for i in range(hs)]
        if subsampling != "gray":
            blocks += [(1, my, mx), (2, my, mx)]
        for c, j, i in blocks:
            blk = coefficients[c][j, i]
            t = 1 if c else 0
            diff = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            s = abs(diff).bit_length()
            symbol(0, t, s)
            extra(diff if diff >= 0 else diff + (1 << s) - 1, s)
            at = 0                                                          # the last coefficient coded
            for k in np.flatnonzero(blk[1:]).tolist():
                k += 1
                run, v = k - at - 1, int(blk[k])
                while run > 15:
                    symbol(1, t, 0xF0)
                    run -= 16
                s = abs(v).bit_length()
                symbol(1, t, run << 4 | s)
                extra(v if v >= 0 else v + (1 << s) - 1, s)
                at = k
            if at != 63:
                symbol(1, t, 0x00)


def jpeg_entropy_encode_host(coefficients: Sequence[np.ndarray], mcus_x: int, mcus_y: int, restart_interval: int = 0,
                             subsampling: str = "4:2:0", tables=None) -> bytes:
    """T.81 F.1.2 over one scan: the stuffed bytes between SOS and EOI, restart markers included.  The scan is interleaved, an MCU's
    luma blocks row by row and then Cb and Cr; "gray" is one component, an MCU one block.  `tables`: per-file tables in STD_HUFFMAN's
    form in place of the standard ones."""
    codes = _STD_CODES if tables is None else {key: _codes(*tab) for key, tab in tables.items()}
    w = _BitWriter()

    def restart(k: int) -> None:
        w.flush()
        w.out += bytes([0xFF, 0xD0 + (k & 7)])

    _scan_walk(coefficients, mcus_x, mcus_y, restart_interval, subsampling, lambda tc, th, v: w.put(*codes[(tc, th)][v]), w.put, restart)
    w.flush()
    return bytes(w.out)


def jpeg_symbol_histograms_host(coefficients: Sequence[np.ndarray], mcus_x: int, mcus_y: int, restart_interval: int = 0,
                                subsampling: str = "4:2:0") -> np.ndarray:
    """How often the entropy coder emits each Huffman symbol over the scan: int64 (4, 256), rows DC 0, AC 0, DC 1, AC 1 (the order of
    the file's DHT segments).  Exactly `jpeg_entropy_encode_host`'s symbols: the dummy blocks, ZRL and EOB count, and the DC differences
    start from 0 again at every restart boundary.  "gray" leaves rows 2 and 3 at 0."""
    hist = np.zeros((4, 256), dtype=np.int64)

    def symbol(tc: int, th: int, v: int) -> None:
        hist[2 * th + tc, v] += 1

    _scan_walk(coefficients, mcus_x, mcus_y, restart_interval, subsampling, symbol, lambda v, s: None, lambda k: None)
    return hist


def jpeg_optimal_table_host(freq) -> Tuple[Tuple[int, ...], bytes, int]:
    """The Huffman table libjpeg's jpeg_gen_optimal_table builds from 256 symbol counts (T.81 K.2): (the 16 counts of codes per length,
    the symbols in code order, the tree's depth before limiting).  A reserved 257th symbol of frequency 1 keeps any code from being all
    ones.  The two smallest non-zero frequencies are merged until one is left, in a tie the larger symbol number first; lengths above
    16 are brought down by Adjust_BITS; the reserved symbol leaves the longest length in use; symbols are sorted by their length in
    the tree, then by value.  A depth above 32 is refused as libjpeg refuses it: `JpegHuffmanDepth`.  Frequencies are exact integers
    of any size (libjpeg's sentinel of 10^9 is above every count a frame of the largest size can give)."""
    f = [int(x) for x in np.asarray(freq).reshape(-1)]
    if len(f) != 256 or min(f) < 0:
        raise ValueError("256 counts, none negative")
    f.append(1)
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):                                                # the smallest, the larger symbol in a tie
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1                                                       # every symbol of both subtrees is one level deeper
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2                                                     # the second subtree's chain behind the first's
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    depth = max(size)
    if depth > HUFF_MAX_DEPTH:
        raise JpegHuffmanDepth([0])
    bits = [0] * (HUFF_MAX_DEPTH + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(HUFF_MAX_DEPTH, 16, -1):                                 # Adjust_BITS: a pair of the longest codes becomes one
        while bits[i] > 0:                                                  # a bit shorter, a shorter code two codes a bit longer
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1                                                        # the reserved symbol
    values = bytes(sorted((j for j in range(256) if size[j]), key=lambda j: (size[j], j)))
    return tuple(bits[1:17]), values, depth


def jpeg_optimal_tables_host(coefficients: Sequence[np.ndarray], mcus_x: int, mcus_y: int, restart_interval: int = 0,
                             subsampling: str = "4:2:0"):
    """The per-file tables of a scan in STD_HUFFMAN's form: those of the tables the layout uses, built from its symbol counts."""
    hist = jpeg_symbol_histograms_host(coefficients, mcus_x, mcus_y, restart_interval, subsampling)
    keys = ((0, 0), (1, 0)) if subsampling == "gray" else ((0, 0), (1, 0), (0, 1), (1, 1))
    return {(tc, th): jpeg_optimal_table_host(hist[2 * th + tc])[:2] for tc, th in keys}


def jpeg_encode_host(rgb: np.ndarray, quality: int = 75, restart_rows: int = 0, subsampling: str = "4:2:0", optimize: bool = False) -> bytes:
    """A uint8 (H, W, 3) RGB frame -> the baseline JPEG file libjpeg writes for it at `quality`, with a restart marker every
    `restart_rows` MCU rows if that is not 0, in the layout `subsampling` names: Pillow's `subsampling=` 2, 1 and 0, or with "gray"
    the single-component file of an (H, W) frame, or of an (H, W, 3) frame's luma (Pillow's `convert("L")`).  `optimize`: the file of
    Pillow's `optimize=True`, whose Huffman tables are built from the scan's own symbol counts (`jpeg_optimal_table_host`).  Slow; the
    statement the device is held to."""
    v = _check_rgb(rgb, _check_subsampling(subsampling))
    H, W = v.shape[:2]
    mcu_w, mcu_h = _MCU[subsampling]
    mcus_x, mcus_y = -(-W // mcu_w), -(-H // mcu_h)
    interval = _restart_interval(restart_rows, mcus_x)
    coef = jpeg_forward_coefficients_host(v, quality, subsampling)
    tables = jpeg_optimal_tables_host(coef, mcus_x, mcus_y, interval, subsampling) if optimize else None
    return (jpeg_header_host(W, H, quality, interval, subsampling, tables)
            + jpeg_entropy_encode_host(coef, mcus_x, mcus_y, interval, subsampling, tables) + b"\xFF\xD9")


# ------------------------------------------------------------------------------------------------------------------------ the product
class PendingJpegs:
    """The files of one `JpegEncoder.encode` call, still on the device and possibly still being written.  `buffer` (uint8) holds one
    slot per item at `offsets` (int64 bytes), `lengths` (int32) the files' lengths — 0 for an item that did not fit — and `status`
    (int32) 0, ENC_OVERFLOW or ENC_HUFF_DEPTH: device tensors, ordered on the stream `encode` ran on, for consumers that stay on the device."""

    def __init__(self, buffer, offsets, lengths, status, host_offsets: Sequence[int], keep=()):
        self.buffer, self.offsets, self.lengths, self.status = buffer, offsets, lengths, status
        self._host_offsets, self._keep = list(host_offsets), keep         # (the frames and the staging buffers outlive the kernels)

    def __len__(self) -> int:
        return len(self._host_offsets)

    def result(self) -> List[bytes]:
        """Wait, download the lengths and then the used bytes alone; `JpegOverflow` names the items whose files exceed their slots,
        `JpegHuffmanDepth` those whose own Huffman trees libjpeg would refuse (and, in `.overflow`, the former, if a call has both)."""
        import torch
        n = len(self._host_offsets)
        if n == 0:
            return []
        verdict = torch.stack([self.lengths, self.status]).cpu().numpy()   # one copy, which waits for the stream
        self._keep = ()
        deep = np.flatnonzero(verdict[1] == ENC_HUFF_DEPTH)
        bad = np.flatnonzero((verdict[1] != 0) & (verdict[1] != ENC_HUFF_DEPTH))
        if deep.size:
            raise JpegHuffmanDepth([int(i) for i in deep], [int(i) for i in bad])
        if bad.size:
            raise JpegOverflow([int(i) for i in bad])
        at = np.concatenate([[0], np.cumsum(verdict[0], dtype=np.int64)])
        host = torch.empty(max(int(at[-1]), 1), dtype=torch.uint8, pin_memory=True)
        for i, off in enumerate(self._host_offsets):
            host[int(at[i]):int(at[i + 1])].copy_(self.buffer[off:off + int(verdict[0, i])], non_blocking=True)
        torch.cuda.current_stream(self.buffer.device).synchronize()
        data = host.numpy()
        return [data[int(at[i]):int(at[i + 1])].tobytes() for i in range(n)]


class JpegEncoder:
    """uint8 (H, W, 3) RGB device tensors -> baseline JPEG files, byte for byte what Pillow's `save(f, "JPEG", quality=q)` writes
    (`restart_rows=r`: what `save(..., restart_marker_rows=r)` writes).  `subsampling` names the file's layout: "4:2:0" (the default),
    "4:2:2" and "4:4:4" are Pillow's `subsampling=` 2, 1 and 0; "gray" writes a single-component file from an (H, W) tensor, or from
    the luma of an (H, W, 3) one (Pillow's `convert("L")`).  `encode` takes a name for the call or one per frame.

    `encode` builds the headers and the records on the host, uploads them from pinned memory in one non-blocking transfer and runs
    `fear_jpeg_encode_u8` once for the whole call: frames of different sizes and qualities in a fixed number of launches.  It never
    waits for the GPU.  Every file gets a slot of `slot_bytes` in one device buffer: by default 1024 + c times the frame's pixels with
    its sides padded to whole MCUs, where c is 3 for "4:2:0" and "gray", 4 for "4:2:2" and 6 for "4:4:4": a little above the raw pixels; `"bound"` takes `fear_jpeg_encode_bound`, the longest file the frame's size can give, and an int is
    the slot of every frame.  A file that exceeds its slot is not written: its length is 0 and `PendingJpegs.result()` raises
    `JpegOverflow`; the other files of the call are unaffected.  `guard_bytes` are left unused behind every slot.

    `optimize=True` writes what Pillow's `save(..., optimize=True)` writes: Huffman tables built from the file's own symbol counts, on
    the device between the transform and the size pass, so that `encode` still never waits.  `encode` takes a bool for the call or one
    per frame, and likewise `restart_rows`; optimised and plain frames mix freely in one call.  With `"bound"` an optimised frame's slot
    is `fear_jpeg_encode_bound_flags`.  An image whose Huffman tree is deeper than 32 before limiting, which libjpeg refuses, is not
    written: `result()` raises `JpegHuffmanDepth`."""

    def __init__(self, device: int = 0, quality: int = 75, restart_rows: int = 0, slot_bytes: Union[None, int, str] = None,
                 guard_bytes: int = 0, subsampling: str = "4:2:0", optimize: bool = False):
        import torch
        from .train_abi import load_train_library
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.quality = _check_quality(quality)
        self.subsampling = _check_subsampling(subsampling)
        _restart_interval(restart_rows, 1)
        self.restart_rows = int(restart_rows)
        if not isinstance(optimize, (bool, np.bool_)):
            raise TypeError("optimize is a bool")
        self.optimize = bool(optimize)
        if not (slot_bytes is None or slot_bytes == "bound" or (isinstance(slot_bytes, (int, np.integer)) and not isinstance(slot_bytes, bool))):
            raise TypeError('slot_bytes is None, "bound" or an int')
        if isinstance(slot_bytes, (int, np.integer)) and not 0 < slot_bytes < 1 << 32:
            raise ValueError("slot_bytes is positive and fits 32 bits")
        if guard_bytes < 0:
            raise ValueError("guard_bytes is not negative")
        self.slot_bytes, self.guard_bytes = slot_bytes, int(guard_bytes)
        self._lib = load_train_library()

    def _frames(self, frames, subsampling) -> Tuple[List, List[str]]:
        import torch
        if subsampling is None:
            subsampling = self.subsampling
        if not isinstance(subsampling, (str, list, tuple)):
            raise ValueError(f"subsampling is one of {', '.join(SUBSAMPLINGS)}, or a sequence of them with one per frame")
        each = None if isinstance(subsampling, str) else [_check_subsampling(m) for m in subsampling]
        if each is None:
            _check_subsampling(subsampling)
        if isinstance(frames, torch.Tensor):
            all_gray = subsampling == "gray" if each is None else all(m == "gray" for m in each)
            if frames.ndim != 4 and not (frames.ndim == 3 and all_gray):
                raise ValueError('a batch of frames is (n, H, W, 3), or (n, H, W) with "gray"')
            frames = list(frames.unbind(0))
        out = list(frames)
        modes = [subsampling] * len(out) if each is None else each
        if len(modes) != len(out):
            raise ValueError("one subsampling per frame")
        for f, mode in zip(out, modes):
            if not isinstance(f, torch.Tensor):
                raise TypeError("a frame is a torch tensor on the device")
            if f.dtype != torch.uint8:
                raise TypeError("a frame is uint8")
            if mode == "gray":
                if f.ndim != 2 and (f.ndim != 3 or f.shape[2] != 3):
                    raise ValueError('a frame is (H, W) or (H, W, 3) with "gray"')
            elif f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("a frame is (H, W, 3)")
            if not f.is_cuda or f.device != self.device:
                raise ValueError(f"a frame lives on {self.device}")
            if not f.is_contiguous():
                raise ValueError("a frame is contiguous")
            if not (1 <= f.shape[0] <= MAX_SIDE and 1 <= f.shape[1] <= MAX_SIDE):
                raise ValueError(f"a frame's sides lie in 1..{MAX_SIDE}")
        if len(out) > 65535:
            raise ValueError("at most 65535 frames per call")
        return out, modes

    def encode(self, frames, quality: Union[None, int, Sequence[int]] = None,
               subsampling: Union[None, str, Sequence[str]] = None, optimize: Union[None, bool, Sequence[bool]] = None,
               restart_rows: Union[None, int, Sequence[int]] = None) -> PendingJpegs:
        import torch
        from .train_abi import (FEAR_JPEG_ENC_GRAY_RGB, FEAR_JPEG_ENC_HEADER_MAX, FEAR_JPEG_ENC_OPTIMIZE, FEAR_JPEG_ENC_TABLE_BYTES,
                                FearJpegEncImage, launch)
        frames, modes = self._frames(frames, subsampling)
        n = len(frames)
        if optimize is None:
            optimize = self.optimize
        if isinstance(optimize, (bool, np.bool_)):
            flags = [FEAR_JPEG_ENC_OPTIMIZE if optimize else 0] * n
        elif isinstance(optimize, (list, tuple, np.ndarray)) and all(isinstance(o, (bool, np.bool_)) for o in optimize):
            flags = [FEAR_JPEG_ENC_OPTIMIZE if o else 0 for o in optimize]
            if len(flags) != n:
                raise ValueError("one optimize per frame")
        else:
            raise TypeError("optimize is a bool, or a sequence of them with one per frame")
        if restart_rows is None:
            restart_rows = self.restart_rows
        if isinstance(restart_rows, (list, tuple, np.ndarray)):
            rows = list(restart_rows)
            if len(rows) != n:
                raise ValueError("one restart_rows per frame")
        else:
            rows = [restart_rows] * n
        if quality is None:
            qualities = [self.quality] * n
        elif isinstance(quality, (int, np.integer)) and not isinstance(quality, bool):
            qualities = [_check_quality(quality)] * n
        else:
            qualities = [_check_quality(q) for q in quality]
            if len(qualities) != n:
                raise ValueError("one quality per frame")
        lib = self._lib
        records = (FearJpegEncImage * max(n, 1))()
        headers, header_at, slot_at, at, out_at = [], [], [], 0, 0
        scratch, used = (ctypes.c_uint8 * FEAR_JPEG_ENC_HEADER_MAX)(), ctypes.c_size_t(0)
        for k, f in enumerate(frames):
            H, W = int(f.shape[0]), int(f.shape[1])
            mode, (mcu_w, mcu_h) = _MODE[modes[k]], _MCU[modes[k]]
            mcus_x, mcus_y = -(-W // mcu_w), -(-H // mcu_h)
            interval = _restart_interval(rows[k], mcus_x)
            # (an optimised frame's header goes up without its DHT segments: the device puts its own in)
            launch(lib, "fear_jpeg_encode_header_flags", W, H, qualities[k], interval, mode, flags[k], scratch, len(scratch), ctypes.byref(used))
            headers.append(bytes(scratch[:used.value]))
            header_at.append(at)
            at += -(-used.value // 16) * 16
            if self.slot_bytes is None:
                slot = 1024 + _SLOT_FACTOR[modes[k]] * (mcu_w * mcus_x) * (mcu_h * mcus_y)
            elif self.slot_bytes == "bound":
                slot = int(lib.fear_jpeg_encode_bound_flags(W, H, interval, mode, flags[k]))
            else:
                slot = int(self.slot_bytes)
            if slot >= 1 << 32:
                raise ValueError("a slot fits 32 bits")
            rec = records[k]
            rec.width, rec.height, rec.quality, rec.restart_interval = W, H, qualities[k], interval
            rec.out_cap, rec.header_bytes = slot, used.value
            rec.sampling = mode | (FEAR_JPEG_ENC_GRAY_RGB if modes[k] == "gray" and f.ndim == 3 else 0)
            rec.flags = flags[k]
            slot_at.append(out_at)
            out_at += -(-(slot + self.guard_bytes) // 16) * 16
        with torch.cuda.device(self.device):
            if n == 0:
                empty = torch.empty(0, dtype=torch.int32, device=self.device)
                return PendingJpegs(torch.empty(0, dtype=torch.uint8, device=self.device), torch.empty(0, dtype=torch.int64, device=self.device),
                                    empty, empty, [])
            launch(lib, "fear_jpeg_encode_plan", records, n)
            ws_bytes = int(lib.fear_jpeg_encode_workspace_bytes(records, n))
            table_bytes = FEAR_JPEG_ENC_TABLE_BYTES(n)
            # one device allocation: the headers, then the workspace, whose first bytes are the records; both go up in one transfer
            dev = torch.empty(at + ws_bytes, dtype=torch.uint8, device=self.device)
            if self.guard_bytes:
                buffer = torch.full((out_at,), 0xA5, dtype=torch.uint8, device=self.device)
            else:
                buffer = torch.empty(out_at, dtype=torch.uint8, device=self.device)
            for k, f in enumerate(frames):
                records[k].src, records[k].out, records[k].header = f.data_ptr(), buffer.data_ptr() + slot_at[k], dev.data_ptr() + header_at[k]
            pinned = torch.empty(at + table_bytes + 8 * n, dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            for k, h in enumerate(headers):
                host[header_at[k]:header_at[k] + len(h)] = np.frombuffer(h, dtype=np.uint8)
            host[at:at + 96 * n] = np.frombuffer(records, dtype=np.uint8)[:96 * n]
            host[at + table_bytes:].view(np.int64)[:] = slot_at
            dev[:at + table_bytes].copy_(pinned[:at + table_bytes], non_blocking=True)
            offsets = torch.empty(n, dtype=torch.int64, device=self.device)
            offsets.view(torch.uint8).copy_(pinned[at + table_bytes:], non_blocking=True)
            verdict = torch.empty((2, n), dtype=torch.int32, device=self.device)
            launch(lib, "fear_jpeg_encode_u8", records, n, ctypes.c_void_p(dev.data_ptr() + at), ws_bytes,
                   ctypes.c_void_p(verdict[0].data_ptr()), ctypes.c_void_p(verdict[1].data_ptr()),
                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return PendingJpegs(buffer, offsets, verdict[0], verdict[1], slot_at, keep=(frames, dev, pinned))


# ---------------------------------------------------------------------------------------------------------------------- Motion-JPEG AVI
def write_mjpeg_avi(path, files: Sequence[bytes], fps: float) -> None:
    """JPEG files of one frame size as a Motion-JPEG AVI: RIFF 'AVI ', LIST hdrl (avih, LIST strl (strh, strf: MJPG)), LIST movi of
    00dc chunks (an odd payload is padded to an even length), idx1.  Plain host code; players read it without a codec library of ours."""
    from fractions import Fraction
    from .jpeg_frames import jpeg_info
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("an AVI needs at least one frame")
    if not fps > 0:
        raise ValueError("fps is positive")
    info = jpeg_info(files[0])
    width, height = info["width"], info["height"]
    for f in files[1:]:
        other = jpeg_info(f)
        if (other["width"], other["height"]) != (width, height):
            raise ValueError("every frame of an AVI has the same size")
    rate = Fraction(fps).limit_denominator(100000)
    largest = max(len(f) for f in files)

    def chunk(tag: bytes, payload: bytes) -> bytes:
        return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")

    def listed(kind: bytes, payload: bytes) -> bytes:
        return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload

    avih = struct.pack("<14I", round(1e6 / fps), int(largest * fps) + 1, 0, 0x10, len(files), 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, len(files), largest, -1, 0,
                                     0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = listed(b"hdrl", chunk(b"avih", avih) + listed(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi, index, at = bytearray(), bytearray(), 4                          # idx1 offsets count from the 'movi' tag
    for f in files:
        index += b"00dc" + struct.pack("<III", 0x10, at, len(f))
        piece = chunk(b"00dc", f)
        movi += piece
        at += len(piece)
    body = b"AVI " + hdrl + listed(b"movi", bytes(movi)) + chunk(b"idx1", bytes(index))
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
