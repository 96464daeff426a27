"""Baseline JPEG frames decoded for the training and validation pipelines.

`jpeg_decode_host` is the contract: a numpy and pure-Python decoder of baseline sequential JPEG that equals libjpeg with its defaults
(islow IDCT, fancy upsampling — what the reference's cv2.imread runs) byte for byte; tests/test_jpeg_decode_host.py holds it to Pillow's
libjpeg-turbo.  `JpegDecoder` is the product: the parser and the Huffman stage run on host threads in the library
(csrc/fear_jpeg_entropy.h), the packed coefficients go up in one transfer and `fear_jpeg_decode_u8` does the rest on the device.  With
`entropy="device"` the Huffman stage runs on the device as well (`fear_jpeg_huffman`; jpeg_huffman.py states its contract)."""
from __future__ import annotations

import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .train_data.jpeg import _jpeg_upsample, _jpeg_ycc_to_rgb, jpeg_idct_islow

MAX_SIDE = 8192
DEVICE_SCAN_MAX = 16 << 20                # include/fear_train.h FEAR_JPEG_DEVICE_SCAN_MAX: a longer restart segment is decoded on the host
ERR_FORMAT, ERR_UNSUPPORTED = -9, -10     # include/fear_train.h FEAR_TRAIN_ERR_FORMAT, FEAR_TRAIN_ERR_UNSUPPORTED

# zigzag position -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class MalformedJPEG(ValueError):
    """The bytes are no complete baseline JPEG: truncated, a code in no table, a bad restart marker, a bad segment."""


class UnsupportedJPEG(ValueError):
    """A valid JPEG of a kind the decoder declines: progressive, arithmetic, 12-bit, other sampling factors, 2 or 4 components, RGB."""


# ------------------------------------------------------------------------------------------------------------------ the host contract
class _Huffman:
    """One table of a DHT segment: canonical codes of T.81 annex C, decoded bit by bit (F.2.2.3)."""

    def __init__(self, counts: Sequence[int], values: bytes):
        self.first, self.index, self.counts, self.values = [0] * 17, [0] * 17, [0] + list(counts), values
        code = k = 0
        for length in range(1, 17):
            self.first[length], self.index[length] = code, k
            if code + self.counts[length] > (1 << length):
                raise MalformedJPEG(f"over-subscribed Huffman table at code length {length}")
            code = (code + self.counts[length]) << 1
            k += self.counts[length]


class _Header:
    pass


def _parse(data: bytes) -> _Header:
    """The segments up to and including SOS.  Mirrors csrc/fear_jpeg_entropy.h check for check, in the same order."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise MalformedJPEG("no SOI marker")
    hd = _Header()
    hd.q, hd.dc, hd.ac, hd.restart, hd.adobe, sof = {}, {}, {}, 0, -1, False
    p = 2
    while True:
        if p >= n or data[p] != 0xFF:
            raise MalformedJPEG("a marker was expected" if p < n else "truncated before the scan")
        while p < n and data[p] == 0xFF:            # fill bytes
            p += 1
        if p >= n:
            raise MalformedJPEG("truncated in a marker")
        m = data[p]
        p += 1
        if m == 0x01:                               # TEM stands alone
            continue
        if m == 0x00 or 0xD0 <= m <= 0xD9:
            raise MalformedJPEG(f"marker FF{m:02X} in front of the scan")
        if p + 2 > n:
            raise MalformedJPEG("truncated in a segment length")
        L = (data[p] << 8) | data[p + 1]
        if L < 2 or p + L > n:
            raise MalformedJPEG("a segment length runs past the end")
        seg = data[p + 2:p + L]
        p += L
        if m == 0xC0:
            if sof:
                raise MalformedJPEG("a second frame header")
            if len(seg) < 6:
                raise MalformedJPEG("short SOF0")
            if seg[0] != 8:
                raise UnsupportedJPEG(f"{seg[0]}-bit samples")
            hd.height, hd.width, nf = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if hd.width == 0:
                raise MalformedJPEG("zero width")
            if hd.height == 0:
                raise UnsupportedJPEG("zero height: the frame's height comes in a DNL segment")
            if hd.width > MAX_SIDE or hd.height > MAX_SIDE:
                raise UnsupportedJPEG(f"sides above {MAX_SIDE}")
            if nf == 0:
                raise MalformedJPEG("a frame without components")
            if nf not in (1, 3):
                raise UnsupportedJPEG(f"{nf} components")
            if len(seg) != 6 + 3 * nf:
                raise MalformedJPEG("SOF0 length")
            hd.ids, hd.h, hd.v, hd.tq = [], [], [], []
            for i in range(nf):
                cid, hv, tq = seg[6 + 3 * i:9 + 3 * i]
                h, v = hv >> 4, hv & 15
                if not (1 <= h <= 4 and 1 <= v <= 4) or tq > 3 or cid in hd.ids:
                    raise MalformedJPEG("a component's sampling factors, table or id")
                hd.ids.append(cid); hd.h.append(h); hd.v.append(v); hd.tq.append(tq)
            if nf == 1:
                hd.h, hd.v = [1], [1]               # one component: the scan is not interleaved, its sampling factors mean nothing
            elif (hd.h[0], hd.v[0]) not in ((1, 1), (2, 1), (2, 2)) or (hd.h[1], hd.v[1], hd.h[2], hd.v[2]) != (1, 1, 1, 1):
                raise UnsupportedJPEG("sampling factors other than 4:4:4, 4:2:2 and 4:2:0")
            sof = True
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xCC):
            raise UnsupportedJPEG({0xC1: "extended sequential", 0xC2: "progressive"}.get(m, f"SOF{m - 0xC0}") + " frame")
        elif m == 0xCC:
            raise UnsupportedJPEG("arithmetic coding")
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                tc, th = seg[s] >> 4, seg[s] & 15
                if tc > 1 or th > 3 or s + 17 > len(seg):
                    raise MalformedJPEG("DHT header")
                counts = list(seg[s + 1:s + 17])
                total = sum(counts)
                if total > 256 or s + 17 + total > len(seg):
                    raise MalformedJPEG("DHT symbol count")
                (hd.ac if tc else hd.dc)[th] = _Huffman(counts, seg[s + 17:s + 17 + total])
                s += 17 + total
        elif m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                if pq == 1:
                    raise UnsupportedJPEG("16-bit quantiser table")
                if pq > 1 or tq > 3 or s + 65 > len(seg):
                    raise MalformedJPEG("DQT header")
                table = np.zeros(64, dtype=np.int64)
                table[ZIGZAG] = np.frombuffer(seg[s + 1:s + 65], dtype=np.uint8)
                hd.q[tq] = table
                s += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise MalformedJPEG("DRI length")
            hd.restart = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise UnsupportedJPEG("DNL segment")
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                hd.adobe = seg[11]
        elif m == 0xDA:
            if not sof:
                raise MalformedJPEG("SOS in front of SOF")
            nf = len(hd.ids)
            if len(seg) < 1 or seg[0] == 0 or seg[0] > 4:
                raise MalformedJPEG("SOS component count")
            if seg[0] != nf:
                raise UnsupportedJPEG("a scan with part of the components (a second scan follows)")
            if len(seg) != 4 + 2 * nf:
                raise MalformedJPEG("SOS length")
            hd.td, hd.ta = [], []
            for i in range(nf):
                cs, t = seg[1 + 2 * i], seg[2 + 2 * i]
                if cs != hd.ids[i]:
                    if cs in hd.ids:
                        raise UnsupportedJPEG("scan components out of frame order")
                    raise MalformedJPEG("a scan component the frame does not have")
                if (t >> 4) > 3 or (t & 15) > 3:
                    raise MalformedJPEG("Huffman table selector")
                hd.td.append(t >> 4); hd.ta.append(t & 15)
            if tuple(seg[1 + 2 * nf:4 + 2 * nf]) != (0, 63, 0):
                raise MalformedJPEG("spectral selection of a baseline scan")
            if nf == 3 and hd.adobe == 0:
                raise UnsupportedJPEG("Adobe transform 0: RGB samples")
            for i in range(nf):
                if hd.tq[i] not in hd.q or hd.td[i] not in hd.dc or hd.ta[i] not in hd.ac:
                    raise MalformedJPEG("a component selects a table no segment defined")
            hd.scan = p
            break
        # APPn, COM and the reserved markers carry nothing the decoder needs
    hd.mcus_x = -(-hd.width // (8 * hd.h[0]))
    hd.mcus_y = -(-hd.height // (8 * hd.v[0]))
    hd.blocks_w = [hd.mcus_x * h for h in hd.h]
    hd.blocks_h = [hd.mcus_y * v for v in hd.v]
    return hd


def _either(data: bytes, progressive: bool, baseline, of_progressive):
    """`baseline(data)`; with `progressive`, a file the baseline rules decline goes to `of_progressive` (jpeg_progressive.py), and one whose
    frame is not SOF2 keeps the baseline verdict."""
    try:
        return baseline(data)
    except UnsupportedJPEG as first:
        if not progressive:
            raise
        from .jpeg_progressive import NotProgressive
        try:
            return of_progressive(data)
        except NotProgressive:
            raise first from None


def jpeg_info(data: bytes, progressive: bool = False) -> Dict[str, object]:
    """What the frame and scan headers say: size, components, sampling, block and MCU counts, restart interval, quantiser tables.
    `progressive=True` reads a progressive file's as well: those of its baseline twin, without a restart interval."""
    from . import jpeg_progressive
    hd = _either(bytes(data), progressive, _parse, jpeg_progressive.progressive_info)
    return dict(width=hd.width, height=hd.height, components=len(hd.ids), h=list(hd.h), v=list(hd.v), mcus_x=hd.mcus_x, mcus_y=hd.mcus_y,
                blocks_w=list(hd.blocks_w), blocks_h=list(hd.blocks_h), restart_interval=hd.restart,
                qt=np.stack([hd.q[t] for t in hd.tq]).astype(np.uint16))


class _Bits:
    """The entropy-coded segment bit by bit: FF 00 is a data byte FF, any other FF xx ends the data."""

    def __init__(self, data: bytes, pos: int):
        self.data, self.pos, self.cur, self.left = data, pos, 0, 0

    def bit(self) -> int:
        if self.left == 0:
            d, p = self.data, self.pos
            if p >= len(d):
                raise MalformedJPEG("truncated entropy data")
            self.cur = d[p]
            if self.cur == 0xFF:
                if p + 1 >= len(d):
                    raise MalformedJPEG("truncated entropy data")
                if d[p + 1] != 0:
                    raise MalformedJPEG(f"marker FF{d[p + 1]:02X} inside an MCU")
                p += 1
            self.pos, self.left = p + 1, 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def bits(self, count: int) -> int:
        v = 0
        for _ in range(count):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, t: _Huffman) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            k = code - t.first[length]
            if 0 <= k < t.counts[length]:
                return t.values[t.index[length] + k]
        raise MalformedJPEG("a code in no Huffman table")

    def restart(self, expected: int) -> None:
        self.left = 0                               # the rest of the byte is padding
        d, p = self.data, self.pos
        if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD0 + expected:
            raise MalformedJPEG("a restart marker is missing or out of order")
        self.pos = p + 2


def _extend(v: int, t: int) -> int:
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def _wrap16(v: int) -> int:
    return ((v + 32768) & 0xFFFF) - 32768


def jpeg_coefficients_host(data: bytes, progressive: bool = False) -> Tuple[_Header, List[np.ndarray]]:
    """Headers and, per component, the quantised coefficients (blocks_h, blocks_w, 64) int16 in zigzag order (T.81 F.2).
    `progressive=True` decodes a progressive file's scans as well (T.81 G.1, jpeg_progressive.py)."""
    if progressive:
        from . import jpeg_progressive
        return _either(bytes(data), True, jpeg_coefficients_host, jpeg_progressive.progressive_coefficients_host)
    data = bytes(data)
    hd = _parse(data)
    nf = len(hd.ids)
    coef = [np.zeros((hd.blocks_h[c], hd.blocks_w[c], 64), dtype=np.int16) for c in range(nf)]
    bits, pred = _Bits(data, hd.scan), [0] * nf
    for mcu in range(hd.mcus_x * hd.mcus_y):
        if hd.restart and mcu and mcu % hd.restart == 0:
            bits.restart((mcu // hd.restart - 1) & 7)
            pred = [0] * nf
        my, mx = divmod(mcu, hd.mcus_x)
        for c in range(nf):
            dc, ac = hd.dc[hd.td[c]], hd.ac[hd.ta[c]]
            for j in range(hd.v[c]):
                for i in range(hd.h[c]):
                    block = coef[c][my * hd.v[c] + j, mx * hd.h[c] + i]
                    t = bits.symbol(dc)
                    if t > 15:
                        raise MalformedJPEG("a DC size above 15")
                    pred[c] = _wrap16(pred[c] + _extend(bits.bits(t), t))          # JCOEF is 16 bits wide
                    block[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break                                              # EOB
                            k += 16                                                # ZRL: a coefficient follows
                            if k > 63:
                                raise MalformedJPEG("a coefficient index past 63")
                            continue
                        k += r
                        if k > 63:
                            raise MalformedJPEG("a coefficient index past 63")
                        block[k] = _extend(bits.bits(s), s)
                        k += 1
    return hd, coef


def _upsample_h2v1(c: np.ndarray) -> np.ndarray:
    left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    return np.stack([(3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2], axis=2).reshape(c.shape[0], 2 * c.shape[1])


SCALES = (1, 2, 4, 8)


def _check_scale(scale) -> int:
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or int(scale) not in SCALES:
        raise ValueError(f"scale is one of {SCALES}, not {scale!r}")
    return int(scale)


def _check_scales(scale, n: int):
    """`scale` of a `JpegStore` call over `n` positions: an int of SCALES as it is (the uniform code path), or a sequence or array of
    `n` of them, returned as an (n,) int64 array.  A wrong length, another value, a bool or a non-integer is a ValueError."""
    if isinstance(scale, (int, np.integer)) and not isinstance(scale, (bool, np.bool_)):
        return _check_scale(scale)
    if isinstance(scale, (str, bytes, bool, np.bool_)) or scale is None or np.ndim(scale) != 1:
        raise ValueError(f"scale is one of {SCALES} or a sequence of them, one per id, not {scale!r}")
    if any(isinstance(s, (bool, np.bool_)) for s in scale):
        raise ValueError(f"scale is one of {SCALES} per id, not a bool")
    arr = np.asarray(scale)
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"scale is one of {SCALES} per id, not {arr.dtype} values")
    if arr.size != n:
        raise ValueError(f"scale has {arr.size} values for {n} ids")
    arr = arr.astype(np.int64).reshape(-1)
    if not np.isin(arr, SCALES).all():
        raise ValueError(f"scale is one of {SCALES} per id, not {int(arr[~np.isin(arr, SCALES)][0])}")
    return arr


def jpeg_scaled_shape(height: int, width: int, scale: int) -> Tuple[int, int, int]:
    """The shape of a frame of `height` x `width` decoded at 1 / `scale`: (ceil(H m / 8), ceil(W m / 8), 3) with m = 8 // scale."""
    m = 8 // _check_scale(scale)
    return -(-int(height) * m // 8), -(-int(width) * m // 8), 3


def jpeg_scaled_transforms(h: Sequence[int], v: Sequence[int], scale: int) -> List[int]:
    """The side `ss` of each component's inverse transform at 1 / `scale` (libjpeg's jdmaster.c): it starts at m = 8 // scale and doubles
    while it is below 8 and the component's plane would still be no larger than the frame on either axis.  A component the frame
    subsamples therefore takes the next larger transform in place of the upsampling: 4:2:0 chroma 2 m on both axes; 4:2:2 chroma stays at
    m (its rows are the frame's) and is upsampled horizontally."""
    m = 8 // _check_scale(scale)
    h_max, v_max, out = max(h), max(v), []
    for hc, vc in zip(h, v):
        ss = m
        while ss < 8 and (h_max * m) % (hc * ss * 2) == 0 and (v_max * m) % (vc * ss * 2) == 0:
            ss *= 2
        out.append(ss)
    return out


def _descale(x: np.ndarray, n: int) -> np.ndarray:
    return (x + (1 << (n - 1))) >> n


def _idct_4x4_pass(x: Dict[int, np.ndarray], n: int) -> List[np.ndarray]:
    t0 = x[0] << 14
    t2 = 15137 * x[2] - 6270 * x[6]
    t10, t12 = t0 + t2, t0 - t2
    o0 = -1730 * x[7] + 11893 * x[5] - 17799 * x[3] + 8697 * x[1]
    o2 = -4176 * x[7] - 4926 * x[5] + 7373 * x[3] + 20995 * x[1]
    return [_descale(t10 + o2, n), _descale(t12 + o0, n), _descale(t12 - o0, n), _descale(t10 - o2, n)]


def _idct_2x2_pass(x: Dict[int, np.ndarray], n: int) -> List[np.ndarray]:
    t10 = x[0] << 15
    t0 = -5906 * x[7] + 6967 * x[5] - 10426 * x[3] + 29692 * x[1]
    return [_descale(t10 + t0, n), _descale(t10 - t0, n)]


def jpeg_idct_scaled(blocks: np.ndarray, ss: int) -> np.ndarray:
    """libjpeg's reduced inverse transforms (jidctred.c) on dequantised int64 blocks [..., 8, 8] -> [..., ss, ss], before the level shift:
    ss 8 is the islow transform, 4 and 2 run columns first and then rows and never read row and column 4 (ss 2: nor 2 and 6), 1 is
    DESCALE(dc, 3).  64-bit integers, as libjpeg's; the device computes in 32 bits, which agree while |dequantised value| < 2^13 or so."""
    blocks = np.asarray(blocks, dtype=np.int64)
    if ss == 8:
        return jpeg_idct_islow(blocks)
    if ss == 1:
        return _descale(blocks[..., :1, :1], 3)
    one_pass, keep = (_idct_4x4_pass, (0, 1, 2, 3, 5, 6, 7)) if ss == 4 else (_idct_2x2_pass, (0, 1, 3, 5, 7))
    first, second = (12, 19) if ss == 4 else (13, 20)
    # columns: out[..., i, c] for the kept columns c
    cols = one_pass({r: blocks[..., r, :] for r in range(8)}, first)                  # ss arrays [..., 8]: the rows of the intermediate
    mid = np.stack(cols, axis=-2)                                                     # [..., ss, 8]
    rows = one_pass({c: mid[..., c] for c in keep}, second)                           # ss arrays [..., ss]
    return np.stack(rows, axis=-1)


def jpeg_decode_host(data: bytes, progressive: bool = False, scale: int = 1) -> np.ndarray:
    """A baseline JPEG file -> uint8 (H, W, 3) RGB, as libjpeg decodes it with its defaults.  Slow; the statement the device is held to.
    `progressive=True` takes a complete progressive file as well.  `scale` 2, 4 or 8 decodes at 1/2, 1/4 or 1/8 of the size in the DCT
    domain, as libjpeg's scale_denom (Pillow's `draft`) does: `jpeg_scaled_shape` is the frame's."""
    scale = _check_scale(scale)
    return jpeg_pixels_host(*jpeg_coefficients_host(data, progressive), scale=scale)


def jpeg_pixels_host(hd: _Header, coef: List[np.ndarray], height: Optional[int] = None, scale: int = 1) -> np.ndarray:
    """The pixel stage of `jpeg_decode_host` on coefficients: dequantisation, islow IDCT, fancy upsampling at the true edges, colour.
    `height` (the header's by default) makes it the decode of a BAND image, as `JpegStore.decode_rows` hands one to
    `fear_jpeg_decode_u8`: `coef` holds the blocks of some consecutive MCU rows alone and `height` is the pixel rows they cover, so the
    edge rules apply at the band's edges.
    `scale` 2, 4 or 8 (m = 8 // scale): component c runs the ss x ss transform of `jpeg_scaled_transforms`, its plane is blocks_h ss x
    blocks_w ss of which ceil(H v_c ss / (8 v_max)) x ceil(W h_c ss / (8 h_max)) is true, and the only upsampling left is 4:2:2's h2v1 —
    fancy when m > 1 and the true chroma width is above 2, replication otherwise (libjpeg turns fancy upsampling off at 1/8).  `height`
    stays the band's FULL-size height."""
    scale = _check_scale(scale)
    m, H, W, nf = 8 // scale, hd.height if height is None else int(height), hd.width, len(hd.ids)
    out_h, out_w, _ = jpeg_scaled_shape(H, W, scale)
    sizes = jpeg_scaled_transforms(hd.h, hd.v, scale)                              # 8 for every component at scale 1
    planes = []
    for c in range(nf):
        q, ss = hd.q[hd.tq[c]], sizes[c]
        nat = np.zeros(coef[c].shape, dtype=np.int64)
        nat[..., ZIGZAG] = coef[c]
        bh, bw = coef[c].shape[:2]
        px = np.clip(jpeg_idct_scaled((nat * q).reshape(bh, bw, 8, 8), ss) + 128, 0, 255)
        plane = px.transpose(0, 2, 1, 3).reshape(bh * ss, bw * ss)
        ch, cw = -(-H * hd.v[c] * ss // (hd.v[0] * 8)), -(-W * hd.h[c] * ss // (hd.h[0] * 8))
        plane = plane[:ch, :cw]                                                    # the true edges, not the padded blocks'
        if hd.h[0] * m == 2 * hd.h[c] * ss:                                        # half the frame's width: chroma of 4:2:2, or of 4:2:0 at scale 1
            fancy = m > 1 and cw > 2                                               # libjpeg replicates planes this narrow, and all of them at 1/8
            if hd.v[0] * m == 2 * hd.v[c] * ss:                                    # and half its height: h2v2, at scale 1 alone
                plane = _jpeg_upsample(plane) if fancy else np.repeat(np.repeat(plane, 2, axis=0), 2, axis=1)
            else:
                plane = _upsample_h2v1(plane) if fancy else np.repeat(plane, 2, axis=1)
        planes.append(plane[:out_h, :out_w])
    if nf == 1:
        return np.repeat(planes[0][..., None], 3, axis=2).astype(np.uint8)
    return _jpeg_ycc_to_rgb(planes[0], planes[1] - 128, planes[2] - 128)


# ------------------------------------------------------------------------------------------------------------------------ the product
Item = Union[bytes, bytearray, memoryview, str, os.PathLike]


def _frame_size(data: bytes) -> Optional[Tuple[int, int]]:
    """(height, width) of the first frame header of any kind, or None where the segments cannot be walked that far."""
    p, n = 2, len(data)
    while p + 4 <= n and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD9:
            p += 2
            continue
        L = (data[p + 2] << 8) | data[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return ((data[p + 5] << 8) | data[p + 6], (data[p + 7] << 8) | data[p + 8]) if p + 9 <= n else None
        if m == 0xDA or L < 2:
            return None
        p += 2 + L
    return None


def _check_fallback_shape(index: int, data: bytes, px: np.ndarray, scale: int) -> None:
    """At a scale the fallback decodes at that scale too: its pixels have the scaled shape of the file's frame header."""
    size = _frame_size(data)
    if size is not None and tuple(px.shape) != jpeg_scaled_shape(size[0], size[1], scale):
        raise ValueError(f"item {index}: the fallback returned {tuple(px.shape)} where scale={scale} of a {size[0]} x {size[1]} file is "
                         f"{jpeg_scaled_shape(size[0], size[1], scale)}")


def _raise_as_python(data: bytes, rc: int, progressive: bool = False):
    """The library's verdict as the exception of the Python decoder, whose message says which check it was."""
    try:
        jpeg_coefficients_host(data, progressive)
    except (MalformedJPEG, UnsupportedJPEG) as exc:
        if isinstance(exc, UnsupportedJPEG) == (rc == ERR_UNSUPPORTED):
            raise
    raise (UnsupportedJPEG if rc == ERR_UNSUPPORTED else MalformedJPEG)(f"the library declined the file with status {rc}")


def _read_items(items: Sequence[Item]) -> List[bytes]:
    """The files' bytes: an item is the bytes themselves or a path."""
    blobs = []
    for item in items:
        if isinstance(item, (bytes, bytearray, memoryview)):
            blobs.append(bytes(item))
        else:
            with open(item, "rb") as fh:
                blobs.append(fh.read())
    return blobs


def _judge(blobs: List[bytes], results: List, fallback, progressive: bool, scale: int = 1, name_item: bool = False):
    """Every file is judged before anything is launched or stored.  `results` holds per file the pool's tuple, a JPEG to decode, or the
    library's status: ERR_UNSUPPORTED with a `fallback` becomes the fallback's pixels, every other status raises as the Python decoder
    does (`name_item`: with "item i: " in front).  Returns the positions of the JPEGs and {position: pixels}."""
    jpegs, raw = [], {}
    for i, (data, res) in enumerate(zip(blobs, results)):
        if isinstance(res, tuple):
            jpegs.append(i)
        elif res == ERR_UNSUPPORTED and fallback is not None:
            px = np.ascontiguousarray(fallback(data))
            if px.ndim != 3 or px.shape[2] != 3 or px.dtype != np.uint8:
                raise ValueError("the fallback must return uint8 (H, W, 3)")
            if scale > 1:
                _check_fallback_shape(i, data, px, scale)
            raw[i] = px
        else:
            try:
                _raise_as_python(data, res, progressive)
            except (MalformedJPEG, UnsupportedJPEG) as exc:
                if not name_item:
                    raise
                raise type(exc)(f"item {i}: {exc}") from None
    return jpegs, raw


def _fill_header(rec, info) -> None:
    """What a FearJpegImage record takes from the file's FearJpegInfo."""
    rec.width, rec.height, rec.components, rec.h, rec.v = info.width, info.height, info.components, info.h[0], info.v[0]
    ctypes.memmove(rec.qt, info.qt, ctypes.sizeof(rec.qt))


def _launch_pixels(lib, records, n: int, table: int, workspace: int, workspace_bytes: int, scale, stream) -> None:
    """The pixel stage over `n` FearJpegImage records whose prefix tables are at the device address `table`: fear_jpeg_decode_u8, at a
    scale fear_jpeg_decode_scaled_u8.  `scale` may be an array of `n` scales, one per record: where they are all equal the launch is the
    uniform one at that scale, else fear_jpeg_decode_mixed_u8, whose records carry the scales in reserved[0] (the caller wrote them)."""
    from .train_abi import launch
    table, workspace = ctypes.c_void_p(table), ctypes.c_void_p(workspace)
    if not isinstance(scale, (int, np.integer)):
        if scale.size and (scale != scale[0]).any():
            launch(lib, "fear_jpeg_decode_mixed_u8", records, n, table, workspace, workspace_bytes, stream)
            return
        scale = int(scale[0]) if scale.size else 1
    if scale == 1:
        launch(lib, "fear_jpeg_decode_u8", records, n, table, workspace, workspace_bytes, stream)
    else:
        launch(lib, "fear_jpeg_decode_scaled_u8", records, n, table, scale, workspace, workspace_bytes, stream)


class JpegDecoder:
    """Baseline JPEG files -> uint8 (H, W, 3) RGB device tensors, byte for byte what libjpeg (cv2.imread, Pillow) decodes.

    `decode` parses and Huffman-decodes on `threads` host threads (the library's C++ through ctypes, which releases the GIL), packs the
    coefficients of all images into one pinned buffer, uploads it non-blocking and runs `fear_jpeg_decode_u8` once.  It never waits for
    the GPU.  The tensors go unchanged into `TrainPairBuilder.build`, `FEARMultiTracker` and `SequenceValidator`.

    `entropy="device"` moves the Huffman stage to the device.  The host threads then only parse the headers and prepare the scans
    (`fear_jpeg_scan_prepare`: the stuffing removed, the bytes split at the restart markers — a header or marker fault still raises inside
    `decode`, before any launch); the unstuffed bytes, the scan records and their tables go up in the one pinned transfer, about the
    files' size; `fear_jpeg_huffman` (`subsequence_bytes` per lane) writes dense coefficients and `fear_jpeg_decode_u8` reads them.  A file
    with a restart segment above DEVICE_SCAN_MAX goes through the host's Huffman stage in the same call, an unsupported file with a
    `fallback` rides along as before.  A call whose dense coefficients (128 bytes per block: 4.1 MB for a 720p 4:2:0 frame) exceed
    `workspace_limit` bytes is split into groups on the same stream; a single image above the limit is a group of its own.
    An error the device finds — a code in no table, truncated entropy data: jpeg_huffman.jpeg_entropy_parallel_host lists them — cannot
    raise inside a call that does not wait: `decode` copies the statuses to pinned memory and records an event, and `check()` waits for
    the calls not yet checked and raises `MalformedJPEG` naming the call's item index; `decode(..., check=True)` does both.  The pixels of
    a failed image are unspecified.  The statuses of the last PENDING_CALLS unchecked calls are kept.

    `progressive=True` takes progressive files (SOF2) as well: the pool decodes all of a file's scans (`fear_jpeg_progressive_decode`,
    T.81 G.1; jpeg_progressive.py states it) and its packed coefficients ride in the call as a host-path item's do, in both entropy
    modes (`last_paths` says "host").  A file that decoder declines — an incomplete or inconsistent progression — reaches the
    `fallback` or raises; baseline files in the same call go the way they went."""
    MAX_THREADS = 16
    PENDING_CALLS = 64

    def __init__(self, device: int = 0, threads: Optional[int] = None, entropy: str = "host", workspace_limit: int = 1 << 30,
                 subsequence_bytes: int = 128, progressive: bool = False):
        import torch
        from .train_abi import load_train_library
        if threads is None:
            threads = min(8, len(os.sched_getaffinity(0)))            # the CPUs this process may use, never the machine's count
        self.threads = max(1, min(int(threads), self.MAX_THREADS))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = load_train_library()
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="fear-jpeg")
        self._pinned: List = []                                       # the last calls' staging buffers: each outlives its copy
        if entropy not in ("host", "device"):
            raise ValueError('entropy is "host" or "device"')
        if subsequence_bytes % 4 or not 4 <= subsequence_bytes <= 1024:
            raise ValueError("subsequence_bytes is a multiple of 4 in 4..1024")
        self.entropy, self.workspace_limit, self.subsequence_bytes = entropy, int(workspace_limit), int(subsequence_bytes)
        self.progressive = bool(progressive)
        self._pending: List = []                                      # device mode: (event, pinned statuses, [(item index, file)]) per group
        self.last_paths: List[str] = []                               # device mode: "device" or "host" per JPEG file of the last call

    def close(self) -> None:
        self._pool.shutdown(wait=True)

    def entropy_decode(self, data: bytes):
        """One file through fear_jpeg_parse and fear_jpeg_entropy_decode: (FearJpegInfo, packed int16 coefficients, uint32 block_start),
        or the library's status for a file it declines.  Host only."""
        return self._packed_coefficients(data, self._lib.fear_jpeg_parse, self._lib.fear_jpeg_entropy_decode, self.progressive)

    def progressive_decode(self, data: bytes):
        """One file through fear_jpeg_progressive_parse and fear_jpeg_progressive_decode: what `entropy_decode` returns for a baseline
        file, or the library's status — FEAR_TRAIN_ERR_UNSUPPORTED also for a file whose frame is not SOF2.  Host only."""
        return self._packed_coefficients(data, self._lib.fear_jpeg_progressive_parse, self._lib.fear_jpeg_progressive_decode, False)

    def _packed_coefficients(self, data: bytes, parse, decode, progressive: bool):
        """`parse` and then `decode` of the library on one file; with `progressive`, a file that `parse` declines as unsupported goes
        to `progressive_decode`."""
        from .train_abi import FearJpegInfo
        lib, info = self._lib, FearJpegInfo()
        rc = parse(data, len(data), ctypes.byref(info))
        if rc == ERR_UNSUPPORTED and progressive:
            return self.progressive_decode(data)
        if rc != 0:
            return rc
        coef = np.empty(lib.fear_jpeg_packed_bound(ctypes.byref(info)), dtype=np.int16)
        start = np.empty(info.total_blocks + 1, dtype=np.uint32)
        used = ctypes.c_size_t(0)
        rc = decode(data, len(data), ctypes.byref(info), coef.ctypes.data, coef.size, start.ctypes.data, ctypes.byref(used))
        if rc != 0:
            return rc
        return info, coef[:used.value], start

    def to_baseline(self, data: bytes):
        """One progressive file through fear_jpeg_progressive_to_baseline: the baseline file's bytes, or the library's status.  Host only."""
        from .train_abi import FearJpegInfo
        lib, info = self._lib, FearJpegInfo()
        rc = lib.fear_jpeg_progressive_parse(data, len(data), ctypes.byref(info))
        if rc != 0:
            return rc
        out = np.empty(lib.fear_jpeg_baseline_bound(ctypes.byref(info)), dtype=np.uint8)
        used = ctypes.c_size_t(0)
        rc = lib.fear_jpeg_progressive_to_baseline(data, len(data), out.ctypes.data, out.size, ctypes.byref(used))
        if rc != 0:
            return rc
        return out[:used.value].tobytes()

    def scan_prepare(self, data: bytes):
        """One file through fear_jpeg_parse and fear_jpeg_scan_prepare: (FearJpegInfo, unstuffed bytes, uint32 seg_start, FearJpegScan),
        or the library's status for a file it declines.  Host only."""
        from .train_abi import FearJpegInfo, FearJpegScan
        lib, info, scan = self._lib, FearJpegInfo(), FearJpegScan()
        rc = lib.fear_jpeg_parse(data, len(data), ctypes.byref(info))
        if rc != 0:
            return rc
        n_mcu = info.mcus_x * info.mcus_y
        out = np.empty(len(data), dtype=np.uint8)
        seg = np.empty((-(-n_mcu // info.restart_interval) if info.restart_interval else 1) + 1, dtype=np.uint32)
        rc = lib.fear_jpeg_scan_prepare(data, len(data), ctypes.byref(info), out.ctypes.data, out.size, seg.ctypes.data, seg.size, ctypes.byref(scan))
        if rc != 0:
            return rc
        return info, out[:scan.n_bytes], seg, scan

    def _prepare(self, data: bytes):
        res = self.scan_prepare(data)
        if res == ERR_UNSUPPORTED and self.progressive:
            return self.progressive_decode(data)                      # every scan on the host; the coefficients ride as a host-path item's
        if isinstance(res, tuple) and res[3].max_seg_bytes > DEVICE_SCAN_MAX:
            return self.entropy_decode(data)                          # too long for one workgroup's bounded walk: the host's stage
        return res

    def check(self) -> None:
        """Device mode: wait for the calls not yet checked and raise MalformedJPEG for the first image the device refused."""
        pending, self._pending = self._pending, []
        for k, (event, status, items) in enumerate(pending):
            event.synchronize()
            bad = np.flatnonzero(status.numpy())
            if bad.size:
                self._pending = pending[k + 1:]
                index, data = items[int(bad[0])]
                try:
                    _raise_as_python(data, int(status[int(bad[0])]))
                except MalformedJPEG as exc:
                    raise MalformedJPEG(f"item {index}: {exc}") from None

    def _decode_group(self, blobs, prepared, group, raw, frames, scale: int = 1) -> None:
        """One group of `decode`, in either entropy mode: one upload, fear_jpeg_huffman over the group's device-path images (a
        prepared scan, four values) and the pixel stage over all of them; a host-path image (packed coefficients, three values) brings
        its coefficients and block_start in the upload.  A group without a device-path image launches the pixel stage alone."""
        import torch
        from .train_abi import (FEAR_JPEG_GROUP_BLOCKS, FEAR_JPEG_GROUP_PIXELS, FearJpegImage, FearJpegInfo, FearJpegScan, launch)
        from .train_data.staging import Staging
        n = len(group)
        on_device = [k for k in range(n) if len(prepared[group[k]]) == 4]
        nd, place = len(on_device), {k: d for d, k in enumerate(on_device)}
        stage = Staging()
        records, infos, scans = (FearJpegImage * max(n, 1))(), (FearJpegInfo * max(n, 1))(), (FearJpegScan * max(nd, 1))()
        prefix, seg_prefix = np.zeros((2, n + 1), dtype=np.uint32), np.zeros(nd + 1, dtype=np.uint32)
        out_at, out_bytes, plane_at, values, most = [], 0, 0, 0, 0
        for k, i in enumerate(group):
            info = prepared[i][0]
            infos[k] = info
            rec = records[k]
            _fill_header(rec, info)
            rec.plane_offset = plane_at
            plane_at += int(info.total_blocks) * 64
            prefix[0, k + 1] = prefix[0, k] + -(-int(info.total_blocks) // FEAR_JPEG_GROUP_BLOCKS)
            sh, sw, _ = jpeg_scaled_shape(info.height, info.width, scale)          # the frame's size: the file's at scale 1
            prefix[1, k + 1] = prefix[1, k] + -(-sw * sh // FEAR_JPEG_GROUP_PIXELS)
            if len(prepared[i]) == 4:
                d = place[k]
                ctypes.memmove(ctypes.byref(scans[d]), ctypes.byref(prepared[i][3]), ctypes.sizeof(FearJpegScan))
                scans[d].coef_offset = values
                values += 64 * int(info.total_blocks)
                most = max(most, int(info.total_blocks))
                seg_prefix[d + 1] = seg_prefix[d] + scans[d].n_seg
                stage.add(f"bytes{k}", prepared[i][1])
                stage.add(f"seg{k}", prepared[i][2])
            else:
                stage.add(f"coef{k}", prepared[i][1])
                stage.add(f"start{k}", prepared[i][2])
            out_at.append(out_bytes)
            out_bytes += -(-sw * sh * 3 // 16) * 16
            # the staging is now the buffers' only holder and releases them in the order they were allocated; the list would release
            # them from its end, where malloc trims its heap at every free (25 ms more per call on 256 files of 1280 x 720)
            prepared[i] = None
        for i, px in raw.items():
            stage.add(f"raw{i}", px)
        table = np.zeros(-(-prefix.nbytes // 16) * 16 + ctypes.sizeof(records), dtype=np.uint8)
        table[:prefix.nbytes] = prefix.reshape(-1).view(np.uint8)
        stage.add("table", table)
        if nd:
            scan_table = np.zeros(-(-seg_prefix.nbytes // 16) * 16 + ctypes.sizeof(scans), dtype=np.uint8)
            scan_table[:seg_prefix.nbytes] = seg_prefix.view(np.uint8)
            stage.add("scans", scan_table)
        with torch.cuda.device(self.device):
            pinned = torch.empty(stage.nbytes, dtype=torch.uint8, pin_memory=True)
            dev = torch.empty(stage.nbytes, dtype=torch.uint8, device=self.device)
            out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=self.device)
            if nd:                                                    # the dense coefficients, their block_start table and the verdicts
                coef = torch.empty(values, dtype=torch.int16, device=self.device)
                dense_start = torch.empty(most + 1, dtype=torch.int32, device=self.device)
                status = torch.empty(nd, dtype=torch.int32, device=self.device)
            base, out_base = dev.data_ptr(), out.data_ptr()
            for k in range(n):
                if k in place:
                    d = place[k]
                    scans[d].bytes = base + stage.sections[f"bytes{k}"][0]
                    scans[d].seg_start = base + stage.sections[f"seg{k}"][0]
                    records[k].coef = coef.data_ptr() + 2 * scans[d].coef_offset
                    records[k].block_start = dense_start.data_ptr()
                else:
                    records[k].coef = base + stage.sections[f"coef{k}"][0]
                    records[k].block_start = base + stage.sections[f"start{k}"][0]
                records[k].out = out_base + out_at[k]
            if n:
                table[-ctypes.sizeof(records):] = np.frombuffer(records, dtype=np.uint8)
            if nd:
                scan_table[-ctypes.sizeof(scans):] = np.frombuffer(scans, dtype=np.uint8)
            stage.write(pinned.numpy())
            dev.copy_(pinned, non_blocking=True)
            self._pinned = self._pinned[-1:] + [pinned]
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if nd:
                launch(self._lib, "fear_jpeg_dense_block_start", ctypes.c_void_p(dense_start.data_ptr()), most, stream)
                launch(self._lib, "fear_jpeg_huffman", scans, nd, ctypes.c_void_p(base + stage.sections["scans"][0]),
                       ctypes.c_void_p(coef.data_ptr()), ctypes.c_void_p(status.data_ptr()), self.subsequence_bytes, stream)
            if n:
                ws_bytes = self._lib.fear_jpeg_decode_workspace_bytes(infos, n)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                _launch_pixels(self._lib, records, n, base + stage.sections["table"][0], ws.data_ptr(), ws_bytes, scale, stream)
            if nd:
                verdict = torch.empty(nd, dtype=torch.int32, pin_memory=True)
                verdict.copy_(status, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                self._pending = (self._pending + [(event, verdict, [(group[k], blobs[group[k]]) for k in on_device])])[-self.PENDING_CALLS:]
        for k, i in enumerate(group):
            h, w, _ = jpeg_scaled_shape(records[k].height, records[k].width, scale)
            frames[i] = out[out_at[k]:out_at[k] + h * w * 3].view(h, w, 3)
        for i, px in raw.items():
            at = stage.sections[f"raw{i}"][0]
            frames[i] = dev[at:at + px.nbytes].view(px.shape)

    def decode(self, items: Sequence[Item], fallback: Optional[Callable[[bytes], np.ndarray]] = None, check: bool = False,
               scale: int = 1) -> List:
        """`scale` 2, 4 or 8 decodes every file of the call at 1/2, 1/4 or 1/8 of its size in the DCT domain, as libjpeg's scale_denom
        and Pillow's `draft` do (`jpeg_decode_host(scale=)` is the statement, `jpeg_scaled_shape` the frames' shape): the coefficient
        stage is untouched, in both entropy modes and with `progressive=True`, and `fear_jpeg_decode_scaled_u8` takes the place of
        `fear_jpeg_decode_u8`.  A `fallback`'s pixels must then have the scaled shape (ValueError naming the item).  Another value of
        `scale` is a ValueError before anything is parsed."""
        scale = _check_scale(scale)
        blobs = _read_items(items)
        if not blobs:
            return []
        # the pool: the host's Huffman stage, or in device mode the scans prepared (a file too long for the device: the host's stage)
        device = self.entropy == "device"
        prepared = list(self._pool.map(self._prepare if device else self.entropy_decode, blobs))
        jpegs, raw = _judge(blobs, prepared, fallback, self.progressive, scale)
        if device:
            self.last_paths = ["device" if len(prepared[i]) == 4 else "host" for i in jpegs]
        # groups by the dense coefficients of the device-path images, 128 bytes per block; a host-path image needs none, so host
        # mode is one group
        groups, dense = [[]], 0
        for i in jpegs:
            need = 128 * int(prepared[i][0].total_blocks) if len(prepared[i]) == 4 else 0
            if groups[-1] and dense + need > self.workspace_limit:
                groups.append([])
                dense = 0
            groups[-1].append(i)
            dense += need
        frames: List = [None] * len(blobs)
        for g, group in enumerate(groups):
            if len(group) > 65535:
                raise ValueError("at most 65535 JPEG files per call")
            self._decode_group(blobs, prepared, group, raw if g == 0 else {}, frames, scale)
        if device and check:
            self.check()
        return frames
