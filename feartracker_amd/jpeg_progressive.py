"""Progressive JPEG files (SOF2) on the host ("Progressive files"): the Python statement of
csrc/fear_jpeg_progressive.h, check for check and in the same order.

`progressive_coefficients_host` decodes every scan of a file to quantised coefficients (ITU-T T.81 G.1 and G.2) — what
`fear_jpeg_progressive_decode` packs — and `jpeg_to_baseline_host` writes those coefficients again as a baseline file with a restart marker
after every MCU row, byte for byte `fear_jpeg_progressive_to_baseline`'s output.  `jpeg_frames.jpeg_info`, `jpeg_coefficients_host` and
`jpeg_decode_host` reach this module with `progressive=True`; tests/test_jpeg_progressive_host.py holds it to Pillow's pixels and the
library to it."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .jpeg_frames import MAX_SIDE, ZIGZAG, MalformedJPEG, UnsupportedJPEG, _Bits, _extend, _Header, _Huffman, _wrap16

MAX_SCANS = 100


class NotProgressive(UnsupportedJPEG):
    """The frame is not SOF2: the file is the baseline decoder's to judge."""


def _scan(data: bytes, p: int, hd: _Header, coef, comp, td, ta, Ss: int, Se: int, Ah: int, Al: int) -> int:
    """One scan's entropy-coded data from `p` on; returns where the marker behind it begins."""
    bits, ns = _Bits(data, p), len(comp)
    pred, eobrun = [0, 0, 0], 0
    ri, c0 = hd.restart, comp[0]
    across = hd.mcus_x if ns > 1 else hd.own_w[c0]
    units = hd.mcus_x * hd.mcus_y if ns > 1 else hd.own_w[c0] * hd.own_h[c0]
    p1, m1 = 1 << Al, -(1 << Al)

    def correct(blk, k):
        if bits.bit() and (int(blk[k]) & p1) == 0:
            blk[k] = _wrap16(int(blk[k]) + (p1 if blk[k] >= 0 else m1))

    for u in range(units):
        if ri and u and u % ri == 0:
            bits.restart((u // ri - 1) & 7)
            pred, eobrun = [0, 0, 0], 0
        uy, ux = divmod(u, across)
        if Ss == 0:                                                        # a DC scan: the MCU's blocks, or the one block
            for s, c in enumerate(comp):
                bh, bv = (hd.h[c], hd.v[c]) if ns > 1 else (1, 1)
                for j in range(bv):
                    for i in range(bh):
                        blk = coef[c][uy * bv + j, ux * bh + i]
                        if Ah == 0:
                            t = bits.symbol(hd.dc[td[s]])
                            if t > 15:
                                raise MalformedJPEG("a DC size above 15")
                            pred[c] = _wrap16(pred[c] + _extend(bits.bits(t), t))
                            blk[0] = _wrap16((pred[c] << Al) & 0xFFFFFFFF)
                        elif bits.bit():
                            blk[0] = _wrap16(int(blk[0]) | p1)
            continue
        blk, ac = coef[c0][uy, ux], hd.ac[ta[0]]
        if Ah == 0:                                                        # G.1.2.2: the first scan of a band
            if eobrun > 0:
                eobrun -= 1
                continue
            k = Ss
            while k <= Se:
                rs = bits.symbol(ac)
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    if k > Se:
                        raise MalformedJPEG("a coefficient index past the band")
                    blk[k] = _wrap16((_extend(bits.bits(s), s) << Al) & 0xFFFFFFFF)
                    k += 1
                elif r == 15:                                              # ZRL: a coefficient follows
                    if k + 16 > Se:
                        raise MalformedJPEG("a coefficient index past the band")
                    k += 16
                else:                                                      # EOBn: this block and eobrun more end here
                    eobrun = (1 << r) + bits.bits(r) - 1
                    break
            continue
        k = Ss                                                             # G.1.2.3: refinement
        if eobrun == 0:
            while k <= Se:
                rs = bits.symbol(ac)
                r, s, value = rs >> 4, rs & 15, 0
                if s:
                    if s != 1:
                        raise MalformedJPEG("a refinement symbol of a size other than 1")
                    value = p1 if bits.bit() else m1
                elif r != 15:
                    eobrun = (1 << r) + bits.bits(r)
                    break
                while k <= Se:                                             # the coefficients with a history, and r (ZRL: 16) without
                    if blk[k] != 0:
                        correct(blk, k)
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if s:
                    if k > Se:
                        raise MalformedJPEG("a coefficient index past the band")
                    blk[k] = value
                k += 1
        if eobrun > 0:
            while k <= Se:
                if blk[k] != 0:
                    correct(blk, k)
                k += 1
            eobrun -= 1
    return bits.pos                                                        # the rest of the byte is padding: a marker follows at once


def _run(data: bytes, headers_only: bool):
    """The whole file: (header, coefficients per component on the padded grid); with `headers_only`, the header behind the first SOS."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise MalformedJPEG("no SOI marker")
    hd = _Header()
    hd.q, hd.q_file, hd.dc, hd.ac, hd.restart, hd.adobe, sof = {}, {}, {}, {}, 0, -1, False
    hd.jfif, hd.adobe_segment, hd.scans, coef, nf = b"", b"", 0, None, 0
    p = 2
    while True:
        if p >= n or data[p] != 0xFF:
            raise MalformedJPEG("a marker was expected" if p < n else "truncated before EOI")
        while p < n and data[p] == 0xFF:            # fill bytes
            p += 1
        if p >= n:
            raise MalformedJPEG("truncated in a marker")
        m = data[p]
        p += 1
        if m == 0x01:                               # TEM stands alone
            continue
        if m == 0xD9:
            if hd.scans == 0:
                raise MalformedJPEG("EOI in front of the first scan")
            break
        if m == 0x00 or 0xD0 <= m <= 0xD8:
            raise MalformedJPEG(f"marker FF{m:02X} between the segments")
        if p + 2 > n:
            raise MalformedJPEG("truncated in a segment length")
        L = (data[p] << 8) | data[p + 1]
        if L < 2 or p + L > n:
            raise MalformedJPEG("a segment length runs past the end")
        seg, whole = data[p + 2:p + L], data[p - 2:p + L]
        p += L
        if m == 0xC2:                               # jpeg_frames._parse's SOF0 rules
            if sof:
                raise MalformedJPEG("a second frame header")
            if len(seg) < 6:
                raise MalformedJPEG("short SOF2")
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
                raise MalformedJPEG("SOF2 length")
            hd.ids, hd.h, hd.v, hd.tq, hd.hv = [], [], [], [], []
            for i in range(nf):
                cid, hv, tq = seg[6 + 3 * i:9 + 3 * i]
                h, v = hv >> 4, hv & 15
                if not (1 <= h <= 4 and 1 <= v <= 4) or tq > 3 or cid in hd.ids:
                    raise MalformedJPEG("a component's sampling factors, table or id")
                hd.ids.append(cid); hd.h.append(h); hd.v.append(v); hd.tq.append(tq); hd.hv.append(hv)
            if nf == 1:
                hd.h, hd.v = [1], [1]
            elif (hd.h[0], hd.v[0]) not in ((1, 1), (2, 1), (2, 2)) or (hd.h[1], hd.v[1], hd.h[2], hd.v[2]) != (1, 1, 1, 1):
                raise UnsupportedJPEG("sampling factors other than 4:4:4, 4:2:2 and 4:2:0")
            hd.mcus_x = -(-hd.width // (8 * hd.h[0]))
            hd.mcus_y = -(-hd.height // (8 * hd.v[0]))
            hd.blocks_w = [hd.mcus_x * h for h in hd.h]
            hd.blocks_h = [hd.mcus_y * v for v in hd.v]
            hd.own_w = [-(-(-(-hd.width * h // hd.h[0])) // 8) for h in hd.h]        # a component's own block grid
            hd.own_h = [-(-(-(-hd.height * v // hd.v[0])) // 8) for v in hd.v]
            hd.coef_bits = [[-1] * 64 for _ in range(nf)]
            sof = True
        elif 0xC0 <= m <= 0xCF and m != 0xC4:
            raise NotProgressive("a baseline frame" if m == 0xC0 else "arithmetic coding" if m == 0xCC else f"SOF{m - 0xC0} frame")
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
            if hd.scans:
                raise UnsupportedJPEG("a quantiser table after the first scan")
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                if pq == 1:
                    raise UnsupportedJPEG("16-bit quantiser table")
                if pq > 1 or tq > 3 or s + 65 > len(seg):
                    raise MalformedJPEG("DQT header")
                table = np.zeros(64, dtype=np.int64)
                table[ZIGZAG] = np.frombuffer(seg[s + 1:s + 65], dtype=np.uint8)
                hd.q[tq], hd.q_file[tq] = table, seg[s + 1:s + 65]
                s += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise MalformedJPEG("DRI length")
            hd.restart = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise UnsupportedJPEG("DNL segment")
        elif m == 0xE0:
            if hd.scans == 0 and len(seg) >= 5 and seg[:5] == b"JFIF\x00":
                hd.jfif = whole
        elif m == 0xEE:
            if hd.scans == 0 and len(seg) >= 12 and seg[:5] == b"Adobe":
                hd.adobe, hd.adobe_segment = seg[11], whole
        elif m == 0xDA:
            if not sof:
                raise MalformedJPEG("SOS in front of SOF")
            if len(seg) < 1 or seg[0] == 0 or seg[0] > 4:
                raise MalformedJPEG("SOS component count")
            ns = seg[0]
            if ns > nf or len(seg) != 4 + 2 * ns:
                raise MalformedJPEG("SOS length")
            if hd.scans == MAX_SCANS:
                raise UnsupportedJPEG(f"more than {MAX_SCANS} scans")
            comp, td, ta = [], [], []
            for i in range(ns):
                cs, t = seg[1 + 2 * i], seg[2 + 2 * i]
                c = comp[-1] + 1 if i else 0                               # a subset of the frame's, in frame order
                while c < nf and hd.ids[c] != cs:
                    c += 1
                if c >= nf:
                    raise MalformedJPEG("a scan component the frame does not have, or out of frame order")
                if (t >> 4) > 3 or (t & 15) > 3:
                    raise MalformedJPEG("Huffman table selector")
                comp.append(c); td.append(t >> 4); ta.append(t & 15)
            Ss, Se, Ah, Al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if (Se != 0) if Ss == 0 else (ns != 1 or Se < Ss or Se > 63):
                raise MalformedJPEG("spectral selection of a progressive scan")
            if Al > 13 or (Ah != 0 and Ah != Al + 1):
                raise MalformedJPEG("successive approximation of a progressive scan")
            if hd.scans == 0:
                if nf == 3 and hd.adobe == 0:
                    raise UnsupportedJPEG("Adobe transform 0: RGB samples")
                for i in range(nf):
                    if hd.tq[i] not in hd.q:
                        raise MalformedJPEG("a component selects a quantiser table no segment defined")
                hd.qt = np.stack([hd.q[t] for t in hd.tq]).astype(np.uint16)
            for i in range(ns):
                if Ss == 0 and Ah == 0 and td[i] not in hd.dc:
                    raise MalformedJPEG("a scan selects a DC table no segment defined")
                if Ss > 0 and ta[i] not in hd.ac:
                    raise MalformedJPEG("a scan selects an AC table no segment defined")
            for c in comp:                                                 # the progression, as libjpeg's coef_bits tracks it
                cb = hd.coef_bits[c]
                if Ss > 0 and cb[0] < 0:
                    raise UnsupportedJPEG("inconsistent progression: an AC scan in front of the component's DC scan")
                for k in range(Ss, Se + 1):
                    if (cb[k] >= 0) if Ah == 0 else (cb[k] != Ah):
                        raise UnsupportedJPEG("inconsistent progression: a scan does not continue where the coefficient stands")
                    cb[k] = Al
            if headers_only:
                return hd, None
            if hd.scans == 0:
                coef = [np.zeros((hd.blocks_h[c], hd.blocks_w[c], 64), dtype=np.int16) for c in range(nf)]
            hd.scans += 1
            p = _scan(data, p, hd, coef, comp, td, ta, Ss, Se, Ah, Al)
        # the other APPn, COM and the reserved markers carry nothing the decoder needs
    if any(b != 0 for cb in hd.coef_bits for b in cb):
        raise UnsupportedJPEG("incomplete progression: libjpeg would smooth the blocks")
    hd.restart = 0                                                         # what the baseline decoders read of the header: no interval
    return hd, coef


def _bit_length(v: int) -> int:
    return int(abs(v)).bit_length()


def _baseline_walk(hd: _Header, coef, put, restart) -> None:
    """The coefficients as the symbols of one interleaved baseline scan with a restart after every MCU row: put(ac, table, symbol, bits,
    value) per code, restart(k) in front of every MCU row but the first.  UnsupportedJPEG for a value the baseline alphabet lacks."""
    nf = len(hd.ids)
    for my in range(hd.mcus_y):
        pred = [0, 0, 0]
        if my:
            restart((my - 1) & 7)
        for mx in range(hd.mcus_x):
            for c in range(nf):
                t = 1 if c else 0
                for j in range(hd.v[c]):
                    for i in range(hd.h[c]):
                        blk = coef[c][my * hd.v[c] + j, mx * hd.h[c] + i].tolist()
                        diff = blk[0] - pred[c]
                        pred[c] = blk[0]
                        if not -2047 <= diff <= 2047:
                            raise UnsupportedJPEG("coefficients beyond the baseline alphabet: a DC difference outside +-2047")
                        cat = _bit_length(diff)
                        put(0, t, cat, cat, diff - 1 if diff < 0 else diff)
                        r = 0
                        for k in range(1, 64):
                            v = blk[k]
                            if v == 0:
                                r += 1
                                continue
                            if not -1023 <= v <= 1023:
                                raise UnsupportedJPEG("coefficients beyond the baseline alphabet: an AC term outside +-1023")
                            while r > 15:
                                put(1, t, 0xF0, 0, 0)
                                r -= 16
                            s = _bit_length(v)
                            put(1, t, r << 4 | s, s, v - 1 if v < 0 else v)
                            r = 0
                        if r > 0:
                            put(1, t, 0, 0, 0)


def optimal_table(freq: List[int]) -> Tuple[List[int], List[int]]:
    """T.81 K.2 as libjpeg's jpeg_gen_optimal_table states it: (the 16 counts, the symbols) from 256 symbol counts."""
    freq = list(freq) + [1]                                                # symbol 256 is reserved: no code is all ones
    bits, codesize, others = [0] * 258, [0] * 257, [-1] * 257
    while True:
        c1, c2, v = -1, -1, 0xFFFFFFFF
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        v = 0xFFFFFFFF
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(257, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    last = 16
    while bits[last] == 0:
        last -= 1
    bits[last] -= 1                                                        # the reserved symbol's code
    values = [j for length in range(1, 257) for j in range(256) if codesize[j] == length]
    return bits[1:17], values


class _Writer:
    def __init__(self):
        self.out, self.acc, self.have, self.code = bytearray(), 0, 0, {}

    def word(self, v: int) -> None:
        self.out += bytes([v >> 8, v & 255])

    def push(self, v: int, k: int) -> None:
        self.acc = (self.acc << k) | (v & ((1 << k) - 1))
        self.have += k
        while self.have >= 8:
            b = (self.acc >> (self.have - 8)) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.have -= 8
        self.acc &= 0xFF

    def flush(self) -> None:
        if self.have:
            self.push(0xFF, 8 - self.have)                                 # ones up to the byte boundary

    def put(self, ac: int, t: int, symbol: int, k: int, value: int) -> None:
        code, size = self.code[ac, t, symbol]
        self.push(code, size)
        self.push(value, k)

    def restart(self, k: int) -> None:
        self.flush()
        self.out += bytes([0xFF, 0xD0 + k])

    def table(self, ac: int, t: int, counts: List[int], values: List[int]) -> None:
        self.out += b"\xFF\xC4"
        self.word(2 + 1 + 16 + len(values))
        self.out += bytes([ac << 4 | t]) + bytes(counts) + bytes(values)
        c = k = 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                self.code[ac, t, values[k]] = (c, length)
                c += 1
                k += 1
            c <<= 1


def progressive_info(data: bytes) -> _Header:
    """The header `fear_jpeg_progressive_parse` reads: a baseline file's of that frame, without a restart interval."""
    hd, _ = _run(bytes(data), True)
    hd.restart = 0
    return hd


def progressive_coefficients_host(data: bytes):
    """(_Header, per component (blocks_h, blocks_w, 64) int16 in zigzag order): `jpeg_frames.jpeg_coefficients_host` of a progressive file.
    The verdict includes the transcoder's: values a baseline scan cannot carry are declined here as well."""
    hd, coef = _run(bytes(data), False)
    _baseline_walk(hd, coef, lambda *a: None, lambda k: None)
    return hd, coef


def jpeg_to_baseline_host(data: bytes) -> bytes:
    """A progressive file -> a baseline file of the same coefficients, byte for byte `fear_jpeg_progressive_to_baseline`'s: SOI, the JFIF
    and Adobe segments, DQT, SOF0, DHT (T.81 K.2 per file), DRI = mcus_x, one interleaved SOS, RSTn after every MCU row, EOI."""
    data = bytes(data)
    hd, coef = _run(data, False)
    nf = len(hd.ids)
    freq = {(ac, t): [0] * 256 for ac in range(2) for t in range(2)}

    def count(ac, t, symbol, k, value):
        freq[ac, t][symbol] += 1

    _baseline_walk(hd, coef, count, lambda k: None)
    w = _Writer()
    w.out += b"\xFF\xD8" + hd.jfif + hd.adobe_segment
    for c in range(nf):                                                    # every quantiser table a component selects, once
        if hd.tq[c] not in hd.tq[:c]:
            w.out += b"\xFF\xDB\x00\x43" + bytes([hd.tq[c]]) + bytes(hd.q_file[hd.tq[c]])
    w.out += b"\xFF\xC0"
    w.word(8 + 3 * nf)
    w.out.append(8)
    w.word(hd.height)
    w.word(hd.width)
    w.out.append(nf)
    for c in range(nf):
        w.out += bytes([hd.ids[c], hd.hv[c], hd.tq[c]])
    for t in range(2 if nf == 3 else 1):
        for ac in range(2):
            w.table(ac, t, *optimal_table(freq[ac, t]))
    w.out += b"\xFF\xDD\x00\x04"
    w.word(hd.mcus_x)
    w.out += b"\xFF\xDA"
    w.word(6 + 2 * nf)
    w.out.append(nf)
    for c in range(nf):
        w.out += bytes([hd.ids[c], 0x11 if c else 0x00])
    w.out += b"\x00\x3F\x00"
    _baseline_walk(hd, coef, w.put, w.restart)
    w.flush()
    w.out += b"\xFF\xD9"
    return bytes(w.out)
