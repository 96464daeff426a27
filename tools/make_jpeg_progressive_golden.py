"""Writes tests/golden/jpeg_progressive.npz: small progressive JPEG files, their baseline twins and what Pillow (libjpeg-turbo) decodes
them to — the fixture jpeg_progressive.py and csrc/fear_jpeg_progressive.h are held to ("Progressive files").
Needs Pillow.

    python tools/make_jpeg_progressive_golden.py

Pillow-made grid: five sizes (W, H) by four modes, each pair once; content (smooth | noise), quality (30 | 75 | 95) and option (plain |
restart_marker_blocks=3 | restart_marker_rows=1) cycle across the cases.  One 512 x 512 gray image, flat but for a small patch: long EOB
runs.  Three files that Pillow did not write ("written_..."): `write_progressive` below codes the coefficients of a baseline file under a
given scan script with that file's own (Annex K) Huffman tables — spectral selection alone, DC scans one component at a time, and the full
approximation Al = 2 -> 1 -> 0 on every band with restart markers in the AC scans.
The file holds `names`, and per case i `jpg_i` (the progressive file), `px_i` (Pillow's convert("RGB") of it, (H, W, 3) uint8) and
`base_i` (the baseline file of the same image, quality and sampling: the same coefficients)."""
import io
import os
import sys

import numpy as np
from PIL import Image, ImageFile, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feartracker_amd.jpeg_frames import ZIGZAG, jpeg_coefficients_host  # noqa: E402
from feartracker_amd.jpeg_progressive import _Writer  # noqa: E402

ImageFile.MAXBLOCK = 1 << 24              # a progressive save needs the whole file in one buffer ("Suspension not allowed here")
SIZES = ((1, 1), (8, 8), (17, 9), (33, 31), (130, 70))
MODES = ("444", "422", "420", "gray")
QUALITIES = (30, 75, 95)
OPTIONS = ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})
OPTION_NAMES = ("plain", "rst3", "rstrows1")
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_progressive.npz")


def content(kind, w, h, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + 2 * yy) * 5) % 256], axis=-1).astype(np.uint8)


def encode(rgb, mode, quality, **options):
    buf = io.BytesIO()
    if mode == "gray":
        Image.fromarray(rgb).convert("L").save(buf, format="JPEG", quality=quality, **options)
    else:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[mode], **options)
    return buf.getvalue()


def pillow_pixels(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


class _Coder(_Writer):
    """jpeg_progressive's bit writer with a decoder's table (_Huffman) turned round."""

    def symbol(self, table, value):
        k = table.values.index(value)
        length = next(n for n in range(1, 17) if table.index[n] <= k < table.index[n] + table.counts[n])
        self.push(table.first[length] + k - table.index[length], length)


def write_progressive(base, script):
    """The coefficients of the baseline file `base` as a progressive file.  `script` lists the scans: (components, Ss, Se, Ah, Al,
    restart interval).  No EOB runs (every block ends with its own EOB), so the baseline file's tables have every symbol."""
    hd, coef = jpeg_coefficients_host(base)
    nf = len(hd.ids)
    out = bytearray(b"\xFF\xD8\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tq in sorted(hd.q):
        out += b"\xFF\xDB\x00\x43" + bytes([tq]) + bytes(int(v) for v in hd.q[tq][ZIGZAG])
    hv = [(hd.h[c] << 4) | hd.v[c] for c in range(nf)]
    out += b"\xFF\xC2" + bytes([0, 8 + 3 * nf, 8, hd.height >> 8, hd.height & 255, hd.width >> 8, hd.width & 255, nf])
    for c in range(nf):
        out += bytes([hd.ids[c], hv[c], hd.tq[c]])
    for tc, tables in ((0, hd.dc), (1, hd.ac)):
        for th, t in sorted(tables.items()):
            out += b"\xFF\xC4" + bytes([0, 19 + len(t.values), tc << 4 | th]) + bytes(t.counts[1:]) + bytes(t.values)
    own_w = [-(-(-(-hd.width * h // hd.h[0])) // 8) for h in hd.h]
    own_h = [-(-(-(-hd.height * v // hd.v[0])) // 8) for v in hd.v]
    for comps, Ss, Se, Ah, Al, ri in script:
        out += b"\xFF\xDD\x00\x04" + bytes([ri >> 8, ri & 255])
        out += b"\xFF\xDA" + bytes([0, 6 + 2 * len(comps), len(comps)])
        for c in comps:
            out += bytes([hd.ids[c], hd.td[c] << 4 | hd.ta[c]])
        out += bytes([Ss, Se, Ah << 4 | Al])
        w = _Coder()
        if len(comps) > 1:
            units = [[(c, my * hd.v[c] + j, mx * hd.h[c] + i) for c in comps for j in range(hd.v[c]) for i in range(hd.h[c])]
                     for my in range(hd.mcus_y) for mx in range(hd.mcus_x)]
        else:
            c = comps[0]
            units = [[(c, y, x)] for y in range(own_h[c]) for x in range(own_w[c])]
        pred = [0] * nf
        for u, blocks in enumerate(units):
            if ri and u and u % ri == 0:
                w.restart((u // ri - 1) & 7)
                pred = [0] * nf
            for c, y, x in blocks:
                blk = [int(v) for v in coef[c][y, x]]
                if Ss == 0 and Ah == 0:
                    val = blk[0] >> Al
                    diff, pred[c] = val - pred[c], val
                    cat = abs(diff).bit_length()
                    w.symbol(hd.dc[hd.td[c]], cat)
                    w.push(diff - 1 if diff < 0 else diff, cat)
                elif Ss == 0:
                    w.push((blk[0] >> Al) & 1, 1)
                elif Ah == 0:
                    ac, r = hd.ac[hd.ta[c]], 0
                    for k in range(Ss, Se + 1):
                        a = abs(blk[k]) >> Al
                        if a == 0:
                            r += 1
                            continue
                        while r > 15:
                            w.symbol(ac, 0xF0)
                            r -= 16
                        s = a.bit_length()
                        w.symbol(ac, r << 4 | s)
                        w.push(~a if blk[k] < 0 else a, s)
                        r = 0
                    if r > 0:
                        w.symbol(ac, 0)
                else:                                                  # T.81 G.1.2.3, every block closed with its own EOB
                    ac, r, pending = hd.ac[hd.ta[c]], 0, []
                    mags = [abs(v) >> Al for v in blk]
                    new = [k for k in range(Ss, Se + 1) if mags[k] == 1]
                    last_new = new[-1] if new else -1
                    for k in range(Ss, Se + 1):
                        a = mags[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= last_new:
                            w.symbol(ac, 0xF0)
                            r -= 16
                            for b in pending:
                                w.push(b, 1)
                            pending = []
                        if a > 1:
                            pending.append(a & 1)
                            continue
                        w.symbol(ac, r << 4 | 1)
                        w.push(0 if blk[k] < 0 else 1, 1)
                        for b in pending:
                            w.push(b, 1)
                        pending, r = [], 0
                    if r > 0 or pending:
                        w.symbol(ac, 0)
                        for b in pending:
                            w.push(b, 1)
        w.flush()
        out += w.out
    return bytes(out + b"\xFF\xD9")


def written(rng):
    all3 = (0, 1, 2)
    spectral = [(all3, 0, 0, 0, 0, 0), ((0,), 1, 5, 0, 0, 0), ((0,), 6, 63, 0, 0, 0), ((1,), 1, 63, 0, 0, 0), ((2,), 1, 63, 0, 0, 0)]
    dc_alone = ([((c,), 0, 0, 0, 1, 0) for c in all3] + [((c,), 1, 63, 0, 0, 0) for c in all3] + [((c,), 0, 0, 1, 0, 0) for c in all3])
    full = [(all3, 0, 0, 0, 2, 0), (all3, 0, 0, 2, 1, 2), (all3, 0, 0, 1, 0, 0)]
    for c in all3:
        for lo, hi in ((1, 5), (6, 63)):
            full += [((c,), lo, hi, 0, 2, 3), ((c,), lo, hi, 2, 1, 3), ((c,), lo, hi, 1, 0, 5)]
    return [("written_33x31_420_smooth_q75_spectral", encode(content("smooth", 33, 31, rng), "420", 75), spectral),
            ("written_17x9_422_noise_q75_dcalone", encode(content("noise", 17, 9, rng), "422", 75), dc_alone),
            ("written_33x31_444_noise_q75_approx210_rst", encode(content("noise", 33, 31, rng), "444", 75), full)]


def cases():
    rng = np.random.default_rng(20241019)
    out, i = [], 0
    for w, h in SIZES:
        for mode in MODES:
            kind, quality, opt = ("smooth", "noise")[i % 2], QUALITIES[(i // 2) % 3], (i + i // 4) % 3
            rgb = content(kind, w, h, rng)
            out.append((f"{w}x{h}_{mode}_{kind}_q{quality}_{OPTION_NAMES[opt]}", encode(rgb, mode, quality, progressive=True, **OPTIONS[opt]),
                        encode(rgb, mode, quality)))
            i += 1
    flat = np.full((512, 512, 3), 90, dtype=np.uint8)
    flat[200:215, 300:322] = rng.integers(0, 256, (15, 22, 3), dtype=np.uint8)
    out.append(("512x512_gray_flatpatch_q75_plain", encode(flat, "gray", 75, progressive=True), encode(flat, "gray", 75)))
    for name, base, script in written(rng):
        out.append((name, write_progressive(base, script), base))
    return out


def main():
    if not features.check_feature("libjpeg_turbo"):
        print("warning: this Pillow is not linked against libjpeg-turbo", file=sys.stderr)
    made = cases()
    arrays = dict(names=np.array([name for name, _, _ in made]))
    for i, (name, data, base) in enumerate(made):
        arrays[f"jpg_{i}"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"base_{i}"] = np.frombuffer(base, dtype=np.uint8)
        arrays[f"px_{i}"] = pillow_pixels(data)
        if not np.array_equal(arrays[f"px_{i}"], pillow_pixels(base)):
            print(f"warning: {name}: Pillow decodes the progressive file and its baseline twin differently", file=sys.stderr)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", len(made), "cases; Pillow", Image.__version__, "jpeg", features.version_codec("jpg"))


if __name__ == "__main__":
    main()
