"""Plumbing shared by the tests of the store's windows (test_jpeg_windows_host, test_jpeg_windows_gpu, test_train_pairs_windows_gpu,
test_loader_windows_gpu): the files, written with Pillow once per session, and the windows of a frame that the tests walk.  A plain
module, imported by name as jpegrows is."""
import io

import numpy as np

MODES = (("420", "4:2:0"), ("422", "4:2:2"), ("444", "4:4:4"), ("gray", None))
NOISE = "noise_400x48_420_q95"
_files = None


def _picture(width, height, seed, noise):
    """A gradient with a few edges under `noise` levels of noise: every block has its own coefficients."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    base = np.stack([(3 * x + 2 * y) % 256, (5 * y + x * x // 7) % 256, (255 - 2 * x + 3 * y) % 256], axis=2).astype(np.int64)
    base[height // 3:, width // 2:] = 255 - base[height // 3:, width // 2:]
    return np.clip(base + rng.integers(-noise, noise + 1, base.shape), 0, 255).astype(np.uint8)


def _write(pixels, subsampling, quality=90, **kw):
    from PIL import Image
    image = Image.fromarray(pixels if subsampling is not None else pixels[:, :, 1])
    out = io.BytesIO()
    if subsampling is not None:
        kw["subsampling"] = subsampling
    image.save(out, "JPEG", quality=quality, **kw)
    return out.getvalue()


def files():
    """[(name, the file's bytes, progressive?)]: 4:2:0, 4:2:2, 4:4:4 and gray, each at 50 x 37 and 97 x 65 (no multiple of an MCU), each
    with and without a restart marker after every MCU row; a progressive 4:2:0 file; one 400 x 48 noise file at quality 95, whose MCU
    rows span many 128-byte subsequences; one 8 x 8 file."""
    global _files
    if _files is None:
        out = []
        for k, (name, subsampling) in enumerate(MODES):
            for width, height in ((50, 37), (97, 65)):
                pixels = _picture(width, height, 10 * k + width, 12)
                out.append((f"{width}x{height}_{name}", _write(pixels, subsampling), False))
                out.append((f"{width}x{height}_{name}_restart", _write(pixels, subsampling, restart_marker_rows=1), False))
        out.append(("97x65_420_progressive", _write(_picture(97, 65, 77, 12), "4:2:0", progressive=True), True))
        out.append((NOISE, _write(_picture(400, 48, 5, 120), "4:2:0", quality=95), False))
        out.append(("8x8_420", _write(_picture(8, 8, 3, 12), "4:2:0"), False))
        _files = out
    return _files


def unsupported():
    """A file the decoder declines as unsupported (four components): what a store keeps as decoded pixels, given a fallback."""
    from PIL import Image
    out = io.BytesIO()
    Image.new("CMYK", (24, 16), (10, 20, 30, 40)).save(out, "JPEG")
    return out.getvalue()


def sampling(name):
    """(h, v) of the luma component of the file with this name."""
    return (2, 2) if "_420" in name else ((2, 1) if "_422" in name else (1, 1))


def named(name):
    return next(f for f in files() if f[0] == name)


def windows(H, W, mcu_h, mcu_w):
    """(y0, y1, x0, x1) windows of an H x W frame whose MCUs are mcu_h x mcu_w pixels (all in pixels of the frame as it is decoded): the
    whole frame, a single pixel at each corner, one inside one MCU, one ending on an MCU boundary, one starting on one, one reaching the
    true right and bottom edges, one whose columns begin in the middle of an MCU row (and so, in a file whose rows span several
    subsequences, in the middle of a subsequence), one that leaves the frame on every side, and the empty window."""
    out = [(0, H, 0, W),
           (0, 1, 0, 1), (0, 1, W - 1, W), (H - 1, H, 0, 1), (H - 1, H, W - 1, W),
           (min(1, H - 1), min(3, H), min(2, W - 1), min(5, W)),
           (max(mcu_h - 3, 0), mcu_h, max(mcu_w - 5, 0), mcu_w),
           (mcu_h, mcu_h + 5, mcu_w, mcu_w + 7),
           (max(H - 5, 0), H, max(W - 9, 0), W),
           (H // 2, H // 2 + 3, W // 2 + 1, W // 2 + 4),
           (-4, H + 9, -2, W + 3),
           (5, 5, 0, 10)]
    return np.array(out, dtype=np.int64)


def clipped(window, H, W):
    y0, y1, x0, x1 = (int(v) for v in window)
    y0, y1, x0, x1 = min(max(y0, 0), H), min(max(y1, 0), H), min(max(x0, 0), W), min(max(x1, 0), W)
    return (y0, y1, x0, x1) if y0 < y1 and x0 < x1 else (0, 0, 0, 0)
