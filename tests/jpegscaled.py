"""Plumbing shared by the tests of reduced-size JPEG decoding (test_jpeg_scaled_host, test_jpeg_scaled_gpu): the fixture
tests/golden/jpeg_scaled.npz (tools/make_jpeg_scaled_golden.py) next to jpeg_decode.npz, whose files it names.  A plain module, imported
by name as jpegdec is."""
import os

import numpy as np

import jpegdec

GOLDEN = os.path.join(jpegdec.HERE, "golden", "jpeg_scaled.npz")
SCALES = (2, 4, 8)
_loaded = None
_model = {}


def _load():
    global _loaded
    if _loaded is None:
        with np.load(GOLDEN) as d:
            new = [(str(name), d[f"jpg_{i}"].tobytes()) for i, name in enumerate(d["names"])]
            pinned = {str(key): d[f"px_{k}"] for k, key in enumerate(d["keys"])}
        for px in pinned.values():
            px.setflags(write=False)
        _loaded = (new, pinned)
    return _loaded


def new_files():
    """[(name, bytes)] of the files the scaled fixture adds; the last is progressive."""
    return _load()[0]


def files(progressive=False):
    """[(name, bytes)]: the 43 supported files of jpeg_decode.npz and the new baseline files; with `progressive` the progressive twin too."""
    out = [(name, data) for name, data, _ in jpegdec.supported()]
    return out + [(name, data) for name, data in new_files() if progressive or "progressive" not in name]


def pinned():
    """{"<name>@<scale>": Pillow's pixels}."""
    return _load()[1]


def expected(name, data, scale):
    """(pixels, pinned to Pillow?): the fixture's pixels, or the host model's where Pillow's draft cannot take the scale.  Computed
    once, shared and read-only."""
    key = f"{name}@{scale}"
    if key in pinned():
        return pinned()[key], True
    if key not in _model:
        from feartracker_amd import jpeg_decode_host
        _model[key] = jpeg_decode_host(data, progressive="progressive" in name, scale=scale)
        _model[key].setflags(write=False)
    return _model[key], False
