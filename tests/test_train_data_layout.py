"""The layout of the data stage (feartracker_amd/train_data/): the host restatement against digests recorded before the module became a
package (tests/golden/train_data_digests.json, tools/make_train_data_digest.py), the staging packer, the JPEG record split, the record
dtypes against their literals, and the names the package exports.  No GPU."""
import importlib
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest

from feartracker_amd import train_data as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_train_data_digest", os.path.join(ROOT, "tools", "make_train_data_digest.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


# ------------------------------------------------------------------------------------------------------------- host restatement
@pytest.mark.parametrize("name", list(recorder.CONFIGS))
def test_build_host_equals_the_recorded_digest(name):
    with open(os.path.join(ROOT, "tests", "golden", "train_data_digests.json")) as f:
        recorded = json.load(f)
    builder, frames, pairs, params = recorder.scenario(recorder.CONFIGS[name])
    assert [f.shape[:2] for f in frames] == [(40, 56), (97, 61)] and len(pairs) == 8
    assert (pairs[:, 1] < 0).any() and (pairs[:, 5] >= len(frames)).any() and (pairs[:, 10] == 0).any()
    for member in builder.colour_members:                                   # coverage does not depend on the seed
        assert (params.colour == td.COLOUR_MEMBERS[member]).any(), member
    assert set(params.tone.tolist()) == {td.TONE_NONE, td.TONE_GRAY, td.TONE_SEPIA}
    if builder.config["photometric"]:
        assert set(params.photo.blur.reshape(-1).tolist()) == {0, 1, 2, 3, 4}
        assert set(params.photo.noise.reshape(-1).tolist()) == {0} | {td.NOISE_MEMBERS[m] for m in builder.noise_members}
    else:
        assert params.photo is None
    batch = builder.build_host(frames, pairs, params)
    assert len(batch) == 6
    assert recorder.digest(batch) == recorded[name]


# ------------------------------------------------------------------------------------------------------------------------ packer
SECTION_BYTES = (0, 1, 7, 96, 768 * 3)


@pytest.mark.parametrize("align", [16, 4, 64])
def test_packer_layout(align):
    rng = np.random.default_rng(align)
    for order in list(itertools.permutations(range(5)))[::7]:
        stage = td.Staging()
        data = {}
        for i in order:
            data[f"s{i}"] = rng.integers(0, 256, SECTION_BYTES[i], dtype=np.uint8)
            stage.add(f"s{i}", data[f"s{i}"], align=align)
        spans = sorted((off, off + a.nbytes) for off, a in stage.sections.values())
        assert all(off % align == 0 for off, _ in spans)
        assert all(prev_end <= off for (_, prev_end), (off, _) in zip(spans, spans[1:]))
        assert stage.nbytes >= max(spans[-1][1], 16)
        out = np.full(stage.nbytes + 8, 0xEE, dtype=np.uint8)
        stage.write(out)
        assert np.all(out[stage.nbytes:] == 0xEE)
        for name, (off, a) in stage.sections.items():
            assert np.array_equal(out[off:off + a.nbytes], data[name]), name


def test_packer_takes_records_and_transposes():
    """Structured and non-contiguous arrays go in as the bytes of their C-contiguous form; the default alignment is 16."""
    ops = np.zeros((3, 2), dtype=td.PHOTO_DTYPE)
    ops["ksize"] = np.arange(6).reshape(3, 2)
    stage = td.Staging()
    stage.add("odd", np.zeros(5, np.uint8))
    stage.add("ops", ops.T)
    stage.add("taps", np.zeros((0, 49), np.float32))
    off = stage.sections["ops"][0]
    assert off == 16 and stage.sections["taps"][0] % 16 == 0
    out = np.zeros(stage.nbytes, dtype=np.uint8)
    stage.write(out)
    back = out[off:off + ops.nbytes].view(td.PHOTO_DTYPE).reshape(2, 3)
    assert np.array_equal(back["ksize"], ops["ksize"].T)                      # the templates' records first, then the searches'


def test_empty_packer_still_has_a_buffer():
    stage = td.Staging()
    assert stage.nbytes >= 16
    stage.write(np.zeros(stage.nbytes, dtype=np.uint8))
    stage.add("nothing", np.zeros(0, np.float32))
    assert stage.nbytes >= 16


# ------------------------------------------------------------------------------------------------------------- JPEG record split
def test_jpeg_record_split():
    rng = np.random.default_rng(3)
    B = 6
    ops = np.zeros((B, 2), dtype=td.PHOTO_DTYPE)
    ops["blur"], ops["ksize"] = rng.integers(0, 5, (B, 2)), 3 + 2 * rng.integers(0, 3, (B, 2))
    ops["noise"] = np.arange(2 * B).reshape(B, 2) % 4                         # none, multiplicative, gauss, JPEG in turn
    ops["scale"], ops["key"] = rng.uniform(0.9, 6.0, (B, 2)), rng.integers(0, 2 ** 32, (B, 2, 2))
    ops["downscale"] = (np.arange(2 * B).reshape(B, 2) // 4) % 2              # JPEG crops with and without Downscale
    ops["tap_row"] = rng.integers(-1, 3, (B, 2))
    quality = rng.integers(50, 101, (B, 2)).astype(np.int32)
    before = ops.copy()
    first, tail, q = td.split_jpeg_records(ops, quality)
    drew = before["noise"] == td.NOISE_JPEG
    assert drew.any() and not drew.all() and before["downscale"][drew].any() and not before["downscale"][drew].all()
    assert np.array_equal(ops, before)                                        # the argument is left alone
    assert first.dtype == tail.dtype == td.PHOTO_DTYPE and first.shape == tail.shape == (B, 2)
    assert np.all(first["noise"][drew] == td.NOISE_NONE) and np.all(first["downscale"][drew] == 0)
    assert np.array_equal(first[~drew], before[~drew])
    for name in ("blur", "ksize", "scale", "key", "tap_row"):
        assert np.array_equal(first[name], before[name]), name
    assert np.array_equal(tail["downscale"], np.where(drew, before["downscale"], 0)) and np.all(tail["tap_row"] == -1)
    for name in ("blur", "ksize", "noise", "scale", "key"):
        assert not tail[name].any(), name
    assert q.dtype == np.int32 and np.array_equal(q, np.where(drew, quality, 0))


# ------------------------------------------------------------------------------------------------------------------------ dtypes
LITERALS = {
    "GEOM_DTYPE": (96, [("t_frame", "<i4"), ("s_frame", "<i4"), ("t_ctx", "<i4", 4), ("s_ctx", "<i4", 4), ("box", "<i4", 4),
                        ("presence", "<i4"), ("tone", "<i4"), ("inv", "<f8", 4)]),
    "FRAME_DTYPE": (16, [("data", "<u8"), ("h", "<i4"), ("w", "<i4")]),
    "PHOTO_DTYPE": (32, [("blur", "<i4"), ("ksize", "<i4"), ("noise", "<i4"), ("scale", "<f4"), ("key", "<u4", 2), ("downscale", "<i4"),
                         ("tap_row", "<i4")]),
    "COLOUR_DTYPE": (64, [("kind", "<i4"), ("order", "u1", 4), ("contrast", "<f8"), ("alpha", "<f4"), ("beta", "<f4"), ("taps", "<f4", 9),
                          ("reserved", "<i4")]),
}


@pytest.mark.parametrize("name", list(LITERALS))
def test_record_dtypes_equal_their_literals(name):
    size, fields = LITERALS[name]
    literal, derived = np.dtype(fields), getattr(td, name)
    assert derived == literal
    assert derived.itemsize == literal.itemsize == size
    assert derived.names == literal.names
    for field in literal.names:
        assert derived.fields[field][1] == literal.fields[field][1], field              # the offset
        assert derived.fields[field][0] == literal.fields[field][0], field              # the type and shape
    assert np.zeros(2, dtype=derived).view(np.uint8).size == 2 * size


# ----------------------------------------------------------------------------------------------------------------------- surface
# every name tests/ and tools/ imported from feartracker_amd.train_data, or reached through the module, before it became a package
SURFACE = """
BLUR_BOX BLUR_GAUSSIAN BLUR_MEDIAN BLUR_MOTION BLUR_NONE COLOUR_BRIGHTNESS_CONTRAST COLOUR_DTYPE COLOUR_EMBOSS COLOUR_EQUALIZE
COLOUR_GAMMA COLOUR_HSV COLOUR_JITTER COLOUR_MEMBERS COLOUR_NONE COLOUR_RGB_SHIFT COLOUR_TONE_CURVE DEFAULT_TRAIN_DATA_CONFIG
FRAME_DTYPE GAUSS_WEIGHTS GEOM_DTYPE JITTER_BRIGHTNESS JITTER_CONTRAST JITTER_HUE JITTER_SATURATION JPEG_LUMA_BASE NOISE_GAUSS
NOISE_JPEG NOISE_MEMBERS NOISE_MULTIPLICATIVE NOISE_NONE PHOTO_DTYPE TONE_GRAY TONE_NONE TONE_SEPIA TrainBatch TrainPairBuilder
TrainPairParams _INV_STD _MEAN _TAB _colour_normalise _normalise_u8 apply_tone colour_luts colour_tables colour_u8_host crop_u8
emboss_taps encode_targets extend_bbox hsv_to_rgb_u8 jitter_brightness_u8 jitter_contrast_u8 jitter_hue_lut jitter_hue_u8
jitter_saturation_u8 jpeg_fdct_islow jpeg_idct_islow jpeg_quant_tables jpeg_roundtrip_u8_host line_u8 motion_kernel motion_taps
normal_quantiles philox4x32_10 photo_tables photometric_host photometric_u8_host remap_affine_u8 rgb_to_hsv_u8 tone_curve_lut
warp_affine_u8 warp_matrix
""".split()
# and the rest of what the module defined in public, which callers outside the tree may hold
SURFACE += """
CONTEXT_SIZE DEVICE_COLOUR_KINDS JPEG_CHROMA_BASE N_QUANTILES PAIR_COLUMNS PhotoParams SCORE_SIZE SEARCH_SIZE TEMPLATE_SIZE TOTAL_STRIDE
apply_to_bbox emboss_u8 equalize_u8 invert_affine jitter_brightness_lut jittered_crop
""".split()


def test_every_name_is_importable_from_the_package():
    module = importlib.import_module("feartracker_amd.train_data")
    missing = [name for name in SURFACE if not hasattr(module, name)]
    assert not missing, missing
    assert module.__doc__ and "TrainPairBuilder" in module.__doc__
    namespace = {}
    exec("from feartracker_amd.train_data import " + ", ".join(SURFACE), namespace)            # the `from` form, private names included
    assert namespace["TrainPairBuilder"] is module.TrainPairBuilder
