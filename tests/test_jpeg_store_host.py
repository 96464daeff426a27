"""The resident JPEG store's host side ("The resident store"): the index of a baseline scan stated in Python
(jpeg_huffman.jpeg_scan_index_host, jpeg_entropy_indexed_host) against the sequential decoder — every subsequence decoded from its index
entry alone, in natural and shuffled order, equals `jpeg_coefficients_host` with `==`, every position written once — on the supported
files and on the hostile corpus; and `jpeg_store.plan_decode`, the host's share of `JpegStore.decode`, against a per-file loop."""
import ctypes

import numpy as np
import pytest

import jpeghuff
from jpegdec import ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, OK
from feartracker_amd import (MalformedJPEG, UnsupportedJPEG, jpeg_entropy_indexed_host, jpeg_entropy_parallel_host, jpeg_scan_index_host,
                             jpeg_scan_prepare_host, plan_decode)
from feartracker_amd import jpeg_frames as jf
from feartracker_amd import train_abi as abi
from feartracker_amd.jpeg_huffman import SUBSEQ_DTYPE, scan_sub_start
from feartracker_amd.jpeg_store import COLUMNS, KIND_PIXELS, KIND_SCAN


def _same(coef, ref):
    return len(coef) == len(ref) and all(a.shape == b.shape and bool((a == b).all()) for a, b in zip(coef, ref))


@pytest.mark.parametrize("subsequence_bytes", [4, 16, 128])
def test_index_model_on_the_supported_files(subsequence_bytes):
    cases, reference = jpeghuff.supported(), jpeghuff.reference()
    assert len(cases) == 51
    rng = np.random.default_rng(subsequence_bytes)
    for name, data, _ in cases:
        hd, sub_start, index, status = jpeg_scan_index_host(data, subsequence_bytes)
        assert status == 0, name
        _, seg_start = jpeg_scan_prepare_host(data, hd)
        counts = [-(-(8 * (b - a)) // (8 * subsequence_bytes)) for a, b in zip(seg_start[:-1], seg_start[1:])]
        assert sub_start.dtype == np.uint32 and sub_start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), name
        assert index.dtype == SUBSEQ_DTYPE and index.shape == (sub_start[-1],), name
        nslots = 1 if len(hd.ids) == 1 else hd.h[0] * hd.v[0] + 2
        # (p < 2^27 + 31 in general; these segments are far below the 16 MiB at which the 31 bits of overshoot matter)
        assert int(index["p"].max()) < 1 << 27 and int(index["begun"].max()) <= 3 << 20, name
        assert int((index["sz"] >> 8).max()) <= min(5, nslots - 1) and int((index["sz"] & 255).max()) <= 63, name
        for s in range(len(seg_start) - 1):                                          # a segment's first entry is the segment's start
            if sub_start[s] < sub_start[s + 1]:
                first = index[sub_start[s]]
                assert (first["p"], first["begun"], first["sz"], first["dc"].tolist()) == (0, 0, 0, [0, 0, 0]), name
        for order in (None, rng.permutation(len(index))):
            coef, status = jpeg_entropy_indexed_host(data, sub_start, index, subsequence_bytes, order=order)   # asserts one write each
            assert status == 0 and _same(coef, reference[name]), f"{name}, {'natural' if order is None else 'shuffled'} order"


def test_index_model_on_the_hostile_corpus():
    """Every flipped entropy byte and every prefix of the 16 x 16 4:2:0 file that gets past the header and the markers: the index build's
    verdict and the indexed decode's are the self-synchronising model's, which the existing tests hold to the sequential decoder."""
    accepted = refused = 0
    rng = np.random.default_rng(5)
    for what, data in jpeghuff.corpus():
        try:
            _, ref, want, _ = jpeg_entropy_parallel_host(data, 128)
        except (MalformedJPEG, UnsupportedJPEG):
            with pytest.raises((MalformedJPEG, UnsupportedJPEG)):
                jpeg_scan_index_host(data, 128)
            continue
        hd, sub_start, index, status = jpeg_scan_index_host(data, 128)
        assert status == want, what
        coef, again = jpeg_entropy_indexed_host(data, sub_start, index, 128, order=rng.permutation(len(index)))
        assert again == want, what
        if want == 0:
            accepted += 1
            assert _same(coef, jf.jpeg_coefficients_host(data)[1]) and _same(coef, ref), what
        else:
            refused += 1
    assert accepted > 100 and refused > 100


def test_sub_start_through_the_library():
    """fear_jpeg_sub_start, the host function behind JpegStore.add and fear_jpeg_index_build's capacity check, against scan_sub_start:
    exact-size arrays with a sentinel behind them, the count-only form, and its argument checks."""
    lib = abi.load_train_library()
    n_sub = ctypes.c_uint32(0)

    def call(seg, n_seg, n_bytes, sb, out, cap):
        return lib.fear_jpeg_sub_start(None if seg is None else seg.ctypes.data, n_seg, n_bytes, sb, None if out is None else out.ctypes.data,
                                       cap, ctypes.byref(n_sub))
    for name, data, _ in jpeghuff.supported():
        _, _, seg, scan = jpeghuff.c_prepare(lib, data)
        for sb in (4, 16, 128, 1024):
            want = scan_sub_start(seg, sb)
            out = np.full(seg.size + 4, 0xA5A5A5A5, dtype=np.uint32)
            assert call(seg, scan.n_seg, scan.n_bytes, sb, out, seg.size) == OK, name
            assert np.array_equal(out[:seg.size], want) and np.all(out[seg.size:] == 0xA5A5A5A5) and n_sub.value == want[-1], name
            n_sub.value = 0
            assert call(seg, scan.n_seg, scan.n_bytes, sb, None, 0) == OK and n_sub.value == want[-1], name
    import jpegdec
    _, _, seg, scan = jpeghuff.c_prepare(lib, jpegdec.case("15x50_420_random_q100_rst3")[1])
    out = np.zeros(seg.size, dtype=np.uint32)
    assert scan.n_seg >= 2
    assert call(seg, scan.n_seg, scan.n_bytes, 128, out, seg.size - 1) == ERR_WORKSPACE
    assert call(None, scan.n_seg, scan.n_bytes, 128, out, seg.size) == ERR_NULL
    assert lib.fear_jpeg_sub_start(seg.ctypes.data, scan.n_seg, scan.n_bytes, 128, out.ctypes.data, seg.size, None) == ERR_NULL
    for sb in (0, 2, 6, 130, 1028, -128):
        assert call(seg, scan.n_seg, scan.n_bytes, sb, out, seg.size) == ERR_SHAPE, sb
    assert call(seg, 0, scan.n_bytes, 128, out, seg.size) == ERR_SHAPE
    assert call(seg, scan.n_seg, scan.n_bytes + 1, 128, out, seg.size) == ERR_SHAPE         # the offsets do not end at n_bytes
    assert call(seg[1:], scan.n_seg - 1, scan.n_bytes, 128, out, seg.size) == ERR_SHAPE     # nor start at 0
    bad = seg.copy()
    bad[1] = bad[2] + 1
    assert call(bad, scan.n_seg, scan.n_bytes, 128, out, seg.size) == ERR_SHAPE             # decreasing


def _naive_plan(columns, ids, limit):
    """plan_decode one file at a time."""
    groups, cur, dense = [], None, 0
    for pos, i in enumerate(ids):
        row = columns[i]
        need = 128 * int(row["total_blocks"]) if row["kind"] == KIND_SCAN else 0
        if cur is None or dense + need > limit:
            cur = dict(lo=pos, scan=[], sub=[0], blk=[0], pix=[0], coef=[], out=[], values=0, out_bytes=0, most=0)
            groups.append(cur)
            dense = 0
        dense += need
        cur["hi"] = pos + 1
        cur["out"].append(cur["out_bytes"])
        cur["out_bytes"] += -(-int(row["H"]) * int(row["W"]) * 3 // 16) * 16
        if row["kind"] == KIND_SCAN:
            cur["scan"].append(pos - cur["lo"])
            cur["sub"].append(cur["sub"][-1] + -(-int(row["n_sub"]) // 256))
            cur["blk"].append(cur["blk"][-1] + -(-int(row["total_blocks"]) // 32))
            cur["pix"].append(cur["pix"][-1] + -(-int(row["H"]) * int(row["W"]) // 256))
            cur["coef"].append(cur["values"])
            cur["values"] += 64 * int(row["total_blocks"])
            cur["most"] = max(cur["most"], int(row["total_blocks"]))
    return groups


@pytest.mark.parametrize("limit", [1 << 30, 300_000, 1, 0])
def test_decode_planner_against_a_per_file_loop(limit):
    rng = np.random.default_rng(11)
    columns = np.zeros(40, dtype=COLUMNS)
    columns["H"], columns["W"] = rng.integers(1, 300, 40), rng.integers(1, 300, 40)
    columns["total_blocks"] = 3 * (-(-columns["H"] // 8)) * (-(-columns["W"] // 8))
    columns["n_sub"] = rng.integers(0, 3000, 40)
    columns["n_seg"] = rng.integers(1, 9, 40)
    columns["kind"] = np.where(rng.random(40) < 0.2, KIND_PIXELS, KIND_SCAN)
    ids = rng.integers(0, 40, 200)                                                   # any order, with repeats
    got, want = plan_decode(columns, ids, limit), _naive_plan(columns, ids, limit)
    assert len(got) == len(want) and (limit < 1 << 30 or len(got) == 1)
    assert limit > 1 or (len(got) > 150 and max(g["scan"].size for g in got) == 1)      # every "scan" entry is a group of its own
    for g, w in zip(got, want):
        assert (g["lo"], g["hi"], g["values"], g["out_bytes"], g["most"]) == (w["lo"], w["hi"], w["values"], w["out_bytes"], w["most"])
        assert g["scan"].tolist() == w["scan"]
        assert g["sub_prefix"].dtype == np.uint32 and g["sub_prefix"].tolist() == w["sub"]
        assert g["block_prefix"].tolist() == w["blk"] and g["pixel_prefix"].tolist() == w["pix"]
        assert g["coef_offset"].tolist() == w["coef"] and g["plane_offset"].tolist() == w["coef"] and g["out_offset"].tolist() == w["out"]
        assert g["workspace_bytes"] == 16 + w["values"]
        assert not (g["plane_offset"] % 16).any() and not (g["out_offset"] % 16).any()
        dense = sum(128 * int(columns[i]["total_blocks"]) for i in ids[g["lo"]:g["hi"]] if columns[i]["kind"] == KIND_SCAN)
        assert dense <= limit or g["hi"] - g["lo"] == 1 or dense - 128 * int(columns[ids[g["lo"]]]["total_blocks"]) == 0
    assert plan_decode(columns, [], limit) == []
    assert [(g["lo"], g["hi"]) for g in plan_decode(columns, ids, 1 << 40, max_group=64)] == [(0, 64), (64, 128), (128, 192), (192, 200)]
