"""The host side of the step metrics and the validation IoU (feartracker_amd/metrics.py) against the reference's recorded results
(tests/golden/metrics_iou.npz, tools/make_metrics_golden.py) and against the cited formulas, without a GPU."""
import numpy as np
import pytest

import metricsgen as mg
from feartracker_amd.metrics import box_iou_xywh, decode_host, get_iou, step_metrics_host


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/metrics_iou.npz")


def test_get_iou_equals_the_reference_on_every_recorded_pair(golden):
    a, b = mg.iou_box_pairs()
    np.testing.assert_array_equal(a, golden["iou_a"])
    np.testing.assert_array_equal(b, golden["iou_b"])
    got = np.array([get_iou(p, q) for p, q in zip(a, b)], dtype=np.float64)
    assert len(got) >= 190
    np.testing.assert_array_equal(got, golden["iou"])
    assert (got == 1.0).any() and (got == 0.0).any() and ((got > 0) & (got < 1)).any()
    # lists of Python ints, as the validator passes them
    assert get_iou(list(map(int, a[-1])), list(map(int, b[-1]))) == golden["iou"][-1]


@pytest.mark.parametrize("B", mg.STEP_SIZES)
def test_decoded_boxes_equal_the_reference_decode(golden, B):
    for seed in range(mg.N_STEPS):
        m = mg.step_maps(B, seed)
        assert mg.maps_crc(m) == golden[f"maps_crc32_{B}"][seed], "tests/metricsgen.py no longer generates the fixture's maps"
        margins = mg.logit_margins(m["cls"])
        plain = [i for i in range(B) if i not in mg.special_pairs(B)]
        assert margins[plain].min() >= 1e-3
        assert all(margins[i] == 0.0 for i in mg.special_pairs(B) - {mg.SATURATED_PAIR})
        out = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
        assert out["boxes"].dtype == np.float64
        np.testing.assert_array_equal(out["boxes"], golden[f"decode_boxes_{B}"][seed])
        np.testing.assert_array_equal(decode_host(m["cls"], m["bbox"]), golden[f"decode_boxes_{B}"][seed])
        # the planted ties resolve to the first cell
        rc = golden[f"decode_rc_{B}"][seed]
        assert tuple(rc[mg.TIE_PAIR]) == (5, 7) and tuple(rc[mg.SATURATED_PAIR]) == (2, 9)


def _iou_direct(pred, gt):
    """torchvision.ops.box_iou's diagonal after box_convert(xywh -> xyxy), one pair at a time in Python floats (float64)."""
    out = []
    for (px, py, pw, ph), (gx, gy, gw, gh) in zip(pred.tolist(), gt.tolist()):
        p = (px, py, px + pw, py + ph)
        g = (float(gx), float(gy), float(gx) + float(gw), float(gy) + float(gh))
        area_p = (p[2] - p[0]) * (p[3] - p[1])
        area_g = (g[2] - g[0]) * (g[3] - g[1])
        w = max(min(p[2], g[2]) - max(p[0], g[0]), 0.0)
        h = max(min(p[3], g[3]) - max(p[1], g[1]), 0.0)
        inter = w * h
        out.append(inter / (area_p + area_g - inter))
    return np.array(out)


def test_ious_equal_a_direct_evaluation_of_the_box_iou_formula():
    m = mg.step_maps(128, 0)
    out = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
    direct = _iou_direct(out["boxes"], m["gt_box"])
    vis = m["visible"] != 0
    np.testing.assert_array_equal(out["iou"][vis], direct[vis])
    np.testing.assert_array_equal(box_iou_xywh(out["boxes"], m["gt_box"]), direct)
    assert ((direct > 0) & (direct < 1)).sum() > 50 and (direct == 0).sum() >= 2
    # hand-checked: a 10 x 10 box against itself shifted by half its width
    np.testing.assert_array_equal(box_iou_xywh(np.array([[0.0, 0.0, 10.0, 10.0]]), np.array([[5, 0, 10, 10]])), [50.0 / 150.0])


def test_visible_mask_and_per_dataset_sums():
    m = mg.step_maps(128, 1)
    out = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
    vis = m["visible"] != 0
    assert 0 < vis.sum() < 128 and out["n_visible"] == vis.sum()
    assert (out["iou"][~vis] == -1.0).all() and (out["iou"][vis] >= 0.0).all()
    full = box_iou_xywh(out["boxes"], m["gt_box"])
    assert abs(out["box_iou"] - full[vis].mean()) < 1e-13
    assert out["failure_rate"] == 1.0 - np.count_nonzero(full[vis]) / vis.sum()
    assert out["failure_rate"] > 0.0                                         # the planted misses count as failures
    for d in range(mg.N_DATASETS):
        sel = vis & (m["dataset_id"] == d)
        assert out["dataset_count"][d] == sel.sum() > 0
        assert abs(out["dataset_sum"][d] - full[sel].sum()) < 1e-12
    assert abs(out["dataset_sum"].sum() - out["box_iou"] * out["n_visible"]) < 1e-12
    # flipping an invisible pair's ground truth changes nothing
    gt = m["gt_box"].copy()
    gt[~vis] = (0, 0, 1, 1)
    again = step_metrics_host(m["cls"], m["bbox"], gt, m["visible"], m["dataset_id"], mg.N_DATASETS)
    np.testing.assert_array_equal(again["iou"], out["iou"])
    assert again["box_iou"] == out["box_iou"]


def test_a_step_without_a_visible_pair_counts_for_nothing():
    m = mg.step_maps(5, 0)
    out = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], np.zeros(5, np.int32), m["dataset_id"], mg.N_DATASETS)
    assert out["n_visible"] == 0 and out["box_iou"] == 0.0 and out["failure_rate"] == 0.0
    assert (out["iou"] == -1.0).all() and not out["dataset_sum"].any() and not out["dataset_count"].any()
