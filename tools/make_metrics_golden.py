#!/usr/bin/env python3
"""Generate tests/golden/metrics_iou.npz from the REAL reference (needs the reference checkout, like tools/make_golden.py, whose
import stubs this tool uses).  Only arrays are written.

  get_iou (model_training/utils/utils.py:15-26) on the integer box pairs of tests/metricsgen.iou_box_pairs: identical, nested,
      edge-touching, disjoint and zero-size boxes among about 200
  FEARBoxCoder.decode (dataset/box_coder.py:75-107) on the maps of tests/metricsgen.step_maps — four steps each of 128 and of 5
      pairs: 3 * N(0, 1) logits, bit-equal maxima, saturated sigmoids, positive ltrb maps — with the maps' CRC32s and the margin
      between each pair's two largest logits (checked here: at least 1e-3 on every pair without a planted tie)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_golden import OUT, TRACKING_CONFIG, import_reference  # noqa: E402


def main():
    import metricsgen as mg
    _, ref_box_coder, _, ref_utils = import_reference()
    fx = {}
    a, b = mg.iou_box_pairs()
    fx["iou_a"], fx["iou_b"] = a, b
    fx["iou"] = np.array([ref_utils.get_iou(np.array(p), np.array(q)) for p, q in zip(a, b)], dtype=np.float64)
    coder = ref_box_coder.FEARBoxCoder(tracker_config=TRACKING_CONFIG)
    for B in mg.STEP_SIZES:
        boxes, rc, crc, margin = [], [], [], []
        for seed in range(mg.N_STEPS):
            m = mg.step_maps(B, seed)
            mar = mg.logit_margins(m["cls"])
            plain = [i for i in range(B) if i not in mg.special_pairs(B)]
            assert mar[plain].min() >= 1e-3, (B, seed, mar[plain].min())
            dec = coder.decode(regression_map=torch.from_numpy(m["bbox"]), classification_map=torch.from_numpy(m["cls"]))
            boxes.append(dec.bbox.numpy())
            rc.append(np.array(dec.pred_coords))
            crc.append(mg.maps_crc(m))
            margin.append(mar)
        assert boxes[0].dtype == np.float64
        fx[f"decode_boxes_{B}"], fx[f"decode_rc_{B}"] = np.stack(boxes), np.stack(rc)
        fx[f"maps_crc32_{B}"], fx[f"logit_margin_{B}"] = np.array(crc, dtype=np.uint32), np.stack(margin)
    path = os.path.join(OUT, "metrics_iou.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
