"""Deterministic inputs for the step-metrics tests (test infrastructure).

`step_maps(B, seed)` is one training step's worth of metric inputs: classification logits, positive ltrb regression maps,
integer ground-truth boxes, a visibility mask and dataset ids (D = 3).  The maps are generated, not stored;
tests/golden/metrics_iou.npz holds their CRC32s next to the boxes the REFERENCE's FEARBoxCoder.decode produced on them
(tools/make_metrics_golden.py), so a drifting generator is detected before any box is compared.

Pairs with a special classification map (the rest are 3 * N(0, 1) logits whose two largest values differ by at least 1e-3, which
the fixture tool and the CPU test check):
    pair 1   bit-equal maximal logits in three cells                    -> the first cell wins
    pair 2   three logits >= 20, where the fp32 sigmoid is exactly 1     -> the first cell wins, though a later logit is larger
    pair B-1 (B > 5) both at once, the first maximal cell being cell 255's neighbour 254
"""
import zlib

import numpy as np

N_DATASETS = 3
DATASETS = ["got10k", "lasot", "coco"]
STEP_SIZES = (128, 5)
N_STEPS = 4
TIE_PAIR, SATURATED_PAIR = 1, 2


def step_maps(B: int, seed: int):
    rng = np.random.RandomState(1000 * B + seed)
    cls = (3.0 * rng.standard_normal((B, 1, 16, 16))).astype(np.float32)
    bbox = rng.uniform(1.0, 110.0, size=(B, 4, 16, 16)).astype(np.float32)
    close = np.flatnonzero(logit_margins(cls) < 1e-3)          # a drawn near-tie: lift that pair's largest logit by 2^-6
    flat = cls.reshape(B, -1)
    flat[close, np.argmax(flat[close], axis=1)] += np.float32(0.015625)
    cls[TIE_PAIR, 0, 5, 7] = cls[TIE_PAIR, 0, 9, 2] = cls[TIE_PAIR, 0, 12, 12] = np.float32(15.0)
    cls[SATURATED_PAIR, 0, 3, 4] = 25.0
    cls[SATURATED_PAIR, 0, 2, 9] = 20.5           # the first of the three: cell 41
    cls[SATURATED_PAIR, 0, 10, 1] = 31.0
    if B > 5:
        cls[B - 1, 0, 15, 14] = cls[B - 1, 0, 15, 15] = np.float32(22.0)
    gt = np.concatenate([rng.randint(40, 160, size=(B, 2)), rng.randint(20, 120, size=(B, 2))], axis=1).astype(np.int32)
    gt[0] = (250, 250, 6, 6)                      # a corner box most predictions miss: IoU exactly 0
    gt[3] = (100, 100, 0, 0)                      # zero-size ground truth: IoU exactly 0
    visible = (rng.uniform(size=B) < 0.8).astype(np.int32)
    visible[[0, 1, 2]] = 1
    visible[4] = 0
    dataset_id = rng.randint(0, N_DATASETS, size=B).astype(np.int32)
    return dict(cls=cls, bbox=bbox, gt_box=gt, visible=visible, dataset_id=dataset_id)


def special_pairs(B: int):
    return {TIE_PAIR, SATURATED_PAIR} | ({B - 1} if B > 5 else set())


def logit_margins(cls: np.ndarray) -> np.ndarray:
    """Per pair: the largest logit minus the second largest."""
    flat = np.sort(cls.reshape(cls.shape[0], -1).astype(np.float64), axis=1)
    return flat[:, -1] - flat[:, -2]


def maps_crc(m) -> int:
    return zlib.crc32(np.ascontiguousarray(m["cls"]).tobytes() + np.ascontiguousarray(m["bbox"]).tobytes())


def iou_box_pairs():
    """About 200 pairs of integer xywh boxes for `get_iou`: seeded ones and the hand-written edge cases."""
    rng = np.random.RandomState(5)
    a = np.concatenate([rng.randint(-20, 300, size=(180, 2)), rng.randint(0, 150, size=(180, 2))], axis=1)
    b = np.concatenate([rng.randint(-20, 300, size=(180, 2)), rng.randint(0, 150, size=(180, 2))], axis=1)
    b[:40, :2] = a[:40, :2] + rng.randint(-15, 16, size=(40, 2))          # near neighbours: mostly overlapping
    edge = [((10, 10, 50, 40), (10, 10, 50, 40)),        # identical
            ((0, 0, 100, 100), (20, 30, 10, 10)),        # nested
            ((20, 30, 10, 10), (0, 0, 100, 100)),
            ((0, 0, 10, 10), (10, 0, 10, 10)),           # sharing an edge (the "+1" makes that an overlap)
            ((0, 0, 10, 10), (0, 10, 10, 10)),
            ((0, 0, 10, 10), (11, 0, 10, 10)),           # one pixel apart
            ((0, 0, 10, 10), (12, 0, 10, 10)),           # disjoint
            ((0, 0, 10, 10), (200, 200, 5, 5)),
            ((5, 5, 0, 0), (5, 5, 0, 0)),                # zero size, identical
            ((5, 5, 0, 0), (0, 0, 20, 20)),              # zero size inside a box
            ((5, 5, 0, 0), (50, 50, 0, 0)),              # zero size, disjoint
            ((0, 0, 0, 30), (0, 0, 30, 0)),              # degenerate in one direction each
            ((-10, -10, 30, 30), (0, 0, 5, 5)),          # negative origin
            ((163, 53, 45, 174), (170, 60, 40, 160))]
    a = np.concatenate([a, np.array([e[0] for e in edge])]).astype(np.int64)
    b = np.concatenate([b, np.array([e[1] for e in edge])]).astype(np.int64)
    return a, b
