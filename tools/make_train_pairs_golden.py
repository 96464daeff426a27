#!/usr/bin/env python3
"""Generate tests/golden/train_pairs_geometry.npz from the REAL reference's training-pair geometry and targets.

Runs only where the reference sources are (like tools/make_golden.py, whose import machinery it reuses).  The reference's data
pipeline needs cv2 and albumentations; `oracle.cv_ref.install_reference_stubs()` provides the pieces its per-frame path calls, and
this tool adds, at run time and without touching oracle/, inert stand-ins for what `model_training/dataset/aug.py` needs at import
(`A.DualTransform`, `A.to_tuple`, the augmentation classes).  No pixel is computed: only the box arithmetic runs, on recorded draws
(`random.random` / `random.uniform` are replaced by them):

  TrackingDataset._get_search_context                      tracking_dataset.py:102-105
  get_extended_crop's context and box outputs              utils/utils.py:215-253     (template at 128 / 0.2, search at 512 / u)
  BBoxCropWithOffsets.get_params_dependent_on_targets,     dataset/aug.py:88-143      (the jittered crop, affine_crop's matrix)
    apply_to_bbox, affine_crop's mapping
  ensure_bbox_boundaries + handle_empty_bbox               tracking_dataset.py:130-136, siam_dataset.py:41-42
  FEARBoxCoder.encode, get_regression_weight_label         dataset/box_coder.py:58-72, dataset/utils.py:19-31

Only arrays are written.  Usage: python tools/make_train_pairs_golden.py
"""
from __future__ import annotations

import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "train_pairs_geometry.npz")
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

FRAME_SHAPES = [(1080, 1920), (256, 480), (48, 64)]
TRACKER = dict(total_stride=16, score_size=16, instance_size=256)


def import_reference():
    from oracle import cv_ref
    cv2, albu = cv_ref.install_reference_stubs()

    class DualTransform:                      # what BBoxCropWithOffsets needs of albumentations' base class
        def __init__(self, always_apply=False, p=1.0):
            self.always_apply, self.p = always_apply, p

    def to_tuple(param, low=None, bias=None):  # albumentations 1.0.0 for a scalar: (-param, +param)
        if isinstance(param, (int, float)):
            return (-param, param)
        return tuple(param)

    albu.DualTransform, albu.to_tuple = DualTransform, to_tuple
    captured = {}

    def warp_affine(src, M, dsize, flags=1, borderMode=0, borderValue=0):       # affine_crop's call: record the mapping only
        captured["M"] = np.array(M, dtype=np.float64)
        return np.zeros((dsize[1], dsize[0]) + src.shape[2:], dtype=src.dtype)

    cv2.warpAffine = warp_affine
    cv_ref.AlbuResize.apply = lambda self, img: np.zeros((self.height, self.width) + img.shape[2:], dtype=img.dtype)  # no pixels
    if not hasattr(np, "float"):
        np.float = float                      # aug.py:141 uses the NumPy < 1.24 alias
    import make_golden
    sys.meta_path.insert(0, make_golden._StubFinder())
    sys.path.insert(0, make_golden.REF)
    from model_training.dataset import aug, box_coder, tracking_dataset
    from model_training.dataset import utils as dutils
    from model_training.utils import utils as uutils
    return aug, box_coder, tracking_dataset, dutils, uutils, captured


def cases(rng):
    """(template frame, template box, search frame, search box, presence, r_context, jitter): 320 seeded cases, of which the
    reference itself rejects a few (skipped by the caller)."""
    out = []

    def box_in(shape, kind):
        H, W = shape
        if kind == "inside":
            w, h = rng.integers(4, max(5, W // 3)), rng.integers(4, max(5, H // 3))
            return [rng.integers(0, W - w + 1), rng.integers(0, H - h + 1), w, h]
        if kind == "edge":                    # touching a frame edge: the context leaves the frame
            w, h = rng.integers(4, max(5, W // 4)), rng.integers(4, max(5, H // 4))
            side = rng.integers(4)
            x = 0 if side == 0 else (W - w if side == 1 else rng.integers(0, W - w + 1))
            y = 0 if side == 2 else (H - h if side == 3 else rng.integers(0, H - h + 1))
            return [x, y, w, h]
        if kind == "corner":                  # a small box in a corner: the context lies mostly outside the frame
            w, h = rng.integers(2, 12), rng.integers(2, 12)
            return [rng.choice([0, W - w]), rng.choice([0, H - h]), w, h]
        if kind == "tiny":
            w, h = rng.integers(1, 4), rng.integers(1, 4)
            return [rng.integers(0, W - w + 1), rng.integers(0, H - h + 1), w, h]
        if kind == "big":                     # near frame size
            w, h = W - rng.integers(0, 4), H - rng.integers(0, 4)
            return [rng.integers(0, W - w + 1), rng.integers(0, H - h + 1), w, h]
        raise ValueError(kind)

    kinds = ["inside", "edge", "corner", "tiny", "big"]
    for i in range(320):
        tf, sf = rng.integers(0, 3), rng.integers(0, 3)
        tb = box_in(FRAME_SHAPES[tf], kinds[i % 5])
        sb = box_in(FRAME_SHAPES[sf], kinds[(i // 5) % 5])
        r = rng.random()
        jit = [rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), rng.uniform(-48, 48), rng.uniform(-48, 48)]
        if i % 7 == 0:                        # jitter at its extremes
            jit = [rng.choice([-0.35, 0.35]), rng.choice([-0.35, 0.35]), rng.choice([-48.0, 48.0]), rng.choice([-48.0, 48.0])]
        if i % 11 == 0:
            r = rng.choice([0.0, 0.999999])
        presence = 0 if i % 10 == 9 else 1
        out.append((tf, tb, sf, sb, presence, r, jit))
    return out


def main():
    aug, box_coder, tracking_dataset, dutils, uutils, captured = import_reference()
    rng = np.random.default_rng(20261016)
    coder = box_coder.FEARBoxCoder(tracker_config=TRACKER)
    ctx_self = types.SimpleNamespace(sizes_config={"context_range": 3}, search_context=2 * 2)
    images = {s: np.broadcast_to(np.zeros(1, np.uint8), s + (3,)) for s in FRAME_SHAPES}
    rec = {k: [] for k in ("pairs", "r_context", "context", "jitter", "t_ctx", "s_ctx", "box512", "crop", "M", "moved",
                           "search_bbox", "gt_reg", "gt_cls", "gt_weight")}
    skipped = 0
    for tf, tb, sf, sb, presence, r, jit in cases(rng):
        random.random = lambda r=r: r
        u = tracking_dataset.TrackingDataset._get_search_context(ctx_self)
        try:
            _, _, t_ctx = uutils.get_extended_crop(image=images[FRAME_SHAPES[tf]], bbox=np.array(tb), crop_size=128, offset=0.2)
        except ValueError:        # a 1-2 px template box whose box in the context is empty: albumentations rejects it
            skipped += 1
            continue
        _, box512, s_ctx = uutils.get_extended_crop(image=images[FRAME_SHAPES[sf]], bbox=np.array(sb), crop_size=512, offset=u)
        draws = iter(jit)
        random.uniform = lambda a, b: next(draws)
        crop_aug = aug.BBoxCropWithOffsets(bbox_crop=uutils.convert_center_to_bbox([256, 256, 256, 256]), scale=0.35, shift=48,
                                           crop_size=256)
        params = crop_aug.get_params_dependent_on_targets({"image": np.zeros((512, 512, 3), np.uint8)})
        crop_aug.affine_crop(np.zeros((512, 512, 3), np.uint8), params["modified_bbox_crop"], 256)
        moved = crop_aug.apply_to_bbox(box512, **params)
        bbox = dutils.handle_empty_bbox(uutils.ensure_bbox_boundaries(np.array(moved), img_shape=(256, 256)))
        bbox = uutils.ensure_bbox_boundaries(np.array(bbox), img_shape=(256, 256))
        if presence:
            wgt = dutils.get_regression_weight_label(bbox, 256, 16).numpy()
            enc = coder.encode(torch.from_numpy(bbox).reshape(1, 4))
            reg, cls = enc.regression_map[0].numpy(), enc.classification_label[0].numpy()
        else:
            wgt, reg, cls = np.zeros((16, 16)), np.zeros((4, 16, 16)), np.zeros((1, 16, 16))
        assert np.array_equal(reg, np.round(reg)) and np.abs(reg).max() < 2 ** 15
        rec["pairs"].append([tf, *tb, sf, *sb, presence])
        rec["r_context"].append(r)
        rec["context"].append(u)
        rec["jitter"].append(jit)
        rec["t_ctx"].append(t_ctx)
        rec["s_ctx"].append(s_ctx)
        rec["box512"].append(box512)
        rec["crop"].append(params["modified_bbox_crop"])
        rec["M"].append(captured["M"])
        rec["moved"].append(moved)
        rec["search_bbox"].append(bbox)
        rec["gt_reg"].append(reg)
        rec["gt_cls"].append(cls)
        rec["gt_weight"].append(wgt)
    arrays = dict(frame_shapes=np.array(FRAME_SHAPES, dtype=np.int32),
                  pairs=np.array(rec["pairs"], dtype=np.float64),
                  r_context=np.array(rec["r_context"], dtype=np.float64), context=np.array(rec["context"], dtype=np.float64),
                  jitter=np.array(rec["jitter"], dtype=np.float64),
                  t_ctx=np.array(rec["t_ctx"], dtype=np.int32), s_ctx=np.array(rec["s_ctx"], dtype=np.int32),
                  box512=np.array(rec["box512"], dtype=np.float64), crop=np.array(rec["crop"], dtype=np.float64),
                  M=np.array(rec["M"], dtype=np.float64), moved=np.array(rec["moved"], dtype=np.int64),
                  search_bbox=np.array(rec["search_bbox"], dtype=np.int32),
                  gt_reg=np.array(rec["gt_reg"]).astype(np.int16), gt_cls=np.array(rec["gt_cls"]).astype(np.uint8),
                  gt_weight=np.array(rec["gt_weight"]).astype(np.uint8))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(rec['pairs'])} cases ({skipped} the reference rejects skipped), {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
