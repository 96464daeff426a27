"""Training telemetry and the validation IoU: what the reference logs to steer a run.

* `TrainMetrics` — the per-step metrics of the reference's `_training_step` (model_training/train/fear_lightning_model.py:66-87):
  the predicted maps are decoded (`FEARBoxCoder.decode`), the decoded box of every VISIBLE pair is compared with its ground-truth
  box (`box_convert` + `torchvision.ops.box_iou`), and the IoUs feed `BoxIoUMetric`, `TrackingFailureRateMetric`
  (metrics/tracking.py) and the per-dataset `DatasetAwareMetric` (metrics/dataset_aware_metric.py).  Here one operator,
  `fear_train_metrics` (include/fear_train.h), does all of it on the device from the step's own output tensors: `update` copies
  no map and never waits for the stream, the epoch's sums stay in a device buffer, and `compute` is the one copy.
* `step_metrics_host` — the same arithmetic in numpy float64, the operator's reference in the tests.
* `get_iou` — the reference's integer "+1" IoU of two xywh boxes (utils/utils.py:15-26), which `validation_step` applies to the
  tracked box of every frame (`feartracker_amd/validate.py`).

A step with no visible pair: the reference takes a mean over nothing there and logs NaN, which then stays in its epoch mean.
Here such a step counts for nothing — the one deliberate deviation, like `fear_head_loss`'s (include/fear_train.h).  The
reference's failure rate is a float32 division (`torch.count_nonzero(.) / batch_size` of an integer tensor); here it is float64.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .geometry import make_grid
from .train_abi import launch, load_train_library

SCORE_SIZE, TOTAL_STRIDE, INSTANCE_SIZE = 16, 16, 256
MAX_DATASETS = 64           # FEAR_METRICS_MAX_DATASETS


def get_iou(bb1, bb2) -> float:
    """IoU of two [x, y, w, h] boxes with the reference's inclusive-pixel "+1" on every side length (utils/utils.py:15-26)."""
    x1, y1, w1, h1 = bb1
    x2, y2, w2, h2 = bb2
    x_a, y_a = np.max((x1, x2)), np.max((y1, y2))
    x_b, y_b = np.min((x1 + w1, x2 + w2)), np.min((y1 + h1, y2 + h2))
    inter = np.max((x_b - x_a + 1, 0)) * np.max((y_b - y_a + 1, 0))
    area_a = ((x1 + w1) - x1 + 1) * ((y1 + h1) - y1 + 1)
    area_b = ((x2 + w2) - x2 + 1) * ((y2 + h2) - y2 + 1)
    return inter / (area_a + area_b - inter)


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def decode_host(cls, bbox) -> np.ndarray:
    """`FEARBoxCoder.decode` (dataset/box_coder.py:75-107) of (B,1,16,16) logits and (B,4,16,16) ltrb maps -> (B,4) float64 xywh:
    fp32 sigmoid, the FIRST maximum cell, the float64 grid."""
    cls = np.ascontiguousarray(_np(cls), dtype=np.float32)
    reg = np.ascontiguousarray(_np(bbox), dtype=np.float32)
    n = cls.shape[0]
    score = torch.from_numpy(cls).sigmoid().numpy().reshape(n, -1)
    flat = np.argmax(score, axis=1)                                  # first maximum, like torch.argmax
    gx, gy = make_grid(SCORE_SIZE, TOTAL_STRIDE, INSTANCE_SIZE)
    gx, gy = gx.reshape(-1)[flat], gy.reshape(-1)[flat]
    l, t, r, b = (reg.reshape(n, 4, -1)[np.arange(n), k, flat].astype(np.float64) for k in range(4))
    x0, y0, x1, y1 = gx - l, gy - t, gx + r, gy + b
    return np.stack([x0, y0, x1 - x0, y1 - y0], axis=1)


def box_iou_xywh(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """The diagonal of `torchvision.ops.box_iou(box_convert(pred, "xywh", "xyxy"), box_convert(gt, "xywh", "xyxy"))` in float64
    (torchvision/ops/boxes.py: `box_area` = (x2 - x1) * (y2 - y1); `_box_inter_union`: lt = max of the top-left corners, rb = min of
    the bottom-right corners, wh = (rb - lt).clamp(min=0), inter = w * h, union = area1 + area2 - inter; iou = inter / union)."""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    px1, py1, px2, py2 = p[:, 0], p[:, 1], p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]
    gx1, gy1, gx2, gy2 = g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    area_p = (px2 - px1) * (py2 - py1)
    area_g = (gx2 - gx1) * (gy2 - gy1)
    w = np.maximum(np.minimum(px2, gx2) - np.maximum(px1, gx1), 0.0)
    h = np.maximum(np.minimum(py2, gy2) - np.maximum(py1, gy1), 0.0)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_p + area_g - inter)


def step_metrics_host(cls, bbox, gt_box, visible, dataset_id, n_datasets: Optional[int] = None) -> Dict[str, np.ndarray]:
    """One step's metrics in numpy float64 — what `fear_train_metrics` computes.  Returns
    boxes (B,4) decoded xywh | iou (B), -1 for invisible pairs | box_iou, failure_rate, n_visible: the step scalars (0, 0, 0
    without a visible pair) | dataset_sum (D), dataset_count (D): this step's share of the per-dataset accumulators."""
    boxes = decode_host(cls, bbox)
    vis = _np(visible).reshape(-1) != 0
    ds = _np(dataset_id).reshape(-1).astype(np.int64)
    D = int(n_datasets) if n_datasets is not None else (int(ds.max()) + 1 if ds.size else 1)
    iou = np.where(vis, box_iou_xywh(boxes, _np(gt_box)), -1.0)
    n = int(vis.sum())
    total, ds_sum, ds_count = 0.0, np.zeros(D), np.zeros(D)
    for v, d in zip(iou[vis], ds[vis]):                              # pair-index order, like the kernel
        total = total + v
        ds_sum[d] += v
        ds_count[d] += 1
    mean = total / n if n else 0.0
    fail = 1.0 - np.count_nonzero(iou[vis]) / n if n else 0.0
    return dict(boxes=boxes, iou=iou, box_iou=np.float64(mean), failure_rate=np.float64(fail), n_visible=n,
                dataset_sum=ds_sum, dataset_count=ds_count)


class TrainMetrics:
    """The epoch's training metrics, accumulated on the device.

        metrics = TrainMetrics(0, ["got10k", "lasot"])
        out = net.step(batch.template, batch.search, batch.gt_reg, batch.gt_cls, batch.gt_weight)
        metrics.update(out, batch, visible, dataset_ids)        # one operator call on the current stream, nothing waits
        ...
        log = metrics.compute()                                  # at the end of the epoch: one copy
        metrics.reset()

    `visible` and `dataset_ids` are (B) integer device tensors (a host array is uploaded, which the step loop should do with the
    batch, not here); `dataset_ids[i]` indexes `datasets`."""

    def __init__(self, device=0, datasets: Sequence[str] = ("train",)) -> None:
        self.datasets: List[str] = list(datasets)
        if not 1 <= len(self.datasets) <= MAX_DATASETS:
            raise ValueError(f"between 1 and {MAX_DATASETS} datasets")
        self.lib = load_train_library()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        D = len(self.datasets)
        self._accum = torch.zeros(3 + 2 * D, dtype=torch.float64, device=self.device)
        self._step = torch.zeros(3, dtype=torch.float64, device=self.device)
        self._iou = torch.zeros(0, dtype=torch.float64, device=self.device)

    def _i32(self, t, n: int, what: str) -> torch.Tensor:
        t = torch.as_tensor(t)
        if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
            t = t.to(self.device, torch.int32, non_blocking=True).contiguous()
        if t.numel() != n:
            raise ValueError(f"{what}: expected {n} values, got {t.numel()}")
        return t

    @torch.no_grad()
    def update(self, step_out, batch, visible, dataset_ids) -> None:
        """Add one step: `step_out` = what `FEARNetTrainHIP.step` returned ("cls", "bbox"), `batch` = the step's `TrainBatch`
        (its `search_bbox`), or the (B,4) ground-truth boxes themselves."""
        cls, bbox = step_out["cls"], step_out["bbox"]
        gt = getattr(batch, "search_bbox", batch)
        B = cls.shape[0]
        if tuple(cls.shape) != (B, 1, SCORE_SIZE, SCORE_SIZE) or tuple(bbox.shape) != (B, 4, SCORE_SIZE, SCORE_SIZE):
            raise ValueError("expected cls (B,1,16,16) and bbox (B,4,16,16)")
        for t in (cls, bbox):
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError("cls and bbox must be contiguous fp32 tensors on the metrics' device, as `step` returns them")
        gt = self._i32(gt, 4 * B, "ground-truth boxes")
        vis = self._i32(visible, B, "visible")
        ds = self._i32(dataset_ids, B, "dataset_ids")
        with torch.cuda.device(self.device):
            if self._iou.numel() != B:
                self._iou = torch.empty(B, dtype=torch.float64, device=self.device)
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            launch(self.lib, "fear_train_metrics", p(cls), p(bbox), p(gt), p(vis), p(ds), B, len(self.datasets), p(self._iou),
                   p(self._step), p(self._accum), st)

    @property
    def last_iou(self) -> torch.Tensor:
        """(B) float64 device tensor: the last step's per-pair IoUs, -1 for invisible pairs."""
        return self._iou

    @property
    def last_step(self) -> torch.Tensor:
        """(3) float64 device tensor: the last step's mean IoU | failure rate | visible pairs."""
        return self._step

    def compute(self) -> Dict[str, float]:
        """The epoch's values under the reference's logging keys (one device-to-host copy).  Keys of steps or datasets that never
        counted are left out."""
        a = self._accum.cpu().numpy()
        D = len(self.datasets)
        out: Dict[str, float] = {}
        if a[2] > 0:
            out["train/metrics/box_iou"] = float(a[0] / a[2])
            out["train/metrics/failure_rate"] = float(a[1] / a[2])
        for d, name in enumerate(self.datasets):
            if a[3 + D + d] > 0:
                out[f"train/metrics/{name}_box_iou"] = float(a[3 + d] / a[3 + D + d])
        return out

    def reset(self) -> None:
        self._accum.zero_()
