"""The three consumers of the monitored metric (host only): what the reference's training run does with `valid/metrics/box_iou`
(model_training/config/train_stage/tracker.yaml: `metric_to_monitor`, `metric_mode: max`).

* `PlateauSchedule` — `torch.optim.lr_scheduler.ReduceLROnPlateau` (train/base_lightning_model.py:63-71) on anything with an `lr`
  attribute: `AdamHIP.lr` is a plain attribute read at every step.  Defaults: config/scheduler/plateau_max.yaml (factor 0.5,
  patience 10, min_lr 1e-6; its `warmup_steps` is read by no code of the reference, so there is no warm-up here either) and torch's
  own (relative threshold 1e-4, eps 1e-8; no cooldown).
* `TopKCheckpoints` — the checkpoint callback's `save_top_k: 3` (train/callbacks.py:52-64), writing deployable `.fearw` files with
  `export_training_state` instead of Lightning checkpoints.
* `EarlyStopping` — `early_stopping: 20` (train/callbacks.py:72-82: pytorch_lightning's EarlyStopping with min_delta 0).
* `save_training_checkpoint` / `load_training_checkpoint` — what Lightning's own checkpoints add to the weights: the optimiser state
  and the BatchNorm running statistics, so that a run can be continued (`TopKCheckpoints` exports inference weights only).

    schedule, keep, stop = PlateauSchedule(opt), TopKCheckpoints("checkpoints"), EarlyStopping()
    for epoch in ...:
        ...                                                   # train
        value = validator.run(sequences)["valid/metrics/box_iou"]
        schedule.step(value)
        keep.step(value, net.state_dict(), epoch)
        if stop.step(value):
            break
"""
from __future__ import annotations

import math
import os
from typing import Any, Callable, Dict, List, Optional, Tuple


def _check_mode(mode: str) -> str:
    if mode not in ("min", "max"):
        raise ValueError("mode must be 'min' or 'max'")
    return mode


class PlateauSchedule:
    """ReduceLROnPlateau's rule with torch's default relative threshold: a value is better than the best so far when it beats
    best * (1 + threshold) for "max", best * (1 - threshold) for "min"; after more than `patience` epochs in a row without a better
    value the learning rate becomes max(lr * factor, min_lr) — when that changes it by more than `eps` — and the count starts again."""

    def __init__(self, optimizer: Any, mode: str = "max", factor: float = 0.5, patience: int = 10, min_lr: float = 1e-6,
                 threshold: float = 1e-4, eps: float = 1e-8) -> None:
        if factor >= 1.0:
            raise ValueError("factor must be below 1")
        self.optimizer = optimizer
        self.mode, self.factor, self.patience, self.min_lr = _check_mode(mode), float(factor), int(patience), float(min_lr)
        self.threshold, self.eps = float(threshold), float(eps)
        self.best = math.inf if mode == "min" else -math.inf
        self.num_bad_epochs = 0

    def is_better(self, value: float, best: float) -> bool:
        return value < best * (1.0 - self.threshold) if self.mode == "min" else value > best * (self.threshold + 1.0)

    def step(self, value) -> float:
        """One epoch's metric; returns the learning rate now in force."""
        current = float(value)
        if self.is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            old = float(self.optimizer.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.optimizer.lr = new
            self.num_bad_epochs = 0
        return float(self.optimizer.lr)


class TopKCheckpoints:
    """Keeps the `.fearw` exports of the k best states: `step(value, state, tag)` writes `<directory>/fear_<tag>.fearw` when
    the value enters the best k (ties keep the earlier file) and deletes the file that drops out."""

    def __init__(self, directory: str, k: int = 3, mode: str = "max", payload: str = "fp16",
                 exporter: Optional[Callable[..., None]] = None) -> None:
        if int(k) < 1:
            raise ValueError("k must be at least 1")
        self.directory, self.k, self.mode, self.payload = str(directory), int(k), _check_mode(mode), payload
        self._exporter = exporter
        self._kept: List[Tuple[float, int, str]] = []          # (value, order of arrival, path), best first
        self._seen = 0

    def _export(self, state: Dict[str, Any], path: str) -> None:
        if self._exporter is not None:
            self._exporter(state, path, payload=self.payload)
            return
        from .export import export_training_state
        export_training_state(state, path, payload=self.payload)

    def step(self, value, state: Dict[str, Any], tag: Any = None) -> Optional[str]:
        """Returns the path written, or None when the value is not among the best k."""
        value = float(value)
        order, self._seen = self._seen, self._seen + 1
        if math.isnan(value):
            return None
        key = -value if self.mode == "max" else value
        rank = sum(1 for v, _, _ in self._kept if (-v if self.mode == "max" else v) <= key)
        if rank >= self.k:
            return None
        os.makedirs(self.directory, exist_ok=True)
        path = os.path.join(self.directory, f"fear_{order if tag is None else tag}.fearw")
        self._export(state, path)
        self._kept.insert(rank, (value, order, path))
        for _, _, old in self._kept[self.k:]:
            if old != path and os.path.exists(old):
                os.remove(old)
        del self._kept[self.k:]
        return path

    def best(self) -> Optional[str]:
        return self._kept[0][2] if self._kept else None

    def paths(self) -> List[str]:
        """The kept files, best first."""
        return [p for _, _, p in self._kept]


class EarlyStopping:
    """pytorch_lightning's EarlyStopping with min_delta 0: a value strictly better than the best so far resets the count, any
    other value adds one, and `step` returns True once `patience` values in a row have not improved."""

    def __init__(self, patience: int = 20, mode: str = "max") -> None:
        self.patience, self.mode = int(patience), _check_mode(mode)
        self.best = math.inf if mode == "min" else -math.inf
        self.wait = 0

    def step(self, value) -> bool:
        value = float(value)
        if value < self.best if self.mode == "min" else value > self.best:
            self.best = value
            self.wait = 0
        else:
            self.wait += 1
        return self.wait >= self.patience


def save_training_checkpoint(path: str, net: Any, opt: Any, **extra: Any) -> None:
    """Everything a run needs to continue, in one `torch.save` file — what the reference's Lightning checkpoints carry next to the
    weights: `net.state_dict()` (parameters and BatchNorm running statistics), `opt.state_dict()` (moments / momentum buffer, step
    count, hyper-parameters with `lr` as the schedule left it) and the caller's `extra` values (epoch, schedule counters, ...)."""
    import torch
    torch.save({"model": net.state_dict(), "optimizer": opt.state_dict(), "optimizer_class": type(opt).__name__, "extra": dict(extra)}, path)


def load_training_checkpoint(path: str, net: Any, opt: Any) -> Dict[str, Any]:
    """Restore `net` (in place: `FEARNetTrainHIP.load_state_dict`) and `opt` from a file of `save_training_checkpoint`; returns its
    `extra` values.  The optimiser must be of the class that was saved."""
    import torch
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if ckpt["optimizer_class"] != type(opt).__name__:
        raise ValueError(f"the checkpoint holds the state of {ckpt['optimizer_class']}, not of {type(opt).__name__}")
    net.load_state_dict(ckpt["model"])
    opt.load_state_dict(ckpt["optimizer"])
    return ckpt["extra"]
