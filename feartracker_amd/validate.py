"""Sequence validation: the reference's `validation_step` (model_training/train/fear_lightning_model.py:93-125) over all
validation sequences at once.

The reference tracks one sequence at a time at batch 1: `tracker.initialize` on the first frame with the first annotation, then
`tracker.update` on frames 1 ... min(max_val_samples, T) - 1, `get_iou` of every tracked box against the frame's annotation, and
per sequence the mean IoU and the share of frames with IoU < 0.01.  `valid/metrics/box_iou` — the mean over the sequences of their
mean IoU — is what its learning-rate schedule, checkpoint selection and early stopping watch (`feartracker_amd/schedule.py`).

`SequenceValidator` makes every sequence one stream of ONE `FEARMultiTracker`: a frame of all sequences is one batched network
pass, and each sequence's boxes equal those of a `FEARTracker` of its own (tests/test_validate_host.py, test_validate_gpu.py).
Sequences are ragged: a sequence that has ended has its target removed, and its stream slot keeps its last frame.  No kernel is
added for the IoU: `submit` already lands every frame's boxes in pinned host memory, and `get_iou` on K integer boxes is host
work of microseconds; the boxes of frame t are read after frame t + 1 has been submitted, so the device never idles on it.

A sequence whose frames are JPEG files resident in a `JpegStore` is given as `StoreFrames(store, ids)`.  Its first frame is decoded
whole (`add` reads the frame's mean colour); from then on each time step asks the tracker for the rows its next search windows read
(`FEARMultiTracker.search_rows`, a device tensor) and decodes only those — one `store.decode_rows` call per step for the live streams,
nothing waits for the GPU — with the same boxes as on frames decoded whole (tests/test_multi_tracker_store_gpu.py).

    val = SequenceValidator.from_training_state(train_net.state_dict())          # or SequenceValidator(FEARNetHIP(path))
    log = val.run([(frames, annotations, "got10k"), ...])
    schedule.step(log["valid/metrics/box_iou"])
"""
from __future__ import annotations

import os
import tempfile
from typing import Any, Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from .constants import DEFAULT_TRACKING_CONFIG
from .metrics import get_iou
from .multi_tracker import FEARMultiTracker


class SequenceValidator:
    def __init__(self, net: Any, max_samples: int = 200, iou_threshold: float = 0.01, **tracking_config: Any) -> None:
        """net: `FEARNetHIP`, or any model the trackers take (a CPU network runs the tracker's host path).  max_samples and
        iou_threshold: the reference's `max_val_samples` and `_iou_threshold`.  tracking_config: the tracker's keys
        (`DEFAULT_TRACKING_CONFIG` when none is given)."""
        if int(max_samples) < 2:
            raise ValueError("max_samples must be at least 2: the first frame initialises, the others are scored")
        self.net = net
        self.max_samples = int(max_samples)
        self.iou_threshold = float(iou_threshold)
        self.tracking_config = dict(tracking_config) if tracking_config else dict(DEFAULT_TRACKING_CONFIG)
        dev = getattr(net, "device", None)
        self._cuda_id = dev if isinstance(dev, torch.device) else "cpu"

    @classmethod
    def from_training_state(cls, state_dict: Dict[str, Any], payload: str = "fp32", device: int = 0, max_batch: int = 64,
                            **kwargs: Any) -> "SequenceValidator":
        """A validator on the inference engine loaded with a training run's weights: `export_training_state` (BatchNorms folded on
        their running statistics) into a temporary `.fearw` file, then `FEARNetHIP` on it.  kwargs: the constructor's."""
        from .export import export_training_state
        from .hip_backend import FEARNetHIP
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "validate.fearw")
            export_training_state(state_dict, path, payload=payload)
            net = FEARNetHIP(path, device=device, max_batch=max_batch)         # (reads the whole file)
        return cls(net, **kwargs)

    def run(self, sequences: Iterable[Tuple[Any, Any, str]]) -> Dict[str, Any]:
        """sequences: items (frames, annotations (T,4) xywh, dataset name); frames is indexable or iterable and yields what the
        tracker takes (uint8 arrays, device tensors, `YUVFrame`s), or is a `StoreFrames` — then every sequence of the run must be one, of
        the same store: a mix is a ValueError before any launch.  Returns the reduced values under the reference's logging keys
        — "valid/metrics/box_iou", "valid/metrics/<dataset>_box_iou", "valid/metrics/<dataset>_failure_rate" — and, under
        "sequences", per sequence {"dataset", "ious" (float64 array), "box_iou", "failure_rate"}."""
        items = list(sequences)
        if not items:
            raise ValueError("no validation sequence")
        from .jpeg_store import StoreFrames
        backed = [isinstance(frames, StoreFrames) for frames, _, _ in items]
        store = items[0][0].store if all(backed) else None
        if any(backed) and (store is None or any(frames.store is not store for frames, _, _ in items)):
            raise ValueError("a run takes sequences kept in ONE JpegStore (StoreFrames of the same store), or none: not a mix")
        anns, counts, names, iters = [], [], [], []
        for frames, ann, name in items:
            ann = np.asarray(ann)
            n = min(self.max_samples, len(ann))
            if ann.ndim != 2 or ann.shape[1] != 4 or n < 2:
                raise ValueError("a validation sequence needs (T,4) annotations with T >= 2: one frame to initialise on, "
                                 "at least one to score (the reference would take a mean over nothing)")
            anns.append(ann)
            counts.append(n)
            names.append(str(name))
            if store is not None and len(frames) < n:
                raise ValueError(f"sequence {len(iters)} has an annotation for frame {len(frames)} but no such frame")
            iters.append(None if store is not None else iter(frames))
        mt = FEARMultiTracker(self.net, self._cuda_id, **self.tracking_config)
        current, ids = [], []
        firsts = store.decode([int(frames.ids[0]) for frames, _, _ in items]) if store is not None else None
        for s, (it, ann) in enumerate(zip(iters, anns)):
            frame = firsts[s] if store is not None else self._next(it, s, 0)
            (i,) = mt.add(frame, list(map(int, ann[0])), stream=s)      # tracker.initialize(read_img(files[0]), list(map(int, ann[0])))
            current.append(frame)
            ids.append(i)
        ious: List[List[float]] = [[] for _ in items]

        def score(t, pending, live):
            boxes = pending.result()
            for s in live:
                ious[s].append(get_iou(boxes[ids[s]], list(map(int, anns[s][t]))))

        waiting = None
        for t in range(1, max(counts)):
            live = [s for s, n in enumerate(counts) if t < n]
            if store is not None:                                      # only the rows the tracker is about to read; no wait
                rows = mt.search_rows(len(items))
                if len(live) < len(items):
                    rows = rows.index_select(0, self._indices(tuple(live), rows.device))
                band = store.decode_rows([int(items[s][0].ids[t]) for s in live], rows)
                for k, s in enumerate(live):
                    current[s] = band[k]
            else:
                for s in live:
                    current[s] = self._next(iters[s], s, t)
            pending = mt.submit(current)
            if waiting is not None:
                score(*waiting)                                        # frame t - 1, read behind frame t's submit
            waiting = (t, pending, live)
            ended = [ids[s] for s in live if t == counts[s] - 1]
            if ended:
                mt.remove(ended)
        score(*waiting)
        return self._reduce(names, ious)

    def _indices(self, live: Tuple[int, ...], device) -> torch.Tensor:
        """The live streams as a device index tensor, uploaded from pinned memory without waiting; kept while the set does not change."""
        if getattr(self, "_live", (None, None))[0] != live:
            pinned = torch.tensor(live, dtype=torch.int64).pin_memory()
            self._live = (live, pinned.to(device, non_blocking=True), pinned)
        return self._live[1]

    @staticmethod
    def _next(it, s: int, t: int):
        try:
            return next(it)
        except StopIteration:
            raise ValueError(f"sequence {s} has an annotation for frame {t} but no such frame") from None

    def _reduce(self, names: Sequence[str], ious: Sequence[Sequence[float]]) -> Dict[str, Any]:
        seqs = []
        for name, v in zip(names, ious):
            v = np.asarray(v, dtype=np.float64)
            seqs.append(dict(dataset=name, ious=v, box_iou=np.mean(v), failure_rate=np.mean(v < self.iou_threshold)))
        out: Dict[str, Any] = {"sequences": seqs, "valid/metrics/box_iou": np.mean([q["box_iou"] for q in seqs])}
        for name in dict.fromkeys(names):
            mine = [q for q in seqs if q["dataset"] == name]
            out[f"valid/metrics/{name}_box_iou"] = np.mean([q["box_iou"] for q in mine])
            out[f"valid/metrics/{name}_failure_rate"] = np.mean([q["failure_rate"] for q in mine])
        return out
