"""From annotation tables to the step's tensors: `fill_store` puts a table's files into a `JpegStore`, `PairLoader` iterates over an
epoch's batches — sample (sampling.py), clip, number the distinct files, `draw`, `frame_rows`, `decode_rows`, `build(borders=)` (with
`windows=True`: `frame_windows`, `decode_windows`, `build(WindowFrames, borders=)`, compact frames of the rectangles the pairs read) — and
keeps the data stage of the next batch in flight on a stream of its own while the caller trains on the current one.

Stream discipline.  With `prefetch=1` every launch and copy of a batch's data stage is enqueued on the loader's
data stream; an event recorded behind it is what the consumer's stream waits for (on the device: the host never waits) when the batch
is handed out, and every tensor handed out is marked with `record_stream` for the consumer's stream, so the caching allocator does not
give its memory to the data stream again while the consumer still reads it.  The data stage takes nothing from the consumer: the store is
resident and complete (`JpegStore.add` synchronises), and every buffer of the stage is allocated on the data stream.  With `prefetch=0`
everything runs on the current stream.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from .records import TrainBatch, TrainPairParams, scale_pairs
from .sampling import EpochPlan, TrackTable, _generator_state, _set_generator_state


def fill_store(store, tables: Sequence[TrackTable], chunk: int = 4096) -> List[np.ndarray]:
    """Add every distinct file of `tables` (`table.paths()`: `root` joined in front of `img_path`) to `store`, in table order, `chunk`
    files per `JpegStore.add`.  Returns per table the store id of every row (int64).  `StoreFull` and the decoder's exceptions pass
    through; the `add` calls that completed before one stay in the store."""
    if int(chunk) < 1:
        raise ValueError("chunk is at least 1")
    known: Dict[str, int] = {}
    fresh: List[str] = []
    per_table = []
    for table in tables:
        paths = table.paths()
        for p in paths:
            if p not in known:
                known[p] = len(known)
                fresh.append(p)
        per_table.append(np.array([known[p] for p in paths], dtype=np.int64))
    ids = [store.add(fresh[at:at + int(chunk)]) for at in range(0, len(fresh), int(chunk))]
    ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    return [ids[order] for order in per_table]


def clip_boxes(boxes: np.ndarray, shapes: np.ndarray) -> np.ndarray:
    """`geometry.ensure_bbox_boundaries(box, (H, W))` for (N, 4) xywh boxes and (N, 2) shapes at once: the same comparisons in the same
    order, the truncation to int32 included."""
    boxes, shapes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(shapes).reshape(-1, 2)
    img_h, img_w = shapes[:, 0].astype(np.float64), shapes[:, 1].astype(np.float64)
    x_lo = np.minimum(np.maximum(0, boxes[:, 0]), img_w)
    y_lo = np.minimum(np.maximum(0, boxes[:, 1]), img_h)
    x_hi = np.minimum(np.maximum(0, x_lo + boxes[:, 2]), img_w)
    y_hi = np.minimum(np.maximum(0, y_lo + boxes[:, 3]), img_h)
    return np.stack([x_lo, y_lo, x_hi - x_lo, y_hi - y_lo], axis=1).astype(np.int32)


@dataclass
class LoadedBatch:
    """One item of a `PairLoader`."""
    batch: TrainBatch                # the builder's six tensors
    visible: torch.Tensor            # (B,) int32 on the device: the search row's presence
    dataset_ids: torch.Tensor        # (B,) int32 on the device, into `loader.datasets`: the search row's dataset
    pairs: np.ndarray                # (B, 11) float64: the table `build` was given (boxes clipped, then divided by `scale`; with
                                     # scale="auto" by each frame's own of `scales`)
    params: TrainPairParams          # the draws `build` was given
    ids: np.ndarray                  # the distinct store ids, in `pairs`' frame numbering
    rows: np.ndarray                 # (B, 2) int64: the rows [template, search] of the pair's table
    sampler: np.ndarray              # (B,) which sampler of the plan each pair came from
    scales: Optional[np.ndarray] = None   # (F,) int64: the decode scale of each frame of `ids`


class PairLoader:
    """An iterator over the batches of one epoch of `plan`; every `iter()` continues the epoch in progress or, when there is none,
    starts the next one (`EpochPlan.start_epoch`: a fresh permutation).  `row_ids[s][row]` is the store id of row `row` of sampler
    s's table (what `fill_store` returns).  `scale` 2, 4 or 8 decodes the frames at that fraction and divides the boxes
    (`scale_pairs`); `rows=False` decodes whole frames; `windows=True` decodes per frame the rectangle the batch reads, as compact
    tensors (`JpegStore.decode_windows`), and hands out the same batches.  `scale="auto"` picks a scale per frame and batch: the draws
    are made once on the full-size table, `TrainPairBuilder.frame_scales(..., max_scale=)` gives each frame the largest scale that
    upsamples no crop read from it, `scale_pairs` divides each box by its frame's scale and the store decodes the mixed call
    (`decode_rows` / `decode_windows` / `decode` with `scale=item.scales`); the draws and the generator stream are those of scale 1,
    the crops are not (they are resampled from smaller frames), and there is no new generator state, so resuming is unaffected.
    The loader never waits for the GPU and never reads from it; call
    `store.check()` at the end of an epoch to see the decode statuses.  `datasets` are the tables' dataset names, sorted."""

    def __init__(self, plan: EpochPlan, store, row_ids: Sequence[np.ndarray], builder, scale=1, rows: bool = True, prefetch: int = 1,
                 windows: bool = False, max_scale: int = 8):
        if prefetch not in (0, 1):
            raise ValueError("prefetch is 0 or 1")
        if max_scale not in (1, 2, 4, 8) or isinstance(max_scale, bool):
            raise ValueError("max_scale is 1, 2, 4 or 8")
        self.auto, self.max_scale = isinstance(scale, str), int(max_scale)
        if self.auto and scale != "auto":
            raise ValueError(f'scale is 1, 2, 4, 8 or "auto", not {scale!r}')
        if not self.auto and (isinstance(scale, bool) or scale not in (1, 2, 4, 8)):
            raise ValueError(f'scale is 1, 2, 4, 8 or "auto", not {scale!r}')
        scale = 1 if self.auto else scale
        if len(row_ids) != len(plan.samplers):
            raise ValueError(f"row_ids has {len(row_ids)} entries, the plan {len(plan.samplers)} samplers")
        self.plan, self.store, self.builder = plan, store, builder
        self.scale, self.rows, self.prefetch, self.windows = int(scale), bool(rows), int(prefetch), bool(windows)
        self.row_ids = [np.asarray(r, dtype=np.int64) for r in row_ids]
        for s, r in zip(plan.samplers, self.row_ids):
            if r.shape != (len(s.table),):
                raise ValueError("row_ids gives one store id per table row")
        self.datasets: List[str] = sorted({str(d) for s in plan.samplers for d in s.table.dataset.tolist()})
        code = {name: k for k, name in enumerate(self.datasets)}
        self._dataset_code = [np.array([code[str(d)] for d in s.table.dataset.tolist()], dtype=np.int32) for s in plan.samplers]
        self.device = builder.device
        self._stream: Optional[torch.cuda.Stream] = None
        self._position: Optional[int] = None                   # the next batch to hand out; None between epochs
        self._ahead = None                                     # (number, snapshot, item, event): the batch in flight

    def __len__(self) -> int:
        return len(self.plan)

    # ------------------------------------------------------------------------------------------------------------------ one batch
    def _host(self, positions: np.ndarray):
        """The host side up to the pair table: the sampled rows, the clipped boxes, the distinct files."""
        B = positions.size
        which, index = self.plan.locate(positions)
        rows = np.zeros((B, 2), dtype=np.int64)
        ids, boxes = np.zeros((B, 2), dtype=np.int64), np.zeros((B, 2, 4), dtype=np.float64)
        visible, dataset = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        for s, sampler in enumerate(self.plan.samplers):       # (a loop over the samplers, in their order: never over pairs)
            mine = np.flatnonzero(which == s)
            if mine.size == 0:
                continue
            r = sampler.pairs(index[mine])
            rows[mine] = r
            ids[mine] = self.row_ids[s][r]
            boxes[mine] = sampler.table.bbox[r]
            visible[mine] = sampler.table.presence[r[:, 1]] != 0
            dataset[mine] = self._dataset_code[s][r[:, 1]]
        distinct, frame = np.unique(ids.reshape(-1), return_inverse=True)
        frame = frame.reshape(B, 2)
        clipped = clip_boxes(boxes.reshape(-1, 4), self.store.shape(ids.reshape(-1))).reshape(B, 2, 4)
        pairs = np.zeros((B, 11), dtype=np.float64)
        pairs[:, 0], pairs[:, 1:5] = frame[:, 0], clipped[:, 0]
        pairs[:, 5], pairs[:, 6:10] = frame[:, 1], clipped[:, 1]
        pairs[:, 10] = visible
        if self.scale > 1:
            pairs = scale_pairs(pairs, self.scale)
        return pairs, distinct, visible, dataset, rows, which

    def _load(self, positions: np.ndarray) -> LoadedBatch:
        """The whole data stage of one batch on the current stream."""
        pairs, ids, visible, dataset, rows, which = self._host(positions)
        store, builder = self.store, self.builder
        scale = self.scale
        shapes = store.shape(ids, scale)
        params = builder.draw(pairs, shapes)
        if self.auto:                                          # the draws are the full-size table's; the frames and boxes each frame's own
            scale = builder.frame_scales(pairs, params, shapes, self.max_scale)
            pairs, shapes = scale_pairs(pairs, scale), store.shape(ids, scale)
            params = replace(params, frame_shapes=tuple((int(h), int(w)) for h, w in shapes.tolist()))
        if self.windows:
            frames = store.decode_windows(ids, builder.frame_windows(pairs, params, shapes), scale=scale)
        elif self.rows:
            frames = store.decode_rows(ids, builder.frame_rows(pairs, params, shapes), scale=scale)
        else:
            frames = store.decode(ids, scale=scale)
        batch = builder.build(frames, pairs, params, borders=store.borders(ids))
        B = len(visible)
        pinned = torch.empty((2, B), dtype=torch.int32, pin_memory=True)
        np.copyto(pinned.numpy(), np.stack([visible, dataset]))
        with torch.cuda.device(self.device):
            both = pinned.to(self.device, non_blocking=True)
        return LoadedBatch(batch, both[0], both[1], pairs, params, ids, rows, which,
                           scale if self.auto else np.full(ids.size, scale, dtype=np.int64))

    def _snapshot(self, number: int) -> Dict[str, Any]:
        """The generator states in front of batch `number`: what is needed to draw it again."""
        return dict(position=int(number), samplers=[_generator_state(s.generator) for s in self.plan.samplers],
                    builder=_generator_state(self.builder.generator))

    def _enqueue(self, number: int):
        snapshot = self._snapshot(number)
        positions = self.plan.batches[number]
        if not self.prefetch:
            return number, snapshot, self._load(positions), None
        with torch.cuda.device(self.device):
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._stream):
                item = self._load(positions)
                event = torch.cuda.Event()
                event.record(self._stream)
        return number, snapshot, item, event

    def _hand_out(self, item: LoadedBatch, event) -> LoadedBatch:
        if event is not None:
            with torch.cuda.device(self.device):
                consumer = torch.cuda.current_stream(self.device)
                consumer.wait_event(event)
                for t in tuple(item.batch) + (item.visible, item.dataset_ids):
                    t.record_stream(consumer)
        return item

    def __iter__(self) -> Iterator[LoadedBatch]:
        if self._position is None or self._position >= len(self.plan.batches):
            self.plan.start_epoch()
            self._position, self._ahead = 0, None
        n = len(self.plan.batches)
        while self._position is not None and self._position < n:
            k = self._position
            if self._ahead is None or self._ahead[0] != k:
                self._ahead = self._enqueue(k)
            _, _, item, event = self._ahead
            self._ahead = self._enqueue(k + 1) if self.prefetch and k + 1 < n else None
            self._position = k + 1
            yield self._hand_out(item, event)
        self._position, self._ahead = None, None

    # ---------------------------------------------------------------------------------------------------------------------- state
    def state_dict(self) -> Dict[str, Any]:
        """The plan's state (the samplers' epoch rows, frame offsets and generators, the plan's generator, the epoch's batches), the
        builder's generator and the position in the epoch — with a batch in flight, the states in front of it.  Arrays are CPU tensors,
        so the dict goes through `save_training_checkpoint`."""
        state = self.plan.state_dict()
        snapshot = self._ahead[1] if self._ahead is not None else self._snapshot(-1 if self._position is None else self._position)
        for saved, generator in zip(state["samplers"], snapshot["samplers"]):
            saved["generator"] = generator
        state["builder"] = snapshot["builder"]
        state["position"] = snapshot["position"]

        def tensors(v):
            if isinstance(v, dict):
                return {k: tensors(x) for k, x in v.items()}
            if isinstance(v, list):
                return [tensors(x) for x in v]
            return torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        return tensors(state)

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        def arrays(v):
            if isinstance(v, dict):
                return {k: arrays(x) for k, x in v.items()}
            if isinstance(v, list):
                return [arrays(x) for x in v]
            return v.numpy() if isinstance(v, torch.Tensor) else v
        state = arrays(state)
        self.plan.load_state_dict(state)
        _set_generator_state(self.builder.generator, state["builder"])
        self._position = None if int(state["position"]) < 0 else int(state["position"])
        self._ahead = None
