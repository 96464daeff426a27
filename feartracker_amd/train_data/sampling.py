"""Which frames a training pair uses: the reference's annotation tables, its `TrackSampler` and the order of an epoch (host, numpy).

* `TrackTable` — the rows of one annotation CSV (model_training/dataset/track_sampling.py reads them with pandas): `track_id`,
  `frame_index`, `img_path`, `bbox` written as the text "[x, y, w, h]", `presence`, `near_corner`, `dataset`.  Read with the `csv`
  module; the box is parsed by hand, never evaluated.
* `TrackSampler` — the reference's rule restated as a distribution.  Its pandas / `random` streams cannot be matched and are not
  attempted: all randomness comes from one `np.random.Generator`, and every choice among n candidates is floor(u n) of one
  `Generator.random` double, so that a vectorised draw consumes the stream exactly as the same draws made one by one.
* `EpochPlan` — `ConcatDataset` + `DataLoader(shuffle=True, drop_last=True)`, with `DistributedSampler`'s split over ranks, and
  the end of an epoch: every sampler resampled, `update_offset` applied (train/fear_lightning_model.py:260-284).

Row numbers are always rows of the TABLE (file order), also after negatives were dropped: `sampler.rows` lists the rows a sampler
kept, and `pairs` returns table rows, so `table.bbox[row]`, `table.img_path[row]` and a per-row list of store ids index directly.
"""
from __future__ import annotations

import csv
import math
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

COLUMNS = ("track_id", "frame_index", "img_path", "bbox", "presence", "near_corner", "dataset")
_TRUE, _FALSE = ("true", "1", "1.0"), ("false", "0", "0.0", "")


def parse_bbox(text: str) -> List[float]:
    """"[x, y, w, h]" -> four floats; integers, floats, exponents and signs as Python writes them.  ValueError for anything else."""
    s = str(text).strip()
    if len(s) < 2 or s[0] not in "[(" or s[-1] != {"[": "]", "(": ")"}[s[0]]:
        raise ValueError(f"a box is written [x, y, w, h], not {text!r}")
    parts = s[1:-1].split(",")
    if len(parts) != 4:
        raise ValueError(f"a box has four values, {text!r} has {len(parts)}")
    values = [float(p) for p in parts]                       # float() takes digits, signs, a point and an exponent: no names, no calls
    if not all(math.isfinite(v) for v in values):
        raise ValueError(f"a box has finite values, not {text!r}")
    return values


def _flag(text: str, what: str) -> bool:
    s = str(text).strip().lower()
    if s in _TRUE:
        return True
    if s in _FALSE:
        return False
    raise ValueError(f"{what} is True / False or 1 / 0, not {text!r}")


def _generator_state(rng: np.random.Generator) -> Dict[str, Any]:
    """The bit generator's state with its 128-bit integers as decimal text, so that it goes through `torch.save` and back with
    `weights_only=True`."""
    def text(v):
        return {k: text(x) for k, x in v.items()} if isinstance(v, dict) else (str(v) if isinstance(v, int) else v)
    return text(rng.bit_generator.state)


def _set_generator_state(rng: np.random.Generator, state: Dict[str, Any]) -> None:
    def number(v):
        if isinstance(v, dict):
            return {k: number(x) for k, x in v.items()}
        return int(v) if isinstance(v, str) and v.lstrip("-").isdigit() else v
    rng.bit_generator.state = number(state)


class TrackTable:
    """The rows of one annotation file, in file order, as arrays: `track_id` and `dataset` and `img_path` (object arrays of str),
    `frame_index` (int64), `bbox` ((N, 4) float64 xywh), `presence` (int32), `near_corner` (bool).  `track_rows[t]` lists the rows of
    track t in file order — the reference's `data.groupby("track_id").groups`; `track_code[row]` numbers the tracks in order of first
    appearance and `tracks[code]` names them.  `root` is joined in front of every `img_path` by `paths()`."""

    def __init__(self, track_id, frame_index, img_path, bbox, presence, near_corner, dataset, root: Optional[str] = None):
        n = len(track_id)
        self.track_id = np.array([str(t) for t in track_id], dtype=object).reshape(n)
        self.frame_index = np.asarray(frame_index, dtype=np.int64).reshape(n)
        self.img_path = np.array([str(p) for p in img_path], dtype=object).reshape(n)
        self.bbox = np.asarray(bbox, dtype=np.float64).reshape(n, 4)
        self.presence = np.asarray(presence).astype(np.int32).reshape(n)
        self.near_corner = np.asarray(near_corner).astype(bool).reshape(n)
        dataset = [dataset] * n if isinstance(dataset, str) else dataset
        self.dataset = np.array([str(d) for d in dataset], dtype=object).reshape(n)
        self.root = None if root is None else str(root)
        if n == 0:
            raise ValueError("an annotation table needs at least one row")
        names, first, code = np.unique(self.track_id.astype(str), return_index=True, return_inverse=True)
        by_arrival = np.argsort(first, kind="stable")                     # number the tracks in order of first appearance
        rank = np.empty(len(names), dtype=np.int64)
        rank[by_arrival] = np.arange(len(names))
        self.track_code = rank[code.reshape(n)]
        self.tracks = np.array(names[by_arrival], dtype=object)
        order = np.argsort(self.track_code, kind="stable")
        cuts = np.cumsum(np.bincount(self.track_code, minlength=len(names)))[:-1]
        self.track_rows: Dict[str, np.ndarray] = dict(zip(self.tracks.tolist(), np.split(order, cuts)))

    def __len__(self) -> int:
        return int(self.track_id.size)

    @classmethod
    def from_arrays(cls, track_id, frame_index, img_path, bbox, presence, near_corner, dataset, root: Optional[str] = None) -> "TrackTable":
        return cls(track_id, frame_index, img_path, bbox, presence, near_corner, dataset, root=root)

    @classmethod
    def from_csv(cls, path: str, root: Optional[str] = None) -> "TrackTable":
        """Read an annotation file.  Further columns (pandas' unnamed index column among them) are ignored; a missing column, a
        malformed box, number or flag is a ValueError that names the file and the line."""
        cols: Dict[str, list] = {name: [] for name in COLUMNS}
        with open(path, newline="") as fh:
            reader = csv.DictReader(fh)
            missing = [name for name in COLUMNS if name not in (reader.fieldnames or ())]
            if missing:
                raise ValueError(f"{path}: line 1: no column {', '.join(missing)}")
            for record in reader:
                line = reader.line_num
                try:
                    if any(record[name] is None for name in COLUMNS):
                        raise ValueError("the line has fewer fields than the header")
                    values = dict(track_id=record["track_id"], frame_index=int(float(record["frame_index"])), img_path=record["img_path"],
                                  bbox=parse_bbox(record["bbox"]), presence=int(float(record["presence"])),
                                  near_corner=_flag(record["near_corner"], "near_corner"), dataset=record["dataset"])
                except ValueError as err:
                    raise ValueError(f"{path}: line {line}: {err}") from None
                for name in COLUMNS:
                    cols[name].append(values[name])
        if not cols["track_id"]:
            raise ValueError(f"{path}: line 1: no rows")
        return cls(root=root, **cols)

    def to_csv(self, path: str) -> None:
        """Write the file `from_csv` reads (the boxes with `repr`, which reads back to the same doubles)."""
        with open(path, "w", newline="") as fh:
            writer = csv.writer(fh)
            writer.writerow(COLUMNS)
            for i in range(len(self)):
                box = "[" + ", ".join(repr(int(v)) if float(v).is_integer() else repr(float(v)) for v in self.bbox[i]) + "]"
                writer.writerow([self.track_id[i], int(self.frame_index[i]), self.img_path[i], box, int(self.presence[i]),
                                 bool(self.near_corner[i]), self.dataset[i]])

    def paths(self) -> List[str]:
        """Every row's file, `root` joined in front."""
        return [p if self.root is None else os.path.join(self.root, p) for p in self.img_path.tolist()]


def kept_negatives(n_rows: int, n_negative: int, negative_ratio: float) -> int:
    """The reference's count: max(0, int(min(share of negative rows, negative_ratio) * N)) (track_sampling.py:72-73)."""
    return max(0, int(min(n_negative / n_rows, negative_ratio) * n_rows))


def _pick(u: np.ndarray, n: np.ndarray) -> np.ndarray:
    """floor(u n) for u in [0, 1): uniform over 0..n-1 (to 2^-53), one double of the stream per choice."""
    return np.minimum((u * n).astype(np.int64), n - 1)


class TrackSampler:
    """The reference's `TrackSampler` (model_training/dataset/track_sampling.py:46-115) on a `TrackTable`.

    Negatives: `kept_negatives(...)` of the `presence == 0` rows are kept, chosen without replacement; the others are dropped (`rows`:
    the kept table rows, ascending).  Templates: the kept rows with `presence == 1` that are not `near_corner`; `num_tracks` counts
    their distinct tracks.  `resample()` draws the epoch's template rows (`epoch_rows`, `num_samples` of them): without replacement when
    every template row is its own track, else ceil(num_samples / num_tracks) rows per track with replacement and of those a uniformly
    random `num_samples`-subset in uniformly random order.  `pair(idx)` takes epoch row idx as the template and draws the search row
    uniformly from the kept rows of the same track — with `clip_range` from those whose frame_index lies strictly inside
    (template.frame_index - frame_offset, template.frame_index + frame_offset); the template row itself, `near_corner` rows and kept
    negatives are candidates.  `pairs(indices)` is the same for many, vectorised, draw for draw."""

    def __init__(self, table: TrackTable, negative_ratio: float, frame_offset: int, num_samples: int, clip_range: bool = False,
                 seed: Optional[int] = None):
        self.table = table
        self.negative_ratio, self.frame_offset = float(negative_ratio), int(frame_offset)
        self.num_samples, self.clip_range = int(num_samples), bool(clip_range)
        self.generator = np.random.default_rng(seed)
        n = len(table)
        negative = np.flatnonzero(table.presence == 0)
        keep = kept_negatives(n, negative.size, self.negative_ratio)
        kept = self.generator.choice(negative, size=keep, replace=False) if keep else negative[:0]
        mask = table.presence != 0
        mask[kept] = True
        self._index(np.flatnonzero(mask))
        self.epoch_rows = np.zeros(0, dtype=np.int64)
        self.resample()

    def _index(self, rows: np.ndarray) -> None:
        """The lookup arrays for the kept rows: per track its rows sorted by frame_index (ties in file order), as one array with
        per-track offsets, and the template rows grouped by track likewise."""
        t = self.table
        self.rows = rows.astype(np.int64)
        code, frame = t.track_code[self.rows], t.frame_index[self.rows]
        n_tracks = len(t.tracks)
        order = np.lexsort((self.rows, frame, code))
        self._by_track = self.rows[order]                                 # kept rows, by track, then frame_index, then file order
        self._frame = frame[order]
        self._count = np.bincount(code, minlength=n_tracks).astype(np.int64)
        self._start = np.concatenate([[0], np.cumsum(self._count)[:-1]]).astype(np.int64)
        self.track_rows = {name: np.sort(self._by_track[s:s + c]) for name, s, c in zip(t.tracks.tolist(), self._start, self._count) if c}
        # clip_range's bisection key (track, frame_index), ascending in the order above: made here, once per set of kept rows, so that
        # `pairs` costs two bisections per pair whatever the table's size
        self._base = int(self._frame.min()) if self._frame.size else 0
        self._span = int(self._frame.max()) - self._base + 1 if self._frame.size else 1
        self._key = np.repeat(np.arange(n_tracks, dtype=np.int64), self._count) * self._span + (self._frame - self._base)
        is_template = (t.presence[self.rows] == 1) & ~t.near_corner[self.rows]
        self.template_rows = self.rows[is_template]
        tcode = t.track_code[self.template_rows]
        self.num_tracks = int(np.unique(tcode).size)
        if self.template_rows.size == 0:
            raise ValueError("no row has presence == 1 and near_corner == False: nothing can be a template")
        torder = np.argsort(tcode, kind="stable")
        self._t_by_track = self.template_rows[torder]
        tcount = np.bincount(tcode, minlength=n_tracks).astype(np.int64)
        tstart = np.concatenate([[0], np.cumsum(tcount)[:-1]]).astype(np.int64)
        has = tcount > 0
        self._t_start, self._t_count = tstart[has], tcount[has]

    def __len__(self) -> int:
        return int(self.epoch_rows.size)

    def resample(self) -> None:
        rng, n = self.generator, self.num_samples
        if self.num_tracks == self.template_rows.size:
            if n > self.template_rows.size:
                raise ValueError(f"num_samples = {n}, but there are only {self.template_rows.size} template rows to draw from without "
                                 "replacement")
            self.epoch_rows = rng.choice(self.template_rows, size=n, replace=False)
            return
        per_track = int(math.ceil(n / self.num_tracks))
        u = rng.random((self.num_tracks, per_track))
        pool = self._t_by_track[self._t_start[:, None] + _pick(u, self._t_count[:, None])].reshape(-1)
        self.epoch_rows = pool[rng.permutation(pool.size)[:n]]

    def pairs(self, indices) -> np.ndarray:
        """(len(indices), 2) int64: the table rows [template, search] for the epoch rows `indices`."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"an index outside 0..{len(self) - 1}")
        t = self.table
        template = self.epoch_rows[idx]
        code = t.track_code[template]
        lo, hi = self._start[code], self._start[code] + self._count[code]
        if self.clip_range:
            # within a track the rows are sorted by frame_index: the window is a run, found by bisection on (track, frame_index)
            span, key = self._span, self._key
            centre = t.frame_index[template] - self._base
            first = np.clip(centre - self.frame_offset + 1, 0, span)      # frame_index > centre - offset
            last = np.clip(centre + self.frame_offset - 1, -1, span - 1)  # frame_index < centre + offset
            lo = np.maximum(lo, np.searchsorted(key, code * span + first, side="left"))
            hi = np.minimum(hi, np.searchsorted(key, code * span + last, side="right"))
            if (hi <= lo).any():
                raise ValueError(f"frame_offset = {self.frame_offset} leaves a template without a search candidate")
        search = self._by_track[lo + _pick(self.generator.random(idx.size), hi - lo)] if idx.size else template
        return np.stack([template, search], axis=1)

    def pair(self, idx: int) -> np.ndarray:
        """(2,) int64: the table rows [template, search] of epoch row `idx`."""
        return self.pairs([int(idx)])[0]

    def state_dict(self) -> Dict[str, Any]:
        return dict(rows=self.rows.copy(), epoch_rows=self.epoch_rows.copy(), frame_offset=int(self.frame_offset),
                    generator=_generator_state(self.generator))

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        rows = np.asarray(state["rows"], dtype=np.int64)
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= len(self.table)):
            raise ValueError("the state was saved for another table")
        if not np.array_equal(rows, self.rows):
            self._index(rows)
        self.epoch_rows = np.asarray(state["epoch_rows"], dtype=np.int64).copy()
        self.frame_offset = int(state["frame_offset"])
        _set_generator_state(self.generator, state["generator"])


def update_offset(frame_offset: int, epoch: int, start_epoch: int, freq: int, step: int, max_value: int) -> int:
    """The reference's `update_offset` for one sampler (fear_lightning_model.py:266-284); `epoch` is the index of the epoch that ended."""
    if (epoch + 1) >= start_epoch and (epoch + 1) % freq == 0:
        return min(int(max_value), int(frame_offset) + int(step))
    return int(frame_offset)


class EpochPlan:
    """The order of an epoch over several samplers: position p of the concatenation is epoch row p - offsets[s] of sampler s.

        plan = EpochPlan([sampler], batch_size=128, seed=0)
        for positions in plan.start_epoch():              # (batches, B) positions, a fresh random permutation cut into full batches
            sampler_index, index = plan.locate(positions)
        plan.end_epoch(epoch, dynamic_frame_offset=dict(start_epoch=20, freq=5, step=5, max_value=150))

    With `world` > 1 a rank takes the positions rank::world of the permutation after it was wrapped to a multiple of `world`
    (`DistributedSampler`); every rank must be given the same `seed`, the samplers their own."""

    def __init__(self, samplers: Sequence[TrackSampler], batch_size: int, seed: Optional[int], rank: int = 0, world: int = 1):
        self.samplers = list(samplers)
        self.batch_size, self.rank, self.world = int(batch_size), int(rank), int(world)
        if not self.samplers or self.batch_size < 1 or not 0 <= self.rank < self.world:
            raise ValueError("a plan takes at least one sampler, a batch size of at least 1 and a rank in 0..world-1")
        self.generator = np.random.default_rng(seed)
        self.batches = np.zeros((0, self.batch_size), dtype=np.int64)     # the current epoch's, set by `start_epoch`
        self._measure()

    def _measure(self) -> None:
        """`offsets`: where each sampler's positions begin in the concatenation; made again whenever the samplers' epochs change."""
        self.offsets = np.concatenate([[0], np.cumsum([len(s) for s in self.samplers])]).astype(np.int64)

    def __len__(self) -> int:
        """Batches per epoch."""
        total = int(self.offsets[-1])
        mine = -(-total // self.world)
        return mine // self.batch_size

    def start_epoch(self) -> np.ndarray:
        total = int(self.offsets[-1])
        order = self.generator.permutation(total)
        if self.world > 1:
            padded = -(-total // self.world) * self.world
            order = np.concatenate([order, order[:padded - total]])[self.rank::self.world]
        n = order.size // self.batch_size
        self.batches = order[:n * self.batch_size].reshape(n, self.batch_size)
        return self.batches

    def locate(self, positions):
        """(sampler number, index into that sampler's epoch) for positions of the concatenation."""
        positions = np.asarray(positions, dtype=np.int64)
        offsets = self.offsets
        which = np.searchsorted(offsets, positions, side="right") - 1
        return which, positions - offsets[which]

    def end_epoch(self, epoch: int, dynamic_frame_offset: Optional[Dict[str, int]] = None) -> None:
        """What the reference does when a validation epoch ends: `update_offset`, then every sampler resampled."""
        for s in self.samplers:
            if dynamic_frame_offset is not None:
                d = dynamic_frame_offset
                s.frame_offset = update_offset(s.frame_offset, epoch, d["start_epoch"], d["freq"], d["step"], d["max_value"])
            s.resample()
        self._measure()

    def state_dict(self) -> Dict[str, Any]:
        return dict(samplers=[s.state_dict() for s in self.samplers], generator=_generator_state(self.generator),
                    batches=self.batches.copy())

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        if len(state["samplers"]) != len(self.samplers):
            raise ValueError(f"the state holds {len(state['samplers'])} samplers, the plan {len(self.samplers)}")
        for s, saved in zip(self.samplers, state["samplers"]):
            s.load_state_dict(saved)
        self._measure()
        _set_generator_state(self.generator, state["generator"])
        self.batches = np.asarray(state["batches"], dtype=np.int64).reshape(-1, self.batch_size).copy()
