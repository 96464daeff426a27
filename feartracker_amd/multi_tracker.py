"""`FEARMultiTracker`: many targets per frame, one batched network pass, tracker state kept on the device.

`FEARTracker` (tracker.py) follows ONE object at batch 1 and waits on the host after every frame.  This tracker follows K
targets — K objects in one video, one object in each of K videos, or any mix — with the same per-target arithmetic and
the same config keys (`DEFAULT_TRACKING_CONFIG`, `smooth` included), and runs a frame as

    the frames up (one transfer each, on a copy stream)  ->  fear_crop_normalize_frames (K search crops, one launch)
    ->  fear_track (K templates)  ->  fear_tracker_step (decode, rescale, clamp, next crop geometry; one launch)
    ->  boxes and scores down (one non-blocking copy, guarded by an event)

Everything frame t + 1 needs from frame t — each target's context box and previous size — stays in device tensors, so
`submit` never synchronises (host frames and the small tables go up from pinned memory, non-blocking) and the next frame
can be submitted before the previous result is read.  Each target's boxes equal an independent `FEARTracker` on the same
frames (tests/test_multi_tracker.py) — frames the device path reads, see below.

Targets live in "streams": `add(image, rects, stream=s)` starts targets on frame `image` of stream s, and
`submit(images)` takes one frame (stream 0) or a sequence of frames, `images[s]` being the frame of stream s.  Frames of
different streams may differ in size.

With a model that lacks the device entry points (a CPU reference network, any torch model), or with `device_crop=False` /
`device_postprocess=False` in the config, the tracker runs the reference-style host path instead: per target the
`FEARTracker` crop, post-processing and geometry, around one batched `net.track`.  The path is chosen at construction;
the device path reads what `fear_crop_normalize` reads — uint8 H x W x >= 3 frames, numpy arrays or device tensors — and
rejects other frames (float, uint16, grey, CPU tensors) with a TypeError instead of switching paths behind the caller's
back, where FEARTracker would track them on the host.  A tracker built with `device_crop=False` takes them.

NV12 / I420 video frames (`YUVFrame`, host planes or device planes) are taken by both paths.  On the device path host planes go up
on the copy stream (half the bytes of the RGB frame).  A submit whose frames are all RGB runs `frame_table` +
`fear_crop_normalize_frames` as above.  A submit with any `YUVFrame` and fewer than `PLANAR_CROP_MAX_TARGETS` targets runs one
`fear_crop_normalize_planar` launch over a `frame_table_planar` table, which reads the planes directly; with more targets each
YUV frame is converted once (`fear_yuv_to_rgb`) and the RGB launch runs, which measured faster there.
Both give the same crops bit for bit.  The host path tracks the frames' RGB conversion.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .constants import TARGET_CLASSIFICATION_KEY, TARGET_REGRESSION_LABEL_KEY
from .frames import YUVFrame, host_rgb, mean_color
from .geometry import border_color_u8, clamp_bbox, crop_geometry, get_extended_crop
from .tracker import FEARTracker

# A submit with YUV frames and fewer targets than this crops from the planes (fear_crop_normalize_planar); from here on, one
# fear_yuv_to_rgb per frame + the RGB crop launch is faster (1080p, MI355X: planar 15 us against 24 us at K = 16, 178 against
# 156 us at K = 256; profiles/multi_track_yuv_bench.json)
PLANAR_CROP_MAX_TARGETS = 32


def search_rows_host(ctx, stream, n_streams: int, out_hw: int = 256) -> np.ndarray:
    """`FEARMultiTracker.search_rows` in numpy (fear_tracker_rows): (n_streams, 2) int32, per stream the frame rows [y0, y1) that the
    search crops of its targets sample, as one range; (0, 0) for a stream without a target.  `ctx` is (K, 4) context boxes x, y, w, h
    and `stream` (K,) their streams.  The rule is the crop kernel's (crop_resize_normalize_kernel, `geometry.resize_bilinear_u8`): output
    row d of a crop taps the box's rows clip(i, 0, h - 1) and clip(i + 1, 0, h - 1), i = floor(float32((d + 0.5) h / out_hw - 0.5)),
    which move monotonically with d — so a crop taps y + (first tap of row 0) .. y + (second tap of row out_hw - 1).  For 1 <= h <=
    out_hw, and on the identity and 2 x 2 paths, that is every row y .. y + h - 1; a strong reduction starts behind y and ends in front
    of y + h - 1.  A degenerate box, h <= 0, has both taps pinned to h - 1 (the upper clip is applied last): the single row y + h - 1,
    which lies above the box.  The rows are not clipped to the frame, and a target whose columns miss its frame counts all the same."""
    ctx = np.asarray(ctx, dtype=np.int64).reshape(-1, 4)
    stream = np.asarray(stream, dtype=np.int64).reshape(-1)
    out = np.zeros((int(n_streams), 2), dtype=np.int32)
    S = int(out_hw)
    for s in range(int(n_streams)):
        lo = hi = None
        for x, y, w, h in ctx[stream == s]:
            with np.errstate(divide="ignore"):
                scale = np.float64(1.0) / (np.float64(S) / np.float64(h))
            taps = []
            for d in (0, S - 1):
                i = int(np.floor(np.float32((np.float64(d) + 0.5) * scale - 0.5)))
                taps += [min(max(i, 0), int(h) - 1), min(max(i + 1, 0), int(h) - 1)]
            first, last = int(y) + min(taps), int(y) + max(taps) + 1
            lo, hi = (first, last) if lo is None else (min(lo, first), max(hi, last))
        if lo is not None and lo < hi:
            out[s] = np.clip([lo, hi], -(1 << 30), 1 << 30)
    return out


class PendingBoxes:
    """The boxes of one `submit`, possibly still being computed: `result()` waits for that frame's copy only."""

    def __init__(self, ids: Sequence[int], boxes=None, scores=None, host: Optional[torch.Tensor] = None,
                 event: Optional[torch.cuda.Event] = None) -> None:
        self.ids = list(ids)
        self._boxes, self._scores = boxes, scores
        self._host, self._event = host, event

    def done(self) -> bool:
        return self._event is None or self._event.query()

    def _resolve(self) -> None:
        if self._boxes is not None:
            return
        k = len(self.ids)
        if self._event is not None:
            self._event.synchronize()
        raw = self._host.numpy()
        self._boxes = raw[: 16 * k].view(np.int32).reshape(k, 4).astype(np.int64)
        self._scores = raw[16 * k: 20 * k].view(np.float32).copy()
        self._host = self._event = None

    def result(self) -> Dict[int, np.ndarray]:
        """{target id: bbox [x, y, w, h] int ndarray} of this frame."""
        self._resolve()
        return {i: self._boxes[j] for j, i in enumerate(self.ids)}

    def scores(self) -> Dict[int, float]:
        """{target id: score} of this frame: sigmoid(cls) at the chosen cell, as `FEARTracker._postprocess` returns it."""
        self._resolve()
        return {i: float(self._scores[j]) for j, i in enumerate(self.ids)}


class FEARMultiTracker:
    """K targets over one or several video streams, one batched pass per frame (see the module docstring)."""

    def __init__(self, model: Any, cuda_id: Union[int, str] = 0, **tracking_config: Any) -> None:
        self.net = model
        self.tracking_config = tracking_config
        # the single-object tracker supplies the config-derived pieces (window, device) and is the host path's per-target unit
        self._proto = FEARTracker(model, cuda_id, **tracking_config)
        self.device = self._proto.device
        cfg = tracking_config
        self.device_path = (bool(cfg.get("device_crop", True)) and bool(cfg.get("device_postprocess", True)) and
                            self.device.type == "cuda" and hasattr(model, "crop_normalize_frames") and
                            hasattr(model, "tracker_step") and hasattr(model, "crop_normalize"))
        self._next_id = 0
        self._ids: List[int] = []
        self._stream = np.zeros(0, dtype=np.int32)          # the stream of each target, host copy
        self._planar = self.device_path and all(hasattr(model, a) for a in ("frame_table_planar", "crop_normalize_planar",
                                                                             "crop_normalize_yuv"))
        if self.device_path:
            dev = self.device
            self._window = self._proto.window.to(dev, torch.float64).reshape(-1).contiguous()
            self._ctx = torch.zeros((0, 4), dtype=torch.int32, device=dev)         # context box of the next crop
            self._prev = torch.zeros((0, 2), dtype=torch.float64, device=dev)      # box size inside the next crop
            self._pad = torch.zeros((0, 3), dtype=torch.uint8, device=dev)         # border colour (mean colour of the add frame)
            self._fidx = torch.zeros(0, dtype=torch.int32, device=dev)             # stream of each target = frame-table index
            self._tmpl = torch.zeros((0, 256, 8, 8), dtype=torch.float32, device=dev)
            self._out = torch.zeros(0, dtype=torch.uint8, device=dev)              # [boxes (K,4) int32 | scores (K,) fp32]
            self._frame_hw = None                                                    # (key, (K,2) int32 tensor)
            self._copy_stream = None                                                 # host frame uploads (_upload_frames)
        else:
            self._slots: List[FEARTracker] = []
            self._tmpl_host: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ bookkeeping
    @property
    def ids(self) -> List[int]:
        return list(self._ids)

    def __len__(self) -> int:
        return len(self._ids)

    def _readable(self, image) -> bool:
        """The frames fear_crop_normalize reads (FEARTracker._device_crop): uint8 H x W x >= 3, numpy or a device tensor; and
        `YUVFrame`s when the model has the planar entry points."""
        if isinstance(image, YUVFrame):
            return self._planar
        if isinstance(image, np.ndarray):
            return image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] >= 3
        return isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and \
            image.shape[2] >= 3

    def _check_frame(self, image) -> None:
        if self.device_path and not self._readable(image):
            raise TypeError("the device path reads uint8 (H, W, >=3) frames (numpy arrays or device tensors) and YUVFrames; "
                            "construct the tracker with device_crop=False for other frames")

    def _mean_color(self, image) -> np.ndarray:
        """np.mean(image, axis=(0, 1)) — for a device frame the same float64 number: the integer channel sums are exact."""
        if isinstance(image, YUVFrame):
            return mean_color(image, self.net)
        if isinstance(image, torch.Tensor):
            sums = image.to(torch.int64).sum(dim=(0, 1)).cpu().numpy()
            return sums.astype(np.float64) / float(image.shape[0] * image.shape[1])
        return np.mean(image, axis=(0, 1))

    def _to_device(self, arr: np.ndarray) -> torch.Tensor:
        """A host array on the device without waiting for the stream: staged in pinned memory, copied non-blocking (a pageable
        copy waits for all earlier work on the stream — the whole previous frame).  torch's pinned allocator keeps the staging
        block until the copy has run."""
        pinned = torch.empty(arr.shape, dtype=getattr(torch, arr.dtype.name), pin_memory=True)
        np.copyto(pinned.numpy(), arr)
        return pinned.to(self.device, non_blocking=True)

    def _upload(self, image):
        """A frame as the contiguous device uint8 (H, W, 3) tensor the crop kernel reads: host frames go up whole, in one
        non-blocking transfer; device frames are used in place.  A host `YUVFrame` goes up as its planes (one transfer each),
        a device one is used in place."""
        if isinstance(image, YUVFrame):
            if image.is_cuda:
                return image if image.device == self.device else image.to(self.device)
            return YUVFrame(image.format, tuple(self._to_device(p) for p in image.planes), image.height, image.width)
        if isinstance(image, torch.Tensor):
            return image[:, :, :3].to(self.device).contiguous()
        return self._to_device(image[:, :, :3])

    def _upload_frames(self, frames) -> List[torch.Tensor]:
        """The frames of one submit on the device.  Host frames go up on a copy stream of the tracker's own, so that the copy of
        frame t + 1 runs while frame t's kernels do (on the caller's stream it would wait for them); the caller's stream waits
        for the copies through an event.  Device frames stay on the caller's stream, where they may have been produced."""
        main = torch.cuda.current_stream(self.device)
        on_device = [isinstance(f, torch.Tensor) or (isinstance(f, YUVFrame) and f.is_cuda) for f in frames]
        out: list = [f if d else None for f, d in zip(frames, on_device)]
        if any(f is None for f in out):
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self.device)
            with torch.cuda.stream(self._copy_stream):
                for i, f in enumerate(frames):
                    if out[i] is None:
                        out[i] = self._upload(f)
            done = torch.cuda.Event()
            done.record(self._copy_stream)
            main.wait_event(done)
            for i, f in enumerate(frames):
                if not on_device[i]:                    # allocated on the copy stream, read on the caller's
                    for t in (out[i].planes if isinstance(out[i], YUVFrame) else (out[i],)):
                        t.record_stream(main)
        return [self._upload(f) if d else u for f, d, u in zip(frames, on_device, out)]

    # ------------------------------------------------------------------ targets
    def add(self, image, rects, stream: int = 0) -> List[int]:
        """Start tracking the [x, y, w, h] boxes `rects` ((4,) or (n, 4)) on `image`, the current frame of stream `stream`.
        Per target what `FEARTracker.initialize` does (clamp_bbox, the frame's mean colour, the template), with one template
        crop and one `get_features` for all the rects of the call.  Returns the new targets' ids.  Unlike `submit`, `add` may
        wait for the stream (the template crop's upload, the mean colour of a device frame)."""
        cfg = self.tracking_config
        self._check_frame(image)
        if isinstance(image, YUVFrame) and not self.device_path:
            image = host_rgb(image, self.net)
        rects = np.asarray(rects).reshape(-1, 4)
        n = rects.shape[0]
        if n == 0:
            return []
        if int(stream) < 0:
            raise ValueError("stream must be >= 0")
        shape = tuple(image.shape)
        mean = self._mean_color(image)
        boxes = [clamp_bbox(r, shape) for r in rects]
        new_ids = list(range(self._next_id, self._next_id + n))
        if self.device_path:
            dev = self.device
            tctx = np.stack([crop_geometry(shape, b, cfg["template_size"], cfg["template_bbox_offset"])[0] for b in boxes])
            pad = np.tile(border_color_u8(mean), (n, 1))
            if isinstance(image, YUVFrame):
                crop = self.net.crop_normalize_yuv(image, tctx, pad, cfg["template_size"])
            else:
                crop = self.net.crop_normalize(image[:, :, :3], tctx, pad, cfg["template_size"])
            z = self.net.get_features(crop)
            geo = [crop_geometry(shape, b, cfg["instance_size"], cfg["search_context"]) for b in boxes]
            ctx = np.stack([g[0] for g in geo]).astype(np.int32)
            prev = np.stack([np.asarray(g[1][2:], dtype=np.float64) for g in geo])
            self._ctx = torch.cat([self._ctx, torch.from_numpy(ctx).to(dev)])
            self._prev = torch.cat([self._prev, torch.from_numpy(prev).to(dev)])
            self._pad = torch.cat([self._pad, torch.from_numpy(pad).to(dev)])
            self._fidx = torch.cat([self._fidx, torch.full((n,), int(stream), dtype=torch.int32, device=dev)])
            self._tmpl = torch.cat([self._tmpl, z])
            self._out = torch.zeros(20 * (len(self._ids) + n), dtype=torch.uint8, device=dev)
            self._frame_hw = None
        else:
            crops = [get_extended_crop(image=image, bbox=b, offset=cfg["template_bbox_offset"], crop_size=cfg["template_size"])[0]
                     for b in boxes]
            z = self.net.get_features(torch.cat([self._proto._preprocess_image(c, self._proto._template_transform)
                                                 for c in crops]))
            for i, b in enumerate(boxes):
                slot = FEARTracker(self.net, self._proto.cuda_id, **cfg)
                st = slot.tracking_state
                st.bbox = b
                st.paths.append(b)
                st.mean_color = mean
                slot._template_features = z[i:i + 1]
                self._slots.append(slot)
            self._tmpl_host = z if self._tmpl_host is None else torch.cat([self._tmpl_host, z])
        self._ids.extend(new_ids)
        self._stream = np.concatenate([self._stream, np.full(n, int(stream), dtype=np.int32)])
        self._next_id += n
        return new_ids

    def remove(self, ids) -> None:
        """Stop tracking these targets; the state and template tensors are compacted on the device."""
        drop = set(int(i) for i in np.atleast_1d(ids))
        keep = [j for j, i in enumerate(self._ids) if i not in drop]
        if len(keep) == len(self._ids):
            return
        self._ids = [self._ids[j] for j in keep]
        self._stream = self._stream[keep]
        if self.device_path:
            sel = torch.tensor(keep, dtype=torch.int64, device=self.device)
            self._ctx, self._prev, self._pad, self._fidx, self._tmpl = (
                t.index_select(0, sel) for t in (self._ctx, self._prev, self._pad, self._fidx, self._tmpl))
            self._out = torch.zeros(20 * len(keep), dtype=torch.uint8, device=self.device)
            self._frame_hw = None
        else:
            self._slots = [self._slots[j] for j in keep]
            self._tmpl_host = self._tmpl_host[keep] if keep else None

    # ------------------------------------------------------------------ frames
    def _frames(self, images) -> list:
        frames = list(images) if isinstance(images, (list, tuple)) else [images]
        if len(self._stream) and int(self._stream.max()) >= len(frames):
            raise ValueError(f"targets on stream {int(self._stream.max())} but only {len(frames)} frame(s) given")
        for f in frames:
            self._check_frame(f)
        return frames

    def search_rows(self, n_streams: Optional[int] = None) -> torch.Tensor:
        """(S, 2) int32 on the device: per stream the frame rows [y0, y1) that the NEXT `submit` reads — the union, as one range, of
        the rows the search crop of every target on that stream samples (`search_rows_host` states the rule: for a context box
        (x, y, w, h) the rows y + clip(i, 0, h - 1) of the crop's bilinear row table, which for 1 <= h <= instance_size are
        y .. y + h - 1; the single row y + h - 1 for a degenerate box).  UNCLIPPED — `JpegStore.decode_rows` clips them to its
        frames; a stream without targets gets (0, 0).  `n_streams` defaults to the highest stream with a target plus one.  One small
        launch (`fear_tracker_rows`) over the state `add` and `fear_tracker_step` left on the device; it never waits for the GPU, so

            rows   = tracker.search_rows()
            frames = store.decode_rows(ids_t, rows)          # only the rows the tracker is about to read are decoded
            boxes  = tracker.submit(frames)

        runs without a synchronisation.  `add` still takes a fully decoded frame (it reads the frame's mean colour), and the host
        path, whose state lives on the host, raises."""
        if not self.device_path or not hasattr(self.net, "tracker_rows"):
            raise RuntimeError("search_rows needs the device path (a model with the device entry points, device_crop and "
                               "device_postprocess on): the host path keeps its state on the host")
        if n_streams is None:
            n_streams = int(self._stream.max()) + 1 if len(self._stream) else 0
        return self.net.tracker_rows(self._ctx, self._fidx, int(n_streams), int(self.tracking_config["instance_size"]))

    def draw(self, frames, colour=(0, 255, 0), thickness: int = 5) -> None:
        """Draw every target's latest box into its stream's frame, in place (`frames`: one frame, or a sequence indexed by stream):
        `visuals.draw_boxes` on the boxes and frame indices the last `submit` left on the device, on the current stream.  Nothing
        waits and no box reaches the host, so it may be called before the submit's `PendingBoxes` is read.  `colour` is one colour or
        one per target, in `ids` order.  The frames must be contiguous uint8 (H, W, 3) device tensors — the frames given to `submit`,
        or copies of them; a `YUVFrame` or a host frame raises TypeError, and the host path, whose boxes live on the host, raises as
        `search_rows` does."""
        from .visuals import draw_boxes
        if not self.device_path:
            raise RuntimeError("draw needs the device path (a model with the device entry points, device_crop and "
                               "device_postprocess on): the host path keeps its boxes on the host")
        frames = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        for f in frames:
            if not isinstance(f, torch.Tensor) or not f.is_cuda:
                raise TypeError("draw takes uint8 (H, W, 3) RGB frames on the device; convert a YUVFrame with yuv_to_rgb first")
        if len(self._stream) and int(self._stream.max()) >= len(frames):
            raise ValueError(f"targets on stream {int(self._stream.max())} but only {len(frames)} frame(s) given")
        k = len(self._ids)
        if k == 0:
            return
        draw_boxes(frames, self._out[: 16 * k].view(torch.int32).view(k, 4), self._fidx, colour, thickness)

    def submit(self, images) -> PendingBoxes:
        """Track every target on its stream's frame (`images`: one frame, or a sequence indexed by stream).  On the device
        path nothing waits for the GPU — every upload is a non-blocking copy from pinned memory, every launch asynchronous
        (tests/test_multi_tracker.py runs it under torch.cuda.set_sync_debug_mode("error")): the returned `PendingBoxes`
        resolves when its own copy has landed."""
        frames = self._frames(images)
        if not self._ids:
            return PendingBoxes([], np.zeros((0, 4), np.int64), np.zeros(0, np.float32))
        if not self.device_path:
            return self._submit_host(frames)
        cfg, net, k = self.tracking_config, self.net, len(self._ids)
        dev = self._upload_frames(frames)
        planar = any(isinstance(f, YUVFrame) for f in dev)          # all-RGB submits keep the RGB table and kernel
        if planar and k >= PLANAR_CROP_MAX_TARGETS:
            dev = [net.yuv_to_rgb(f) if isinstance(f, YUVFrame) else f for f in dev]
            planar = False
        table = net.frame_table_planar(dev) if planar else net.frame_table(dev)
        key = tuple(tuple(f.shape[:2]) for f in dev)
        if self._frame_hw is None or self._frame_hw[0] != key:
            hw = np.array([key[s] for s in self._stream], dtype=np.int32).reshape(k, 2)
            self._frame_hw = (key, self._to_device(hw))
        crop = net.crop_normalize_planar if planar else net.crop_normalize_frames
        search = crop(table, self._fidx, self._ctx, self._pad, cfg["instance_size"])
        bbox, cls = net.track_maps(search, self._tmpl)
        boxes = self._out[: 16 * k].view(torch.int32).view(k, 4)
        scores = self._out[16 * k:].view(torch.float32)
        net.tracker_step(cls, bbox, self._frame_hw[1], boxes, self._ctx, self._prev, scores, bool(cfg.get("smooth", False)),
                         self._window, cfg["penalty_k"], cfg["window_influence"], cfg["lr"], cfg["score_size"],
                         cfg["total_stride"], cfg["instance_size"], cfg["search_context"])
        host = torch.empty(20 * k, dtype=torch.uint8, pin_memory=True)
        host.copy_(self._out, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.device))
        return PendingBoxes(self._ids, host=host, event=event)

    def _submit_host(self, frames) -> PendingBoxes:
        """The reference-style path: FEARTracker.update's host branch per target around one batched net.track."""
        cfg = self.tracking_config
        frames = [host_rgb(f, self.net) if isinstance(f, YUVFrame) else f for f in frames]
        crops = []
        for slot, s in zip(self._slots, self._stream):
            st = slot.tracking_state
            crop, box_in_crop, context = get_extended_crop(image=frames[s], bbox=st.bbox, crop_size=cfg["instance_size"],
                                                           offset=cfg["search_context"], padding_value=st.mean_color)
            st.mapping = context
            st.prev_size = box_in_crop[2:]
            crops.append(slot._preprocess_image(crop, slot._search_transform))
        out = self.net.track(torch.cat(crops), self._tmpl_host)
        boxes, scores = [], []
        for j, (slot, s) in enumerate(zip(self._slots, self._stream)):
            st = slot.tracking_state
            pred, score = slot._postprocess(track_result={key: out[key][j:j + 1] for key in
                                                          (TARGET_CLASSIFICATION_KEY, TARGET_REGRESSION_LABEL_KEY)})
            pred = clamp_bbox(slot._rescale_bbox(pred, st.mapping), frames[s].shape)
            st.bbox = pred
            st.paths.append(pred)
            boxes.append(np.asarray(pred, dtype=np.int64))
            scores.append(float(score))
        return PendingBoxes(self._ids, np.stack(boxes), np.asarray(scores, dtype=np.float32))

    def update(self, images) -> Dict[int, np.ndarray]:
        """`submit(images).result()`: {target id: bbox} of this frame."""
        return self.submit(images).result()
