"""Pictures made on the device: boxes drawn into frames, and the best / worst batch miner.

* `draw_boxes` — `fear_draw_boxes_u8` (include/fear_train.h): rectangles drawn in place into uint8 (H, W, 3) device frames, in a defined
  order, on the current stream, without a synchronisation.  `FEARMultiTracker.draw` feeds it the boxes `fear_tracker_step` left on the
  device, so a serving pipeline marks its targets without a box or a frame reaching the host.
* `BestWorstMiner` — the reference's `BestWorstMinerCallback` (model_training/train/callbacks.py:95-230) with
  `FEARLightningModel.get_visuals` (train/fear_lightning_model.py:217-258) behind it, as one operator, `fear_miner_update`: the step's
  score is compared with the best and the worst of the epoch on the device, and only a step that becomes one of them renders its batch —
  template next to search crop, the predicted box in green, the ground-truth box in red (blue when the target is invisible) — into that
  side's sheet.  `update` copies nothing and never waits; `sheets` is the one copy.
* `draw_boxes_host`, `miner_host` — the numpy statements of both, the operators' references in the tests.

The rectangle contract is the project's own (include/fear_train.h states it): an outline exactly `thickness` pixels wide with square
corners, `pt2 = (x + w, y + h)` inclusive, the last box in index order wins a shared pixel.  cv2's thick lines (round end caps, a
fixed-point half-width) are not restated and parity with `cv2.rectangle` is not pinned.

Deviations from the reference, all deliberate: the miner renders the maps of the training step itself where the reference runs the kept
batch again in eval mode (one forward pass saved); a denormalised value outside 0..255 is cut to the range where the reference's
`astype(np.uint8)` wraps; the text headers (`vstack_header`: dataset and file names, "Batch Score") are not rendered — `sheets` returns
the score and the step, the key a caller looks the names up with.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .metrics import INSTANCE_SIZE, SCORE_SIZE, decode_host
from .train_abi import FEAR_MINER_MAX_IMAGES, FearFrame, FearMinerState, launch, load_train_library
from .train_data.staging import Staging

MAX_BOXES, MAX_THICKNESS = 65535, 32
TEMPLATE_SIZE, SHEET_W, ITEM_H = 128, 384, 256
PRED_COLOUR, GT_COLOUR, GT_INVISIBLE_COLOUR = (0, 250, 0), (250, 0, 0), (0, 0, 250)
MINER_THICKNESS = 2
BOX_LIMIT = 1 << 20
MINER_STATE_DTYPE = np.dtype(FearMinerState)
_FRAME_DTYPE = np.dtype(FearFrame)
_STD = np.array([0.229, 0.224, 0.225], dtype=np.float64)
_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- the numpy statements
def _fill(img: np.ndarray, ya: int, yb: int, xa: int, xb: int, colour) -> None:
    """Rows ya..yb and columns xa..xb, both inclusive, cut to the image."""
    ya, xa, yb, xb = max(ya, 0), max(xa, 0), min(yb, img.shape[0] - 1), min(xb, img.shape[1] - 1)
    if ya <= yb and xa <= xb:
        img[ya:yb + 1, xa:xb + 1] = colour


def draw_box_host(img: np.ndarray, box, colour, thickness: int) -> None:
    """One box's band into one (H, W, 3) uint8 image, in place: the outer rectangle where the inner one is empty, else the four strips
    around the inner one."""
    x, y, w, h = (int(v) for v in box)
    x0, x1, y0, y1 = min(x, x + w), max(x, x + w), min(y, y + h), max(y, y + h)
    o, i = thickness // 2, (thickness - 1) // 2
    ix0, ix1, iy0, iy1 = x0 + i + 1, x1 - i - 1, y0 + i + 1, y1 - i - 1
    if ix0 > ix1 or iy0 > iy1:
        _fill(img, y0 - o, y1 + o, x0 - o, x1 + o, colour)
        return
    _fill(img, y0 - o, iy0 - 1, x0 - o, x1 + o, colour)
    _fill(img, iy1 + 1, y1 + o, x0 - o, x1 + o, colour)
    _fill(img, iy0, iy1, x0 - o, ix0 - 1, colour)
    _fill(img, iy0, iy1, ix1 + 1, x1 + o, colour)


def draw_boxes_host(frames, boxes, frame_of, colours, thickness: int):
    """`fear_draw_boxes_u8` in numpy: a loop over the boxes in index order that assigns each band by slicing, so "the last box wins" is
    program order.  `frames` are (H, W, 3) uint8 arrays, drawn in place and returned; `boxes` (K, 4), `frame_of` (K), `colours` (K, 3)
    or one colour."""
    if not 1 <= int(thickness) <= MAX_THICKNESS:
        raise ValueError(f"thickness must lie in 1..{MAX_THICKNESS}")
    frames = list(frames)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    K = boxes.shape[0]
    frame_of = np.zeros(K, dtype=np.int64) if frame_of is None else np.asarray(frame_of, dtype=np.int64).reshape(-1)
    colours = np.broadcast_to(np.asarray(colours, dtype=np.uint8).reshape(-1, 3), (K, 3))
    for k in range(K):
        f = int(frame_of[k])
        if 0 <= f < len(frames) and frames[f].shape[0] > 0 and frames[f].shape[1] > 0:
            draw_box_host(frames[f], boxes[k], colours[k], int(thickness))
    return frames


def denormalise_host(x: np.ndarray) -> np.ndarray:
    """(3, H, W) normalised fp32 -> (H, W, 3) uint8: `rgb_image_from_tensor` — 255 (x std + mean) in float64, truncated toward zero — cut
    to 0..255 where the reference wraps; a NaN is 0.  A pixel comes back at the uint8 level it was normalised from, or one below."""
    v = np.moveaxis(np.asarray(x, dtype=np.float32), 0, -1).astype(np.float64) * _STD
    v = 255.0 * (v + _MEAN)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, 0.0, 255.0).astype(np.uint8)


def truncate_boxes_host(boxes: np.ndarray) -> np.ndarray:
    """`map(int, ...)` of decoded float64 boxes: toward zero; a NaN is 0, a magnitude above 2^20 is cut to it.  (n, 4) int32."""
    b = np.asarray(boxes, dtype=np.float64)
    b = np.where(np.isnan(b), 0.0, b)
    return np.trunc(np.clip(b, -float(BOX_LIMIT), float(BOX_LIMIT))).astype(np.int32)


def miner_state_host() -> np.ndarray:
    """A zeroed `FearMinerState` record."""
    return np.zeros((), dtype=MINER_STATE_DTYPE)


def miner_decide_host(state: np.ndarray, s: float, mode_max: bool, min_delta: float, step: int) -> Tuple[int, int]:
    """The decide kernel on a `FearMinerState` record, in place: (take best, take worst)."""
    s = np.float64(s)
    for side in (0, 1):
        take = state["has"][side] == 0
        kept = np.float64(state["score"][side])
        if not take and not np.isnan(s) and not np.isnan(kept):
            down = (side == 0) != bool(mode_max)                      # this side wants a smaller score
            take = s <= kept - np.float64(min_delta) if down else s >= kept + np.float64(min_delta)
        state["take"][side] = int(take)
        if take:
            state["has"][side], state["score"][side], state["step"][side] = 1, s, int(step)
    return int(state["take"][0]), int(state["take"][1])


def render_sheet_host(template, search, pred_boxes, gt_box, visible, n: int) -> np.ndarray:
    """The render kernel for one side: the first n pairs, item k in rows 256 k .. 256 k + 255 of a (n 256, 384, 3) uint8 sheet."""
    sheet = np.zeros((n * ITEM_H, SHEET_W, 3), dtype=np.uint8)
    for k in range(n):
        item = sheet[k * ITEM_H:(k + 1) * ITEM_H]
        item[:TEMPLATE_SIZE, :TEMPLATE_SIZE] = denormalise_host(template[k])
        crop = denormalise_host(search[k])
        gt_colour = GT_COLOUR if int(visible[k]) != 0 else GT_INVISIBLE_COLOUR
        draw_boxes_host([crop], [pred_boxes[k], gt_box[k]], [0, 0], [PRED_COLOUR, gt_colour], MINER_THICKNESS)
        item[:, TEMPLATE_SIZE:] = crop
    return sheet


def miner_host(state, sheets, template, search, cls, bbox, gt_box, visible, score, n_images: int = 16, metric_mode: str = "min",
               min_delta: float = 1e-4, step: int = 0):
    """One `fear_miner_update` in numpy.  `state` is a `FearMinerState` record (`miner_state_host()`), `sheets` the (2, n 256, 384, 3)
    uint8 array or None before the first update; `score` one fp32 value or a pair, added in fp32.  Returns the new (state, sheets); the
    arguments are left as they are."""
    if metric_mode not in ("min", "max"):
        raise ValueError("metric_mode is 'min' or 'max'")
    template, search = _host(template), _host(search)
    B = template.shape[0]
    n = min(B, int(n_images))
    state = state.copy()
    sheets = np.zeros((2, n * ITEM_H, SHEET_W, 3), dtype=np.uint8) if sheets is None else sheets.copy()
    parts = np.asarray(score, dtype=np.float32).reshape(-1)
    s = parts[0] if parts.size == 1 else np.float32(parts[0] + parts[1])
    takes = miner_decide_host(state, float(s), metric_mode == "max", min_delta, step)
    if any(takes):
        with np.errstate(invalid="ignore", over="ignore"):                # (a non-finite map cell decodes to a non-finite box)
            pred = truncate_boxes_host(decode_host(_host(cls)[:n], _host(bbox)[:n]))
        state["pred"][:n] = pred
        sheet = render_sheet_host(template, search, pred, _host(gt_box).reshape(-1, 4), _host(visible).reshape(-1), n)
        for side in (0, 1):
            if takes[side]:
                sheets[side] = sheet
    return state, sheets


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---------------------------------------------------------------------------------------------------------------- the device
def _check_thickness(thickness) -> int:
    if not 1 <= int(thickness) <= MAX_THICKNESS:
        raise ValueError(f"thickness must lie in 1..{MAX_THICKNESS}")
    return int(thickness)


def draw_boxes(frames, boxes, frame_of=None, colours=(0, 255, 0), thickness: int = 5) -> None:
    """Draw `boxes` ((K, 4) int32 x, y, w, h) into `frames` in place, on the current stream: box k goes to frame `frame_of[k]` (default
    0; an index outside the frames skips the box) in `colours[k]` ((K, 3), or one colour for all), by the contract of
    `fear_draw_boxes_u8`.  `frames` is one contiguous uint8 (H, W, 3) device tensor or a sequence of them, of any sizes; anything else
    raises ValueError.  `boxes`, `frame_of` and `colours` may be device tensors — then nothing reaches the host and nothing waits — or
    host arrays, which go up with the frame table in one non-blocking transfer from pinned memory."""
    frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
    thickness = _check_thickness(thickness)
    if not frames:
        raise ValueError("no frame to draw into")
    device = frames[0].device if isinstance(frames[0], torch.Tensor) else None
    for f in frames:
        if not isinstance(f, torch.Tensor) or not f.is_cuda or f.device != device or f.dtype != torch.uint8 or f.dim() != 3 or \
                f.shape[2] != 3 or not f.is_contiguous():
            raise ValueError("frames must be contiguous uint8 (H, W, 3) tensors on one GPU")
    stage = Staging()
    table = np.zeros(len(frames), dtype=_FRAME_DTYPE)
    for i, f in enumerate(frames):
        table[i] = (f.data_ptr(), f.shape[0], f.shape[1])
    stage.add("frames", table)

    def arg(name, value, dtype, width):
        """A device tensor of the right kind as it is; anything else through the staging buffer."""
        if isinstance(value, torch.Tensor) and value.is_cuda:
            if value.device != device or value.dtype != getattr(torch, np.dtype(dtype).name) or not value.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous {np.dtype(dtype).name} tensor on the frames' device")
            return value, value.numel() // width
        a = np.ascontiguousarray(_host(value), dtype=dtype).reshape(-1, width)
        stage.add(name, a)
        return None, a.shape[0]

    d_boxes, K = arg("boxes", boxes, np.int32, 4)
    if isinstance(boxes, torch.Tensor) and boxes.numel() != 4 * K:
        raise ValueError("boxes: expected (K, 4) values")
    if not 0 <= K <= MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} boxes")
    d_of, n_of = arg("frame_of", np.zeros(K, dtype=np.int32) if frame_of is None else frame_of, np.int32, 1)
    if isinstance(colours, torch.Tensor) and colours.is_cuda:
        d_col, n_col = arg("colours", colours, np.uint8, 3)
    else:
        c = np.asarray(_host(colours), dtype=np.uint8).reshape(-1, 3)
        d_col, n_col = arg("colours", np.broadcast_to(c, (K, 3)) if c.shape[0] == 1 else c, np.uint8, 3)
    if n_of != K or n_col != K:
        raise ValueError(f"{K} boxes, but {n_of} frame indices and {n_col} colours")
    if K == 0:
        return
    lib = load_train_library()
    with torch.cuda.device(device):
        stage.upload(device)
        ptr = lambda t, name: ctypes.c_void_p(t.data_ptr()) if t is not None else stage.ptr(name)
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        launch(lib, "fear_draw_boxes_u8", stage.ptr("frames"), len(frames), ptr(d_boxes, "boxes"), ptr(d_of, "frame_of"),
               ptr(d_col, "colours"), K, thickness, st)


class BestWorstMiner:
    """The epoch's best and worst training batch, kept as pictures on the device.

        miner = BestWorstMiner(0, max_images=16, metric_mode="min")
        out = net.step(batch.template, batch.search, batch.gt_reg, batch.gt_cls, batch.gt_weight)
        miner.update(out, batch, visible)                  # one operator call on the current stream, nothing waits
        ...
        pictures = miner.sheets()                          # at the end of the epoch: one copy
        miner.reset()

    The score is `loss_cls + loss_reg` of the step (added in fp32 on the device), or any one-element fp32 device tensor given as
    `score` — a view of `TrainMetrics.last_step` with `metric_mode="max"` mines by the step IoU.  The sheets hold the first
    min(B, max_images) pairs of the batch and are allocated by the first update; a later batch of another size raises."""

    def __init__(self, device=0, max_images: int = 16, metric_mode: str = "min", min_delta: float = 1e-4) -> None:
        if not 1 <= int(max_images) <= FEAR_MINER_MAX_IMAGES:
            raise ValueError(f"max_images must lie in 1..{FEAR_MINER_MAX_IMAGES}")
        if metric_mode not in ("min", "max"):
            raise ValueError("metric_mode is 'min' or 'max'")
        self.max_images, self.metric_mode, self.min_delta = int(max_images), metric_mode, float(min_delta)
        self.lib = load_train_library()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._buf: Optional[torch.Tensor] = None            # [FearMinerState | sheets (2, n 256, 384, 3)], one buffer: one copy
        self._B = self._n = 0
        self._steps = 0

    def _f32(self, t, shape, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or \
                (shape is not None and tuple(t.shape) != shape) or (shape is None and t.numel() != 1):
            raise ValueError(f"{what}: expected a contiguous fp32 tensor{'' if shape is None else ' ' + str(shape)} on the miner's device")
        return t

    def _i32(self, t, n: int, what: str) -> torch.Tensor:
        t = torch.as_tensor(t)
        if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
            t = t.to(self.device, torch.int32, non_blocking=True).contiguous()
        if t.numel() != n:
            raise ValueError(f"{what}: expected {n} values, got {t.numel()}")
        return t

    @torch.no_grad()
    def update(self, step_out, batch, visible, step: Optional[int] = None, score=None) -> None:
        """Show the miner one step: `step_out` = what `FEARNetTrainHIP.step` returned ("cls", "bbox", and the two losses unless `score`
        is given), `batch` = the step's `TrainBatch` (its `template`, `search` and `search_bbox`), `visible` a (B) integer device
        tensor.  `step` is the number `sheets` reports for a kept batch; it defaults to a counter of the updates since `reset`."""
        cls, bbox = step_out["cls"], step_out["bbox"]
        B = int(cls.shape[0])
        if self._buf is not None and B != self._B:
            raise ValueError(f"the miner was sized for batches of {self._B} pairs, got {B}")
        if not 1 <= B <= MAX_BOXES:
            raise ValueError(f"between 1 and {MAX_BOXES} pairs")
        cls = self._f32(cls, (B, 1, SCORE_SIZE, SCORE_SIZE), "cls")
        bbox = self._f32(bbox, (B, 4, SCORE_SIZE, SCORE_SIZE), "bbox")
        tmpl = self._f32(batch.template, (B, 3, TEMPLATE_SIZE, TEMPLATE_SIZE), "template")
        srch = self._f32(batch.search, (B, 3, INSTANCE_SIZE, INSTANCE_SIZE), "search")
        gt = self._i32(batch.search_bbox, 4 * B, "ground-truth boxes")
        vis = self._i32(visible, B, "visible")
        if score is None:
            a, b = self._f32(step_out["loss_cls"], None, "loss_cls"), self._f32(step_out["loss_reg"], None, "loss_reg")
        else:
            a, b = self._f32(score, None, "score"), None
        with torch.cuda.device(self.device):
            if self._buf is None:
                self._B, self._n = B, min(B, self.max_images)
                self._buf = torch.zeros(MINER_STATE_DTYPE.itemsize + 2 * self._n * ITEM_H * SHEET_W * 3, dtype=torch.uint8,
                                        device=self.device)
            p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            launch(self.lib, "fear_miner_update", p(tmpl), p(srch), p(cls), p(bbox), p(gt), p(vis), p(a), p(b), B, self.max_images,
                   int(self.metric_mode == "max"), self.min_delta, self._steps if step is None else int(step), p(self._buf),
                   ctypes.c_void_p(self._buf.data_ptr() + MINER_STATE_DTYPE.itemsize), st)
        self._steps += 1

    def _split(self, raw: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        size = MINER_STATE_DTYPE.itemsize
        return raw[:size].view(MINER_STATE_DTYPE)[0], raw[size:].reshape(2, self._n * ITEM_H, SHEET_W, 3)

    def state(self) -> np.ndarray:
        """The `FearMinerState` record, copied to the host (for tests and debugging; a step loop never needs it)."""
        if self._buf is None:
            return miner_state_host()
        return self._buf[:MINER_STATE_DTYPE.itemsize].cpu().numpy().view(MINER_STATE_DTYPE)[0]

    def sheets(self) -> Dict[str, Tuple[float, int, np.ndarray]]:
        """{"best": (score, step, (n 256, 384, 3) uint8 array), "worst": ...} from one device-to-host copy; {} before any update."""
        if self._buf is None:
            return {}
        state, sheets = self._split(self._buf.cpu().numpy())
        return {name: (float(state["score"][side]), int(state["step"][side]), sheets[side])
                for side, name in enumerate(("best", "worst")) if state["has"][side]}

    def reset(self) -> None:
        """Start an epoch: clear the state (and the sheets) on the device."""
        if self._buf is not None:
            self._buf.zero_()
        self._steps = 0
