"""ctypes binding of the C ABI in include/fear_hip.h and the drop-in model object.

`FEARNetHIP` exposes the surface of the reference `FEARNet` that the tracker, the CoreML
wrapper and the thop wrapper use (model_training/model/fear_net.py:58-96,
evaluate/coreml_convert.py:55-57, evaluate/macs_params.py:15-17):
`get_features(crop)`, `track(search, template_features)`, `forward((template, search))`,
`connector(...)` is internal to the fused engine, `.eval()/.cuda()/.to()` are no-ops returning
self.  All tensors are fp32 NCHW torch tensors on the handle's GPU; torch is only the
allocator/stream provider here — every FLOP runs in the hand-written HIP kernels.

There is NO fallback: if the shared library is missing or the GPU is absent the constructor
raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch  # must be imported before the library so that both share one libamdhip64

from .constants import TARGET_CLASSIFICATION_KEY, TARGET_REGRESSION_LABEL_KEY
from .frames import FMT_NV12, FMT_RGB, YUVFrame

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FEAR_LIB", os.path.join(_PKG, "libfear_hip.so"))   # FEAR_LIB: development builds (tools/)
DEFAULT_WEIGHTS = os.path.join(_PKG, "weights", "fear_xs_noembs.fearw")
WEIGHTS_FEAR_M = os.path.join(_PKG, "weights", "fear_m_synth.fearw")   # synthetic deeper trunk (tools/make_fear_m.py), random weights

FEAR_OPT_MAX_BATCH = 1
FEAR_OPT_PROFILE = 2
FEAR_OPT_PROFILE_OP = 3
FEAR_OPT_FUSE = 4
FEAR_OPT_MATH = 5
FEAR_OPT_CHAIN = 6
FEAR_OPT_SMALL_PASS = 7
FEAR_OPT_PLAN_CROPS = 8
FEAR_OPT_DUAL_HEAD = 9
FEAR_OPT_HEAD_STAGGER = 10
FEAR_OPT_TILE_V4 = 11
FEAR_OPT_TINY_SEP = 12
FEAR_OPT_HEAD_CHAIN = 13
FEAR_OPT_BF16_STORE = 14
FEAR_OPT_E1_PAIR = 15
FEAR_OPT_SPLIT_STREAMS = 16
FEAR_OPT_CHAIN32 = 17

_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen libfear_hip.so and declare the prototypes of include/fear_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found. Build it with `python -m feartracker_amd._build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, i32, i64, f32p = c.c_void_p, c.c_int, c.c_int64, c.c_void_p
    lib.fear_create.argtypes = [vp, c.c_size_t, i32, c.POINTER(vp)]
    lib.fear_create.restype = i32
    lib.fear_destroy.argtypes = [vp]
    lib.fear_destroy.restype = i32
    lib.fear_features.argtypes = [vp, f32p, i32, i32, f32p, vp]
    lib.fear_features.restype = i32
    lib.fear_track.argtypes = [vp, f32p, f32p, f32p, i32, f32p, f32p, vp]
    lib.fear_track.restype = i32
    lib.fear_track_packed.argtypes = [vp, f32p, f32p, f32p, i32, f32p, vp]
    lib.fear_track_packed.restype = i32
    lib.fear_decode.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, vp, vp, f32p, vp]
    lib.fear_decode.restype = i32
    f64 = ctypes.c_double
    lib.fear_decode_smooth.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, vp, vp, f64, f64, f64, vp, vp, f32p, vp]
    lib.fear_decode_smooth.restype = i32
    lib.fear_normalize_u8.argtypes = [vp, vp, i32, i32, f32p, vp]
    lib.fear_normalize_u8.restype = i32
    lib.fear_crop_normalize.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, f32p, vp]
    lib.fear_crop_normalize.restype = i32
    lib.fear_crop_normalize_frames.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, f32p, vp]
    lib.fear_crop_normalize_frames.restype = i32
    lib.fear_yuv_to_rgb.argtypes = [vp, vp, vp, vp]
    lib.fear_yuv_to_rgb.restype = i32
    lib.fear_crop_normalize_planar.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, f32p, vp]
    lib.fear_crop_normalize_planar.restype = i32
    lib.fear_tracker_step.argtypes = [vp, f32p, f32p, i32, vp, vp, vp, vp, i32, vp, f64, f64, f64, i32, i32, i32, f64, vp, f32p,
                                      vp]
    lib.fear_tracker_step.restype = i32
    lib.fear_tracker_rows.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.fear_tracker_rows.restype = i32
    lib.fear_set_option.argtypes = [vp, i32, i64]
    lib.fear_set_option.restype = i32
    lib.fear_get_option.argtypes = [vp, i32]
    lib.fear_get_option.restype = i64
    lib.fear_plan_size.argtypes = [vp, i32, i32]
    lib.fear_plan_size.restype = i32
    lib.fear_plan_op.argtypes = [vp, i32, i32, i32, c.c_char_p, c.POINTER(c.c_double), c.POINTER(c.c_double)]
    lib.fear_plan_op.restype = i32
    lib.fear_profile_read.argtypes = [vp, i32, i32, i32, c.POINTER(c.c_double), c.POINTER(i64)]
    lib.fear_profile_read.restype = i32
    lib.fear_profile_reset.argtypes = [vp]
    lib.fear_profile_reset.restype = i32
    lib.fear_workspace_bytes.argtypes = [vp]
    lib.fear_workspace_bytes.restype = c.c_size_t
    lib.fear_strerror.argtypes = [i32]
    lib.fear_strerror.restype = c.c_char_p
    lib.fear_last_hip_error.argtypes = [vp]
    lib.fear_last_hip_error.restype = i32
    lib.fear_version.argtypes = []
    lib.fear_version.restype = c.c_char_p
    _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "fear_create", "fear_destroy", "fear_features", "fear_track", "fear_track_packed", "fear_decode", "fear_decode_smooth", "fear_normalize_u8",
    "fear_crop_normalize", "fear_crop_normalize_frames", "fear_tracker_step", "fear_tracker_rows", "fear_yuv_to_rgb", "fear_crop_normalize_planar",
    "fear_set_option", "fear_get_option", "fear_plan_size", "fear_plan_op", "fear_profile_read",
    "fear_profile_reset", "fear_workspace_bytes", "fear_strerror", "fear_last_hip_error", "fear_version",
)


# fear_frame_planar (include/fear_hip.h): 48 bytes, no padding
PLANAR_FRAME_DTYPE = np.dtype([("plane", "<u8", (3,)), ("pitch", "<i4", (3,)), ("h", "<i4"), ("w", "<i4"), ("format", "<i4")])
assert PLANAR_FRAME_DTYPE.itemsize == 48


def _fill_planar_entry(entry, frame, device: torch.device) -> None:
    """One fear_frame_planar for a device frame: a YUVFrame, or a uint8 (H, W, 3) RGB tensor whose rows may be pitched."""
    if isinstance(frame, YUVFrame):
        if not frame.is_cuda or frame.device != device:
            raise ValueError("YUVFrame planes must be tensors on the engine's device (YUVFrame.to(device) uploads host planes)")
        ptrs = [p.data_ptr() for p in frame.planes]
        entry["plane"] = ptrs + [0] * (3 - len(ptrs))
        entry["pitch"] = frame.pitches()
        entry["h"], entry["w"], entry["format"] = frame.height, frame.width, frame.format
        return
    f = frame
    if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.device != device or \
            f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
        raise ValueError("RGB frames must be uint8 (H,W,3) tensors on the engine's device with contiguous rows")
    entry["plane"] = [f.data_ptr(), 0, 0]
    entry["pitch"] = [f.stride(0), 0, 0]
    entry["h"], entry["w"], entry["format"] = f.shape[0], f.shape[1], FMT_RGB


class FearError(RuntimeError):
    pass


def context_rectangle(frame_h: int, frame_w: int, ctx_xywh: np.ndarray) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1): the part of an H x W frame that context boxes (n, 4) int xywh can sample — their union clipped to the
    frame; when nothing of the frame is visible one pixel keeps the shapes legal (every sample is border colour then anyway)."""
    ctx = np.asarray(ctx_xywh).reshape(-1, 4)
    x0 = y0 = x1 = y1 = 0
    if ctx.shape[0] == 1:                                   # the tracker's case: plain integers
        cx, cy, cw, ch = (int(v) for v in ctx[0])
        x0, y0 = min(max(cx, 0), frame_w), min(max(cy, 0), frame_h)
        x1, y1 = min(max(cx + cw, x0), frame_w), min(max(cy + ch, y0), frame_h)
    elif ctx.shape[0]:
        ctx = ctx.astype(np.int64)
        x0 = int(np.clip(ctx[:, 0].min(), 0, frame_w))
        y0 = int(np.clip(ctx[:, 1].min(), 0, frame_h))
        x1 = int(np.clip((ctx[:, 0] + ctx[:, 2]).max(), x0, frame_w))
        y1 = int(np.clip((ctx[:, 1] + ctx[:, 3]).max(), y0, frame_h))
    if x1 <= x0 or y1 <= y0:
        x0, y0 = min(x0, frame_w - 1), min(y0, frame_h - 1)
        x1, y1 = x0 + 1, y0 + 1
    return x0, y0, x1, y1


def _trunk_geometry(blob: bytes) -> Tuple[int, Tuple[int, ...]]:
    """(neck output channels, strides of the trunk in order) of a `.fearw` blob (include/fearw_format.h): the stem's 2, then
    the depthwise conv's stride of every inverted-residual block in front of the neck.  fear_create has validated the tables."""
    import struct
    _, _, n_convs, n_blocks, _, _ = struct.unpack_from("<8s4IQ", blob, 0)
    convs = [struct.unpack_from("<8I", blob, 64 + 72 * i) for i in range(n_convs)]   # cout, cin_g, groups, k, stride, ...
    boff = 64 + 72 * n_convs
    strides = []
    for i in range(n_blocks):
        kind, _, c0, c1, _ = struct.unpack_from("<2I3i", blob, boff + 32 * i)
        if kind == 0:                       # FEARW_STEM: 3x3 s2 (the plan builder halves the crop)
            strides.append(2)
        elif kind == 1:                     # FEARW_IR: the depthwise conv carries the stride
            strides.append(convs[c1][4])
        elif kind == 2:                     # FEARW_NECK
            return convs[c0][0], tuple(strides)
    raise ValueError("weight file without a neck")


class FEARNetHIP:
    """FEAR network running on one MI355X through libfear_hip.so.

    One handle = one device, one workspace: calls are ordered on the device even when they are issued on different torch
    streams (the engine makes a call on a new stream wait for the previous call's work); the object is not thread-safe."""

    def __init__(self, weights_path: str = DEFAULT_WEIGHTS, device: int = 0, max_batch: int = 64):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        if not torch.cuda.is_available():
            raise RuntimeError("FEARNetHIP needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device(f"cuda:{int(device)}")
        torch.cuda.init()
        with torch.cuda.device(self.device):
            torch.zeros(1, device=self.device)  # make sure the HIP context exists before the engine uploads
            with open(weights_path, "rb") as fh:
                blob = fh.read()
            self._check(self._lib.fear_create(blob, len(blob), int(device), ctypes.byref(self._h)))
        self.weights_path = weights_path
        self.set_max_batch(max_batch)
        self.feat_channels, self.trunk_strides = _trunk_geometry(blob)

    # ------------------------------------------------------------------ plumbing
    def _check(self, status: int) -> None:
        if status != 0:
            hip = self._lib.fear_last_hip_error(self._h) if self._h else 0
            raise FearError(f"libfear_hip: {self._lib.fear_strerror(status).decode()} (status {status}, hip {hip})")

    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _prep(self, t: torch.Tensor, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.device != self.device:
            t = t.to(self.device)
        if t.dtype != torch.float32:
            t = t.float()
        return t.contiguous()

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h:
                self._lib.fear_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ nn.Module look-alikes
    def eval(self):
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    def set_max_batch(self, n: int) -> None:
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_MAX_BATCH, int(n)))

    def set_fuse(self, on: bool) -> None:
        """Fused block kernels (default) vs one kernel per conv layer (bring-up / A-B measurements)."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_FUSE, 1 if on else 0))

    def set_chain(self, on: bool) -> None:
        """Stride-16 trunk stage + neck as one chain kernel (default, fp32 mode) vs one fused kernel per block."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_CHAIN, 1 if on else 0))

    def set_small_pass(self, crops: int) -> None:
        """Passes of at most `crops` crops run the small-batch plan (split-K 16x16 kernels, two-stream head); 0 = never."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_SMALL_PASS, int(crops)))

    def set_dual_head(self, on: bool) -> None:
        """Throughput plan: the head's two branches on two streams (default) vs one."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_DUAL_HEAD, 1 if on else 0))

    def set_head_chain(self, on: bool) -> None:
        """A/B switch for the one-launch BoxTower (FEAR_OPT_HEAD_CHAIN, default on; throughput plan): off = the eight sep16
        launches it replaces.  fp32 mode (set_math(0)): headchain_kernel, maps bit-identical either way.  bf16 mode (set_math(2)):
        headchain_b_kernel, same rounding points as the launches but another summation order — NOT bit-identical (2e-3 relative on
        the maps; tests/test_gpu_parity.py).  set_math(1) keeps the launches.  While the chain is on, set_dual_head has no effect
        on the throughput plan (there are no separate branch launches to put on two streams)."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_HEAD_CHAIN, 1 if on else 0))

    def set_bf16_store(self, on: bool) -> None:
        """A/B switch (FEAR_OPT_BF16_STORE, default on; only with set_math(2)): bf16 storage of the activations between the kernels of
        the trunk's HBM-bound front."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_BF16_STORE, 1 if on else 0))

    def set_e1_pair(self, on: bool) -> None:
        """A/B switch (FEAR_OPT_E1_PAIR, default on; fp32 mode, throughput plan): two consecutive 24-channel e1 blocks as one launch
        (the map between them stays in LDS) vs one tile-kernel launch per block."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_E1_PAIR, 1 if on else 0))

    def set_chain32(self, mode) -> None:
        """A/B switch (FEAR_OPT_CHAIN32; fp32 mode, throughput plan): the four blocks of the 32 x 32 trunk stage as a register-resident
        chain — 2 (default, also True): in one launch with the stride-16 stage + neck (chain32_16_kernel), 1: a launch of its own
        (chain32_kernel), 0 / False: one tile-kernel launch per block."""
        mode = 2 if mode is True else int(mode)
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_CHAIN32, mode))

    def set_split_streams(self, on: bool) -> None:
        """FEAR_OPT_SPLIT_STREAMS (default off): a throughput pass of `track` / `track_maps` runs as two half-batches on two HIP
        streams of the same handle — a serving option (+3 % crops/s at 256 crops), bit-identical maps; bench.py keeps it off for
        `value` so that its per-kernel figures stay full-grid launches and prints its number beside it."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_SPLIT_STREAMS, 1 if on else 0))

    def set_tile_v4(self, on: bool) -> None:
        """Throughput plan: the phase-overlapped tile kernel for the blocks that have one (default on) vs ir_tile_v2 everywhere."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_TILE_V4, 1 if on else 0))


    def set_tiny_sep(self, on: bool) -> None:
        """A/B switch for the tiny plan's row-split SepConv slice kernel (FEAR_OPT_TINY_SEP, default on)."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_TINY_SEP, 1 if on else 0))
    def set_head_stagger(self, microseconds: int) -> None:
        """Two head streams: hold the second branch back by this many microseconds (FEAR_OPT_HEAD_STAGGER)."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_HEAD_STAGGER, int(microseconds)))

    def set_plan_crops(self, crops: int) -> None:
        """Crop count whose launch plan `plan()` / `profile_read()` describe (0 = a full pass of max_batch crops)."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_PLAN_CROPS, int(crops)))

    def set_math(self, mode: int) -> None:
        """0: exact fp32 MFMA (default); 1: fp16 hi+lo split operands on the matrix pipe, fp32 accumulate (fp32-grade);
        2: bf16 operands, fp32 accumulate (reduced precision: the bf16 MFMA pointwise-conv path of BASELINE configs[3])."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_MATH, int(mode)))

    def set_profile(self, on: bool, op: int = -1) -> None:
        """Bracket kernel launches with hipEvents; op >= 0 restricts it to one op of the plan."""
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_PROFILE_OP, int(op)))
        self._check(self._lib.fear_set_option(self._h, FEAR_OPT_PROFILE, 1 if on else 0))

    # ------------------------------------------------------------------ reference API
    def feature_size(self, hw: int) -> int:
        """Side of the feature map of an hw x hw crop: hw halved by the stem, then divided by each block's depthwise stride
        (the plan builder's integer steps)."""
        for s in self.trunk_strides:
            hw //= s
        return hw

    @torch.no_grad()
    def get_features(self, crop: torch.Tensor) -> torch.Tensor:
        """(N,3,H,H) normalised fp32 -> (N,C,H/s,H/s), C the neck's channels and s the trunk's total stride (FEAR-XS: 256, 16);
        fear_net.py:63-66."""
        crop = self._prep(crop, "crop")
        if crop.dim() != 4 or crop.shape[1] != 3 or crop.shape[2] != crop.shape[3]:
            raise ValueError(f"crop must be (N,3,H,H), got {tuple(crop.shape)}")
        n, hw = crop.shape[0], crop.shape[2]
        fhw = self.feature_size(hw)
        out = torch.empty((n, self.feat_channels, fhw, fhw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_features(self._h, crop.data_ptr(), n, hw, out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def track(self, search: torch.Tensor, template_features: torch.Tensor,
              update: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """fear_net.py:90-96; `update` = optional cls-branch template (blocks.py:174-179)."""
        bbox, cls = self.track_maps(search, template_features, update)
        return {TARGET_REGRESSION_LABEL_KEY: bbox, TARGET_CLASSIFICATION_KEY: cls}

    def _track_inputs(self, search, template_features, update):
        """Shared argument checks of `track_maps` / `track_packed`: (search, z, pointer of the optional cls template, n).
        A single template (N = 1) is broadcast over the batch, as the reference's `expand` does."""
        search = self._prep(search, "search")
        z = self._prep(template_features, "template_features")
        n = search.shape[0]
        if tuple(search.shape[1:]) != (3, 256, 256):
            raise ValueError(f"search must be (N,3,256,256), got {tuple(search.shape)}")
        if z.shape[0] == 1 and n > 1:
            z = z.expand(n, -1, -1, -1).contiguous()
        if tuple(z.shape) != (n, self.feat_channels, 8, 8):
            raise ValueError(f"template_features must be ({n},256,8,8), got {tuple(z.shape)}")
        zu = None
        if update is not None:
            zu = self._prep(update, "update")
            if zu.shape[0] == 1 and n > 1:
                zu = zu.expand(n, -1, -1, -1).contiguous()
            if tuple(zu.shape) != tuple(z.shape):
                raise ValueError("update template must have the shape of template_features")
        return search, z, zu, n

    @torch.no_grad()
    def track_maps(self, search, template_features, update=None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        search, z, zu, n = self._track_inputs(search, template_features, update)
        if out is None:
            bbox = torch.empty((n, 4, 16, 16), dtype=torch.float32, device=self.device)
            cls = torch.empty((n, 1, 16, 16), dtype=torch.float32, device=self.device)
        else:
            bbox, cls = out
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_track(self._h, search.data_ptr(), z.data_ptr(), zu.data_ptr() if zu is not None else None, n,
                                             bbox.data_ptr(), cls.data_ptr(), self._stream()))
        return bbox, cls

    @torch.no_grad()
    def track_packed(self, search, template_features, update=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`track` with both maps written into one (N,5,16,16) tensor — bbox in channels 0..3, cls in channel 4 —
        the payload of the multi-GPU all-gather (sharding.py); no pack/cat kernel."""
        search, z, zu, n = self._track_inputs(search, template_features, update)
        if out is None:
            out = torch.empty((n, 5, 16, 16), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (n, 5, 16, 16) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous fp32 (N,5,16,16) tensor on the engine's device")
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_track_packed(self._h, search.data_ptr(), z.data_ptr(), zu.data_ptr() if zu is not None else None,
                                                    n, out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def forward(self, x: Tuple[torch.Tensor, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """fear_net.py:83-88: both branches through the trunk."""
        template, search = x
        return self.track(search, self.get_features(template))

    __call__ = forward

    # ------------------------------------------------------------------ device-side helpers
    def _decode_outputs(self, n: int):
        """The three outputs of the decode kernels as views of ONE device buffer [xywh f64 (n,4) | rc i32 (n,2) | score f32 (n)],
        so that a caller who wants them on the host fetches 44 bytes per crop in one transfer (`decoded_to_host`)."""
        buf = torch.empty(n * 44 + 4, dtype=torch.uint8, device=self.device)
        xywh = buf[: n * 32].view(torch.float64).view(n, 4)
        rc = buf[n * 32: n * 40].view(torch.int32).view(n, 2)
        score = buf[n * 40: n * 44].view(torch.float32)
        return buf, rc, xywh, score

    @staticmethod
    def decoded_to_host(rc: torch.Tensor, xywh: torch.Tensor, score: torch.Tensor):
        """(rc, xywh, score) of `decode` / `decode_smooth` as numpy arrays with ONE device-to-host copy (they are views of one
        buffer; three `.cpu()` calls would be three synchronising transfers)."""
        n = xywh.shape[0]
        # only the exact views `_decode_outputs` makes share one 44-byte-per-crop buffer: check the layout instead of assuming it
        base = xywh.storage_offset() * 8
        st = xywh.untyped_storage()
        ok = (xywh.dtype == torch.float64 and rc.dtype == torch.int32 and score.dtype == torch.float32 and
              tuple(xywh.shape) == (n, 4) and tuple(rc.shape) == (n, 2) and tuple(score.shape) == (n,) and
              xywh.is_contiguous() and rc.is_contiguous() and score.is_contiguous() and
              rc.untyped_storage().data_ptr() == st.data_ptr() and score.untyped_storage().data_ptr() == st.data_ptr() and
              rc.storage_offset() * 4 == base + n * 32 and score.storage_offset() * 4 == base + n * 40 and
              st.nbytes() >= base + n * 44)
        if not ok:              # any other tensors (slices, another backend's outputs): three plain copies
            return rc.cpu().numpy(), xywh.cpu().numpy(), score.cpu().numpy()
        host = torch.empty(0, dtype=torch.uint8, device=xywh.device).set_(st, base, (n * 44,)).cpu().numpy()
        return (host[n * 32: n * 40].view(np.int32).reshape(n, 2), host[: n * 32].view(np.float64).reshape(n, 4),
                host[n * 40: n * 44].view(np.float32))

    @torch.no_grad()
    def decode(self, cls: torch.Tensor, bbox: torch.Tensor, score_size: int = 16, total_stride: int = 16,
               instance_size: int = 256):
        """Device arg-max decode (box_coder.py:75-107 with use_sigmoid=True).
        Returns (rc int32 (N,2), xywh float64 (N,4), score fp32 (N,))."""
        cls = self._prep(cls, "cls")
        bbox = self._prep(bbox, "bbox")
        n = cls.shape[0]
        _, rc, xywh, score = self._decode_outputs(n)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_decode(self._h, cls.data_ptr(), bbox.data_ptr(), n, score_size, total_stride,
                                              instance_size, rc.data_ptr(), xywh.data_ptr(), score.data_ptr(),
                                              self._stream()))
        return rc, xywh, score

    @torch.no_grad()
    def decode_smooth(self, cls: torch.Tensor, bbox: torch.Tensor, prev_size, window, penalty_k: float,
                      window_influence: float, lr: float, score_size: int = 16, total_stride: int = 16,
                      instance_size: int = 256):
        """Device `smooth=True` post-processing (base_tracker.py:149-205), batched: penalty against `prev_size`
        (N,2), window blend, arg-max, decode, size smoothing.  Returns (rc int32 (N,2), xywh float64 (N,4), score (N,))."""
        cls = self._prep(cls, "cls")
        bbox = self._prep(bbox, "bbox")
        n = cls.shape[0]
        prev = torch.as_tensor(prev_size, dtype=torch.float64).reshape(-1, 2).to(self.device).contiguous()
        win = torch.as_tensor(window, dtype=torch.float64).reshape(-1).to(self.device).contiguous()
        if prev.shape[0] != n or win.numel() != score_size * score_size:
            raise ValueError("prev_size must be (N,2) and window (score_size, score_size)")
        _, rc, xywh, score = self._decode_outputs(n)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_decode_smooth(self._h, cls.data_ptr(), bbox.data_ptr(), n, score_size, total_stride,
                                                     instance_size, prev.data_ptr(), win.data_ptr(), float(penalty_k),
                                                     float(window_influence), float(lr), rc.data_ptr(), xywh.data_ptr(),
                                                     score.data_ptr(), self._stream()))
        return rc, xywh, score

    @torch.no_grad()
    def normalize_u8(self, crops_u8_nhwc: torch.Tensor) -> torch.Tensor:
        """uint8 (N,H,H,3) RGB -> normalised fp32 (N,3,H,H) on device (base_tracker.py:97-103)."""
        x = crops_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2]:
            raise ValueError("expected uint8 (N,H,H,3)")
        x = x.to(self.device).contiguous()
        n, hw = x.shape[0], x.shape[1]
        out = torch.empty((n, 3, hw, hw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_normalize_u8(self._h, x.data_ptr(), n, hw, out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def crop_normalize(self, frame_u8, ctx_xywh, pad_rgb_u8, out_hw: int) -> torch.Tensor:
        """Device get_extended_crop + normalise (utils.py:215-253 + base_tracker.py:97-103): frame (H,W,3) uint8 — a numpy
        array / CPU tensor (uploaded here) or a tensor already on the GPU —, ctx_xywh (n,4) int context boxes, pad_rgb_u8
        (n,3) uint8 border colours -> (n,3,out_hw,out_hw) fp32.

        Of a HOST frame only the rectangle the context boxes can sample travels over PCIe (their union clipped to the frame:
        a 225x870 context in a 1080p frame is 0.3 MB of the frame's 6.2 MB; the boxes are shifted to that rectangle's
        origin, everything outside it is border colour for the kernel exactly as the rest of the frame's outside is), and
        the context boxes and border colours go up in ONE small transfer."""
        is_np = isinstance(frame_u8, np.ndarray)          # (kept as numpy until the rectangle is cut: views with negative strides —
        if is_np:                                         #  a BGR -> RGB flip `img[:, :, ::-1]` — are fine for numpy, not for from_numpy)
            if frame_u8.dtype != np.uint8 or frame_u8.ndim != 3 or frame_u8.shape[2] != 3:
                raise ValueError("frame must be uint8 (H,W,3)")
        elif frame_u8.dtype != torch.uint8 or frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
            raise ValueError("frame must be uint8 (H,W,3)")
        ctx_np = np.ascontiguousarray(np.asarray(ctx_xywh, dtype=np.int32).reshape(-1, 4))
        pad_np = np.ascontiguousarray(np.asarray(pad_rgb_u8, dtype=np.uint8).reshape(-1, 3))
        n = ctx_np.shape[0]
        if pad_np.shape[0] != n:
            raise ValueError("one border colour per context box")
        meta_bytes = (n * 16 + n * 3 + 15) // 16 * 16                       # [n x 4 int32 boxes | n x 3 uint8 colours], 16-byte padded
        if is_np or not frame_u8.is_cuda:
            # ONE transfer: [meta | the context rectangle of the frame] assembled in one host buffer (a reused pinned staging
            # buffer was tried — ADVICE r1 — and measured 10x SLOWER per frame on the 256-core host: torch's CPU->pinned copy_
            # costs milliseconds there; a plain pageable .to() of a fresh small array does not)
            fh, fw = int(frame_u8.shape[0]), int(frame_u8.shape[1])
            x0, y0, x1, y1 = context_rectangle(fh, fw, ctx_np)
            if (x1 - x0, y1 - y0) != (fw, fh):
                ctx_np = ctx_np.copy()
                ctx_np[:, 0] -= x0
                ctx_np[:, 1] -= y0
            rh, rw = y1 - y0, x1 - x0
            host = np.empty(meta_bytes + rh * rw * 3, dtype=np.uint8)
            host[: n * 16] = ctx_np.view(np.uint8).reshape(-1)
            host[n * 16: n * 16 + n * 3] = pad_np.reshape(-1)
            roi = frame_u8[y0:y1, x0:x1]
            host[meta_bytes:].reshape(rh, rw, 3)[...] = roi if is_np else roi.numpy()    # (numpy copies any strides, also negative ones)
            dev = torch.from_numpy(host).to(self.device)
            meta_ptr, frame_ptr = dev.data_ptr(), dev.data_ptr() + meta_bytes
        else:
            frame_u8 = frame_u8.to(self.device).contiguous()
            rh, rw = int(frame_u8.shape[0]), int(frame_u8.shape[1])
            meta = np.zeros(meta_bytes, dtype=np.uint8)
            meta[: n * 16] = ctx_np.view(np.uint8).reshape(-1)
            meta[n * 16: n * 16 + n * 3] = pad_np.reshape(-1)
            dev = torch.from_numpy(meta).to(self.device)
            meta_ptr, frame_ptr = dev.data_ptr(), frame_u8.data_ptr()
        out = torch.empty((n, 3, out_hw, out_hw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_crop_normalize(self._h, frame_ptr, rh, rw, meta_ptr, meta_ptr + n * 16, n, int(out_hw),
                                                      out.data_ptr(), self._stream()))
        return out

    def frame_table(self, frames) -> torch.Tensor:
        """The (n_frames) `fear_frame` table of include/fear_hip.h for device uint8 (H,W,3) contiguous frames, uploaded: 16 bytes
        per frame, {data pointer, H, W}.  The frames must stay alive until the launches that read the table have run.  The table
        goes up from pinned memory without waiting for the stream (a pageable copy would wait for all earlier work on it)."""
        host = torch.empty((len(frames), 2), dtype=torch.int64, pin_memory=True)
        tab = host.numpy()
        for i, f in enumerate(frames):
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous() or f.device != self.device:
                raise ValueError("frames must be contiguous uint8 (H,W,3) tensors on the engine's device")
            tab[i, 0] = f.data_ptr()
            tab[i, 1] = int(f.shape[0]) | (int(f.shape[1]) << 32)
        return host.to(self.device, non_blocking=True)

    @torch.no_grad()
    def crop_normalize_frames(self, table: torch.Tensor, frame_idx: torch.Tensor, ctx_xywh: torch.Tensor, pad_rgb_u8: torch.Tensor,
                              out_hw: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fear_crop_normalize_frames: crop i out of frame `frame_idx[i]` of `table` (`frame_table`); every argument a device
        tensor — frame_idx (n,) int32, ctx_xywh (n,4) int32, pad_rgb_u8 (n,3) uint8 -> (n,3,out_hw,out_hw) fp32."""
        n = int(frame_idx.shape[0])
        for t, dt, shape in ((frame_idx, torch.int32, (n,)), (ctx_xywh, torch.int32, (n, 4)), (pad_rgb_u8, torch.uint8, (n, 3))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"expected a contiguous {dt} {shape} tensor on the engine's device")
        if out is None:
            out = torch.empty((n, 3, out_hw, out_hw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_crop_normalize_frames(self._h, table.data_ptr(), int(table.shape[0]), frame_idx.data_ptr(),
                                                             ctx_xywh.data_ptr(), pad_rgb_u8.data_ptr(), n, int(out_hw),
                                                             out.data_ptr(), self._stream()))
        return out

    # ------------------------------------------------------------------ YUV frames (feartracker_amd/frames.py)
    @torch.no_grad()
    def yuv_to_rgb(self, frame: YUVFrame, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fear_yuv_to_rgb: an NV12 / I420 `YUVFrame` -> (H, W, 3) uint8 RGB on the device (host planes are uploaded first)."""
        if not isinstance(frame, YUVFrame):
            raise TypeError("frame must be a YUVFrame")
        if not frame.is_cuda or frame.device != self.device:
            frame = frame.to(self.device)
        if out is None:
            out = torch.empty(frame.shape, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != frame.shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous uint8 (H,W,3) tensor on the engine's device")
        desc = np.zeros(1, dtype=PLANAR_FRAME_DTYPE)
        _fill_planar_entry(desc[0], frame, self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_yuv_to_rgb(self._h, desc.ctypes.data, out.data_ptr(), self._stream()))
        return out

    def frame_table_planar(self, frames) -> torch.Tensor:
        """The (n_frames) `fear_frame_planar` table of include/fear_hip.h, uploaded: 48 bytes per frame, for device frames of any
        format — `YUVFrame`s and uint8 (H,W,3) RGB tensors (rows may be pitched).  The frames must stay alive until the launches
        that read the table have run.  Like `frame_table` it goes up from pinned memory without waiting for the stream."""
        host = torch.empty(len(frames) * PLANAR_FRAME_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        tab = host.numpy().view(PLANAR_FRAME_DTYPE)
        for i, f in enumerate(frames):
            _fill_planar_entry(tab[i], f, self.device)
        return host.to(self.device, non_blocking=True)

    @torch.no_grad()
    def crop_normalize_planar(self, table: torch.Tensor, frame_idx: torch.Tensor, ctx_xywh: torch.Tensor, pad_rgb_u8: torch.Tensor,
                              out_hw: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fear_crop_normalize_planar: `crop_normalize_frames` over a `frame_table_planar` table (RGB, NV12 and I420 frames mixed);
        every argument a device tensor — frame_idx (n,) int32, ctx_xywh (n,4) int32, pad_rgb_u8 (n,3) uint8 -> (n,3,out_hw,out_hw)."""
        n = int(frame_idx.shape[0])
        for t, dt, shape in ((frame_idx, torch.int32, (n,)), (ctx_xywh, torch.int32, (n, 4)), (pad_rgb_u8, torch.uint8, (n, 3))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"expected a contiguous {dt} {shape} tensor on the engine's device")
        n_frames = table.numel() // PLANAR_FRAME_DTYPE.itemsize
        if table.dtype != torch.uint8 or table.numel() != n_frames * PLANAR_FRAME_DTYPE.itemsize or n_frames < 1:
            raise ValueError("table must be the uint8 tensor frame_table_planar returns")
        if out is None:
            out = torch.empty((n, 3, out_hw, out_hw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_crop_normalize_planar(self._h, table.data_ptr(), n_frames, frame_idx.data_ptr(),
                                                             ctx_xywh.data_ptr(), pad_rgb_u8.data_ptr(), n, int(out_hw),
                                                             out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def crop_normalize_yuv(self, frame: YUVFrame, ctx_xywh, pad_rgb_u8, out_hw: int) -> torch.Tensor:
        """`crop_normalize` for a `YUVFrame`: the crops of its RGB conversion, bit for bit, cut from the planes by
        fear_crop_normalize_planar.  Of a HOST frame only the rectangle the context boxes can sample goes up (`context_rectangle`,
        widened to even coordinates so that every pixel keeps its chroma sample), its planes and the small tables in ONE
        transfer; device planes are read in place."""
        if not isinstance(frame, YUVFrame):
            raise TypeError("frame must be a YUVFrame")
        ctx_np = np.ascontiguousarray(np.asarray(ctx_xywh, dtype=np.int32).reshape(-1, 4))
        pad_np = np.ascontiguousarray(np.asarray(pad_rgb_u8, dtype=np.uint8).reshape(-1, 3))
        n = ctx_np.shape[0]
        if pad_np.shape[0] != n:
            raise ValueError("one border colour per context box")
        tab_b = PLANAR_FRAME_DTYPE.itemsize
        meta_bytes = (tab_b + n * 4 + n * 16 + n * 3 + 15) // 16 * 16     # [table | n x frame index 0 | n x 4 int32 | n x 3 uint8]
        planes = []
        if frame.is_cuda:
            if frame.device != self.device:
                frame = frame.to(self.device)
            total = meta_bytes
        else:
            fh, fw = frame.height, frame.width
            x0, y0, x1, y1 = context_rectangle(fh, fw, ctx_np)
            x0, y0, x1, y1 = x0 & ~1, y0 & ~1, x1 + (x1 & 1), y1 + (y1 & 1)     # even: the rectangle keeps the chroma siting
            if (x0, y0) != (0, 0):
                ctx_np = ctx_np.copy()
                ctx_np[:, 0] -= x0
                ctx_np[:, 1] -= y0
            rh, rw = y1 - y0, x1 - x0
            src = frame.planes
            if frame.format == FMT_NV12:
                planes = [src[0][y0:y1, x0:x1], np.asarray(src[1]).reshape(fh // 2, fw)[y0 // 2:y1 // 2, x0:x1]]
            else:
                planes = [src[0][y0:y1, x0:x1], src[1][y0 // 2:y1 // 2, x0 // 2:x1 // 2],
                          src[2][y0 // 2:y1 // 2, x0 // 2:x1 // 2]]
            total = meta_bytes + sum(p.size for p in planes)
        dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        base = dev.data_ptr()
        host = np.zeros(total, dtype=np.uint8)
        entry = host[:tab_b].view(PLANAR_FRAME_DTYPE)[0]
        if frame.is_cuda:
            _fill_planar_entry(entry, frame, self.device)
        else:
            off, ptrs = meta_bytes, []
            for p in planes:
                ptrs.append(base + off)
                host[off: off + p.size].reshape(p.shape)[...] = p
                off += p.size
            entry["plane"] = ptrs + [0] * (3 - len(ptrs))
            entry["pitch"] = [p.shape[1] for p in planes] + [0] * (3 - len(planes))
            entry["h"], entry["w"], entry["format"] = rh, rw, frame.format
        host[tab_b + n * 4: tab_b + n * 20] = ctx_np.view(np.uint8).reshape(-1)      # the frame indices stay 0
        host[tab_b + n * 20: tab_b + n * 23] = pad_np.reshape(-1)
        dev.copy_(torch.from_numpy(host))
        out = torch.empty((n, 3, out_hw, out_hw), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_crop_normalize_planar(self._h, base, 1, base + tab_b, base + tab_b + n * 4,
                                                             base + tab_b + n * 20, n, int(out_hw), out.data_ptr(),
                                                             self._stream()))
        return out

    @torch.no_grad()
    def tracker_step(self, cls: torch.Tensor, bbox: torch.Tensor, frame_hw: torch.Tensor, box_xywh: torch.Tensor,
                     ctx_xywh: torch.Tensor, prev_size: torch.Tensor, score: torch.Tensor, smooth: bool, window: torch.Tensor,
                     penalty_k: float, window_influence: float, lr: float, score_size: int = 16, total_stride: int = 16,
                     instance_size: int = 256, search_context: float = 2.0, xywh: Optional[torch.Tensor] = None) -> None:
        """fear_tracker_step on device tensors, IN PLACE: decode the maps of one `track_maps` call, rescale into each target's
        context `ctx_xywh` (n,4) int32, clamp to its frame `frame_hw` (n,2) int32 -> `box_xywh` (n,4) int32, and overwrite
        `ctx_xywh` / `prev_size` (n,2) float64 with the next frame's context and size; `score` (n,) fp32, optional `xywh` (n,4)
        float64 = the decoded boxes.  `window` (score_size^2) float64 on the device (read when smooth)."""
        cls = self._prep(cls, "cls")
        bbox = self._prep(bbox, "bbox")
        n = int(cls.shape[0])
        for t, dt, shape in ((frame_hw, torch.int32, (n, 2)), (box_xywh, torch.int32, (n, 4)), (ctx_xywh, torch.int32, (n, 4)),
                             (prev_size, torch.float64, (n, 2)), (score, torch.float32, (n,)),
                             (window, torch.float64, (score_size * score_size,))) + \
                (((xywh, torch.float64, (n, 4)),) if xywh is not None else ()):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"expected a contiguous {dt} {shape} tensor on the engine's device")
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_tracker_step(
                self._h, cls.data_ptr(), bbox.data_ptr(), n, frame_hw.data_ptr(), box_xywh.data_ptr(), ctx_xywh.data_ptr(),
                prev_size.data_ptr(), 1 if smooth else 0, window.data_ptr(), float(penalty_k), float(window_influence), float(lr),
                int(score_size), int(total_stride), int(instance_size), float(search_context),
                xywh.data_ptr() if xywh is not None else None, score.data_ptr(), self._stream()))

    @torch.no_grad()
    def tracker_rows(self, ctx_xywh: torch.Tensor, frame_idx: torch.Tensor, n_streams: int, out_hw: int = 256) -> torch.Tensor:
        """fear_tracker_rows on device tensors: the frame rows [y0, y1) per stream that the next `crop_normalize_frames` launch over
        `ctx_xywh` (n,4) int32 and `frame_idx` (n,) int32 samples -> (n_streams, 2) int32 on the device, unclipped.  One launch; the
        call does not wait for the GPU."""
        n = int(frame_idx.shape[0])
        for t, dt, shape in ((frame_idx, torch.int32, (n,)), (ctx_xywh, torch.int32, (n, 4))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"expected a contiguous {dt} {shape} tensor on the engine's device")
        if not 0 <= int(n_streams) <= 65535:
            raise ValueError("n_streams must lie in 0..65535")
        rows = torch.empty((int(n_streams), 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.fear_tracker_rows(self._h, ctx_xywh.data_ptr() if n else None, frame_idx.data_ptr() if n else None, n,
                                                    int(n_streams), int(out_hw), rows.data_ptr() if n_streams else None, self._stream()))
        return rows

    # ------------------------------------------------------------------ measurement
    def plan(self, hw: int = 256, with_head: bool = True):
        """[(name, flops_per_crop, bytes_per_crop)] for every kernel launch of the plan."""
        n = self._lib.fear_plan_size(self._h, hw, int(with_head))
        if n < 0:
            self._check(n)
        ops = []
        for i in range(n):
            name = ctypes.create_string_buffer(64)
            fl, by = ctypes.c_double(), ctypes.c_double()
            self._check(self._lib.fear_plan_op(self._h, hw, int(with_head), i, name, ctypes.byref(fl), ctypes.byref(by)))
            ops.append((name.value.decode(), fl.value, by.value))
        return ops

    def profile_read(self, hw: int = 256, with_head: bool = True):
        """[(total_ms, launches)] per op since the last reset (needs set_profile(True))."""
        n = self._lib.fear_plan_size(self._h, hw, int(with_head))
        res = []
        for i in range(n):
            ms, cnt = ctypes.c_double(), ctypes.c_int64()
            self._check(self._lib.fear_profile_read(self._h, hw, int(with_head), i, ctypes.byref(ms), ctypes.byref(cnt)))
            res.append((ms.value, cnt.value))
        return res

    def profile_reset(self) -> None:
        self._check(self._lib.fear_profile_reset(self._h))

    def workspace_bytes(self) -> int:
        return int(self._lib.fear_workspace_bytes(self._h))
