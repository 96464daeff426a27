"""ctypes declaration of the training ABI (include/fear_train.h): the prototypes of every training operator in libfear_hip.so, the
mirrors of its structs, and the few helpers every module that calls them shares.  `train_head`, `train_net`, `optim` and
`train_data` sequence these operators; none of them declares a prototype of its own."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .hip_backend import load_library

_P = ctypes.c_void_p
_i, _l, _f, _d, _sz = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

TRAIN_SYMBOLS = {
    "fear_train_workspace_bytes": ([_l, _i], _sz),
    "fear_pw_forward": ([_P, _i, _P, _P, _P, _i, _l, _i, _i, _P], _i),
    "fear_pw_backward_data": ([_P, _i, _P, _P, _i, _P, _i, _l, _i, _i, _P], _i),
    "fear_pw_backward_weight": ([_P, _i, _P, _i, _P, _P, _sz, _l, _i, _i, _P], _i),
    "fear_col_sum": ([_P, _i, _P, _P, _sz, _l, _i, _P], _i),
    "fear_dw_forward": ([_P, _i, _P, _P, _P, _i, _i, _i, _i, _i, _i, _i, _P], _i),
    "fear_dw_backward_data": ([_P, _i, _P, _P, _i, _i, _i, _i, _i, _i, _i, _P], _i),
    "fear_dw_backward_weight": ([_P, _i, _P, _i, _P, _P, _sz, _i, _i, _i, _i, _i, _i, _P], _i),
    "fear_stem_im2col": ([_P, _P, _l, _i, _i, _P], _i),
    "fear_bn_train_forward": ([_P, _i, _P, _P, _P, _i, _P, _P, _P, _P, _d, _d, _l, _i, _i, _P, _sz, _P], _i),
    "fear_bn_train_backward": ([_P, _i, _P, _i, _P, _i, _P, _P, _P, _P, _i, _P, _P, _l, _i, _P, _sz, _P], _i),
    "fear_bn_reduce": ([_P, _i, _P, _l, _i, _P, _sz, _P], _i),
    "fear_bn_forward_from_sums": ([_P, _i, _P, _d, _P, _P, _P, _i, _P, _P, _P, _P, _d, _d, _l, _i, _i, _P], _i),
    "fear_bn_backward_reduce": ([_P, _i, _P, _i, _P, _i, _P, _P, _P, _l, _i, _P, _sz, _P], _i),
    "fear_bn_backward_from_sums": ([_P, _i, _P, _i, _P, _i, _P, _P, _P, _P, _d, _P, _P, _i, _P, _P, _P, _sz, _l, _i, _P], _i),
    "fear_pw_forward_stats": ([_P, _i, _P, _P, _i, _P, _P, _i, _l, _i, _i, _P, _P, _sz, _P], _i),
    "fear_dw_forward_stats": ([_P, _i, _P, _P, _i, _P, _P, _i, _i, _i, _i, _i, _i, _i, _P, _P, _sz, _P], _i),
    "fear_train_stats_workspace_bytes": ([_l, _i], _sz),
    "fear_bn_finalize": ([_P, _d, _P, _P, _P, _P, _P, _P, _P, _P, _d, _d, _i, _P], _i),
    "fear_bn_act": ([_P, _i, _P, _P, _i, _P, _i, _P, _i, _l, _i, _P], _i),
    "fear_bn_backward_reduce_x": ([_P, _i, _P, _i, _P, _P, _i, _P, _P, _P, _l, _i, _P, _sz, _P], _i),
    "fear_bn_backward_apply_x": ([_P, _i, _P, _i, _P, _P, _i, _P, _P, _P, _P, _d, _P, _P, _i, _P, _P, _P, _sz, _l, _i, _P], _i),
    "fear_bn_train_forward_ab": ([_P, _i, _P, _P, _i, _P, _i, _P, _i, _P, _P, _P, _P, _P, _P, _d, _d, _l, _i, _P, _sz, _P], _i),
    "fear_bn_train_backward_x": ([_P, _i, _P, _i, _P, _P, _i, _P, _P, _P, _P, _i, _P, _P, _l, _i, _P, _sz, _P], _i),
    "fear_pw_backward_weight_act": ([_P, _i, _P, _i, _P, _P, _i, _P, _P, _sz, _l, _i, _i, _P], _i),
    "fear_dw_backward_weight_act": ([_P, _i, _P, _i, _P, _P, _i, _P, _P, _sz, _i, _i, _i, _i, _i, _i, _P], _i),
    "fear_xcorr_forward": ([_P, _i, _P, _P, _i, _i, _i, _i, _i, _P], _i),
    "fear_xcorr_backward": ([_P, _i, _P, _i, _P, _P, _i, _P, _i, _P, _i, _i, _i, _i, _P], _i),
    "fear_exp_head_forward": ([_P, _P, _P, _P, _l, _P], _i),
    "fear_exp_head_backward": ([_P, _P, _P, _P, _P, _P, _P, _P, _sz, _l, _P], _i),
    "fear_head_loss": ([_P, _P, _P, _P, _P, _f, _f, _P, _P, _P, _P, _sz, _l, _P], _i),
    "fear_nchw_to_nhwc": ([_P, _P, _l, _i, _i, _i, _i, _P], _i),
    "fear_nhwc_to_nchw": ([_P, _P, _l, _i, _i, _i, _i, _P], _i),
    "fear_scale_column": ([_P, _i, _i, _f, _P, _i, _i, _l, _P], _i),
    "fear_add": ([_P, _P, _P, _l, _P], _i),
    "fear_adam_step": ([_P, _P, _P, _P, _l, _d, _d, _d, _d, _d, _i, _P], _i),
    # the optimiser family and gradient-norm clipping (optim.py; FearOptim below)
    "fear_grad_sumsq_partials": ([_l], _l),
    "fear_grad_sumsq": ([_P, _l, _P, _P], _i),
    "fear_grad_norm_finalize": ([_P, _l, _d, _P, _P], _i),
    "fear_optim_step": ([_P, _P, _P, _P, _P, _l, _i, _P, _P], _i),
    # block-fused trunk operators (structs below mirror include/fear_train.h)
    "fear_irb_workspace_bytes": ([_P, _i, _i, _i], _sz),
    "fear_irb_scratch_floats": ([_P, _i, _i, _i], _sz),
    "fear_irb_virtual_ok": ([_P], _i),
    "fear_irb_plan_info": ([_P, _i, _i, _i, _P], _i),            # host only: FearIrbPlanInfo below
    "fear_pwbn_plan_info": ([_l, _i, _i, _i, _i, _P], _i),       # host only: FearPwbnPlanInfo below
    "fear_layer_plan_info": ([_l, _i, _i, _sz, _P, _P], _i),      # host only: FearLayerPlanInfo below
    "fear_irb_train_forward": ([_P, _P, _P, _P, _i, _i, _i, _d, _d, _P, _sz, _P], _i),
    "fear_irb_train_backward": ([_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _P, _sz, _P, _P], _i),
    "fear_bn_running_update": ([_P, _d, _P, _P, _d, _d, _i, _P], _i),
    "fear_bn_running_update_multi": ([_P, _i, _d, _d, _P], _i),
    "fear_pwbn_workspace_bytes": ([_l, _i, _i], _sz),
    "fear_pwbn_train_forward": ([_P, _i, _P, _P, _P, _P, _P, _P, _P, _i, _P, _l, _i, _i, _d, _d, _P, _sz, _P], _i),
    "fear_pwbn_train_backward": ([_P, _P, _P, _i, _P, _i, _P, _P, _P, _P, _P, _P, _l, _i, _i, _P, _sz, _P, _P], _i),
    "fear_stem_workspace_bytes": ([_l, _i, _i], _sz),
    "fear_stem_train_forward": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _l, _i, _i, _d, _d, _P, _sz, _P], _i),
    "fear_stem_train_backward": ([_P, _P, _P, _P, _P, _P, _P, _P, _l, _i, _i, _P, _sz, _P, _P], _i),
    # the head's SepConv + BatchNorm + ReLU layer, one call per direction
    "fear_sepbn_workspace_bytes": ([_P, _i, _i, _i], _sz),
    "fear_sepbn_train_forward": ([_P, _P, _i, _P, _P, _P, _P, _i, _i, _i, _i, _d, _d, _P, _sz, _P], _i),
    "fear_sepbn_train_backward": ([_P, _P, _P, _i, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _P, _sz, _P, _P], _i),
    # SyncBatchNorm hook of the block-fused operators: (stream, FearSync*)
    "fear_train_sync_bind": ([_P, _P], _i),
    # training pairs from frames (train_data.TrainPairBuilder)
    "fear_frame_border_u8": ([_P, _i, _P, _P], _i),
    "fear_train_pairs": ([_P, _i, _P, _P, _P, _i, _P, _P, _P, _P, _P, _P], _i),
    # the photometric stage behind the pairs (FearPhotoOp below)
    "fear_train_pairs_u8": ([_P, _i, _P, _P, _P, _i, _P, _P, _P, _P, _P, _P], _i),
    # the same two for frames of which a rectangle is stored (FearFrameWindow below; JpegStore.decode_windows)
    "fear_train_pairs_windows": ([_P, _i, _P, _P, _P, _i, _P, _P, _P, _P, _P, _P], _i),
    "fear_train_pairs_windows_u8": ([_P, _i, _P, _P, _P, _i, _P, _P, _P, _P, _P, _P], _i),
    "fear_photometric_u8": ([_P, _i, _i, _i, _P, _P, _P, _P, _P], _i),
    "fear_photometric_stage_u8": ([_P, _i, _i, _i, _P, _P, _P, _P, _P], _i),
    # ImageCompression: the JPEG round trip between the stage above and fear_photometric_u8
    "fear_jpeg_u8": ([_P, _i, _i, _i, _P, _P, _sz, _P, _P], _i),
    "fear_jpeg_workspace_bytes": ([_i, _i, _i], _sz),
    # JPEG frames (jpeg_frames.JpegDecoder; FearJpegInfo and FearJpegImage below): the host's parser and Huffman stage, the device's rest
    "fear_jpeg_parse": ([_P, _sz, _P], _i),
    "fear_jpeg_packed_bound": ([_P], _sz),
    "fear_jpeg_entropy_decode": ([_P, _sz, _P, _P, _sz, _P, _P], _i),
    # progressive files, host only (jpeg_progressive.py): the scans to packed coefficients, or to a baseline file with a restart per MCU row
    "fear_jpeg_progressive_parse": ([_P, _sz, _P], _i),
    "fear_jpeg_progressive_decode": ([_P, _sz, _P, _P, _sz, _P, _P], _i),
    "fear_jpeg_baseline_bound": ([_P], _sz),
    "fear_jpeg_progressive_to_baseline": ([_P, _sz, _P, _sz, _P], _i),
    "fear_jpeg_decode_u8": ([_P, _i, _P, _P, _sz, _P], _i),
    "fear_jpeg_decode_workspace_bytes": ([_P, _i], _sz),
    # the Huffman stage on the device (FearJpegScan below): the host's scan preparation, the decode, the dense block_start table
    "fear_jpeg_scan_prepare": ([_P, _sz, _P, _P, _sz, _P, _sz, _P], _i),
    "fear_jpeg_huffman": ([_P, _i, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_dense_block_start": ([_P, ctypes.c_uint32, _P], _i),
    # scans resident on the device (jpeg_store.JpegStore; FearJpegSubseq, FearJpegIndex and FearJpegIndexed below)
    "fear_jpeg_sub_start": ([_P, ctypes.c_uint32, ctypes.c_uint32, _i, _P, _sz, _P], _i),
    "fear_jpeg_index_build": ([_P, _i, _P, _P, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_huffman_indexed": ([_P, _i, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_huffman_indexed_rows": ([_P, _i, _P, _P, _P, _i, _P], _i),
    # the band's lanes that touch a range of MCU columns, window-dense (JpegStore.decode_windows)
    "fear_jpeg_huffman_indexed_windows": ([_P, _i, _P, _P, _P, _i, _P], _i),
    # the band of rows taken from device memory (JpegStore.decode_rows with a device tensor)
    "fear_jpeg_huffman_indexed_rows_dev": ([_P, _i, _P, _P, _P, _P, _i, _P], _i),
    # the same four for scans whose bytes lie in pinned host memory (JpegStore(residence="host")): the staged fetch, the device-side
    # address of a pinned allocation, and the byte range a run of lanes covers (host only)
    "fear_jpeg_huffman_indexed_host": ([_P, _i, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_huffman_indexed_rows_host": ([_P, _i, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_huffman_indexed_rows_dev_host": ([_P, _i, _P, _P, _P, _P, _i, _P], _i),
    "fear_jpeg_huffman_indexed_windows_host": ([_P, _i, _P, _P, _P, _i, _P], _i),
    "fear_host_mapped_pointer": ([_P, _P], _i),
    "fear_jpeg_stage_range": ([_P, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _i, _P, _P], _i),
    "fear_jpeg_decode_u8_rows_dev": ([_P, _i, _P, _P, _P, _sz, _P], _i),
    "fear_jpeg_decode_scaled_u8": ([_P, _i, _P, _i, _P, _sz, _P], _i),
    "fear_jpeg_decode_mixed_u8": ([_P, _i, _P, _P, _sz, _P], _i),      # a scale per record, in FearJpegImage.reserved[0]
    # the colour stage's members that are no lookup table (FearColourOp below)
    "fear_colour_u8": ([_P, _i, _i, _i, _P, _P, _P, _P], _i),
    # ISONoise, RandomRain and RandomShadow of the photometric stage (FearHlsOp below)
    "fear_hls_u8": ([_P, _i, _i, _i, _P, _P, _P, _P, _P, _P], _i),
    # GlassBlur of the photometric stage's blur group, in front of fear_photometric_u8 (FearPhotoOp's records)
    "fear_glass_u8": ([_P, _i, _i, _i, _P, _P, _P], _i),
    # step metrics (metrics.TrainMetrics)
    "fear_train_metrics": ([_P, _P, _P, _P, _P, _i, _i, _P, _P, _P, _P], _i),
    # boxes drawn into frames, and the best / worst batch miner (visuals.py; FearMinerState below)
    "fear_draw_boxes_u8": ([_P, _i, _P, _P, _P, _i, _i, _P], _i),
    "fear_miner_update": ([_P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _d, _i, _P, _P, _P], _i),
    # JPEG files written on the device (jpeg_encode.JpegEncoder; FearJpegEncImage below): the host's header, bound and plan, the encode
    "fear_jpeg_encode_header": ([_i, _i, _i, _i, _P, _sz, _P], _i),
    "fear_jpeg_encode_bound": ([_i, _i, _i], _sz),
    "fear_jpeg_encode_header_mode": ([_i, _i, _i, _i, _i, _P, _sz, _P], _i),
    "fear_jpeg_encode_bound_mode": ([_i, _i, _i, _i], _sz),
    "fear_jpeg_encode_plan": ([_P, _i], _i),
    "fear_jpeg_encode_workspace_bytes": ([_P, _i], _sz),
    "fear_jpeg_encode_u8": ([_P, _i, _P, _sz, _P, _P, _P], _i),
    # per-file Huffman tables: the header without its DHT segments and the bound of an optimised record; the table stage on its own
    "fear_jpeg_encode_header_flags": ([_i, _i, _i, _i, _i, ctypes.c_uint32, _P, _sz, _P], _i),
    "fear_jpeg_encode_bound_flags": ([_i, _i, _i, _i, ctypes.c_uint32], _sz),
    "fear_jpeg_huff_optimal": ([_P, _i, _P, _P, _P, _P, _P, _P], _i),
}


class FearIrbBlock(ctypes.Structure):
    """include/fear_train.h: one inverted-residual block's shape and parameters (device pointers, kernel layouts)."""
    _fields_ = [("cin", _i), ("cexp", _i), ("cout", _i), ("k", _i), ("stride", _i), ("expand", _i), ("residual", _i), ("flags", _i),
                ("w_pw", _P), ("w_dw", _P), ("w_pwl", _P), ("gamma", _P * 3), ("beta", _P * 3), ("running_mean", _P * 3), ("running_var", _P * 3)]


class FearIrbSaved(ctypes.Structure):
    _fields_ = [("e", _P), ("d", _P), ("p", _P), ("vec", _P * 3)]


class FearIrbGrads(ctypes.Structure):
    _fields_ = [("w_pw", _P), ("w_dw", _P), ("w_pwl", _P), ("gamma", _P * 3), ("beta", _P * 3)]


_i32 = ctypes.c_int32


class FearGemmPlan(ctypes.Structure):
    """include/fear_train.h: one row-tiled pointwise GEMM of a plan query."""
    _fields_ = [(n, _i32) for n in ("present", "lds", "rows", "k", "n", "x2", "row_tiles", "grid_x", "grid_y", "nt")]


class FearWgradPlan(ctypes.Structure):
    """include/fear_train.h: one pointwise weight gradient of a plan query."""
    _fields_ = [(n, _i32) for n in ("present", "rows", "k", "n", "swapped", "lds_tile", "rows_per_slice", "slices")]


class FearDwPlan(ctypes.Structure):
    """include/fear_train.h: one depthwise launch of a plan query."""
    _fields_ = [(n, _i32) for n in ("tiles_x", "tiles_y", "tile_side", "nslab", "wgs_per_slab", "items_per_wg", "small_map")]


class FearIrbPlanInfo(ctypes.Structure):
    """include/fear_train.h: what fear_irb_train_forward / _backward would launch (fear_irb_plan_info; host only)."""
    _fields_ = [("rows_in", _i32), ("rows_out", _i32), ("lin", _i32), ("virtual_e", _i32), ("expand", FearGemmPlan), ("project", FearGemmPlan),
                ("g2", FearGemmPlan), ("dx", FearGemmPlan), ("col_rows_in", _i32), ("col_rows_out", _i32), ("wgrad_rows_per_slice", _i32),
                ("w3", FearWgradPlan), ("w1", FearWgradPlan), ("dw_fwd", FearDwPlan), ("dw_bwd", FearDwPlan), ("gram_rows_per_wg", _i32)]


class FearPwbnPlanInfo(ctypes.Structure):
    """include/fear_train.h: what fear_pwbn_train_* / fear_stem_train_* would launch (fear_pwbn_plan_info; host only)."""
    _fields_ = [("rows", _i32), ("forward", FearGemmPlan), ("dx", FearGemmPlan), ("col_rows", _i32), ("w", FearWgradPlan)]


class FearLayerGemmPlan(ctypes.Structure):
    """include/fear_train.h: fear_pw_forward's or fear_pw_backward_data's launch (fear_layer_plan_info)."""
    _fields_ = [(n, _i32) for n in ("lds", "row_tile", "ntw", "col_blocks", "grid_x", "grid_y", "nt")]


class FearLayerWgradPlan(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("swapped", "lds_tile", "small_k", "n_tiles", "k_tiles", "rows_per_slice", "slices")]


class FearLayerDwShape(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("B", "H", "W", "C", "k", "stride", "ld")]


class FearLayerDwPlan(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("strips", "workgroups", "dgrad_workgroups", "wgrad_rows", "wgrad_workgroups", "wgrad_row_run",
                                    "fwd_plain", "dgrad_plain")]


class FearLayerPlanInfo(ctypes.Structure):
    """include/fear_train.h: what the layer operators would launch for (M, K, N) and one depthwise shape (fear_layer_plan_info; host only)."""
    _fields_ = [("forward", FearLayerGemmPlan), ("dx", FearLayerGemmPlan), ("stats_blocks", _i32), ("stats_nt", _i32),
                ("w", FearLayerWgradPlan), ("w_act", FearLayerWgradPlan), ("col_rows", _i32), ("col_blocks", _i32), ("dw", FearLayerDwPlan)]


class FearBnRunning(ctypes.Structure):
    _fields_ = [("vec", _P), ("running_mean", _P), ("running_var", _P), ("C", _i), ("count", _d)]


class FearSepLayer(ctypes.Structure):
    """include/fear_train.h: one SepConv + BatchNorm + ReLU layer of the head (device pointers, kernel layouts)."""
    _fields_ = [("cin", _i), ("cout", _i), ("w_dw", _P), ("b_dw", _P), ("w_pw", _P), ("b_pw", _P), ("gamma", _P), ("beta", _P),
                ("running_mean", _P), ("running_var", _P)]


class FearSepGrads(ctypes.Structure):
    _fields_ = [("w_dw", _P), ("w_pw", _P), ("gamma", _P), ("beta", _P)]


FEAR_OPT_ADAM, FEAR_OPT_ADAMW, FEAR_OPT_SGD = 0, 1, 2
FEAR_GRAD_SUMSQ_CHUNK = 4096      # floats per partial sum of fear_grad_sumsq


class FearOptim(ctypes.Structure):
    """include/fear_train.h: the rule and hyper-parameters of one fear_optim_step."""
    _fields_ = [("kind", _i), ("nesterov", _i), ("lr", _d), ("beta1", _d), ("beta2", _d), ("eps", _d), ("weight_decay", _d),
                ("momentum", _d), ("dampening", _d)]


class FearFrame(ctypes.Structure):
    """include/fear_hip.h `fear_frame`: one uint8 RGB (h, w, 3) device frame (train_data.records.FRAME_DTYPE is its numpy form)."""
    _fields_ = [("data", ctypes.c_uint64), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


assert ctypes.sizeof(FearFrame) == 16 and ctypes.sizeof(ctypes.c_void_p) == 8


class FearFrameWindow(ctypes.Structure):
    """include/fear_train.h `fear_frame_window`: the rectangle (y0, x0, wh, ww) of a uint8 RGB frame of shape (h, w), stored compactly
    (train_data.records.WINDOW_DTYPE is its numpy form)."""
    _fields_ = [("data", ctypes.c_uint64), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32),
                ("wh", ctypes.c_int32), ("ww", ctypes.c_int32)]


assert ctypes.sizeof(FearFrameWindow) == 32


class FearPairGeom(ctypes.Structure):
    """include/fear_train.h: one pair's geometry record (train_data.records.GEOM_DTYPE is its numpy form)."""
    _fields_ = [("t_frame", ctypes.c_int32), ("s_frame", ctypes.c_int32), ("t_ctx", ctypes.c_int32 * 4), ("s_ctx", ctypes.c_int32 * 4),
                ("box", ctypes.c_int32 * 4), ("presence", ctypes.c_int32), ("tone", ctypes.c_int32), ("inv", _d * 4)]


assert ctypes.sizeof(FearPairGeom) == 96 and FearPairGeom.inv.offset == 64


class FearPhotoOp(ctypes.Structure):
    """include/fear_train.h: one crop's photometric record (train_data.records.PHOTO_DTYPE is its numpy form)."""
    _fields_ = [("blur", ctypes.c_int32), ("ksize", ctypes.c_int32), ("noise", ctypes.c_int32), ("scale", _f),
                ("key", ctypes.c_uint32 * 2), ("downscale", ctypes.c_int32), ("tap_row", ctypes.c_int32)]


assert ctypes.sizeof(FearPhotoOp) == 32


class FearColourOp(ctypes.Structure):
    """include/fear_train.h: one crop's colour record (train_data.records.COLOUR_DTYPE is its numpy form)."""
    _fields_ = [("kind", ctypes.c_int32), ("order", ctypes.c_uint8 * 4), ("contrast", _d), ("alpha", _f), ("beta", _f),
                ("taps", _f * 9), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(FearColourOp) == 64 and FearColourOp.contrast.offset == 8 and FearColourOp.taps.offset == 24


class FearHlsOp(ctypes.Structure):
    """include/fear_train.h: one crop's record of fear_hls_u8 (train_data.records.HLS_DTYPE is its numpy form)."""
    _fields_ = [("kind", ctypes.c_int32), ("seg_offset", ctypes.c_int32), ("seg_count", ctypes.c_int32), ("hue_scale", _f),
                ("intensity", _d), ("key", ctypes.c_uint32 * 2)]


assert ctypes.sizeof(FearHlsOp) == 32 and FearHlsOp.intensity.offset == 16 and FearHlsOp.key.offset == 24


FEAR_MINER_MAX_IMAGES = 64


class FearMinerState(ctypes.Structure):
    """include/fear_train.h: the best / worst miner's device state (visuals.MINER_STATE_DTYPE is its numpy form)."""
    _fields_ = [("has", ctypes.c_int32 * 2), ("step", ctypes.c_int32 * 2), ("score", _d * 2), ("take", ctypes.c_int32 * 2),
                ("reserved", ctypes.c_int32 * 2), ("pred", (ctypes.c_int32 * 4) * FEAR_MINER_MAX_IMAGES)]


assert ctypes.sizeof(FearMinerState) == 1072 and FearMinerState.score.offset == 16 and FearMinerState.pred.offset == 48


class FearJpegInfo(ctypes.Structure):
    """include/fear_train.h: what fear_jpeg_parse reads from a file's headers."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32), ("h", ctypes.c_int32 * 3), ("v", ctypes.c_int32 * 3),
                ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3), ("total_blocks", ctypes.c_uint32),
                ("reserved", ctypes.c_int32), ("qt", (ctypes.c_uint16 * 64) * 3)]


class FearJpegImage(ctypes.Structure):
    """include/fear_train.h: one image of a fear_jpeg_decode_u8 call (device pointers as integers)."""
    _fields_ = [("coef", ctypes.c_uint64), ("block_start", ctypes.c_uint64), ("out", ctypes.c_uint64), ("plane_offset", ctypes.c_uint64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32), ("h", ctypes.c_int32),
                ("v", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3), ("qt", (ctypes.c_uint16 * 64) * 3)]


class FearJpegHuff(ctypes.Structure):
    """include/fear_train.h: one Huffman table, fear_jpeg::Huffman's layout."""
    _fields_ = [("look", ctypes.c_uint16 * 512), ("first", ctypes.c_int32 * 17), ("index", ctypes.c_int32 * 17), ("values", ctypes.c_uint8 * 256),
                ("counts", ctypes.c_uint8 * 17), ("reserved", ctypes.c_uint8 * 7)]


class FearJpegScan(ctypes.Structure):
    """include/fear_train.h: one image's scan of a fear_jpeg_huffman call (device pointers as integers)."""
    _fields_ = [("bytes", ctypes.c_uint64), ("seg_start", ctypes.c_uint64), ("coef_offset", ctypes.c_uint64), ("n_bytes", ctypes.c_uint32),
                ("n_seg", ctypes.c_uint32), ("max_seg_bytes", ctypes.c_uint32), ("total_blocks", ctypes.c_uint32), ("components", ctypes.c_int32),
                ("h", ctypes.c_int32), ("v", ctypes.c_int32), ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("dc", FearJpegHuff * 3), ("ac", FearJpegHuff * 3)]


class FearJpegSubseq(ctypes.Structure):
    """include/fear_train.h: the true entry of one subsequence of a resident scan (jpeg_huffman.SUBSEQ_DTYPE is its numpy form)."""
    _fields_ = [("p", ctypes.c_uint32), ("begun", ctypes.c_uint32), ("sz", ctypes.c_uint16), ("dc", ctypes.c_uint16 * 3)]


class FearJpegIndex(ctypes.Structure):
    """include/fear_train.h: one image of a fear_jpeg_index_build call (device pointers as integers; seg_start_host is a host address)."""
    _fields_ = [("index", ctypes.c_uint64), ("sub_start", ctypes.c_uint64), ("seg_start_host", ctypes.c_uint64), ("n_sub", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class FearJpegIndexed(ctypes.Structure):
    """include/fear_train.h: one image of a fear_jpeg_huffman_indexed, fear_jpeg_huffman_indexed_rows or fear_jpeg_huffman_indexed_rows_dev
    call (device pointers as integers)."""
    _fields_ = [("scan", ctypes.c_uint64), ("index", ctypes.c_uint64), ("sub_start", ctypes.c_uint64), ("coef_offset", ctypes.c_uint64),
                ("n_sub", ctypes.c_uint32), ("sub0", ctypes.c_uint32), ("sub_count", ctypes.c_uint32), ("mcu_row0", ctypes.c_uint32),
                ("mcu_rows", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("row_sub", ctypes.c_uint64)]


assert ctypes.sizeof(FearJpegSubseq) == 16 and ctypes.sizeof(FearJpegIndex) == 32 and ctypes.sizeof(FearJpegIndexed) == 64
assert FearJpegIndexed.row_sub.offset == 56
assert ctypes.sizeof(FearJpegInfo) == 464 and FearJpegInfo.qt.offset == 80
assert ctypes.sizeof(FearJpegHuff) == 1440 and ctypes.sizeof(FearJpegScan) == 8704 and FearJpegScan.dc.offset == 64
assert ctypes.sizeof(FearJpegImage) == 448 and FearJpegImage.qt.offset == 64
assert FearJpegImage.reserved.offset == 52                               # reserved[0]: the record's scale for fear_jpeg_decode_mixed_u8


class FearJpegEncImage(ctypes.Structure):
    """include/fear_train.h: one image of a fear_jpeg_encode_u8 call (device pointers as integers; fear_jpeg_encode_plan fills
    stream_offset, work_offset, stream_cap, start and plan_sampling and keeps sampling)."""
    _fields_ = [("src", ctypes.c_uint64), ("out", ctypes.c_uint64), ("header", ctypes.c_uint64), ("stream_offset", ctypes.c_uint64),
                ("work_offset", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("quality", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("out_cap", ctypes.c_uint32), ("header_bytes", ctypes.c_uint32),
                ("stream_cap", ctypes.c_uint32), ("start", ctypes.c_uint32 * 4), ("sampling", ctypes.c_uint32), ("plan_sampling", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


assert ctypes.sizeof(FearJpegEncImage) == 96 and FearJpegEncImage.width.offset == 40 and FearJpegEncImage.stream_cap.offset == 64
assert FearJpegEncImage.sampling.offset == 84 and FearJpegEncImage.flags.offset == 92
FEAR_JPEG_ENC_420, FEAR_JPEG_ENC_422, FEAR_JPEG_ENC_444, FEAR_JPEG_ENC_GRAY = 0, 1, 2, 3     # a record's sampling
FEAR_JPEG_ENC_GRAY_RGB = 0x100        # or-ed into FEAR_JPEG_ENC_GRAY: the source is (height, width, 3) RGB
FEAR_JPEG_ENC_OVERFLOW = 1
FEAR_JPEG_ENC_HUFF_DEPTH = 2          # a status: the image's Huffman tree is deeper than 32 before limiting
FEAR_JPEG_ENC_OPTIMIZE = 1            # a record's flags: per-file Huffman tables
FEAR_JPEG_ENC_HEADER_MAX = 640
FEAR_JPEG_ENC_GROUP_BLOCKS = 256      # blocks per workgroup of fear_jpeg_encode_u8's sizes and write passes
FEAR_JPEG_ENC_CHUNK_BYTES = 4096      # unstuffed stream bytes per workgroup of its count and assemble passes
FEAR_JPEG_ENC_MCUS = 4                # MCUs per workgroup of its transform pass


def FEAR_JPEG_ENC_TABLE_BYTES(n: int) -> int:
    return (n * 96 + 15) & ~15


FEAR_TRAIN_ERR_WORKSPACE, FEAR_TRAIN_ERR_FORMAT, FEAR_TRAIN_ERR_UNSUPPORTED = -7, -9, -10
FEAR_JPEG_GROUP_BLOCKS, FEAR_JPEG_GROUP_PIXELS = 32, 256
FEAR_JPEG_DEVICE_SCAN_MAX = 16 << 20

_ALLREDUCE_FN =ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p)
FEAR_SYNC_BUF_BYTES = 16384


class FearSync(ctypes.Structure):
    """include/fear_train.h: the all-reduce hook a stream is bound to (fear_train_sync_bind)."""
    _fields_ = [("all_reduce", _ALLREDUCE_FN), ("user", _P), ("buf", _P), ("buf_bytes", _sz), ("world", _i)]


_bound = None


def load_train_library() -> ctypes.CDLL:
    """The training operators live in the same libfear_hip.so; declare their prototypes (include/fear_train.h)."""
    global _bound
    if _bound is None:
        lib = load_library()
        for name, (args, res) in TRAIN_SYMBOLS.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _bound = lib
    return _bound


class TrainError(RuntimeError):
    pass


def launch(lib: ctypes.CDLL, name: str, *args) -> None:
    """Call the operator `name` of the library; a non-zero status is a TrainError."""
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise TrainError(f"{name} failed with status {rc}")


def _p(t: Optional[torch.Tensor], offset: int = 0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset)
