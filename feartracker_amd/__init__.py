"""feartracker_amd — MI355X-native FEAR per-frame inference path.

Hot path only: `FEARTracker.initialize()/update()` — and `FEARMultiTracker` for many targets per frame — on top of
`FEARNetHIP.get_features()/track()`, whose arithmetic runs in hand-written gfx950 HIP kernels
behind the C ABI of include/fear_hip.h.  Both trackers take packed RGB frames or NV12 / I420 video frames (`YUVFrame`);
`JpegDecoder` decodes baseline JPEG files into such RGB frames on the device, `JpegEncoder` writes such frames out as JPEG files.
"""
from .constants import DEFAULT_TRACKING_CONFIG, TARGET_CLASSIFICATION_KEY, TARGET_REGRESSION_LABEL_KEY
from .box_coder import FEARBoxCoder, TrackerDecodeResult, TrackerEncodeResult
from .frames import YUVFrame
from .tracker import FEARTracker, Tracker, TrackingState
from .multi_tracker import FEARMultiTracker, PendingBoxes, search_rows_host
from .hip_backend import FEARNetHIP, FearError, load_library, DEFAULT_WEIGHTS, LIB_PATH
from .jpeg_frames import (JpegDecoder, MalformedJPEG, UnsupportedJPEG, jpeg_decode_host, jpeg_info, jpeg_pixels_host, jpeg_scaled_shape,
                          jpeg_scaled_transforms)
from .jpeg_huffman import (jpeg_entropy_indexed_host, jpeg_entropy_parallel_host, jpeg_entropy_rows_device_host, jpeg_rows_device_host,
                           jpeg_scan_index_host, jpeg_scan_prepare_host, scan_row_sub, stage_range_host, window_lanes)
from .jpeg_progressive import jpeg_to_baseline_host
from .jpeg_encode import (SUBSAMPLINGS, JpegEncoder, JpegHuffmanDepth, JpegOverflow, PendingJpegs, jpeg_encode_host,
                          jpeg_optimal_table_host, jpeg_symbol_histograms_host, write_mjpeg_avi)
from .jpeg_store import JpegStore, StoreFrames, StoreFull, WindowFrames, plan_decode, plan_decode_rows, plan_decode_windows
from .visuals import BestWorstMiner, draw_boxes, draw_boxes_host, miner_host

__all__ = [
    "DEFAULT_TRACKING_CONFIG", "TARGET_CLASSIFICATION_KEY", "TARGET_REGRESSION_LABEL_KEY",
    "FEARBoxCoder", "TrackerDecodeResult", "TrackerEncodeResult", "FEARTracker", "Tracker", "TrackingState",
    "FEARMultiTracker", "PendingBoxes", "YUVFrame",
    "FEARNetHIP", "FearError", "load_library", "DEFAULT_WEIGHTS", "LIB_PATH",
    "JpegDecoder", "MalformedJPEG", "UnsupportedJPEG", "jpeg_decode_host", "jpeg_info", "jpeg_entropy_parallel_host", "jpeg_scan_prepare_host",
    "jpeg_scan_index_host", "jpeg_entropy_indexed_host", "JpegStore", "StoreFull", "plan_decode", "plan_decode_rows", "plan_decode_windows", "WindowFrames", "window_lanes", "scan_row_sub", "stage_range_host", "jpeg_pixels_host", "jpeg_scaled_shape",
    "jpeg_scaled_transforms",
    "jpeg_to_baseline_host", "jpeg_entropy_rows_device_host", "jpeg_rows_device_host",
    "StoreFrames", "search_rows_host",
    "BestWorstMiner", "draw_boxes", "draw_boxes_host", "miner_host",
    "JpegEncoder", "JpegOverflow", "PendingJpegs", "jpeg_encode_host", "write_mjpeg_avi", "SUBSAMPLINGS",
    "JpegHuffmanDepth", "jpeg_symbol_histograms_host", "jpeg_optimal_table_host",
]
