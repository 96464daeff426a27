"""Training pairs from frames on the GPU: the data stage in front of `FEARNetTrainHIP.step`.

`TrainPairBuilder` turns (frames, template box, search box) into exactly the five tensors the step takes, the way the reference's
`SiameseTrackingDataset._transform` does per pair on the CPU (model_training/dataset/siam_dataset.py:33-61):

* template  `get_extended_crop(frame, box, 128, offset=0.2)`, padded with the frame's mean colour   (tracking_dataset.py:139-156)
* search    `get_extended_crop(frame, box, 512, offset=u)`, u = random() * 3 + 2.5, then `BBoxCropWithOffsets` (scale 0.35,
            shift 48): a jittered square of the 512 crop warped to 256 x 256 by `cv2.warpAffine` (tracking_dataset.py:107-137,
            aug.py:52-143); the box follows through `apply_to_bbox`, `ensure_bbox_boundaries`, `handle_empty_bbox`
* colour    `OneOf([ToGray, ToSepia], p=0.05)` and, at p = 0.5, one of RandomBrightnessContrast / RandomGamma / RGBShift — drawn once
            per pair and applied to both crops (siam_dataset.py:64-67; the subset is DESIGN.md section 11's).  `colour_members`
            widens the group to RandomToneCurve (one more lookup table), Equalize, HueSaturationValue, ColorJitter and Emboss, which
            the device's `fear_colour_u8` applies per crop behind the tables; `colour_u8_host` restates it
* photometric  (`photometric=True`, off by default) `PHOTOMETRIC_AUGMENTATIONS` on each crop on its own, between the colour stage and
            the normalisation: a blur group, a noise group and Downscale(0.5), each at p = 0.2 (aug.py:8-25, tracking_dataset.py:
            158-175; the members built are DESIGN.md section 11's); `photometric_host` restates the device's `fear_photometric_u8`.
            `noise_members` widens the noise group to ImageCompression: a JPEG round trip without its entropy coding
            (`fear_jpeg_u8`), which `jpeg_roundtrip_u8_host` restates and the tests hold to Pillow's libjpeg-turbo byte for byte
            `iso_noise` adds ISONoise to the noise group and `weather_members` the group OneOf([RandomRain, RandomShadow], p=0.05)
            behind it: the members that work in HLS, one operator with a workgroup per crop (`fear_hls_u8`), which `hls_u8_host`
            restates (hls.py).  `glass_blur` adds GlassBlur to the blur group: `fear_glass_u8` in front of the other launches, a
            workgroup per tile, which `glass_u8_host` restates (glass.py)
* targets   `FEARBoxCoder.encode(search_bbox)` and `get_regression_weight_label(search_bbox, 256, 16)`, zeros without presence

Every scalar per-pair step runs here on the host, vectorised over the batch: the draws (`draw`), the context boxes (`extend_bbox`,
`crop_geometry` of geometry.py), the jittered box, `apply_to_bbox` with its truncations, the inverse warp matrix (cv2's order of
operations, float64) and the colour lookup tables.  The device (include/fear_train.h: `fear_frame_border_u8`, `fear_train_pairs`)
does the per-pixel and per-cell work.  `build_host` restates the device arithmetic in numpy; `build` equals it bit for bit.

The reference calls cv2 (`copyMakeBorder`, `resize`, `warpAffine`, `cvtColor`) and albumentations, neither of which is installed
here: the restatements follow OpenCV 4.x's 8u code paths and albumentations' uint8 lookup-table forms, but parity with the real
libraries is unpinned (as for the crop).  What pins the geometry and the targets is the reference's own
Python run on recorded draws (tests/golden/train_pairs_geometry.npz, tools/make_train_pairs_golden.py).
"""
from ..geometry import _INV_STD, _MEAN, extend_bbox  # noqa: F401  (extend_bbox: the scalar form)
from .builder import TrainPairBuilder  # noqa: F401
from .colour import (_colour_normalise, _colour_u8, _normalise_u8, apply_tone, colour_luts, colour_tables, colour_u8_host,  # noqa: F401
                     emboss_taps, emboss_u8, equalize_u8, filter2d_u8, hsv_to_rgb_u8, jitter_brightness_lut, jitter_brightness_u8,
                     jitter_contrast_u8, jitter_hue_lut, jitter_hue_u8, jitter_saturation_u8, rgb_to_hsv_u8, tone_curve_lut)
from .glass import *  # noqa: F401,F403  (GlassBlur's contract: glass.__all__)
from .hls import *  # noqa: F401,F403  (the HLS members' contracts: hls.__all__)
from .jpeg import (JPEG_CHROMA_BASE, JPEG_LUMA_BASE, jpeg_fdct_islow, jpeg_idct_islow, jpeg_quant_tables,  # noqa: F401
                   jpeg_roundtrip_u8_host)
from .photometric import (line_u8, motion_kernel, motion_taps, normal_quantiles, philox4x32_10, photo_tables,  # noqa: F401
                          photometric_host, photometric_u8_host, split_jpeg_records)
from .records import *  # noqa: F401,F403  (the constants, the record dtypes and the draws: records.__all__)
from .staging import Staging  # noqa: F401
from .warp import (_TAB, apply_to_bbox, crop_u8, encode_targets, invert_affine, jittered_crop, remap_affine_u8,  # noqa: F401
                   warp_affine_u8, warp_matrix)
