"""SequenceValidator on the HIP engine (both launch plans) against independent FEARTrackers on the same network plus get_iou:
every per-frame IoU and every returned value equal.  Host arrays, device tensors and NV12 frames in one run."""
import numpy as np
import pytest
import torch

from feartracker_amd import DEFAULT_TRACKING_CONFIG, YUVFrame
from feartracker_amd.validate import SequenceValidator
from test_validate_host import assert_equal_runs, ragged_sequences, restated_validation_step
from yuvgen import rgb_to_yuv420

pytestmark = pytest.mark.gpu
NAMES = ("got10k", "lasot", "got10k", "coco", "lasot")


def _nv12(frames):
    out = []
    for k, f in enumerate(frames):
        y, u, v = rgb_to_yuv420(f, seed=k)
        out.append(YUVFrame.nv12(y, np.stack([u, v], -1).reshape(u.shape[0], -1)))
    return out


@pytest.fixture(scope="module")
def sequences():
    seqs = ragged_sequences((40, 25, 12, 7, 2), (0, 30, 60, 100, 150), NAMES)
    assert seqs[0][0].shape[1:3] != seqs[1][0].shape[1:3]
    seqs[3] = (_nv12(seqs[3][0]), seqs[3][1], seqs[3][2])                   # one sequence of NV12 frames (host planes)
    return seqs


def test_five_ragged_sequences_equal_independent_trackers(hip_net, sequences):
    seq_ious, reduced = restated_validation_step(hip_net, sequences, 30, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    assert [len(v) for v in seq_ious] == [29, 24, 11, 6, 1]
    given = list(sequences)
    given[2] = ([torch.from_numpy(f).cuda() for f in sequences[2][0]], sequences[2][1], sequences[2][2])     # device tensors
    val = SequenceValidator(hip_net, max_samples=30, **DEFAULT_TRACKING_CONFIG)
    got = val.run(given)
    print({k: v for k, v in got.items() if k != "sequences"})
    assert_equal_runs(got, seq_ious, reduced, NAMES)
    assert got["valid/metrics/box_iou"] > 0.3


def _state_after_one_step(frames):
    """random_init_state(0) after ONE training-mode step on windows of the clip, with BatchNorm momentum 1: the step's batch
    statistics become the running statistics the export folds.  (The untouched initial state has identity running statistics;
    in eval mode its 60 unnormalised layers overflow to an infinite box on real crops, on which the reference tracker's
    `round` — and so the FEARTracker this test compares with — raises.)"""
    from feartracker_amd.train_data import encode_targets
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    B = 8
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    norm = lambda u8: torch.from_numpy((((u8 / 255.0) - mean) / std).transpose(0, 3, 1, 2).astype(np.float32)).cuda()
    picks = frames[:: max(1, len(frames) // B)][:B]
    srch = norm(np.stack([f[:, 30 * k: 30 * k + 256] for k, f in enumerate(picks)]))
    tmpl = norm(np.stack([f[60:188, 20 * k + 100: 20 * k + 228] for k, f in enumerate(picks)]))
    boxes = np.tile(np.array([[100, 60, 50, 120]]), (B, 1)) + np.arange(B)[:, None]
    reg, cls, wgt = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in encode_targets(boxes, np.ones(B, np.int32)))
    net = FEARNetTrainHIP(random_init_state(0), device=0, momentum=1.0)
    out = net.step(tmpl, srch, reg, cls, wgt)
    assert np.isfinite(float(out["loss_cls"])) and np.isfinite(float(out["loss_reg"]))
    return net.state_dict()


def test_round_trip_from_a_training_state(sequences):
    state = _state_after_one_step(sequences[0][0])
    val = SequenceValidator.from_training_state(state, max_samples=6, **DEFAULT_TRACKING_CONFIG)
    seqs = [sequences[1], sequences[4], sequences[0]]
    names = [q[2] for q in seqs]
    seq_ious, reduced = restated_validation_step(val.net, seqs, 6, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    got = val.run(seqs)
    print({k: v for k, v in got.items() if k != "sequences"})
    assert_equal_runs(got, seq_ious, reduced, names)
    assert all(np.isfinite(q["ious"]).all() for q in got["sequences"])
