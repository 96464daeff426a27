"""SequenceValidator on the tracker's host path (CPU oracle network) against a plain restatement of the reference's
`validation_step` (train/fear_lightning_model.py:93-125): one FEARTracker per sequence, get_iou per frame."""
import numpy as np
import pytest

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARTracker
from feartracker_amd.metrics import get_iou
from feartracker_amd.validate import SequenceValidator


def ragged_sequences(lengths, starts, names):
    """Sequences cut from the demo clip; every second one is a window of the frames (another frame size), its annotations moved."""
    from clipgen import demo_clip
    frames, gt = demo_clip(max(s + n for s, n in zip(starts, lengths)))
    out = []
    for k, (n, s, name) in enumerate(zip(lengths, starts, names)):
        f, a = frames[s:s + n], gt[s:s + n].copy()
        if k % 2 == 1:
            f = np.ascontiguousarray(f[:, 10:250, 60:460])
            a[:, 0] -= 60
            a[:, 1] -= 10
        out.append((f, a.astype(np.float64) + 0.25, name))          # (annotations are read through int(), like the reference's)
    return out


def restated_validation_step(net, sequences, max_samples, iou_threshold=0.01, cuda_id="cpu", **cfg):
    seq_ious, log = [], {}
    for frames, annotations, dataset_name in sequences:
        tracker = FEARTracker(net, cuda_id=cuda_id, **cfg)
        tracker.initialize(frames[0], list(map(int, annotations[0])))
        num_samples = min(max_samples, len(annotations))
        ious, failure_map = [], []
        for i in range(1, num_samples):
            bbox = tracker.update(frames[i])["bbox"]
            iou = get_iou(np.array(bbox), np.array(list(map(int, annotations[i]))))
            ious.append(iou)
            failure_map.append(int(iou < iou_threshold))
        log.setdefault("valid/metrics/box_iou", []).append(np.mean(ious))
        log.setdefault(f"valid/metrics/{dataset_name}_box_iou", []).append(np.mean(ious))
        log.setdefault(f"valid/metrics/{dataset_name}_failure_rate", []).append(np.mean(failure_map))
        seq_ious.append(ious)
    return seq_ious, {k: np.mean(v) for k, v in log.items()}          # (on_epoch: the mean of the logged values)


def assert_equal_runs(got, seq_ious, reduced, names):
    assert set(got) == set(reduced) | {"sequences"}
    for key, value in reduced.items():
        assert got[key] == value, key
    assert [q["dataset"] for q in got["sequences"]] == list(names)
    for q, ious in zip(got["sequences"], seq_ious):
        assert q["ious"].dtype == np.float64
        np.testing.assert_array_equal(q["ious"], np.array(ious))
        assert q["box_iou"] == np.mean(ious)
        assert q["failure_rate"] == np.mean(np.array(ious) < 0.01)


def test_three_ragged_sequences_equal_the_restated_validation_step(oracle_net):
    names = ("got10k", "lasot", "got10k")
    seqs = ragged_sequences((6, 4, 2), (0, 20, 40), names)
    assert seqs[0][0].shape[1:3] != seqs[1][0].shape[1:3]
    seq_ious, reduced = restated_validation_step(oracle_net, seqs, 5, **DEFAULT_TRACKING_CONFIG)
    assert [len(v) for v in seq_ious] == [4, 3, 1]
    val = SequenceValidator(oracle_net, max_samples=5, **DEFAULT_TRACKING_CONFIG)
    # the second sequence's frames come from a generator: frames only have to be iterable
    given = [seqs[0], ((f for f in seqs[1][0]), seqs[1][1], seqs[1][2]), seqs[2]]
    got = val.run(given)
    assert_equal_runs(got, seq_ious, reduced, names)
    assert got["valid/metrics/box_iou"] > 0.3               # the tracker does follow the object on these frames
    # a second run on the same validator starts from scratch
    assert val.run(seqs)["valid/metrics/box_iou"] == reduced["valid/metrics/box_iou"]


def test_a_failure_threshold_and_explicit_host_path(oracle_net):
    names = ("a", "b")
    seqs = ragged_sequences((3, 3), (0, 100), names)
    far = seqs[1][1].copy()
    far[1:] = (2.0, 2.0, 5.0, 5.0)                                       # after the first frame: annotations far from the object
    seqs[1] = (seqs[1][0], far, "b")
    cfg = dict(DEFAULT_TRACKING_CONFIG, device_crop=False)
    seq_ious, reduced = restated_validation_step(oracle_net, seqs, 200, **cfg)
    got = SequenceValidator(oracle_net, **cfg).run(seqs)
    assert_equal_runs(got, seq_ious, reduced, names)
    assert got["valid/metrics/b_failure_rate"] == 1.0 and got["valid/metrics/a_failure_rate"] == 0.0


def test_a_one_frame_sequence_is_an_error(oracle_net):
    seqs = ragged_sequences((3, 1), (0, 20), ("a", "b"))
    val = SequenceValidator(oracle_net, max_samples=5, **DEFAULT_TRACKING_CONFIG)
    with pytest.raises(ValueError):
        val.run(seqs)
    with pytest.raises(ValueError):
        val.run([])
    with pytest.raises(ValueError):
        SequenceValidator(oracle_net, max_samples=1)
    with pytest.raises(ValueError):                       # more annotations than frames
        val.run([(seqs[0][0][:2], seqs[0][1], "a")])
