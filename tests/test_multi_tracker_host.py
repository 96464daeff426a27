"""FEARMultiTracker without a GPU: the host path (CPU oracle network) against independent FEARTrackers, and the C entry points'
declarations and null-handle errors."""
import os

import numpy as np
import pytest

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARTracker, hip_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fixture's init box, one box straddling the right frame edge, one in the top-left corner
EXTRA_BOXES = [np.array([300, 100, 40, 50]), np.array([5, 4, 30, 26])]


def _single_run(net, frames, box, start=0):
    trk = FEARTracker(net, cuda_id="cpu", **DEFAULT_TRACKING_CONFIG)
    trk.initialize(frames[start], box.copy())
    return [np.array(trk.tracking_state.bbox)] + [np.array(trk.update(f)["bbox"]) for f in frames[start + 1:]]


@pytest.fixture(scope="module")
def synth(golden_dir):
    return np.load(f"{golden_dir}/clip_synth.npz")


@pytest.fixture(scope="module")
def singles(oracle_net, synth):
    frames = synth["frames"]
    return [_single_run(oracle_net, frames, b) for b in [synth["init_bbox"]] + EXTRA_BOXES]


def test_three_targets_equal_independent_trackers(oracle_net, synth, singles):
    frames = synth["frames"]
    mt = FEARMultiTracker(oracle_net, cuda_id="cpu", **DEFAULT_TRACKING_CONFIG)
    assert not mt.device_path
    ids = mt.add(frames[0], np.stack([synth["init_bbox"]] + EXTRA_BOXES))
    assert ids == [0, 1, 2] and len(mt) == 3
    got = {i: [] for i in ids}
    for f in frames[1:]:
        pending = mt.submit(f)
        res = pending.result()
        assert set(res) == set(ids) and set(pending.scores()) == set(ids)
        for i in ids:
            got[i].append(res[i])
    for i, single in zip(ids, singles):
        np.testing.assert_array_equal(np.stack(got[i]), np.stack(single[1:]))
    np.testing.assert_array_equal(np.stack([synth["init_bbox"]] + got[0]), synth["tracked"])
    assert (singles[1][0][0] + singles[1][0][2]) == frames.shape[2]          # the second box was clamped at the right edge


def test_target_added_mid_clip_and_removal(oracle_net, synth, singles):
    frames = synth["frames"]
    late = np.array([120, 70, 36, 44])
    ref_late = _single_run(oracle_net, frames, late, start=8)
    mt = FEARMultiTracker(oracle_net, cuda_id="cpu", **DEFAULT_TRACKING_CONFIG)
    a, b, c = mt.add(frames[0], np.stack([synth["init_bbox"]] + EXTRA_BOXES))
    got = {a: [], c: []}
    d = None
    for t in range(1, len(frames)):
        res = mt.update(frames[t])
        for i in got:
            got[i].append(res[i])
        if t == 8:                                   # initialised on frame 8, tracked from frame 9 on
            (d,) = mt.add(frames[8], late)
            got[d] = []
        if t == 12:
            mt.remove([b])
            assert mt.ids == [a, c, d]
        if t > 12:
            assert b not in res
    np.testing.assert_array_equal(np.stack(got[a]), np.stack(singles[0][1:]))
    np.testing.assert_array_equal(np.stack(got[c]), np.stack(singles[2][1:]))
    np.testing.assert_array_equal(np.stack(got[d]), np.stack(ref_late[1:]))


def test_new_entry_points_are_declared_and_check_the_handle():
    header = open(os.path.join(ROOT, "include", "fear_hip.h")).read()
    for sym in ("fear_crop_normalize_frames", "fear_tracker_step"):
        assert f"int {sym}(" in header
        assert sym in hip_backend.EXPORTED_SYMBOLS
    lib = hip_backend.load_library()
    assert lib.fear_crop_normalize_frames(None, None, 1, None, None, None, 1, 256, None, None) == -1
    assert lib.fear_tracker_step(None, None, None, 1, None, None, None, None, 0, None, 0.0, 0.0, 0.0, 16, 16, 256, 2.0, None,
                                 None, None) == -1
