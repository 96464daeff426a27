"""fear_draw_boxes_u8 and fear_miner_update on the GPU against their numpy statements `draw_boxes_host` and `miner_host` (themselves pinned
to the contract by tests/test_visuals_host.py), through `draw_boxes`, `BestWorstMiner` and `FEARMultiTracker.draw`.  Everything is bytes
and integers and is compared with ==; the miner's scores are float64 copies of fp32 sums and compare with == as well."""
import numpy as np
import pytest
import torch

import visualsgen as vg
from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker
from feartracker_amd import visuals as V

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, 0xA5


def _guarded(frame: np.ndarray):
    """The frame inside a larger device buffer: (buffer, the (H, W, 3) view the operator draws into)."""
    n = frame.size
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(frame.shape)
    view.copy_(torch.from_numpy(frame))
    return buf, view


def _inside(buf, shape):
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "guard bytes around a frame written"
    return host[GUARD:GUARD + n].reshape(shape)


def _draw(frames, boxes, frame_of, cols, t, device_args):
    bufs = [_guarded(f) for f in frames]
    if device_args:
        boxes, frame_of, cols = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes, frame_of, cols))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        V.draw_boxes([v for _, v in bufs], boxes, frame_of, cols, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return [_inside(b, f.shape) for (b, _), f in zip(bufs, frames)]


CASES = list(vg.draw_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_draw_boxes_equals_the_host_statement(case):
    name, shapes, boxes, frame_of, cols, t = case
    frames = [vg.frame(h, w, i) for i, (h, w) in enumerate(shapes)]
    want = V.draw_boxes_host([f.copy() for f in frames], boxes, frame_of, cols, t)
    got = _draw(frames, boxes, frame_of, cols, t, device_args=True)
    again = _draw(frames, boxes, frame_of, cols, t, device_args=False)     # fresh copies, the arguments through the staging buffer
    for g, a, w in zip(got, again, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{name}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
        np.testing.assert_array_equal(a, g)
    assert any((w != f).any() for w, f in zip(want, frames))               # (the case draws something)


def test_draw_boxes_defaults_and_argument_checks():
    base = vg.frame(37, 70, 3)
    boxes = np.array([(5, 6, 20, 12), (30, 10, 25, 20)], dtype=np.int32)
    (got,) = _draw([base], boxes, None, (0, 255, 0), 5, device_args=False)              # frame_of: zeros; one colour for all
    np.testing.assert_array_equal(got, V.draw_boxes_host([base.copy()], boxes, None, (0, 255, 0), 5)[0])
    frame = torch.from_numpy(base).cuda()
    before = frame.clone()
    V.draw_boxes(frame, np.zeros((0, 4), np.int32))                                      # no box: no launch
    for bad in (frame[:, :, :2], frame[:, ::2], frame.float(), frame.cpu(), frame[0]):
        with pytest.raises(ValueError):
            V.draw_boxes(bad, boxes)
    with pytest.raises(ValueError):
        V.draw_boxes(frame, boxes, thickness=0)
    with pytest.raises(ValueError):
        V.draw_boxes(frame, boxes, thickness=33)
    with pytest.raises(ValueError):
        V.draw_boxes(frame, boxes, frame_of=[0])
    with pytest.raises(ValueError):
        V.draw_boxes(frame, torch.from_numpy(boxes).cuda().long())
    torch.cuda.synchronize()
    assert torch.equal(frame, before)


# ---------------------------------------------------------------------------------------------------------------- the miner
class _Batch:
    def __init__(self, m, dev):
        self.template, self.search = torch.from_numpy(m["template"]).to(dev), torch.from_numpy(m["search"]).to(dev)
        self.search_bbox = torch.from_numpy(m["gt_box"]).to(dev)


# (score_a, score_b) per step, mode min, min_delta 0.125 (binary fractions: every sum and bound is exact): both | neither (a tie within
# min_delta) | best only | worst only | neither (a NaN) | best only, at the boundary best - min_delta exactly (0.25 - 0.125)
SCORES = ((0.5, 0.5), (0.5, 0.5625), (0.125, 0.125), (1.0, 1.0), (float("nan"), 0.0), (0.0625, 0.0625))
EXPECTED = ((1, 1), (0, 0), (1, 0), (0, 1), (0, 0), (1, 0))


@pytest.mark.parametrize("B,n_images", ((3, 2), (2, 16)))
def test_miner_update_equals_the_host_statement_over_six_steps(B, n_images):
    dev = torch.device("cuda:0")
    miner = V.BestWorstMiner(0, max_images=n_images, metric_mode="min", min_delta=0.125)
    steps = [vg.miner_step(B, seed) for seed in range(len(SCORES))]
    assert any(np.isnan(m["bbox"]).any() for m in steps) and all((m["visible"] == 0).any() for m in steps)
    on_dev = [(dict(cls=torch.from_numpy(m["cls"]).to(dev), bbox=torch.from_numpy(m["bbox"]).to(dev),
                    loss_cls=torch.tensor(s[0], dtype=torch.float32, device=dev), loss_reg=torch.tensor(s[1], dtype=torch.float32, device=dev)),
               _Batch(m, dev), torch.from_numpy(m["visible"]).to(dev)) for m, s in zip(steps, SCORES)]
    miner.update(*on_dev[0], step=100)                      # (buffers allocated)
    miner.reset()
    torch.cuda.synchronize()
    snapshots = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i, args in enumerate(on_dev):
            miner.update(*args, step=10 + i)
            snapshots.append(miner._buf.clone())            # (a device-to-device copy on the stream: no wait)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    state, sheets = V.miner_state_host(), None
    n = min(B, n_images)
    for i, (m, s) in enumerate(zip(steps, SCORES)):
        before = sheets
        state, sheets = V.miner_host(state, sheets, m["template"], m["search"], m["cls"], m["bbox"], m["gt_box"], m["visible"], s,
                                     n_images, "min", 0.125, step=10 + i)
        assert tuple(state["take"]) == EXPECTED[i], f"step {i}: the script's decisions"
        got_state, got_sheets = miner._split(snapshots[i].cpu().numpy())
        for field in ("has", "step", "take", "pred"):
            np.testing.assert_array_equal(got_state[field], state[field], err_msg=f"step {i}: {field}")
        np.testing.assert_array_equal(got_state["score"], state["score"])
        assert got_sheets.shape == (2, n * 256, 384, 3)
        bad = np.argwhere(got_sheets != sheets)
        assert bad.size == 0, f"step {i}: {len(bad)} sheet bytes differ, first at {bad[0].tolist()}"
        if EXPECTED[i] == (0, 0):
            np.testing.assert_array_equal(got_sheets, before)
    out = miner.sheets()
    assert set(out) == {"best", "worst"} and out["best"][:2] == (0.125, 15) and out["worst"][:2] == (2.0, 13)
    np.testing.assert_array_equal(out["best"][2], sheets[0])
    np.testing.assert_array_equal(out["worst"][2], sheets[1])
    miner.reset()
    assert miner.sheets() == {} and not miner._buf.any().item()
    with pytest.raises(ValueError):
        other = vg.miner_step(B + 1, 0)
        miner.update(dict(cls=torch.from_numpy(other["cls"]).to(dev), bbox=torch.from_numpy(other["bbox"]).to(dev)), _Batch(other, dev),
                     torch.from_numpy(other["visible"]).to(dev), score=torch.zeros(1, device=dev))


def test_miner_in_mode_max_with_a_score_tensor():
    """One score tensor (no second pointer), mode max: a larger score is the better one."""
    dev = torch.device("cuda:0")
    miner = V.BestWorstMiner(0, max_images=1, metric_mode="max", min_delta=1e-4)
    state, sheets = V.miner_state_host(), None
    for i, s in enumerate((0.5, 0.75, 0.25, 0.5)):
        m = vg.miner_step(2, i)
        miner.update(dict(cls=torch.from_numpy(m["cls"]).to(dev), bbox=torch.from_numpy(m["bbox"]).to(dev)), _Batch(m, dev),
                     torch.from_numpy(m["visible"]).to(dev), score=torch.tensor([s], dtype=torch.float32, device=dev))
        state, sheets = V.miner_host(state, sheets, m["template"], m["search"], m["cls"], m["bbox"], m["gt_box"], m["visible"], (s,), 1,
                                     "max", 1e-4, step=i)
    assert state["step"].tolist() == [1, 2]
    out = miner.sheets()
    assert out["best"][:2] == (0.75, 1) and out["worst"][:2] == (0.25, 2)
    np.testing.assert_array_equal(out["best"][2], sheets[0])
    np.testing.assert_array_equal(out["worst"][2], sheets[1])
    np.testing.assert_array_equal(miner.state()["pred"], state["pred"])


def test_miner_through_a_real_training_step():
    """`FEARNetTrainHIP.step` on a `TrainPairBuilder.build` batch of 4 pairs cut from the demo clip: `sheets()` against `miner_host` fed
    the same tensors copied to the host."""
    from clipgen import demo_clip
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    clip, _ = demo_clip(12)
    frames = [clip[0], clip[11]]
    pairs = np.array([[0, 163, 53, 45, 174, 1, 170, 50, 45, 174, 1], [1, 60, 60, 40, 30, 0, 70, 66, 44, 30, 1],
                      [0, 300, 30, 70, 50, 1, 310, 40, 60, 50, 0], [1, 20, 150, 90, 100, 0, 24, 140, 90, 96, 1]], dtype=np.float64)
    builder = TrainPairBuilder(device=0)
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(3))
    batch = builder.build(frames, pairs, params)
    visible = torch.from_numpy(pairs[:, 10].astype(np.int32)).cuda()
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    out = net.step(batch.template, batch.search, batch.gt_reg, batch.gt_cls, batch.gt_weight)
    miner = V.BestWorstMiner(0, max_images=16)
    assert miner.sheets() == {}
    miner.update(out, batch, visible)
    got = miner.sheets()
    host = lambda t: t.cpu().numpy()
    score = (host(out["loss_cls"]), host(out["loss_reg"]))
    state, sheets = V.miner_host(V.miner_state_host(), None, host(batch.template), host(batch.search), host(out["cls"]), host(out["bbox"]),
                                 host(batch.search_bbox), host(visible), score, 16, "min", 1e-4, step=0)
    print("real step: score", got["best"][0], "pred", state["pred"][:4].tolist(), "gt", host(batch.search_bbox).tolist())
    assert np.isfinite(got["best"][0]) and got["best"][:2] == got["worst"][:2] == (float(state["score"][0]), 0)
    assert got["best"][2].shape == (4 * 256, 384, 3)
    np.testing.assert_array_equal(got["best"][2], sheets[0])
    np.testing.assert_array_equal(got["worst"][2], sheets[1])
    crop = got["best"][2][:256, 128:]
    assert (crop == (250, 0, 0)).all(axis=2).any() and (got["best"][2][2 * 256:3 * 256, 128:] == (0, 0, 250)).all(axis=2).any()
    assert len(np.unique(got["best"][2][:128, :128])) > 16                 # a picture, not a constant


# ---------------------------------------------------------------------------------------------------------------- the tracker
def test_multi_tracker_draw_before_the_result_is_read(hip_net):
    """3 targets on 2 streams of synthetic device frames: after one submit, `draw` is issued before `result()` is read, with no
    synchronisation in between; the frames then equal `draw_boxes_host` with the boxes the result reports."""
    from clipgen import demo_clip
    clip, _ = demo_clip(3)
    rng = np.random.RandomState(4)
    small = [rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8) for _ in range(2)]
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    a, b = mt.add(torch.from_numpy(clip[0]).cuda(), np.array([(163, 53, 45, 174), (300, 30, 70, 50)]), stream=0)
    (c,) = mt.add(torch.from_numpy(small[0]).cuda(), np.array([(150, 80, 60, 50)]), stream=1)
    frames = [torch.from_numpy(clip[1]).cuda(), torch.from_numpy(small[1]).cuda()]
    cols = np.array([(0, 255, 0), (255, 0, 0), (0, 0, 255)], dtype=np.uint8)
    d_cols = torch.from_numpy(cols).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pending = mt.submit(frames)
        mt.draw(frames, d_cols, thickness=5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    boxes = pending.result()
    want = V.draw_boxes_host([clip[1].copy(), small[1].copy()], [boxes[a], boxes[b], boxes[c]], [0, 0, 1], cols, 5)
    for got, w in zip(frames, want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)
    assert (want[0] != clip[1]).any() and (want[1] != small[1]).any()
    # one colour for all, on fresh copies (the colour goes up from pinned memory: still no wait)
    fresh = [torch.from_numpy(clip[1]).cuda(), torch.from_numpy(small[1]).cuda()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mt.draw(fresh, thickness=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = V.draw_boxes_host([clip[1].copy(), small[1].copy()], [boxes[a], boxes[b], boxes[c]], [0, 0, 1], (0, 255, 0), 2)
    for got, w in zip(fresh, want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)
    with pytest.raises(TypeError):
        mt.draw([clip[1], small[1]])                                        # host frames
    with pytest.raises(ValueError):
        mt.draw(fresh[:1])                                                  # a stream without its frame


def test_multi_tracker_draw_needs_the_device_path(hip_net):
    from clipgen import demo_clip
    clip, _ = demo_clip(2)
    mt = FEARMultiTracker(hip_net, cuda_id=0, **dict(DEFAULT_TRACKING_CONFIG, device_crop=False))
    assert not mt.device_path
    with pytest.raises(RuntimeError):
        mt.draw(torch.from_numpy(clip[1]).cuda())
