"""FEARMultiTracker on the HIP engine: fear_tracker_step bit for bit against the host tracker code, fear_crop_normalize_frames
against fear_crop_normalize, and every target of the multi-target tracker against an independent FEARTracker."""
import numpy as np
import pytest
import torch

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, FEARTracker
from feartracker_amd.geometry import clamp_bbox, crop_geometry

pytestmark = pytest.mark.gpu

# the demo clip's init box (tests/clipgen.py) plus eleven others on its 480 x 256 frames: edge-straddling, outside, tiny, whole-frame
DEMO_BOXES = [(163, 53, 45, 174), (440, 100, 60, 80), (-10, -5, 40, 40), (200, 120, 3, 3), (100, 200, 5, 4), (0, 0, 480, 256),
              (300, 30, 70, 50), (20, 150, 90, 100), (470, 240, 20, 20), (240, 5, 25, 12), (380, 180, 50, 60), (60, 60, 12, 30)]


class _NoNet:
    pass


def _demo(golden_dir, n=None):
    from clipgen import demo_clip, frame_crcs
    d = np.load(f"{golden_dir}/clip_demo.npz")
    frames, _ = demo_clip(int(d["n_frames"]))
    np.testing.assert_array_equal(frame_crcs(frames), d["frame_crc32"])
    return (frames if n is None else frames[:n]), d


def _single(net, frames, box, smooth=False, start=0):
    trk = FEARTracker(net, cuda_id=0, **dict(DEFAULT_TRACKING_CONFIG, smooth=smooth))
    trk.initialize(frames[start], np.array(box))
    return np.stack([np.array(trk.tracking_state.bbox)] + [np.array(trk.update(f)["bbox"]) for f in frames[start + 1:]])


def _multi(net, frames, boxes, smooth=False):
    mt = FEARMultiTracker(net, cuda_id=0, **dict(DEFAULT_TRACKING_CONFIG, smooth=smooth))
    assert mt.device_path
    ids = mt.add(frames[0], np.array(boxes))
    rows = [mt.update(f) for f in frames[1:]]
    return {i: np.stack([r[i] for r in rows]) for i in ids}, ids


def _step_states(n, smooth, seed):
    """Seeded maps and tracker states: contexts inside, straddling and outside their frames, larger than the frame, several frame
    sizes; a share of the maps with tiny ltrb distances (boxes that clamp to 3 x 3)."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.RandomState(seed)
    sizes = np.array([(192, 320), (256, 480), (1080, 1920), (7, 5), (40, 30)], dtype=np.int32)
    hw = sizes[rng.randint(0, len(sizes), n)]
    side = np.array([15, 60, 225, 870, 2500])
    cw, ch = side[rng.randint(0, 5, n)], side[rng.randint(0, 5, n)]
    cx = (rng.uniform(-0.5, 1.2, n) * hw[:, 1]).astype(np.int64) - cw // 2
    cy = (rng.uniform(-0.5, 1.2, n) * hw[:, 0]).astype(np.int64) - ch // 2
    ctx = np.stack([cx, cy, cw, ch], axis=1).astype(np.int32)
    cls = torch.randn(n, 1, 16, 16, generator=g) * 2.0
    reg = torch.rand(n, 4, 16, 16, generator=g) * 70.0 + 5.0
    tiny = torch.from_numpy(rng.rand(n) < 0.25)
    reg[tiny] = reg[tiny] * 0.01
    prev = rng.uniform(5.0, 120.0, (n, 2))
    return cls, reg, hw, ctx, prev


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_tracker_step_matches_the_host_tracker_bit_for_bit(hip_net, smooth, n):
    cfg = dict(DEFAULT_TRACKING_CONFIG, smooth=smooth)
    cls, reg, hw, ctx, prev = _step_states(n, smooth, seed=100 + n + 7 * smooth)
    trk = FEARTracker(_NoNet(), cuda_id="cpu", **cfg)
    window = trk.window.reshape(-1).double().cuda()
    if smooth:
        _, xywh_ref, score_ref = hip_net.decode_smooth(cls.cuda(), reg.cuda(), prev, trk.window, cfg["penalty_k"],
                                                        cfg["window_influence"], cfg["lr"])
    else:
        _, xywh_ref, score_ref = hip_net.decode(cls.cuda(), reg.cuda())
    box_d = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    ctx_d = torch.from_numpy(ctx).cuda()
    prev_d = torch.from_numpy(prev).cuda()
    score_d = torch.zeros(n, dtype=torch.float32, device="cuda")
    xywh_d = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    hip_net.tracker_step(cls.cuda(), reg.cuda(), torch.from_numpy(hw).cuda(), box_d, ctx_d, prev_d, score_d, smooth, window,
                         cfg["penalty_k"], cfg["window_influence"], cfg["lr"], 16, 16, 256, cfg["search_context"], xywh=xywh_d)
    assert torch.equal(xywh_d, xywh_ref) and torch.equal(score_d, score_ref)
    xywh_ref = xywh_ref.cpu().numpy()
    box_d, ctx_d, prev_d = box_d.cpu().numpy(), ctx_d.cpu().numpy(), prev_d.cpu().numpy()
    kinds = set()
    for i in range(n):
        shape = (int(hw[i, 0]), int(hw[i, 1]), 3)
        box = clamp_bbox(trk._rescale_bbox(xywh_ref[i].copy(), ctx[i]), shape)
        nctx, in_crop = crop_geometry(shape, box, cfg["instance_size"], cfg["search_context"])
        assert box_d[i].tolist() == [int(v) for v in box], i
        assert ctx_d[i].tolist() == [int(v) for v in nctx], i
        assert prev_d[i].tobytes() == np.asarray(in_crop[2:], dtype=np.float64).tobytes(), i
        kinds.add("3x3" if box[2] == 3 and box[3] == 3 else "frame" if box[2] == shape[1] and box[3] == shape[0] else "other")
    if n == 300:
        assert {"3x3", "frame", "other"} <= kinds


def test_crop_normalize_frames_equals_one_frame_crops(hip_net):
    rng = np.random.RandomState(5)
    frames = [torch.from_numpy(rng.randint(0, 256, size=s).astype(np.uint8)).cuda()
              for s in ((192, 320, 3), (256, 480, 3), (97, 61, 3))]
    n = 40
    fidx = rng.randint(0, 3, n).astype(np.int32)
    ctx = np.zeros((n, 4), np.int32)
    for i in range(n):
        h, w = frames[fidx[i]].shape[:2]
        cw, ch = rng.choice([30, 128, 256, 512, 870]), rng.choice([30, 128, 256, 512, 870])
        ctx[i] = (rng.randint(-cw, w), rng.randint(-ch, h), cw, ch)
    pad = rng.randint(0, 256, (n, 3)).astype(np.uint8)
    table = hip_net.frame_table(frames)
    got = hip_net.crop_normalize_frames(table, torch.from_numpy(fidx).cuda(), torch.from_numpy(ctx).cuda(),
                                        torch.from_numpy(pad).cuda(), 256)
    for i in range(n):
        ref = hip_net.crop_normalize(frames[fidx[i]], ctx[i:i + 1], pad[i:i + 1], 256)
        assert torch.equal(got[i:i + 1], ref), i


@pytest.mark.parametrize("smooth", [False, True])
def test_demo_clip_twelve_targets_equal_single_trackers(hip_net, golden_dir, smooth):
    frames, d = _demo(golden_dir)
    got, ids = _multi(hip_net, frames, DEMO_BOXES, smooth)
    np.testing.assert_array_equal(np.concatenate([d["init_bbox"][None], got[ids[0]]]), d[f"tracked_smooth{int(smooth)}"])
    for i, box in zip(ids, DEMO_BOXES):
        np.testing.assert_array_equal(got[i], _single(hip_net, frames, box, smooth)[1:], err_msg=str(box))


def test_many_targets_run_another_plan_and_keep_the_fixture_boxes(hip_net, golden_dir):
    frames, d = _demo(golden_dir)
    boxes = [DEMO_BOXES[0]] * 126 + DEMO_BOXES[1:5]
    got, ids = _multi(hip_net, frames, boxes)
    for i in ids[:126]:
        np.testing.assert_array_equal(np.concatenate([d["init_bbox"][None], got[i]]), d["tracked_smooth0"])


def test_two_streams_in_one_tracker(hip_net, golden_dir):
    demo, _ = _demo(golden_dir, 24)
    synth = np.load(f"{golden_dir}/clip_synth.npz")
    frames = synth["frames"]
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    (a,) = mt.add(frames[0], synth["init_bbox"], stream=0)
    b, c = mt.add(demo[0], np.array([DEMO_BOXES[0], DEMO_BOXES[1]]), stream=1)
    rows = [mt.update([frames[t], demo[t]]) for t in range(1, 24)]
    np.testing.assert_array_equal(np.stack([synth["init_bbox"]] + [r[a] for r in rows]), synth["tracked"])
    np.testing.assert_array_equal(np.stack([r[a] for r in rows]), _single(hip_net, frames, synth["init_bbox"])[1:])
    np.testing.assert_array_equal(np.stack([r[b] for r in rows]), _single(hip_net, demo, DEMO_BOXES[0])[1:])
    np.testing.assert_array_equal(np.stack([r[c] for r in rows]), _single(hip_net, demo, DEMO_BOXES[1])[1:])


@pytest.mark.parametrize("device_frames", [False, True])
def test_pipelined_submits_equal_update(hip_net, golden_dir, device_frames):
    frames, _ = _demo(golden_dir, 60)
    ref, ids = _multi(hip_net, frames, DEMO_BOXES)
    src = [torch.from_numpy(f).cuda() for f in frames] if device_frames else list(frames)
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    assert mt.add(src[0], np.array(DEMO_BOXES)) == ids
    pending = mt.submit(src[1])
    rows, scores = [], []
    for f in src[2:]:
        nxt = mt.submit(f)                       # frame t + 1 goes in before frame t is read
        rows.append(pending.result())
        scores.append(pending.scores())
        pending = nxt
    rows.append(pending.result())
    for i in ids:
        np.testing.assert_array_equal(np.stack([r[i] for r in rows]), ref[i])
    assert all(0.0 <= s[i] <= 1.0 for s in scores for i in ids)


def test_add_and_remove_mid_clip(hip_net, golden_dir):
    frames, _ = _demo(golden_dir, 40)
    late = (250, 90, 40, 60)
    refs = [_single(hip_net, frames, b) for b in DEMO_BOXES[:3]]
    ref_late = _single(hip_net, frames, late, start=8)
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    a, b, c = mt.add(frames[0], np.array(DEMO_BOXES[:3]))
    got = {a: [], c: []}
    for t in range(1, len(frames)):
        res = mt.update(frames[t])
        for i in got:
            got[i].append(res[i])
        if t == 8:
            (d,) = mt.add(frames[8], late)
            got[d] = []
        if t == 12:
            mt.remove([b])
        if t > 12:
            assert set(res) == {a, c, d}
    np.testing.assert_array_equal(np.stack(got[a]), refs[0][1:])
    np.testing.assert_array_equal(np.stack(got[c]), refs[2][1:])
    np.testing.assert_array_equal(np.stack(got[d]), ref_late[1:])


@pytest.mark.parametrize("device_frames", [True, False])
def test_submit_never_synchronises(hip_net, golden_dir, device_frames):
    """submit() issues uploads, launches and the result copy without waiting for the stream: under sync-debug mode "error" any
    synchronising torch call inside it (a pageable host-to-device copy, .item(), a stream synchronize) raises."""
    frames, _ = _demo(golden_dir, 12)
    ref, ids = _multi(hip_net, frames, DEMO_BOXES)
    src = [torch.from_numpy(f).cuda() for f in frames] if device_frames else list(frames)
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    assert mt.add(src[0], np.array(DEMO_BOXES)) == ids
    torch.cuda.synchronize()
    pending = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in src[1:]:
            pending.append(mt.submit(f))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = [p.result() for p in pending]
    for i in ids:
        np.testing.assert_array_equal(np.stack([r[i] for r in rows]), ref[i])
