"""Tracking on frames kept in a `JpegStore` ("Rows from the device"): `FEARMultiTracker.search_rows`
against `search_rows_host` of the state copied back; the loop search_rows -> decode_rows -> submit, which never waits, against
decode -> submit on the two clips of tests/golden/jpeg_clip.npz; the same boxes when every row outside `search_rows` holds noise; and
`SequenceValidator` on `StoreFrames` against a run on the decoded frames."""
import os

import numpy as np
import pytest
import torch

from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARMultiTracker, JpegStore, StoreFrames, search_rows_host
from feartracker_amd.validate import SequenceValidator

pytestmark = pytest.mark.gpu
SMALL = (110, 90, 28, 22)                   # a small target on clip 1: its search window is a band of the 197 rows


@pytest.fixture(scope="module")
def clips():
    """The two clips in one store: (store, ids per clip, annotations per clip, every frame decoded whole, per clip)."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_clip.npz")) as d:
        files = [[d[f"jpg_{c}_{t}"].tobytes() for t in range(int(d[f"n_{c}"]))] for c in (0, 1)]
        boxes = [d[f"boxes_{c}"] for c in (0, 1)]
    store = JpegStore(device=0, threads=4)
    ids = [store.add(f) for f in files]
    assert set(store.kinds) == {"scan"} and store.shape(ids[0][:1]).tolist() == [[256, 480]] and store.shape(ids[1][:1]).tolist() == [[197, 247]]
    whole = [store.decode(i, check=True) for i in ids]
    torch.cuda.synchronize()
    yield store, ids, boxes, whole
    store.close()


def _tracker(net, whole, boxes):
    """Three targets on two streams: the demo object, which moves out of the right edge of clip 0, and a small one beside it; a small one
    on clip 1."""
    mt = FEARMultiTracker(net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    a = mt.add(whole[0][0], np.array([boxes[0][0], (300, 100, 30, 24)]), stream=0)
    b = mt.add(whole[1][0], np.array(SMALL), stream=1)
    return mt, a + b


def _host_rows(mt, n_streams):
    return search_rows_host(mt._ctx.cpu().numpy(), mt._fidx.cpu().numpy(), n_streams, DEFAULT_TRACKING_CONFIG["instance_size"])


def test_search_rows_equals_the_host_statement(hip_net, clips):
    store, ids, boxes, whole = clips
    mt = FEARMultiTracker(hip_net, cuda_id=0, **DEFAULT_TRACKING_CONFIG)
    assert mt.search_rows().shape == (0, 2) and mt.search_rows(3).tolist() == [[0, 0]] * 3     # no targets yet
    mt, targets = _tracker(hip_net, whole, boxes)
    seen = []
    for t in range(1, 6):
        rows = mt.search_rows()
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.shape == (2, 2)
        assert np.array_equal(rows.cpu().numpy(), _host_rows(mt, 2)), t
        assert np.array_equal(mt.search_rows(4).cpu().numpy(), _host_rows(mt, 4)) and mt.search_rows(4)[2:].tolist() == [[0, 0]] * 2
        assert np.array_equal(mt.search_rows(1).cpu().numpy(), _host_rows(mt, 1))
        seen.append(rows.cpu().numpy())
        mt.update([whole[0][t], whole[1][t]])
    # after `add`: the tall object's context, 870 rows from -295, leaves the frame at both ends; the small target's is a band of 110 rows
    assert seen[0][0, 0] < 0 and seen[0][0, 1] > 256 and seen[0][1].tolist() == [SMALL[1] - 2 * SMALL[3], SMALL[1] + 3 * SMALL[3]]
    mt.remove(targets[2:])                                                              # stream 1 has no target left
    assert mt.search_rows(2)[1].tolist() == [0, 0] and np.array_equal(mt.search_rows(2).cpu().numpy(), _host_rows(mt, 2))
    host = FEARMultiTracker(hip_net, cuda_id=0, **dict(DEFAULT_TRACKING_CONFIG, device_crop=False))
    with pytest.raises(RuntimeError):
        host.search_rows()


@pytest.fixture(scope="module")
def reference(clips):
    """{plan: (boxes, scores) of every frame from decode + submit}, one run per engine plan, shared."""
    return {}


def _reference(hip_net, clips, cache):
    key = id(hip_net)
    if key not in cache:
        store, ids, boxes, whole = clips
        mt, targets = _tracker(hip_net, whole, boxes)
        out = []
        for t in range(1, 12):
            p = mt.submit(store.decode([ids[0][t], ids[1][t]]))
            out.append((p.result(), p.scores()))
        cache[key] = (targets, out)
    return cache[key]


def _same(pending, want, targets):
    boxes, scores = want
    got_b, got_s = pending.result(), pending.scores()
    for i in targets:
        assert np.array_equal(got_b[i], boxes[i]) and got_s[i] == scores[i], i


def test_the_loop_equals_decode_and_submit_and_never_waits(hip_net, clips, reference):
    store, ids, boxes, whole = clips
    targets, want = _reference(hip_net, clips, reference)
    mt, mine = _tracker(hip_net, whole, boxes)
    assert mine == targets
    pending, bands = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(1, 12):
            rows = mt.search_rows()
            frames = store.decode_rows([ids[0][t], ids[1][t]], rows)
            pending.append(mt.submit(frames))
            bands.append(rows)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    store.check()
    for p, w in zip(pending, want):
        _same(p, w, targets)
    first = bands[0].cpu().numpy()
    assert first[1, 1] - first[1, 0] == 5 * SMALL[3] < 197                              # clip 1 was decoded as a band


def test_the_tracker_reads_nothing_outside_the_rows_it_announces(hip_net, clips, reference):
    store, ids, boxes, whole = clips
    targets, want = _reference(hip_net, clips, reference)
    mt, mine = _tracker(hip_net, whole, boxes)
    rng = np.random.default_rng(53)
    spoiled = 0
    for t in range(1, 12):
        rows = mt.search_rows().cpu().numpy()
        frames = []
        for s in (0, 1):
            f = whole[s][t].cpu().numpy()
            dirty = rng.integers(0, 256, f.shape, dtype=np.uint8)
            lo, hi = (int(np.clip(v, 0, f.shape[0])) for v in rows[s])
            dirty[lo:hi] = f[lo:hi]
            spoiled += not np.array_equal(dirty, f)
            frames.append(torch.from_numpy(dirty).cuda())
        _same(mt.submit(frames), want[t - 1], targets)
    assert spoiled >= 1                                 # rows were overwritten: the small target's first band is 110 of 197 rows


def _equal_runs(a, b):
    assert set(a) == set(b)
    for key in a:
        if key != "sequences":
            assert a[key] == b[key], key
    assert len(a["sequences"]) == len(b["sequences"])
    for p, q in zip(a["sequences"], b["sequences"]):
        assert p["dataset"] == q["dataset"] and np.array_equal(p["ious"], q["ious"]) and p["box_iou"] == q["box_iou"]
        assert p["failure_rate"] == q["failure_rate"]


def test_validator_on_store_frames_equals_the_decoded_frames(hip_net, clips, monkeypatch):
    store, ids, boxes, whole = clips
    small = np.tile(np.array(SMALL), (9, 1))
    given = [(ids[0], boxes[0], "got10k"), (ids[1][:7], boxes[1][:7], "lasot"), (ids[1][3:], small, "got10k")]
    decoded = [(whole[0], boxes[0], "got10k"), (whole[1][:7], boxes[1][:7], "lasot"), (whole[1][3:], small, "got10k")]
    val = SequenceValidator(hip_net, max_samples=12, **DEFAULT_TRACKING_CONFIG)
    want = val.run(decoded)
    assert [len(q["ious"]) for q in want["sequences"]] == [11, 6, 8]
    calls = []
    real = store.decode_rows
    monkeypatch.setattr(store, "decode_rows", lambda i, rows=None, **kw: calls.append((len(i), rows.is_cuda)) or real(i, rows, **kw))
    got = val.run([(StoreFrames(store, i), ann, name) for i, ann, name in given])
    _equal_runs(got, want)
    assert calls == [(3, True)] * 6 + [(2, True)] * 2 + [(1, True)] * 3                  # one call per step, for the live streams
    store.check()
    # a mix, and two stores, are refused before any launch; so is a sequence shorter than its annotations
    other = JpegStore(device=0, threads=1)
    try:
        calls.clear()
        with pytest.raises(ValueError):
            val.run([(StoreFrames(store, ids[0]), boxes[0], "a"), decoded[1]])
        with pytest.raises(ValueError):
            val.run([(StoreFrames(store, ids[0]), boxes[0], "a"), (StoreFrames(other, []), boxes[1], "b")])
        with pytest.raises(ValueError):
            val.run([(StoreFrames(store, ids[0][:5]), boxes[0], "a")])
        assert calls == []
    finally:
        other.close()
    with pytest.raises(IndexError):
        StoreFrames(store, [len(store)])
    assert len(StoreFrames(store, ids[1])) == 12 and torch.equal(next(iter(StoreFrames(store, ids[1][4:]))), whole[1][4])
