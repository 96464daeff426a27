"""`PairLoader(scale="auto")` on the GPU ("A scale per frame"): on a small table whose tracks have objects of four
sizes, so that a batch mixes decode scales, every item against the direct composition — `frame_scales`, `scale_pairs`,
`decode_rows(scale=item.scales)`, `build(borders=)` — and against `build_host` on frames the host decoded one by one at `item.scales`,
bit for bit, with and without windows; `scale=1` and `scale=2` unchanged; no host wait."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from feartracker_amd import JpegStore, jpeg_decode_host
from feartracker_amd.jpeg_encode import jpeg_encode_host
from feartracker_amd.train_data import TrainPairBuilder, scale_pairs
from feartracker_amd.train_data.loader import PairLoader, clip_boxes, fill_store
from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler, TrackTable

pytestmark = pytest.mark.gpu
FIELDS = ("template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox")
B = 8
# per track: the frames' (H, W) and the side of its objects, chosen so that both uses of a frame admit the track's scale: a template
# context is 1.4 sides against 128 s, a search context 6 to 12 sides against 512 s
TRACKS = {"s": ((64, 96), 40, 1), "m": ((208, 224), 192, 2), "l": ((400, 416), 380, 4), "x": ((776, 760), 745, 8)}
FRAMES = 3


def _pixels(H, W, k, t):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 110 + 60 * np.sin(x / (19.0 + 3 * k) + t) * np.cos(y / (17.0 + 2 * k) - 0.5 * t)
    blob = 90 * np.exp(-(((x - W / 2 - 4 * t) / (W / 5.0)) ** 2 + ((y - H / 2 + 2 * t) / (H / 6.0)) ** 2))
    return np.clip(np.stack([base + blob, base * 0.8 + 30 + blob * 0.5, 200 - base * 0.6 + 10 * k], axis=-1), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mixed"))
    rng = np.random.default_rng(8)
    cols = dict(track_id=[], frame_index=[], img_path=[], bbox=[], presence=[], near_corner=[], dataset=[])
    for k, (track, ((H, W), side, _)) in enumerate(TRACKS.items()):
        for t in range(FRAMES):
            w, h = side + int(rng.integers(0, 6)), side + int(rng.integers(0, 6))
            cols["track_id"].append(track)
            cols["frame_index"].append(t)
            cols["img_path"].append(f"{track}/{t:04d}.jpg")
            cols["bbox"].append([int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h])
            cols["presence"].append(1)
            cols["near_corner"].append(False)
            cols["dataset"].append("got10k" if k % 2 else "lasot")
            os.makedirs(os.path.join(root, track), exist_ok=True)
            with open(os.path.join(root, cols["img_path"][-1]), "wb") as fh:
                fh.write(jpeg_encode_host(_pixels(H, W, k, t), quality=60, subsampling=("4:2:0", "4:2:2", "4:4:4", "4:2:0")[k]))
    table = TrackTable.from_arrays(root=root, **cols)
    store = JpegStore(device=0, threads=2)
    (row_ids,) = fill_store(store, [table])
    blobs = {}
    for path, i in zip(table.paths(), row_ids.tolist()):
        with open(path, "rb") as fh:
            blobs[i] = fh.read()
    yield table, store, row_ids, blobs
    store.close()


def make_loader(data, seed=0, samples=24, **kwargs):
    table, store, row_ids, _ = data
    sampler = TrackSampler(table, 0.5, 2, samples, clip_range=True, seed=seed)
    return PairLoader(EpochPlan([sampler], B, seed=seed + 100), store, [row_ids], TrainPairBuilder(device=0, seed=seed + 200), **kwargs)


def _full_table(item, data):
    """The full-size table behind an item: the sampled rows' boxes clipped to their frames, in the item's frame numbering."""
    table, store, row_ids, _ = data
    full = np.zeros((B, 11))
    full[:, [0, 5, 10]] = item.pairs[:, [0, 5, 10]]
    full[:, 1:5] = clip_boxes(table.bbox[item.rows[:, 0]], store.shape(row_ids[item.rows[:, 0]]))
    full[:, 6:10] = clip_boxes(table.bbox[item.rows[:, 1]], store.shape(row_ids[item.rows[:, 1]]))
    assert np.array_equal(item.ids[full[:, 0].astype(int)], row_ids[item.rows[:, 0]])
    assert np.array_equal(item.ids[full[:, 5].astype(int)], row_ids[item.rows[:, 1]])
    return full


@pytest.mark.parametrize("windows", [False, True], ids=["rows", "windows"])
def test_auto_items_equal_the_direct_composition_and_build_host(data, windows):
    table, store, row_ids, blobs = data
    loader = make_loader(data, seed=1, scale="auto", windows=windows)
    builder = loader.builder
    items = list(loader)
    assert len(items) == 3
    seen = set()
    for k, item in enumerate(items):
        # first: the batch mixes at least three scales, found on the CPU from the table alone
        full = _full_table(item, data)
        full_shapes = store.shape(item.ids)
        drawn = dataclasses.replace(item.params, frame_shapes=tuple(map(tuple, full_shapes.tolist())))
        scales = builder.frame_scales(full, drawn, full_shapes)
        assert len(set(scales.tolist())) >= 3, f"batch {k} mixes {sorted(set(scales.tolist()))}"
        seen |= set(scales.tolist())
        assert item.scales.dtype == np.int64 and np.array_equal(item.scales, scales)
        small = scale_pairs(full, scales)
        assert np.array_equal(item.pairs, small)
        shapes = store.shape(item.ids, scales)
        assert tuple(item.params.frame_shapes) == tuple(map(tuple, shapes.tolist()))
        # the direct composition
        bands = store.decode_rows(item.ids, builder.frame_rows(small, item.params, shapes), scale=item.scales)
        direct = builder.build(bands, small, item.params, borders=store.borders(item.ids))
        for name in FIELDS:
            assert torch.equal(getattr(item.batch, name), getattr(direct, name)), f"batch {k}: {name}"
        # the host: every frame decoded on its own at its scale
        frames = [jpeg_decode_host(blobs[int(i)], scale=int(s)) for i, s in zip(item.ids, item.scales)]
        host = builder.build_host(frames, small, item.params, borders=store.borders(item.ids).cpu().numpy())
        for name in FIELDS:
            assert np.array_equal(getattr(item.batch, name).cpu().numpy(), getattr(host, name)), f"batch {k}: {name} against build_host"
    store.check()
    assert seen == {1, 2, 4, 8}


def test_auto_draws_what_scale_1_draws_and_max_scale_caps(data):
    """The same generator stream: from equal seeds the auto loader's params and full-size table are the default loader's; `max_scale=1`
    hands out the default loader's batches, bit for bit."""
    plain, auto, capped = make_loader(data, seed=2), make_loader(data, seed=2, scale="auto"), make_loader(data, seed=2, scale="auto", max_scale=1)
    two = make_loader(data, seed=2, scale="auto", max_scale=2)
    for p, a, c, t in zip(plain, auto, capped, two):
        assert np.array_equal(p.ids, a.ids) and np.array_equal(p.rows, a.rows) and np.array_equal(p.pairs, _full_table(a, data))
        for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
            assert np.array_equal(getattr(p.params, name), getattr(a.params, name)), name
        assert np.array_equal(p.scales, np.ones(len(p.ids), dtype=np.int64)) and np.array_equal(c.scales, p.scales)
        assert np.array_equal(c.pairs, p.pairs) and all(torch.equal(x, y) for x, y in zip(c.batch, p.batch))
        assert np.array_equal(t.scales, np.minimum(a.scales, 2))
    for bad in ("AUTO", "2", "", 3, 0):
        with pytest.raises(ValueError):
            make_loader(data, scale=bad)
    with pytest.raises(ValueError):
        make_loader(data, scale="auto", max_scale=3)
    data[1].check()


@pytest.mark.parametrize("scale", [1, 2])
def test_int_scales_are_unchanged_against_the_direct_composition(data, scale):
    table, store, row_ids, _ = data
    loader = make_loader(data, seed=3, scale=scale)
    builder = loader.builder
    for k, item in enumerate(loader):
        shapes = store.shape(item.ids, scale)
        assert np.array_equal(item.scales, np.full(len(item.ids), scale)) and np.array_equal(item.pairs, scale_pairs(_full_table(item, data), scale))
        bands = store.decode_rows(item.ids, builder.frame_rows(item.pairs, item.params, shapes), scale=scale)
        direct = builder.build(bands, item.pairs, item.params, borders=store.borders(item.ids))
        for name in FIELDS:
            assert torch.equal(getattr(item.batch, name), getattr(direct, name)), f"batch {k}: {name}"
    store.check()


@pytest.mark.parametrize("prefetch", [1, 0])
def test_an_auto_epoch_never_waits_for_the_gpu(data, prefetch):
    loader = make_loader(data, seed=4, samples=40, scale="auto", windows=bool(prefetch), prefetch=prefetch)
    it = iter(loader)
    first = next(it)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        kept = [first] + [item for item in it]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(kept) == 5
    torch.cuda.synchronize()
    assert all(len(set(item.scales.tolist())) >= 2 for item in kept) and kept[-1].batch.template.abs().sum() > 0
    data[1].check()
