"""`PairLoader` and `fill_store` on the GPU (feartracker_amd/train_data/loader.py), on the tiny dataset of pairdata.py: every batch against
the direct composition decode_rows -> build(borders=) and against `build_host`, prefetch on against off, bit for bit; no host wait."""
import os

import numpy as np
import pytest
import torch

from feartracker_amd import JpegStore, jpeg_decode_host
from feartracker_amd.train_data import TrainPairBuilder
from feartracker_amd.train_data.loader import PairLoader, clip_boxes, fill_store
from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler, TrackTable
from pairdata import tiny_table, write_frames

pytestmark = pytest.mark.gpu
FIELDS = ("template", "search", "gt_reg", "gt_cls", "gt_weight", "search_bbox")
B = 4


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The table, its files in a store, and the store id of every row; made once and left unchanged."""
    root = str(tmp_path_factory.mktemp("tiny"))
    table = tiny_table(root=root)
    write_frames(root, table)
    store = JpegStore(device=0, threads=2)
    (row_ids,) = fill_store(store, [table], chunk=4)
    yield table, store, row_ids
    store.close()


@pytest.fixture(scope="module")
def net():
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    return FEARNetTrainHIP(random_init_state(0), device=0)


def make_loader(data, seed=0, samples=12, negative_ratio=1.0, **kwargs):
    table, store, row_ids = data
    sampler = TrackSampler(table, negative_ratio, 2, samples, clip_range=True, seed=seed)
    plan = EpochPlan([sampler], B, seed=seed + 100)
    return PairLoader(plan, store, [row_ids], TrainPairBuilder(device=0, seed=seed + 200), **kwargs)


def assert_equal_batches(got, want, what=""):
    for name in FIELDS:
        assert torch.equal(getattr(got, name), getattr(want, name)), f"{what}{name}"


def test_fill_store_ids_address_the_right_files(data):
    table, store, row_ids = data
    assert row_ids.shape == (15,) and np.unique(row_ids).size == 15 and len(store) == 15
    frames = store.decode(row_ids, check=True)
    for path, frame in zip(table.paths(), frames):
        with open(path, "rb") as fh:
            assert np.array_equal(frame.cpu().numpy(), jpeg_decode_host(fh.read())), path
    assert store.shape(row_ids).tolist() == [[64, 96]] * 5 + [[72, 80]] * 5 + [[64, 96]] * 5
    twice = fill_store(JpegStoreSpy(), [table, table], chunk=6)                  # distinct files once, in table order, by chunks
    assert np.array_equal(twice[0], np.arange(15)) and np.array_equal(twice[1], np.arange(15))


class JpegStoreSpy:
    def __init__(self):
        self.calls = []

    def add(self, items):
        assert len(items) <= 6 and all(os.path.exists(p) for p in items)
        self.calls.append(len(items))
        return np.arange(sum(self.calls) - len(items), sum(self.calls), dtype=np.int64)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "whole"])
@pytest.mark.parametrize("scale", [1, 2])
def test_every_batch_equals_the_direct_composition_and_build_host(data, scale, rows):
    table, store, row_ids = data
    loader = make_loader(data, seed=scale, scale=scale, rows=rows)
    builder = loader.builder
    assert len(loader) == 3
    items = list(loader)
    assert len(items) == 3
    for k, item in enumerate(items):
        shapes = store.shape(item.ids, scale)
        assert item.pairs.shape == (B, 11) and tuple(item.params.frame_shapes) == tuple(map(tuple, shapes.tolist()))
        assert np.array_equal(np.unique(item.ids), item.ids) and set(item.pairs[:, [0, 5]].reshape(-1).astype(int)) == set(range(len(item.ids)))
        bands = store.decode_rows(item.ids, builder.frame_rows(item.pairs, item.params, shapes), scale=scale)
        direct = builder.build(bands, item.pairs, item.params, borders=store.borders(item.ids))
        assert_equal_batches(item.batch, direct, f"batch {k}: ")
        whole = store.decode(item.ids, scale=scale)
        host = builder.build_host([f.cpu().numpy() for f in whole], item.pairs, item.params, borders=store.borders(item.ids).cpu().numpy())
        for name in FIELDS:
            assert np.array_equal(getattr(item.batch, name).cpu().numpy(), getattr(host, name)), f"batch {k}: {name} against build_host"
        # the table behind the batch: the sampled rows' files and boxes, clipped to the frame, divided by the scale
        t_row, s_row = item.rows[:, 0], item.rows[:, 1]
        assert np.array_equal(item.ids[item.pairs[:, 0].astype(int)], row_ids[t_row])
        assert np.array_equal(item.ids[item.pairs[:, 5].astype(int)], row_ids[s_row])
        assert np.array_equal(item.pairs[:, 1:5] * scale, clip_boxes(table.bbox[t_row], store.shape(row_ids[t_row])))
        assert np.array_equal(item.pairs[:, 6:10] * scale, clip_boxes(table.bbox[s_row], store.shape(row_ids[s_row])))
    store.check()
    assert any((table.bbox[item.rows.reshape(-1)] != item.pairs[:, [1, 2, 3, 4, 6, 7, 8, 9]].reshape(-1, 4) * scale).any() for item in items)


def test_visible_and_dataset_ids_match_the_table(data):
    table, store, row_ids = data
    loader = make_loader(data, seed=3, samples=40)
    assert loader.datasets == ["got10k", "lasot"]
    seen_invisible = False
    for item in loader:
        search = item.rows[:, 1]
        assert item.visible.dtype == item.dataset_ids.dtype == torch.int32 and item.visible.is_cuda and item.dataset_ids.is_cuda
        assert item.visible.cpu().tolist() == table.presence[search].tolist() == item.pairs[:, 10].astype(int).tolist()
        assert [loader.datasets[i] for i in item.dataset_ids.cpu().tolist()] == table.dataset[search].tolist()
        assert np.all(table.presence[item.rows[:, 0]] == 1) and not table.near_corner[item.rows[:, 0]].any()
        seen_invisible |= bool((table.presence[search] == 0).any())
    assert seen_invisible


def test_prefetch_equals_no_prefetch_with_a_step_between_batches(data, net):
    ahead, plain = make_loader(data, seed=5, prefetch=1), make_loader(data, seed=5, prefetch=0)
    for epoch in range(2):
        kept = []
        for a, p in zip(ahead, plain):
            net.step(*a.batch[:5])                                               # on the consumer's stream, beside the next data stage
            kept.append((a, p))
        assert len(kept) == 3
        torch.cuda.synchronize()
        for k, (a, p) in enumerate(kept):                                        # still intact after the later batches were built
            assert_equal_batches(a.batch, p.batch, f"epoch {epoch}, batch {k}: ")
            assert torch.equal(a.visible, p.visible) and torch.equal(a.dataset_ids, p.dataset_ids)
            assert np.array_equal(a.pairs, p.pairs) and np.array_equal(a.ids, p.ids)
            direct = plain.builder.build(plain.store.decode(a.ids), a.pairs, a.params, borders=plain.store.borders(a.ids))
            assert_equal_batches(a.batch, direct, f"epoch {epoch}, batch {k}, built again: ")
        ahead.plan.end_epoch(epoch)
        plain.plan.end_epoch(epoch)
        assert np.array_equal(ahead.plan.samplers[0].epoch_rows, plain.plan.samplers[0].epoch_rows)
    data[1].check()


@pytest.mark.parametrize("prefetch", [1, 0])
def test_an_epoch_never_waits_for_the_gpu(data, net, prefetch):
    loader = make_loader(data, seed=7, samples=20, prefetch=prefetch)
    it = iter(loader)
    first = next(it)
    net.step(*first.batch[:5])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        count = 1
        for item in it:
            net.step(*item.batch[:5])
            count += 1
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count == 5
    torch.cuda.synchronize()
    data[1].check()


def test_a_file_shared_by_pairs_is_decoded_once(data, monkeypatch):
    table, store, row_ids = data
    keep = np.flatnonzero((table.track_id == "a") & (table.frame_index < 2))
    small = TrackTable.from_arrays(*(getattr(table, name)[keep] for name in
                                     ("track_id", "frame_index", "img_path", "bbox", "presence", "near_corner", "dataset")), root=table.root)
    plan = EpochPlan([TrackSampler(small, 0, 5, 8, seed=0)], B, seed=1)
    loader = PairLoader(plan, store, [row_ids[keep]], TrainPairBuilder(device=0, seed=2), prefetch=0)
    decoded = []
    real = store.decode_rows
    monkeypatch.setattr(store, "decode_rows", lambda ids, *args, **kwargs: decoded.append(len(ids)) or real(ids, *args, **kwargs))
    items = list(loader)
    assert len(items) == 2
    for item, n in zip(items, decoded):
        assert n == len(item.ids) <= 2 < 2 * B and set(item.ids.tolist()) <= set(row_ids[keep].tolist())
    assert len(decoded) == 2
    store.check()


def test_the_state_continues_an_epoch_batch_for_batch(data):
    straight = make_loader(data, seed=9, samples=20)
    want = [item for item in straight]
    straight.plan.end_epoch(0)
    want += [item for item in straight]
    first = make_loader(data, seed=9, samples=20)
    it = iter(first)
    got = [next(it), next(it)]                                                   # two handed out, the third in flight
    state = first.state_dict()
    assert int(state["position"]) == 2
    second = make_loader(data, seed=1234, samples=20)
    second.load_state_dict(state)
    got += [item for item in second]
    assert len(got) == 5
    second.plan.end_epoch(0)
    got += [item for item in second]
    assert len(got) == len(want) == 10
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.pairs, w.pairs) and np.array_equal(g.ids, w.ids)
        assert_equal_batches(g.batch, w.batch, f"batch {k}: ")
