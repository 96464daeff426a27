"""`PairLoader(windows=True)`: from equal seeds it hands out the batches `PairLoader()` hands out, over one epoch
of 3 batches of 4, at scale 1 and 2, with and without the data stage in flight on its own stream."""
import numpy as np
import pytest
import torch

from feartracker_amd import JpegStore
from feartracker_amd.train_data import TrainPairBuilder
from feartracker_amd.train_data.loader import PairLoader, fill_store
from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
from pairdata import tiny_table, write_frames

pytestmark = pytest.mark.gpu
B = 4


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tiny_windows"))
    table = tiny_table(root=root)
    write_frames(root, table)
    store = JpegStore(device=0, threads=2)
    (row_ids,) = fill_store(store, [table])
    yield table, store, row_ids
    store.close()


def _loader(data, **kw):
    table, store, row_ids = data
    sampler = TrackSampler(table, 1.0, 2, 12, clip_range=True, seed=4)
    return PairLoader(EpochPlan([sampler], B, seed=104), store, [row_ids], TrainPairBuilder(device=0, seed=204), **kw)


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("scale", [1, 2])
def test_windows_hand_out_the_batches_of_the_default_loader(data, scale, prefetch):
    store = data[1]
    want = list(_loader(data, scale=scale, prefetch=prefetch))
    got = list(_loader(data, scale=scale, prefetch=prefetch, windows=True))
    store.check()
    assert len(want) == len(got) == 3
    for a, b in zip(got, want):
        for name, x, y in zip(a.batch._fields, a.batch, b.batch):
            assert torch.equal(x, y), name
        assert torch.equal(a.visible, b.visible) and torch.equal(a.dataset_ids, b.dataset_ids)
        assert np.array_equal(a.pairs, b.pairs) and np.array_equal(a.ids, b.ids) and np.array_equal(a.rows, b.rows)
    assert got[0].batch.template.abs().sum() > 0


def test_the_default_is_off(data):
    assert _loader(data).windows is False and _loader(data, windows=True).windows is True
