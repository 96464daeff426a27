"""`fit` on the GPU (feartracker_amd/fit.py), on the tiny dataset of pairdata.py: against the loop written out, through a resume, without
a host wait inside an epoch, and with validation on sequences kept in the store."""
import os

import numpy as np
import pytest
import torch

from feartracker_amd import BestWorstMiner, JpegStore, StoreFrames
from feartracker_amd.fit import fit
from feartracker_amd.metrics import TrainMetrics
from feartracker_amd.optim import AdamHIP
from feartracker_amd.schedule import EarlyStopping, PlateauSchedule, TopKCheckpoints
from feartracker_amd.train_data import TrainPairBuilder
from feartracker_amd.train_data.loader import PairLoader, clip_boxes, fill_store
from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
from pairdata import tiny_table, write_frames

pytestmark = pytest.mark.gpu
B = 4
OFFSETS = dict(start_epoch=1, freq=1, step=1, max_value=10)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tiny"))
    table = tiny_table(root=root)
    write_frames(root, table)
    store = JpegStore(device=0, threads=2)
    (row_ids,) = fill_store(store, [table])
    yield table, store, row_ids
    store.close()


def parts(data, seed=0, init=0, momentum=0.1, lr=1e-3):
    """A fresh network, optimiser and loader (12 samples: 3 batches of 4 per epoch)."""
    table, store, row_ids = data
    sampler = TrackSampler(table, 1.0, 2, 12, clip_range=True, seed=seed)
    loader = PairLoader(EpochPlan([sampler], B, seed=seed + 100), store, [row_ids], TrainPairBuilder(device=0, seed=seed + 200))
    net = FEARNetTrainHIP(random_init_state(init), device=0, momentum=momentum)
    return net, AdamHIP(net, lr=lr), loader


def assert_same(a, b, what=""):
    """Nested dicts / lists of tensors and values, bit for bit."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), what
        for k in a:
            assert_same(a[k], b[k], f"{what}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{what}/{k}")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), what
    else:
        assert a == b, what


def test_fit_equals_the_loop_written_out(data):
    net, opt, loader = parts(data)
    history = fit(net, opt, loader, epochs=2, dynamic_frame_offset=OFFSETS)
    ref_net, ref_opt, ref_loader = parts(data)
    want = []
    for epoch in range(2):
        cls = reg = both = 0.0
        steps = 0
        for item in ref_loader:
            out = ref_net.step(item.batch.template, item.batch.search, item.batch.gt_reg, item.batch.gt_cls, item.batch.gt_weight)
            ref_opt.step(out["grads"])
            c, r = float(out["loss_cls"]), float(out["loss_reg"])                # float32 values as doubles: summed in float64, as fit does
            cls, reg, both, steps = cls + c, reg + r, both + (c + r), steps + 1
        ref_loader.plan.end_epoch(epoch, OFFSETS)
        want.append({"epoch": epoch, "train/loss": both / steps, "train/cls_loss": cls / steps, "train/reg_loss": reg / steps, "lr": 1e-3})
        assert steps == 3
    print(history)
    assert history == want
    assert all(np.isfinite(h["train/loss"]) and h["train/loss"] > 0 for h in history)
    assert_same(net.state_dict(), ref_net.state_dict(), "model")
    assert_same(opt.state_dict(), ref_opt.state_dict(), "optimizer")
    trained, init = net.state_dict(), random_init_state(0)
    assert set(trained) == set(init) and any(not torch.equal(trained[k], init[k].to(trained[k].dtype)) for k in init)     # it did train
    assert loader.plan.samplers[0].frame_offset == ref_loader.plan.samplers[0].frame_offset == 4
    data[1].check()


def test_two_epochs_equal_one_epoch_a_resume_and_one_more(data, tmp_path):
    path = str(tmp_path / "last.pt")
    net, opt, loader = parts(data)
    straight = fit(net, opt, loader, epochs=2, dynamic_frame_offset=OFFSETS)
    net1, opt1, loader1 = parts(data)
    first = fit(net1, opt1, loader1, epochs=1, dynamic_frame_offset=OFFSETS, checkpoint_path=path)
    assert first == straight[:1]
    extra = torch.load(path, map_location="cpu", weights_only=True)["extra"]          # what a resume needs, in a file that loads safely
    assert extra["epoch"] == 0 and {"loader", "schedule", "early_stopping", "checkpoints", "history"} <= set(extra)
    net2, opt2, loader2 = parts(data, seed=77, init=1, lr=5e-2)                       # other weights, other seeds: the file decides
    resumed = fit(net2, opt2, loader2, epochs=2, dynamic_frame_offset=OFFSETS, resume=path)
    assert resumed == straight
    assert_same(net2.state_dict(), net.state_dict(), "model")
    assert_same(opt2.state_dict(), opt.state_dict(), "optimizer")
    a, b = loader.plan.samplers[0], loader2.plan.samplers[0]
    assert np.array_equal(a.epoch_rows, b.epoch_rows) and a.frame_offset == b.frame_offset == 4
    assert np.array_equal(a.pairs(np.arange(12)), b.pairs(np.arange(12)))             # and the streams go on together


class FromTheSecondStep:
    """A loader whose consumer runs under sync-debug "error" from the moment it asks for the second batch until the epoch's last
    batch has been handed out and worked on: a host wait in the step, the metrics, the miner or the data stage raises."""

    def __init__(self, inner):
        self.inner, self.plan, self.datasets, self.guarded = inner, inner.plan, inner.datasets, 0

    def __iter__(self):
        it = iter(self.inner)
        yield next(it)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for item in it:
                yield item
                self.guarded += 1
        finally:
            torch.cuda.set_sync_debug_mode("default")

    def state_dict(self):
        return self.inner.state_dict()


def test_steps_two_to_n_run_without_a_host_wait(data):
    net, opt, loader = parts(data)
    metrics, miner = TrainMetrics(0, loader.datasets), BestWorstMiner(0, max_images=2)
    guarded = FromTheSecondStep(loader)
    try:
        history = fit(net, opt, guarded, epochs=2, metrics=metrics, miner=miner)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert guarded.guarded == 4                                                       # steps 2 and 3 of both epochs
    assert {"train/metrics/box_iou", "train/metrics/failure_rate", "train/loss"} <= set(history[1])
    assert any(k.startswith("train/metrics/got10k") for k in history[1])
    sheets = miner.sheets()
    assert "best" in sheets and np.isfinite(sheets["best"][0])


def test_validation_feeds_the_schedule_and_the_checkpoints(data, tmp_path):
    table, store, row_ids = data
    net, opt, loader = parts(data, momentum=1.0, lr=1e-4)      # momentum 1: the running statistics the export folds are a real batch's
    sequences = []
    for track in ("a", "b"):
        rows = table.track_rows[track][:4]
        sequences.append((StoreFrames(store, row_ids[rows]), clip_boxes(table.bbox[rows], store.shape(row_ids[rows])), table.dataset[rows[0]]))
    schedule, keep = PlateauSchedule(opt), TopKCheckpoints(str(tmp_path / "kept"))
    stopper = EarlyStopping(patience=1)
    history = fit(net, opt, loader, epochs=2, min_epochs=2, val_sequences=sequences, schedule=schedule, checkpoints=keep,
                  early_stopping=stopper, check_val_every_n_epoch=2)
    print(history)
    assert len(history) == 2 and "valid/metrics/box_iou" not in history[0]
    names = {"valid/metrics/box_iou", "valid/metrics/got10k_box_iou", "valid/metrics/got10k_failure_rate", "valid/metrics/lasot_box_iou",
             "valid/metrics/lasot_failure_rate"}
    assert names <= set(history[1]) and "sequences" not in history[1]
    value = history[1]["valid/metrics/box_iou"]
    assert np.isfinite(value) and 0.0 <= value <= 1.0
    assert schedule.best == value and stopper.best == value
    assert keep.paths() == [os.path.join(str(tmp_path / "kept"), "fear_1.fearw")] and os.path.getsize(keep.best()) > 10_000


def test_the_command_line_trains_validates_and_resumes(data, tmp_path):
    """tools/train.py end to end on the tiny dataset: one epoch, then a second from last.pt."""
    import importlib.util
    import json
    table, store, row_ids = data
    spec = importlib.util.spec_from_file_location("train_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    anno, val, out = str(tmp_path / "anno.csv"), tmp_path / "val", str(tmp_path / "run")
    table.to_csv(anno)
    for track in ("a", "b"):                                   # GOT-10k's layout: frames and groundtruth.txt per sequence
        rows = table.track_rows[track][:4]
        os.makedirs(val / track)
        for k, path in enumerate(np.array(table.paths())[rows]):
            with open(path, "rb") as src, open(val / track / f"{k:08d}.jpg", "wb") as dst:
                dst.write(src.read())
        boxes = clip_boxes(table.bbox[rows], store.shape(row_ids[rows]))
        (val / track / "groundtruth.txt").write_text("".join(",".join(f"{v:.4f}" for v in b) + "\n" for b in boxes))
    common = ["--data", anno, table.root, "--num-samples", "12", "--batch", "4", "--frame-offset", "2", "--clip-range", "--negative-ratio", "1",
              "--dynamic-frame-offset", "1", "1", "1", "10", "--val-dir", str(val), "--max-val-samples", "4", "--out", out,
              "--bn-momentum", "1.0"]         # (momentum 1: the running statistics the export folds are a real batch's)
    tool.main(common + ["--epochs", "1"])
    with open(os.path.join(out, "history.json")) as fh:
        first = json.load(fh)
    assert len(first) == 1 and "valid/metrics/val_box_iou" in first[0] and "train/metrics/box_iou" in first[0]
    assert os.path.exists(os.path.join(out, "last.pt")) and os.listdir(os.path.join(out, "checkpoints")) == ["fear_0.fearw"]
    tool.main(common + ["--epochs", "2", "--resume", os.path.join(out, "last.pt")])
    with open(os.path.join(out, "history.json")) as fh:
        both = json.load(fh)
    assert [h["epoch"] for h in both] == [0, 1] and both[0] == first[0] and np.isfinite(both[1]["train/loss"])
