"""The epoch bookkeeping of `fit` (feartracker_amd/fit.py) on stub objects: history keys, validation cadence, min_epochs, the monitored
value's consumers, end_epoch, and what the checkpoint's `extra` carries.  No GPU."""
from types import SimpleNamespace

import pytest
import torch

from feartracker_amd.fit import fit
from feartracker_amd.schedule import EarlyStopping, PlateauSchedule, TopKCheckpoints


class Net:
    def __init__(self):
        self.w = torch.zeros(1)
        self.steps = []

    def step(self, template, search, gt_reg, gt_cls, gt_weight):
        self.steps.append(float(template))
        return {"loss_cls": torch.tensor(float(template), dtype=torch.float32), "loss_reg": torch.tensor(0.25, dtype=torch.float32),
                "cls": None, "bbox": None, "grads": {"w": torch.ones(1)}}

    def state_dict(self):
        return {"w": self.w.clone()}

    def load_state_dict(self, sd):
        self.w = sd["w"].clone()


class Opt:
    def __init__(self, net, lr=0.5):
        self.net, self.lr = net, lr

    def step(self, grads):
        self.net.w -= self.lr * grads["w"]

    def state_dict(self):
        return {"lr": self.lr}

    def load_state_dict(self, sd):
        self.lr = sd["lr"]


class Plan:
    def __init__(self):
        self.ended = []

    def end_epoch(self, epoch, dynamic_frame_offset=None):
        self.ended.append((epoch, dynamic_frame_offset))


class Loader:
    """Three batches per epoch whose template 'tensor' is the number of the batch since the start of the run."""

    def __init__(self):
        self.plan, self.count, self.datasets = Plan(), 0, ["d"]

    def __iter__(self):
        for _ in range(3):
            self.count += 1
            t = torch.tensor(float(self.count))
            yield SimpleNamespace(batch=(t, t, t, t, t, t), visible="vis", dataset_ids="ds")

    def state_dict(self):
        return {"count": self.count}

    def load_state_dict(self, state):
        self.count = state["count"]


class Validator:
    def __init__(self, values):
        self.values, self.calls = list(values), []

    def run(self, sequences):
        self.calls.append(sequences)
        v = self.values[len(self.calls) - 1]
        return {"valid/metrics/box_iou": v, "valid/metrics/d_box_iou": v, "valid/metrics/d_failure_rate": 0.0, "sequences": [{"ious": [v]}]}


class Metrics:
    def __init__(self):
        self.updates, self.resets = [], 0

    def reset(self):
        self.resets += 1
        self.updates.append([])

    def update(self, out, batch, visible, dataset_ids):
        self.updates[-1].append((float(out["loss_cls"]), visible, dataset_ids))

    def compute(self):
        return {"train/metrics/box_iou": 0.1 * len(self.updates[-1])}


def test_history_and_the_per_step_calls():
    net = Net()
    loader, metrics = Loader(), Metrics()
    seen = []
    history = fit(net, Opt(net), loader, epochs=2, metrics=metrics, dynamic_frame_offset={"k": 1}, log=seen.append)
    assert len(history) == 2 and seen == history
    assert set(history[0]) == {"epoch", "train/loss", "train/cls_loss", "train/reg_loss", "lr", "train/metrics/box_iou"}
    assert [h["epoch"] for h in history] == [0, 1]
    assert history[0]["train/cls_loss"] == 2.0 and history[1]["train/cls_loss"] == 5.0 and history[0]["train/reg_loss"] == 0.25
    assert history[1]["train/loss"] == 5.25 and history[0]["lr"] == 0.5 and history[0]["train/metrics/box_iou"] == pytest.approx(0.3)
    assert net.steps == [1, 2, 3, 4, 5, 6] and float(net.w) == -3.0
    assert metrics.resets == 2 and metrics.updates[1] == [(4.0, "vis", "ds"), (5.0, "vis", "ds"), (6.0, "vis", "ds")]
    assert loader.plan.ended == [(0, {"k": 1}), (1, {"k": 1})]                       # once per epoch


def test_validation_cadence_and_the_monitored_values_consumers(tmp_path):
    net = Net()
    opt = Opt(net, lr=1.0)
    validator = Validator([0.5, 0.4, 0.3, 0.2])
    schedule = PlateauSchedule(opt, patience=0, factor=0.5)
    written = []
    keep = TopKCheckpoints(str(tmp_path / "k"), k=2, exporter=lambda state, path, payload: written.append((path, float(state["w"]))))
    history = fit(net, opt, Loader(), epochs=8, validator=validator, val_sequences="seqs", schedule=schedule, checkpoints=keep,
                  check_val_every_n_epoch=2)
    assert validator.calls == ["seqs"] * 4
    assert [("valid/metrics/box_iou" in h) for h in history] == [False, True] * 4
    assert [h["valid/metrics/box_iou"] for h in history[1::2]] == [0.5, 0.4, 0.3, 0.2]
    assert set(history[1]) - set(history[0]) == {"valid/metrics/box_iou", "valid/metrics/d_box_iou", "valid/metrics/d_failure_rate"}
    # the schedule saw every value: a worse one halves the rate at patience 0, and the next epoch trains (and logs) at it
    assert schedule.best == 0.5 and [h["lr"] for h in history] == [1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.25] and opt.lr == 0.125
    assert [p.rsplit("fear_", 1)[1] for p, _ in written] == ["1.fearw", "3.fearw"] and len(keep.paths()) == 2     # tagged with the epoch
    assert written[0][1] == -6.0                                                      # the state at the end of epoch 1
    # without sequences nothing validates and nothing is stepped
    idle = PlateauSchedule(opt, patience=0)
    history = fit(net, opt, Loader(), epochs=2, validator=Validator([1.0]), schedule=idle)
    assert idle.best == -float("inf") and all("valid/metrics/box_iou" not in h for h in history)


def test_a_stop_is_honoured_only_from_min_epochs_on():
    def run(min_epochs):
        net = Net()
        loader = Loader()
        history = fit(net, Opt(net), loader, epochs=10, min_epochs=min_epochs, validator=Validator([0.5] + [0.1] * 9),
                      val_sequences="s", early_stopping=EarlyStopping(patience=2))
        return len(history), len(loader.plan.ended)
    assert run(0) == (3, 3)              # 0.5, then two values that are no better
    assert run(3) == (3, 3)
    assert run(6) == (6, 6)              # the stopper has been saying stop since epoch 2; honoured at epoch index 5
    assert run(20) == (10, 10)


def test_extra_carries_what_a_resume_needs(tmp_path):
    path = str(tmp_path / "last.pt")

    def parts():
        net = Net()
        opt = Opt(net, lr=1.0)
        return net, opt, Loader(), PlateauSchedule(opt, patience=0), EarlyStopping(patience=50), \
            TopKCheckpoints(str(tmp_path / "k"), k=2, exporter=lambda state, p, payload: open(p, "w").close())
    values = [0.5, 0.4, 0.6, 0.3]
    net, opt, loader, schedule, stopper, keep = parts()
    straight = fit(net, opt, loader, epochs=4, validator=Validator(values), val_sequences="s", schedule=schedule, early_stopping=stopper,
                   checkpoints=keep)
    net2, opt2, loader2, schedule2, stopper2, keep2 = parts()
    fit(net2, opt2, loader2, epochs=2, validator=Validator(values), val_sequences="s", schedule=schedule2, early_stopping=stopper2,
        checkpoints=keep2, checkpoint_path=path)
    extra = torch.load(path, map_location="cpu", weights_only=True)["extra"]
    assert set(extra) == {"epoch", "loader", "schedule", "early_stopping", "checkpoints", "history"}
    assert extra["epoch"] == 1 and extra["loader"] == {"count": 6} and len(extra["history"]) == 2
    assert extra["schedule"] == {"best": 0.5, "num_bad_epochs": 0} and extra["early_stopping"] == {"best": 0.5, "wait": 1}
    assert extra["checkpoints"]["seen"] == 2 and [k[0] for k in extra["checkpoints"]["kept"]] == [0.5, 0.4]
    net3, opt3, loader3, schedule3, stopper3, keep3 = parts()
    resumed = fit(net3, opt3, loader3, epochs=4, validator=Validator(values[2:]), val_sequences="s", schedule=schedule3,
                  early_stopping=stopper3, checkpoints=keep3, resume=path)
    assert resumed == straight and len(resumed) == 4
    assert float(net3.w) == float(net.w) and opt3.lr == opt.lr == 0.25 and loader3.count == loader.count == 12
    assert (schedule3.best, schedule3.num_bad_epochs) == (schedule.best, schedule.num_bad_epochs)
    assert (stopper3.best, stopper3.wait) == (stopper.best, stopper.wait) and keep3.paths() == keep.paths()
    assert loader3.plan.ended == [(2, None), (3, None)]


def test_several_ranks_average_the_gradients_before_the_optimiser_steps(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    order = []

    class RankedNet(Net):
        def allreduce_gradients(self, grads, group=None):
            order.append(("allreduce", group, float(grads["w"])))
            return {"w": grads["w"] * 0.5}                                  # the mean with a rank whose gradient is zero

    class WatchedOpt(Opt):
        def step(self, grads):
            order.append(("step", float(grads["w"])))
            super().step(grads)
    net = RankedNet()
    fit(net, WatchedOpt(net), Loader(), epochs=1, group="the group")
    assert order == [("allreduce", "the group", 1.0), ("step", 0.5)] * 3 and float(net.w) == -0.75
    order.clear()
    alone = RankedNet()
    fit(alone, WatchedOpt(alone), Loader(), epochs=1)                       # no group: no collective
    assert order == [("step", 1.0)] * 3
