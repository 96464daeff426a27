"""`fit`: the training run — the loop of the reference's `train/trainer.py` and `train/fear_lightning_model.py` over this project's
operators.  Per step `net.step`, the gradient all-reduce, `opt.step`, the metrics and the miner, all enqueued without a host wait; per
epoch one read of the losses, validation, the monitored metric's three consumers, the samplers' resampling and one checkpoint.

    loader = PairLoader(plan, store, row_ids, TrainPairBuilder(seed=0))
    history = fit(net, opt, loader, epochs=50, metrics=TrainMetrics(0, loader.datasets), val_sequences=sequences,
                  schedule=PlateauSchedule(opt), checkpoints=TopKCheckpoints("checkpoints"), early_stopping=EarlyStopping(),
                  dynamic_frame_offset=dict(start_epoch=20, freq=5, step=5, max_value=150), checkpoint_path="last.pt")

Between the first and the last step of an epoch the host reads nothing from the device.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional

MONITOR = "valid/metrics/box_iou"          # config/train_stage/tracker.yaml: metric_to_monitor


def _counters(obj: Any, names) -> Optional[Dict[str, Any]]:
    return None if obj is None else {name: getattr(obj, name) for name in names}


def _restore(obj: Any, saved: Optional[Dict[str, Any]]) -> None:
    if obj is not None and saved is not None:
        for name, value in saved.items():
            setattr(obj, name, value)


def fit(net, opt, loader, epochs: int, min_epochs: int = 0, metrics=None, miner=None, validator=None, val_sequences=None, schedule=None,
        checkpoints=None, early_stopping=None, check_val_every_n_epoch: int = 1, dynamic_frame_offset: Optional[Dict[str, int]] = None,
        resume: Optional[str] = None, checkpoint_path: Optional[str] = None, group=None,
        log: Optional[Callable[[Dict[str, Any]], None]] = None) -> List[Dict[str, Any]]:
    """Train `net` with `opt` on `loader`'s batches until `epochs` epochs are done (counted from the start of the run, also after a
    `resume`), or until `early_stopping` says so at an epoch from `min_epochs` on (Lightning's rule).  Returns `history`: per epoch
    {"epoch", "train/loss", "train/cls_loss", "train/reg_loss" (means over the steps), "lr" (in force during the epoch), the keys of
    `metrics.compute()`, and on a validation epoch the validator's values but its per-sequence list}.

    metrics: a `TrainMetrics` over `loader.datasets`; miner: a `BestWorstMiner` (both reset when an epoch starts — read the miner's
    sheets in `log`).  Validation runs every `check_val_every_n_epoch` epochs when `val_sequences` are given: `validator.run`, or a
    `SequenceValidator.from_training_state(net.state_dict())` made for the epoch.  Its "valid/metrics/box_iou" feeds `schedule.step`,
    `checkpoints.step(value, net.state_dict(), epoch)` and `early_stopping.step`.  `loader.plan.end_epoch(epoch, dynamic_frame_offset)`
    ends every epoch.  With `checkpoint_path` every epoch ends with `save_training_checkpoint(path, net, opt, **extra)`, `extra` being
    epoch (the one completed), loader, schedule, early_stopping, checkpoints (their states) and history; `resume=path` restores all
    of it into the objects given and the run continues bit for bit.  group: a process group — with more than one rank the gradients
    are averaged by `allreduce_gradients` before the optimiser's step.  log: called with every epoch's dict."""
    import torch
    from .schedule import load_training_checkpoint, save_training_checkpoint
    history: List[Dict[str, Any]] = []
    first = 0
    if resume is not None:
        extra = load_training_checkpoint(resume, net, opt)
        first = int(extra["epoch"]) + 1
        history = [dict(h) for h in extra["history"]]
        loader.load_state_dict(extra["loader"])
        _restore(schedule, extra.get("schedule"))
        _restore(early_stopping, extra.get("early_stopping"))
        if checkpoints is not None and extra.get("checkpoints") is not None:
            checkpoints._kept = [tuple(k) for k in extra["checkpoints"]["kept"]]
            checkpoints._seen = int(extra["checkpoints"]["seen"])
    ranks = 1
    if group is not None:
        import torch.distributed as dist
        ranks = dist.get_world_size(group)
    device = getattr(net, "device", None)
    for epoch in range(first, int(epochs)):
        if metrics is not None:
            metrics.reset()
        if miner is not None:
            miner.reset()
        lr = float(opt.lr)
        sums, steps = None, 0
        for item in loader:
            batch = item.batch
            out = net.step(*batch[:5])
            grads = out["grads"]
            if ranks > 1:
                grads = net.allreduce_gradients(grads, group)
            opt.step(grads)
            if metrics is not None:
                metrics.update(out, batch, item.visible, item.dataset_ids)
            if miner is not None:
                miner.update(out, batch, item.visible)
            # the epoch's sums stay on the device, in float64: cls, reg, cls + reg
            c, r = out["loss_cls"].to(torch.float64).reshape(1), out["loss_reg"].to(torch.float64).reshape(1)
            term = torch.cat([c, r, c + r])
            sums = term if sums is None else sums + term
            steps += 1
        if steps == 0:
            raise ValueError("the loader gave no batch: fewer samples than one batch")
        totals = sums.cpu().tolist()                         # the epoch's one read of the losses
        record: Dict[str, Any] = {"epoch": epoch, "train/loss": totals[2] / steps, "train/cls_loss": totals[0] / steps,
                                  "train/reg_loss": totals[1] / steps, "lr": lr}
        if metrics is not None:
            record.update(metrics.compute())
        validate = val_sequences is not None and (epoch + 1) % int(check_val_every_n_epoch) == 0
        stop = False
        if validate:
            if validator is not None:
                runner = validator
            else:
                from .validate import SequenceValidator
                kwargs = {} if device is None or device.index is None else {"device": device.index}
                runner = SequenceValidator.from_training_state(net.state_dict(), **kwargs)
            values = runner.run(val_sequences)
            record.update({k: float(v) for k, v in values.items() if k != "sequences"})
            value = float(values[MONITOR])
            if schedule is not None:
                schedule.step(value)
            if checkpoints is not None:
                checkpoints.step(value, net.state_dict(), epoch)
            if early_stopping is not None:
                stop = bool(early_stopping.step(value)) and (epoch + 1) >= int(min_epochs)
        loader.plan.end_epoch(epoch, dynamic_frame_offset)
        history.append(record)
        if checkpoint_path is not None:
            kept = None if checkpoints is None else {"kept": [list(k) for k in checkpoints._kept], "seen": checkpoints._seen}
            save_training_checkpoint(checkpoint_path, net, opt, epoch=epoch, loader=loader.state_dict(),
                                     schedule=_counters(schedule, ("best", "num_bad_epochs")),
                                     early_stopping=_counters(early_stopping, ("best", "wait")), checkpoints=kept,
                                     history=[dict(h) for h in history])
        if log is not None:
            log(record)
        if stop:
            break
    return history
