"""The consumers of the monitored metric (feartracker_amd/schedule.py), host only: the plateau schedule against torch's
ReduceLROnPlateau epoch by epoch, top-k checkpoint keeping with a stub exporter, early stopping against the patience rule."""
import os

import numpy as np
import pytest
import torch

from feartracker_amd.schedule import EarlyStopping, PlateauSchedule, TopKCheckpoints


class _Opt:
    """What PlateauSchedule needs of an optimiser: `AdamHIP.lr`, a plain attribute."""

    def __init__(self, lr):
        self.lr = lr


def _series():
    rng = np.random.RandomState(4)
    n = 80
    t = np.arange(n)
    rising = 0.2 + 0.6 * (1 - np.exp(-t / 12.0)) + 0.002 * rng.standard_normal(n)       # climbs, then saturates into noise
    flat = np.full(n, 0.41)
    noisy = 0.5 + 0.05 * rng.standard_normal(n)
    falling = 0.7 - 0.004 * t
    steps = np.repeat([0.3, 0.30002, 0.5, 0.49, 0.50004], 16)                            # improvements around the 1e-4 threshold
    return dict(rising=rising, flat=flat, noisy=noisy, falling=falling, steps=steps)


SERIES = _series()


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("name", sorted(SERIES))
@pytest.mark.parametrize("kw", [dict(), dict(factor=0.3, patience=3, min_lr=2e-5), dict(patience=0, factor=0.1, min_lr=1e-6)])
def test_plateau_schedule_equals_reduce_lr_on_plateau(name, mode, kw):
    values = SERIES[name]
    assert len(values) >= 60
    param = torch.nn.Parameter(torch.zeros(3))
    adam = torch.optim.Adam([param], lr=1e-4)
    full = dict(dict(factor=0.5, patience=10, min_lr=1e-6), **kw)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(adam, mode=mode, **full)
    opt = _Opt(1e-4)
    mine = PlateauSchedule(opt, mode=mode, **kw)
    lrs = []
    for v in values:
        ref.step(float(v))
        got = mine.step(v)
        assert got == opt.lr == adam.param_groups[0]["lr"]
        lrs.append(got)
    if name in ("flat", "noisy") or (name, mode) in (("falling", "max"), ("rising", "min")):
        assert lrs[-1] < 1e-4                      # the series does plateau: the comparison saw reductions
    assert min(lrs) >= full["min_lr"]


def test_plateau_schedule_defaults_are_the_reference_configuration():
    s = PlateauSchedule(_Opt(1e-4))
    assert (s.mode, s.factor, s.patience, s.min_lr, s.threshold) == ("max", 0.5, 10, 1e-6, 1e-4)
    with pytest.raises(ValueError):
        PlateauSchedule(_Opt(1e-4), mode="best")


def test_top_k_keeps_exactly_the_best_files(tmp_path):
    written = []

    def exporter(state, path, payload="fp16"):
        written.append((state["epoch"], payload))
        with open(path, "w") as fh:
            fh.write(str(state["epoch"]))

    values = [0.30, 0.42, 0.35, 0.42, 0.10, 0.55, 0.50, 0.20, 0.56, 0.41]
    keep = TopKCheckpoints(str(tmp_path / "ckpt"), k=3, mode="max", payload="fp32", exporter=exporter)
    assert keep.best() is None
    for epoch, v in enumerate(values):
        path = keep.step(v, {"epoch": epoch}, epoch)
        top = sorted(range(epoch + 1), key=lambda e: (-values[e], e))[:3]
        assert (path is not None) == (epoch in top)
        files = sorted(os.listdir(tmp_path / "ckpt"))
        assert files == sorted(f"fear_{e}.fearw" for e in top)
        assert keep.paths() == [str(tmp_path / "ckpt" / f"fear_{e}.fearw") for e in top]
        assert keep.best() == str(tmp_path / "ckpt" / f"fear_{top[0]}.fearw")
    assert open(keep.best()).read() == "8"
    assert [e for e, _ in written] == [0, 1, 2, 3, 5, 6, 8] and all(p == "fp32" for _, p in written)
    # mode "min" keeps the smallest
    low = TopKCheckpoints(str(tmp_path / "low"), k=2, mode="min", exporter=exporter)
    for epoch, v in enumerate(values):
        low.step(v, {"epoch": epoch}, epoch)
    assert sorted(os.listdir(tmp_path / "low")) == ["fear_4.fearw", "fear_7.fearw"]
    assert low.best().endswith("fear_4.fearw")


def _patience_rule(values, patience, mode):
    """pytorch_lightning's EarlyStopping with min_delta 0: the epoch (0-based) at which `patience` values in a row have failed to
    beat the best strictly, or None."""
    best, wait = None, 0
    for epoch, v in enumerate(values):
        if best is None or (v > best if mode == "max" else v < best):
            best, wait = v, 0
        else:
            wait += 1
            if wait >= patience:
                return epoch
    return None


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("name", sorted(SERIES))
def test_early_stopping_stops_at_the_patience_rules_epoch(name, mode):
    values = SERIES[name]
    for patience in (1, 5, 20):
        stop = EarlyStopping(patience=patience, mode=mode)
        got = next((epoch for epoch, v in enumerate(values) if stop.step(v)), None)
        assert got == _patience_rule(values, patience, mode)
    assert EarlyStopping().patience == 20 and EarlyStopping().mode == "max"
    flat = EarlyStopping(patience=20)
    assert [flat.step(0.4) for _ in range(22)] == [False] * 20 + [True, True]
