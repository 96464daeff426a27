"""fear_train_metrics through TrainMetrics on the GPU against the numpy restatement step_metrics_host (itself pinned to the
reference's decode and to the box_iou formula by tests/test_metrics_host.py): per-pair IoUs bit for bit, the step scalars and the
epoch accumulators to 1e-12 (summing up to 1024 values in [0, 1] in another order moves the sum by at most 1024 * 2^-53 = 1.1e-13)."""
import numpy as np
import pytest
import torch

import metricsgen as mg
from feartracker_amd.metrics import TrainMetrics, step_metrics_host

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _device(m):
    dev = torch.device("cuda:0")
    out = {k: torch.from_numpy(v).to(dev) for k, v in m.items()}
    return {"cls": out["cls"], "bbox": out["bbox"]}, out["gt_box"], out["visible"], out["dataset_id"]


def _expected_epoch(hosts):
    """The reference's epoch values from the per-step host results (steps without a visible pair count for nothing)."""
    counted = [h for h in hosts if h["n_visible"]]
    exp = {"train/metrics/box_iou": sum(h["box_iou"] for h in counted) / len(counted),
           "train/metrics/failure_rate": sum(h["failure_rate"] for h in counted) / len(counted)}
    sums = sum(h["dataset_sum"] for h in hosts)
    counts = sum(h["dataset_count"] for h in hosts)
    for d, name in enumerate(mg.DATASETS):
        if counts[d]:
            exp[f"train/metrics/{name}_box_iou"] = sums[d] / counts[d]
    return exp


@pytest.mark.parametrize("B", mg.STEP_SIZES)
def test_four_updates_equal_the_host_restatement(B):
    metrics = TrainMetrics(0, mg.DATASETS)
    hosts = []
    for seed in range(mg.N_STEPS):
        m = mg.step_maps(B, seed)
        plain = [i for i in range(B) if i not in mg.special_pairs(B)]
        assert mg.logit_margins(m["cls"])[plain].min() >= 1e-3
        host = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
        hosts.append(host)
        step_out, gt, vis, ds = _device(m)
        metrics.update(step_out, gt, vis, ds)
        iou = metrics.last_iou.cpu().numpy()
        step = metrics.last_step.cpu().numpy()
        print(f"B={B} step {seed}: max |iou - host| = {np.abs(iou - host['iou']).max():.3e}, step scalars {step}, host "
              f"{host['box_iou']!r} {host['failure_rate']!r} {host['n_visible']}")
        np.testing.assert_array_equal(iou, host["iou"])
        assert step[2] == host["n_visible"]
        assert abs(step[0] - host["box_iou"]) <= TOL and abs(step[1] - host["failure_rate"]) <= TOL
        for special in mg.special_pairs(B):                        # the planted ties took part (they are visible or the check is empty)
            assert m["visible"][special] == 0 or iou[special] >= 0.0
    got, exp = metrics.compute(), _expected_epoch(hosts)
    print("epoch:", got, "expected:", exp)
    assert set(got) == set(exp) and len(got) == 2 + mg.N_DATASETS
    for key, value in exp.items():
        assert abs(got[key] - value) <= TOL, key
    metrics.reset()
    assert metrics.compute() == {}


def test_a_step_without_a_visible_pair_adds_nothing():
    metrics = TrainMetrics(0, mg.DATASETS)
    m = mg.step_maps(5, 0)
    step_out, gt, vis, ds = _device(m)
    metrics.update(step_out, gt, vis, ds)
    before = metrics.compute()
    metrics.update(step_out, gt, torch.zeros_like(vis), ds)
    assert metrics.last_step.cpu().tolist() == [0.0, 0.0, 0.0]
    assert (metrics.last_iou.cpu().numpy() == -1.0).all()
    assert metrics.compute() == before and len(before) >= 3
    only = TrainMetrics(0, mg.DATASETS)
    only.update(step_out, gt, torch.zeros_like(vis), ds)
    assert only.compute() == {}


def test_update_never_synchronises():
    """update() is one operator call on the current stream: under sync-debug mode "error" any synchronising torch call inside it
    (a copy of the maps, a pageable upload, .item()) raises."""
    metrics = TrainMetrics(0, mg.DATASETS)
    m = mg.step_maps(128, 2)
    host = step_metrics_host(m["cls"], m["bbox"], m["gt_box"], m["visible"], m["dataset_id"], mg.N_DATASETS)
    step_out, gt, vis, ds = _device(m)
    metrics.update(step_out, gt, vis, ds)                      # (buffers allocated)
    metrics.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            metrics.update(step_out, gt, vis, ds)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    np.testing.assert_array_equal(metrics.last_iou.cpu().numpy(), host["iou"])
    got = metrics.compute()
    assert abs(got["train/metrics/box_iou"] - host["box_iou"]) <= TOL


def test_bad_arguments_are_reported():
    metrics = TrainMetrics(0, mg.DATASETS)
    step_out, gt, vis, ds = _device(mg.step_maps(5, 0))
    with pytest.raises(ValueError):
        metrics.update({"cls": step_out["cls"][:, 0], "bbox": step_out["bbox"]}, gt, vis, ds)
    with pytest.raises(ValueError):
        metrics.update(step_out, gt, vis[:3], ds)
    with pytest.raises(ValueError):
        TrainMetrics(0, [str(i) for i in range(65)])
    lib = metrics.lib
    assert lib.fear_train_metrics(None, None, None, None, None, 0, 3, None, None, None, None) == 0
    assert lib.fear_train_metrics(None, None, None, None, None, 4, 3, None, None, None, None) == -1
    assert lib.fear_train_metrics(None, None, None, None, None, 4, 65, None, None, None, None) == -2


def test_a_real_training_step_feeds_both_paths():
    """The maps of one FEARNetTrainHIP.step (B = 8, seeded random initial state) through TrainMetrics, as the training loop calls
    it, and — copied to the host — through step_metrics_host."""
    from feartracker_amd.train_data import TrainBatch, encode_targets
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    B = 8
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(17)
    tmpl = torch.randn(B, 3, 128, 128, generator=g).to(dev)
    srch = torch.randn(B, 3, 256, 256, generator=g).to(dev)
    rng = np.random.RandomState(2)
    # (large boxes: an untrained network's decoded boxes land anywhere in the crop, and most IoUs should not be exactly 0)
    boxes = np.concatenate([rng.randint(0, 40, size=(B, 2)), rng.randint(150, 216, size=(B, 2))], axis=1).astype(np.int64)
    presence = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=np.int32)
    reg, cls, wgt = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in encode_targets(boxes, presence))
    batch = TrainBatch(tmpl, srch, reg, cls, wgt, torch.from_numpy(boxes.astype(np.int32)).to(dev))
    visible = torch.from_numpy(presence).to(dev)
    ds = torch.from_numpy(np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.int32)).to(dev)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    out = net.step(batch.template, batch.search, batch.gt_reg, batch.gt_cls, batch.gt_weight)
    metrics = TrainMetrics(0, mg.DATASETS)
    metrics.update(out, batch, visible, ds)
    host = step_metrics_host(out["cls"].cpu().numpy(), out["bbox"].cpu().numpy(), boxes, presence, ds.cpu().numpy(), mg.N_DATASETS)
    iou, step = metrics.last_iou.cpu().numpy(), metrics.last_step.cpu().numpy()
    print("real step: iou", iou, "host", host["iou"], "step", step)
    assert torch.isfinite(out["cls"]).all().item() and torch.isfinite(out["bbox"]).all().item()
    np.testing.assert_array_equal(iou, host["iou"])
    assert step[2] == host["n_visible"] == 6
    assert abs(step[0] - host["box_iou"]) <= TOL and abs(step[1] - host["failure_rate"]) <= TOL
    got = metrics.compute()
    assert abs(got["train/metrics/box_iou"] - host["box_iou"]) <= TOL
