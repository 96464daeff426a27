#!/usr/bin/env python3
"""What the optimiser update costs on the 128-pair network's buffers (needs the MI355X).  Writes
profiles/optim_bench.json and prints it as one JSON line.

  python tools/optim_bench.py [--batch 128] [--steps 20] [--runs 9] [--out profiles/optim_bench.json]

Cases, all on the gradients of one `FEARNetTrainHIP.step` (1.37 M floats in one flat buffer):
  adam                 (a) AdamHIP.step, unclipped: bench.py's `adam_update_ms`, the same loop
  adam_clipped         (b) AdamHIP(max_grad_norm).step: sum of squares + finalize + update, no host synchronisation
  torch_clip_then_adam (c) what clipping costs without (b): torch's clip_grad_norm_ arithmetic over the GradDict's values (in-place
                           `mul_`, which edits the re-laid-out depthwise / stem copies), then AdamHIP.step — which then lays all
                           195 tensors out again one by one
  sgd, adamw           (d) SGDHIP (momentum 0.9, Nesterov) and AdamWHIP, unclipped
Each run is a window of `steps` updates issued back to back and synchronised once, as bench.py times its update; the runs of
(a), (b) and (d) alternate, so that they share whatever else the machine is doing; (c) edits the gradients and runs after them.  Reported: median, min and max over the runs of the
per-update time, `runs * steps` timed updates per case after one warm-up window each.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def torch_clip_(grads, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_'s arithmetic on a dict of gradient tensors (the function itself wants parameters with
    `.grad`): per-tensor norms, their norm, the clamped coefficient, an in-place multiply of every tensor."""
    tensors = list(grads.values())
    total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(tensors)))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    torch._foreach_mul_(tensors, coef)
    return total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on the GPU; none is visible")
    if args.steps * args.runs < 50:
        raise SystemExit("at least 50 timed updates per case")
    from feartracker_amd.optim import AdamHIP, AdamWHIP, SGDHIP
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(7)
    net = FEARNetTrainHIP(random_init_state(3), device=0)
    tmpl, srch = torch.randn(B, 3, 128, 128, generator=g).to(dev), torch.randn(B, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(B, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.9).float().to(dev)
    grads = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)["grads"]
    torch.cuda.synchronize()
    norm = float(torch.linalg.vector_norm(torch.stack([v.norm() for v in grads.values()])))
    max_norm = 0.5 * norm                              # clipping is active in (b) and (c)
    start = net.param_flat.clone()

    def updater(opt, clip_with_torch=False):
        def window() -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if clip_with_torch:
                    torch_clip_(grads, max_norm)
                opt.step(grads)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps
        return window

    # (c) edits the gradients: after its first window `current_flat()` is None for good, which is the state a user who clips with
    # torch is in at every step.  So the other cases alternate on the untouched dict first and (c) runs after them.
    cases = {"adam": updater(AdamHIP(net)), "adam_clipped": updater(AdamHIP(net, max_grad_norm=max_norm)),
             "sgd": updater(SGDHIP(net, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-6)),
             "adamw": updater(AdamWHIP(net, lr=3e-3, eps=1e-6, weight_decay=2e-6))}
    times = {k: [] for k in cases}
    for window in cases.values():
        window()
    for _ in range(args.runs):
        for k, window in cases.items():
            times[k].append(window())
    fast_path = grads.current_flat() is not None
    c_window = updater(AdamHIP(net), clip_with_torch=True)
    c_window()
    times["torch_clip_then_adam"] = [c_window() for _ in range(args.runs)]
    net.param_flat.copy_(start)
    result = dict(measurement="optimiser_update", batch=B, parameters=int(net.param_flat.numel()), steps_per_run=args.steps,
                  timed_updates_per_case=args.steps * args.runs, gradient_norm=round(norm, 6), max_grad_norm=round(max_norm, 6),
                  flat_fast_path_in_a_b_d=bool(fast_path), device=torch.cuda.get_device_name(0),
                  ms_per_update={k: _spread(v) for k, v in times.items()})
    b, c = statistics.median(times["adam_clipped"]), statistics.median(times["torch_clip_then_adam"])
    result["clipped_vs_torch_clip"] = dict(adam_clipped_ms=round(b, 4), torch_clip_then_adam_ms=round(c, 4), ratio=round(c / b, 2),
                                           faster=bool(b < c))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
