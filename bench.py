#!/usr/bin/env python3
"""Throughput bench of the FEAR-XS per-frame hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1] per GPU; configs[2] is the same sharded over 8 GPUs):
`FEARNet.track` (model_training/model/fear_net.py:90-96) on a batch of 256 independent synthetic
search crops per GPU — seeded uint8 256x256 RGB crops normalised like base_tracker.py:70-81,
each with its own cached template features from a 128x128 template crop (computed once, outside
the timed region, by `get_features`), FEAR-XS-NoEmbs weights, fp32.  Inputs are resident in HBM
when the timed region starts.  A step = one pass of the hot path over the batch; with N > 1 the
batch is sharded (independent crops) and a step also includes the single RCCL
all-gather of the packed (bbox, cls) maps.  Protocol mirrors the reference's own
(README.md:43, Benchmark.swift:55-77): warm-up calls, then the mean over K timed calls.

Prints ONE JSON line (rank 0): metric, value, unit, n_gpus, steps, warmup, ms_per_step (one timed step), higher_is_better,
scaling, vs_baseline, dtype, data, config.  A plain run does only that: set-up, warm-up, the K timed steps, the line.
  --dump-outputs DIR  after the timed steps, the maps the last timed step returned are written as DIR/bbox.npy (N,4,16,16)
               and DIR/cls.npy (N,1,16,16), fp32 (N = the global batch; a fixed seeded sample of crops beyond 64 MB).  The
               inputs are seeded, so two builds run with the same arguments can be compared map for map.
  --full       everything else this bench measures, in the same process after the timed steps (the --no-* flags switch single
               legs off): the per-kernel profile of the first warm-up steps and the dominant kernel bracketed with HIP events
               inside the timed region (for `roofline`), shader clock under load, the two-handle / split-stream / other-math
               supplementary numbers, the collective alone (N > 1), and the objects below.
Extra objects (--full):
  roofline     dominant kernel (largest share of device time): algorithmic FLOPs or bytes per launch /
               its average launch duration, measured with HIP events recorded around that kernel on the
               launch stream inside the timed region.
  cpu_baseline the CPU oracle (torch fp32, best thread count on the host) timed on a bounded sample of the same workload,
               with the B=1 and B=32 legs of BASELINE.md §3.2 and the host's lscpu model string.
  config4_fear_m_bf16  BASELINE configs[3]: synthetic deeper trunk (no reference definition), bf16 MFMA pointwise path, B=512.
  config5_train_step  BASELINE configs[4]: the whole network's training step (fwd in train mode + FEARLoss + bwd) per rank.
  latency_batch1  BASELINE configs[0] stand-in: the drop-in tracker's update() at batch 1 on the 480x256 demo-geometry clip
               (no H.264 decoder exists on the box, profiles/r02_box_probe.txt), ms/frame for the reference-style host crop
               path and for device crop + device post-processing, the CPU-oracle tracker beside it, boxes compared.

`python bench.py --gpus N` with N > 1 and no torch.distributed environment runs itself as a child under
torch.distributed.run (one rank per GPU, 127.0.0.1 rendezvous) and exits with its status; the driver's explicit torchrun launch
works as before.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 = fp32 vector rate
PEAK_HBM_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E spec peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (no sparsity)
FLOPS_PER_CROP = 922_787_840    # 2 x 461 393 920 MAC
BYTES_PER_CROP = 857_088        # compulsory fp32 bytes per crop
DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs: at most this much in all


def dump_outputs(out_dir: str, arrays: dict, limit: int = DUMP_LIMIT_BYTES) -> None:
    """--dump-outputs: write {name: array} as out_dir/<name>.npy.  The arrays share their first (crop) axis; when together they
    exceed `limit` bytes, the same fixed sample of crops (seed 0, in crop order) is written of each."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"--dump-outputs: {k} is {a.dtype}, not float32 / float64")
    n = next(iter(arrays.values())).shape[0]
    total = sum(a.nbytes for a in arrays.values())
    if total > limit:
        keep = max(1, n * limit // total)
        idx = np.sort(np.random.RandomState(0).choice(n, keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)


def norm_u8(u8_nchw: torch.Tensor) -> torch.Tensor:
    mean = torch.tensor([0.485, 0.456, 0.406], device=u8_nchw.device).view(1, 3, 1, 1) * 255.0
    inv = 1.0 / (torch.tensor([0.229, 0.224, 0.225], device=u8_nchw.device).view(1, 3, 1, 1) * 255.0)
    return (u8_nchw.float() - mean) * inv


def synth_batch(batch: int, rank: int):
    """Seeded synthetic crops: ONE generator stream, seed 0, sliced by rank — rank r owns the r-th block of
    (search crops, template crops) of that stream, so the N-GPU global batch is the concatenation of the blocks."""
    g = torch.Generator().manual_seed(0)
    for _ in range(rank + 1):
        search = torch.randint(0, 256, (batch, 3, 256, 256), dtype=torch.uint8, generator=g)
        tmpl = torch.randint(0, 256, (batch, 3, 128, 128), dtype=torch.uint8, generator=g)
    return search, tmpl


def _lscpu_model() -> str:
    try:
        import subprocess
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            if line.startswith("Model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def _cpu_node_worker(idx, cpus, threads, weights, seconds, q):
    """One of the node-level baseline's processes: the CPU oracle on `threads` threads pinned to `cpus`, batches of 8 of the
    same seeded synthetic crops, for ~`seconds`; reports (crops, elapsed)."""
    try:
        if cpus:
            os.sched_setaffinity(0, cpus)
    except Exception:      # noqa: BLE001 — affinity is an optimisation, not a requirement
        pass
    torch.set_num_threads(threads)
    from oracle.fear_oracle import OracleNet  # checker/baseline only
    net = OracleNet(weights)
    g = torch.Generator().manual_seed(idx)
    x = norm_u8(torch.randint(0, 256, (8, 3, 256, 256), dtype=torch.uint8, generator=g))
    z = net.get_features(norm_u8(torch.randint(0, 256, (8, 3, 128, 128), dtype=torch.uint8, generator=g)))
    net.track(x, z)
    q.put(("ready", idx))
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < seconds:
        net.track(x, z)
        n += 8
    q.put(("done", idx, n, time.perf_counter() - t0))


def cpu_quota_cpus():
    """CPUs' worth of CPU time the container may use (cgroup v2 cpu.max / v1 cfs quota), None when unlimited.  The GPU boxes of
    this pool show 256 logical CPUs of a shared 2x64-core host but cap the job at 16 (`cpu.max = 1600000 100000`,
    profiles/r03_box_cpu_probe.txt): more than 16 busy threads are throttled, which is why the oracle peaks at 16 threads."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:      # noqa: BLE001
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:      # noqa: BLE001
        return None


def cpu_node_baseline(weights, threads_per_proc: int = 16, seconds: float = 8.0):
    """The NODE's CPU throughput on this path (north_star: "timed on the node's host cores (count stated)"): one oracle
    process per `threads_per_proc` logical CPUs (the per-process optimum, tools/cpu_sweep.py), each pinned to its own block,
    all running the same bounded sample at once; value = the sum.  Bounded: ~`seconds` of wall clock plus process start-up."""
    import multiprocessing as mp
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except Exception:      # noqa: BLE001
        cpus = list(range(os.cpu_count() or 1))
    quota = cpu_quota_cpus()
    usable = len(cpus) if quota is None else max(1, min(len(cpus), int(quota)))
    nproc = max(1, usable // threads_per_proc)
    if quota is not None and quota < len(cpus):
        cpus = None                 # under a CPU-time quota pinning to fixed blocks only hurts: let the scheduler place the threads
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_cpu_node_worker, args=(i, set(cpus[i * threads_per_proc:(i + 1) * threads_per_proc]) if cpus else None,
                                                         threads_per_proc, weights, seconds, q)) for i in range(nproc)]
    t_start = time.perf_counter()
    for p in procs:
        p.start()
    done = []
    try:
        import queue as _queue
        deadline = time.perf_counter() + 300
        while len(done) < nproc:
            try:
                msg = q.get(timeout=2)
            except _queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or time.perf_counter() > deadline:
                    raise RuntimeError(f"cpu baseline workers failed (exit codes {dead})")
                continue
            if msg[0] == "done":
                done.append(msg)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    rates = [n / dt for _, _, n, dt in done]
    return {"value": float(sum(rates)), "unit": "crops/s", "processes": nproc, "threads_per_process": threads_per_proc,
            "cores": nproc * threads_per_proc, "host_cpus": os.cpu_count(), "cpu_quota_cpus": quota,
            "per_process_min_max": [min(rates), max(rates)],
            "sample": f"{sum(n for _, _, n, _ in done)} crops: {nproc} oracle processes x batches of 8 of the same synthetic 256x256 "
                      f"workload, {seconds:.0f} s each, all at once (wall {time.perf_counter() - t_start:.0f} s incl. start-up)"}


def cpu_baseline(search_u8, tmpl_u8, weights, budget_s: float = 10.0):
    """Oracle (kind='port') on the host cores, bounded sample.  `value` / `cores` = the whole NODE (one 16-thread oracle process
    per 16 logical CPUs, all at once: cpu_node_baseline); `single_process` = one process on its best thread count (batches of 8
    crops for ~budget_s) plus the two legs BASELINE.md §3.2 names — B=1 (20 warm-up + up to 100 timed calls) and B=32 — each
    bounded to a few seconds so that the default bench run stays within minutes."""
    from oracle.fear_oracle import OracleNet  # checker/baseline only, never on the product path
    # torch/oneDNN fp32 conv throughput on this graph peaks at ~16 threads on the 2x64-core EPYC host
    # (tools/cpu_sweep.py: 16 thr 93 crops/s, 32 thr 85, 64 thr 42, 128 thr 15); use the best setting.
    cores = min(16, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    net = OracleNet(weights)

    def leg(bs, warm, max_iters, budget):
        x = norm_u8(search_u8[:bs])
        z = net.get_features(norm_u8(tmpl_u8[:bs]))
        for _ in range(warm):
            net.track(x, z)
        t0 = time.perf_counter()
        it = 0
        while True:
            net.track(x, z)
            it += 1
            dt = time.perf_counter() - t0
            if dt > budget or it >= max_iters:
                return it * bs / dt, it, dt

    v8, it8, dt8 = leg(8, 1, 512, budget_s)
    v1, it1, dt1 = leg(1, 20, 100, 5.0)
    v32, it32, dt32 = leg(32, 1, 20, 6.0)
    single = {"value": v8, "unit": "crops/s", "cores": torch.get_num_threads(),
              "sample": f"{it8 * 8} crops (batches of 8) of the same synthetic 256x256 workload, torch fp32 oracle, {dt8:.1f}s",
              "batch1": {"value": v1, "unit": "crops/s", "ms_per_crop": 1e3 / v1, "iters": it1,
                         "protocol": "20 warm-up + <=100 timed calls (README.md:43, Benchmark.swift:55-77)"},
              "batch32": {"value": v32, "unit": "crops/s", "iters": it32, "seconds": dt32}}
    del net
    try:
        node = cpu_node_baseline(weights)
    except Exception as exc:      # noqa: BLE001 — the single-process number still stands
        node = {"error": f"{type(exc).__name__}: {exc}"}
    if "value" in node:
        return {"value": node["value"], "unit": "crops/s", "cores": node["cores"], "kind": "port", "host_cpus": os.cpu_count(),
                "cpu_quota_cpus": node.get("cpu_quota_cpus"),
                "cores_note": "cores = every CPU the job may use: the container's cgroup CPU quota when there is one (the host's "
                              "other logical CPUs belong to other tenants), else all logical CPUs, 16 oracle threads per process",
                "cpu_model": _lscpu_model(), "sample": node["sample"], "processes": node["processes"],
                "threads_per_process": node["threads_per_process"], "per_process_min_max": node["per_process_min_max"],
                "single_process": single}
    return dict(single, kind="port", host_cpus=os.cpu_count(), cpu_model=_lscpu_model(), node=node)


def config4_fear_m(dev, steps: int = 20, warmup: int = 5, batch: int = 512):
    """BASELINE.json configs[3]: "FEAR-M (deeper FBNet) bf16, batch=512 on 1xMI355X — MFMA pointwise-conv path".  The
    reference defines no FEAR-M (blocks.py:22-25), so this is the synthetic deeper trunk of tools/make_fear_m.py (every
    residual block of FEAR-XS twice, seeded random weights) — a perf/numerics configuration with no reference parity
    target; its parity target is this engine's own fp32 path on the same file (deviation reported here)."""
    from feartracker_amd import FEARNetHIP
    from feartracker_amd.hip_backend import WEIGHTS_FEAR_M
    net = FEARNetHIP(WEIGHTS_FEAR_M, device=dev.index, max_batch=batch)
    g = torch.Generator().manual_seed(4)
    search = norm_u8(torch.randint(0, 256, (batch, 3, 256, 256), dtype=torch.uint8, generator=g).to(dev)).contiguous()
    z = net.get_features(norm_u8(torch.randint(0, 256, (batch, 3, 128, 128), dtype=torch.uint8, generator=g).to(dev)).contiguous())
    bbox = torch.empty((batch, 4, 16, 16), dtype=torch.float32, device=dev)
    cls = torch.empty((batch, 1, 16, 16), dtype=torch.float32, device=dev)
    res = {}
    ref = None
    for mode, tag in ((0, "fp32"), (2, "bf16")):
        net.set_math(mode)
        for _ in range(warmup):
            net.track_maps(search, z, out=(bbox, cls))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            net.track_maps(search, z, out=(bbox, cls))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        res[tag] = {"value": batch / dt, "unit": "crops/s", "ms_per_step": 1e3 * dt}
        if mode == 2:
            # roofline of this configuration's dominant kernel: every launch bracketed with HIP events on the launch stream
            plan = net.plan(256, True)
            net.set_profile(True, op=-1)
            net.profile_reset()
            for _ in range(3):
                net.track_maps(search, z, out=(bbox, cls))
            torch.cuda.synchronize()
            prof = net.profile_read(256, True)
            net.set_profile(False)
            per_launch = [ms / max(cnt, 1) for ms, cnt in prof]
            per_step = [ms / 3 for ms, _ in prof]
            groups = {}
            for i, (nm, _, _) in enumerate(plan):
                groups[nm] = groups.get(nm, 0.0) + per_step[i]
            dom_name = max(groups, key=groups.get)
            di = [i for i, (nm, _, _) in enumerate(plan) if nm == dom_name][0]
            _, fl, by = plan[di]
            crops_per_launch = batch / max(prof[di][1] / 3, 1)
            t = per_launch[di] * 1e-3
            tf, gbs = fl * crops_per_launch / t / 1e12, by * crops_per_launch / t / 1e9
            ridge = PEAK_BF16_MFMA_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
            if fl / by >= ridge:
                roof = {"bound": "mfma", "achieved": tf, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_BF16_MFMA_TFLOPS}
            else:
                roof = {"bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS}
            tr, tr_file = pmc_traffic(dom_name, "fear_m")
            roof.update({"traffic": tr, "traffic_source": tr_file, "kernel": dom_name, "avg_launch_ms": per_launch[di],
                         "share_of_step": groups[dom_name] / max(sum(per_step), 1e-12),
                         "arithmetic_intensity_flop_per_byte": fl / by, "tflops_of_that_kernel": tf,
                         "frac_of_bf16_mfma_peak": tf / PEAK_BF16_MFMA_TFLOPS, "frac_of_hbm_peak": gbs / PEAK_HBM_GBS,
                         "sum_of_kernels_ms_per_step": sum(per_step),
                         "note": "bf16 operands on the matrix pipe (dense peak ~2.5 PFLOP/s): at this kernel's algorithmic intensity "
                                 "the bounding roofline is the one named in `bound`"})
            res["roofline"] = roof
        if ref is None:
            ref = (bbox[:32].clone(), cls[:32].clone())
            flops = sum(f for _, f, _ in net.plan(256, True))
        else:
            res[tag]["max_rel_dev_bbox_vs_fp32"] = float(((bbox[:32] - ref[0]).abs() / ref[0].abs()).max())
            res[tag]["max_abs_dev_cls_logit_vs_fp32"] = float((cls[:32] - ref[1]).abs().max())
            rc0, _, _ = net.decode(ref[1], ref[0])
            rc1, _, _ = net.decode(cls[:32], bbox[:32])
            res[tag]["argmax_cell_agreement_vs_fp32"] = float((rc0 == rc1).all(dim=1).float().mean())
    return {"workload": f"synthetic FEAR-M (tools/make_fear_m.py: FEAR-XS with every residual block twice, 28 IR blocks, "
                        f"{flops / 2e6:.0f} M MAC/crop, seeded random weights; NO reference definition), batch={batch}, 256x256 search",
            "metric": "search-region crops/sec", "dtype": "bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulate (FEAR_OPT_MATH=2); "
                                                         "depthwise / bias / residuals fp32",
            "value": res["bf16"]["value"], "unit": "crops/s", "steps": steps, "warmup": warmup,
            "tflops_bf16_path": res["bf16"]["value"] * flops / 1e12, "bf16": res["bf16"], "fp32_same_model": res["fp32"],
            "roofline": res.get("roofline")}


def config5_train_step(dev, batch: int = 128, steps: int = 20, warmup: int = 4):
    """BASELINE.json configs[4] ("training step: backbone+xcorr fwd/bwd, random-init, batch=1024 on 8xMI355X"): ONE data-parallel
    rank's share (1024 / 8 = 128 template/search pairs) of the full training step — FEARNet.forward((template, search)) in train
    mode (both crops through the trunk + neck, BatchNorm on batch statistics), FEARLoss, backward to all 195 parameter tensors —
    on the HIP operators of include/fear_train.h (feartracker_amd/train_net.py), random init, synthetic crops and targets.  With
    several ranks the gradients are averaged by one all-reduce of the flat 1.37 M-float buffer (not part of this 1-GPU number).
    Correctness: tests/test_train_head.py (every gradient vs autograd; the head additionally vs the reference's own classes).
    The trunk runs block-fused (one C-ABI call per inverted-residual block and direction, csrc/fear_train_block.h), the template
    pass and the regression tower on a second HIP stream; DESIGN.md §7 N3 has the per-kernel map."""
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    torch.cuda.empty_cache()          # (the other configurations' buffers: the step allocates ~13 GB of saved activations per call)
    g = torch.Generator().manual_seed(7)
    net = FEARNetTrainHIP(random_init_state(3), device=dev.index)
    tmpl = torch.randn(batch, 3, 128, 128, generator=g).to(dev)
    srch = torch.randn(batch, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(batch, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(batch, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(batch, 16, 16, generator=g) > 0.9).float().to(dev)
    for _ in range(warmup):
        out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
    host_issue_ms = 1e3 * (time.perf_counter() - t0) / steps      # the host's share: the step is GPU-bound while this stays below ms_per_step
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    # the optimiser update of the reference (Adam, lr 1e-4) on the same parameters, timed on its own (not part of "fwd/bwd")
    from feartracker_amd.optim import AdamHIP
    opt = AdamHIP(net)
    opt.step(out["grads"])
    torch.cuda.synchronize()
    ta = time.perf_counter()
    for _ in range(steps):
        opt.step(out["grads"])
    torch.cuda.synchronize()
    adam_ms = 1e3 * (time.perf_counter() - ta) / steps
    # a stand-alone measurement of one pointwise weight gradient (NOT the step's roofline: kept under its own key) — the heaviest
    # shape of the step, dW[672][112] over the 32 768 rows of the 16 x 16 maps, through the C-ABI operator the layer-wise step calls
    # (the block-fused step runs the same GEMM with the BatchNorm backward formed on its dY operand)
    from feartracker_amd.train_head import _p
    lib = net.lib
    Mw, Kw, Nw = batch * 256, 112, 672
    gw = torch.Generator().manual_seed(11)
    dyw, xw = torch.randn(Mw, Nw, generator=gw).to(dev), torch.randn(Mw, Kw, generator=gw).to(dev)
    dww = torch.empty(Nw, Kw, device=dev)
    wsw = torch.empty(int(lib.fear_train_workspace_bytes(Mw, 672)) // 4 + 1024, device=dev)
    reps = 20
    call = lambda: lib.fear_pw_backward_weight(_p(dyw), Nw, _p(xw), Kw, _p(dww), _p(wsw), wsw.numel() * 4, Mw, Kw, Nw, None)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record()
    torch.cuda.synchronize()
    wg_ms = e0.elapsed_time(e1) / reps          # (includes the fixed-order slice sum that follows every launch)
    wg_bytes = 4.0 * (Mw * Nw + Mw * Kw + Nw * Kw)
    wg_flops = 2.0 * Mw * Nw * Kw
    micro = {"operator": "fear_pw_backward_weight", "shape": f"dW[{Nw}][{Kw}] = sum over {Mw} rows", "avg_call_ms": wg_ms,
             "tflops": wg_flops / (wg_ms * 1e-3) / 1e12, "frac_of_fp32_peak": wg_flops / (wg_ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
             "algorithmic_gbs": wg_bytes / (wg_ms * 1e-3) / 1e9,
             "note": "random operands, one shape, without the fused BatchNorm-backward operand of the block-fused step"}
    # the step's own roofline: the whole step against both roofs (live time; FLOPs from the model, bytes from the committed PMC
    # passes of the same step), and the symbol with the largest share of its kernel time under its real name with its PMC bytes per
    # launch (profiles/rNN_train_traffic.txt: kernel trace + FETCH_SIZE / WRITE_SIZE passes of tools/train_prof.py)
    prof = train_profile()
    step_flops = 3 * 2 * (461_393_920 + 75_970_000) * batch
    whole_frac_fp32 = step_flops / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS
    whole_frac_hbm = (prof["pmc_gb_per_step"] / dt / PEAK_HBM_GBS) if prof else None
    if prof:
        d = prof["dominant"]
        train_roof = {"bound": "hbm", "achieved": d["achieved_gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": d["achieved_gbs"] / PEAK_HBM_GBS,
                      "traffic": d["traffic_bytes_per_launch"], "kernel": d["kernel"], "avg_launch_ms": d["avg_launch_us"] * 1e-3,
                      "calls_per_step": d["calls_per_step"], "share_of_kernel_time": d["ms_per_step"] / max(prof["kernel_ms_per_step"], 1e-9),
                      "source": prof["file"],
                      "note": "the symbol with the largest share of the step's kernel time; duration and bytes are the profiled step's "
                              "(rocprofv3 kernel trace and PMC passes of tools/train_prof.py, three streams in flight: the average duration "
                              "is an upper bound) — `achieved` = PMC bytes per launch / that duration.  The step as a whole is bound by "
                              "neither roof: see whole_step_*"}
    else:
        train_roof = None
    del dyw, xw, dww, wsw
    fwd_macs = 461_393_920 + 75_970_000           # search path + template path, forward MACs per pair
    nparams = sum(v.numel() for v in out["grads"].values())
    loss_vals = [float(out["loss_cls"]), float(out["loss_reg"])]
    ngrads = len(out["grads"])
    peak_gb = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    mode_name, two = net.mode, bool(net.two_streams)
    adam_launches = 1 if getattr(net, "param_flat", None) is not None else ngrads
    del out, opt, net
    torch.cuda.empty_cache()
    with _c_stdout_to_stderr():       # (RCCL prints its version banner to stdout from C: the line this script prints must stay the only one)
        sync_one = sync_bn_one_rank_ms(dev, batch, max(steps // 2, 3), 2, (tmpl, srch, gt_reg, gt_cls, gt_w))
    return {"workload": f"FEARNet training step (trunk + neck on both crops, correlation head, FEARLoss; forward in train mode + "
                        f"backward), batch={batch} pairs per rank (configs[4]: 1024 over 8 ranks), fp32, random init, synthetic data",
            "value": batch / dt, "unit": "pairs/s per GPU", "ms_per_step": 1e3 * dt, "steps": steps, "warmup": warmup,
            "approx_tflops": 3 * 2 * fwd_macs * batch / dt / 1e12,
            "loss": loss_vals, "dtype": "f32",
            "parameter_tensors_with_gradients": ngrads, "parameters": nparams, "adam_update_ms": adam_ms, "roofline": train_roof,
            "whole_step_frac_of_fp32_peak": whole_frac_fp32, "whole_step_hbm_frac": whole_frac_hbm,
            "whole_step_pmc_gb": prof["pmc_gb_per_step"] if prof else None, "launches_per_step": prof["launches_per_step"] if prof else None,
            "wgrad_microbenchmark": micro, "sync_bn_one_rank_ms": sync_one["ms_per_step"], "sync_bn_one_rank": sync_one,
            "host_issue_ms_per_step": host_issue_ms, "trunk_implementation": mode_name, "adam_launches": adam_launches,
            "two_streams": two, "peak_memory_gb": peak_gb}


def clocks_under_load(step_fn, steps: int = 300):
    """Shader clock and socket power while the GPU is busy with the bench's own step (boxes of this pool differ by ~7 % in
    throughput at an unchanged kernel mix; the roofline peak is quoted at 2.4 GHz): enqueue `steps` steps, read rocm-smi while
    they run.  Never fails the bench: any problem gives None."""
    import re
    import subprocess
    try:
        for _ in range(steps):
            step_fn()
        res = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        card = next(iter(json.loads(res.stdout).values()))
        mhz = lambda k: int(re.search(r"(\d+)", card.get(k, "")).group(1)) if re.search(r"(\d+)", card.get(k, "")) else None
        power = next((float(v) for k, v in card.items() if "Power" in k), None)
        return {"sclk_mhz": mhz("sclk clock speed:"), "mclk_mhz": mhz("mclk clock speed:"), "socket_power_w": power,
                "source": "rocm-smi while the step loop runs"}
    except Exception:      # noqa: BLE001
        try:
            torch.cuda.synchronize()
        except Exception:  # noqa: BLE001
            pass
        return None


def config5_train_step_ddp(dev, world: int, batch: int = 128, steps: int = 3, warmup: int = 1):
    """BASELINE configs[4] with its data parallelism: every rank runs the training step on its own 128 pairs with
    SyncBatchNorm (the reference's multi-GPU setting, config/backend/*.yaml), the gradients are averaged by ONE RCCL all-reduce
    of the flat buffer, Adam updates the parameters.  Whole-job pairs/s over all ranks (max step time over ranks)."""
    import torch.distributed as dist
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    g = torch.Generator().manual_seed(70 + dist.get_rank())
    net = FEARNetTrainHIP(random_init_state(3), device=dev.index, sync_bn=True)
    opt = AdamHIP(net)
    tmpl = torch.randn(batch, 3, 128, 128, generator=g).to(dev)
    srch = torch.randn(batch, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(batch, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(batch, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(batch, 16, 16, generator=g) > 0.9).float().to(dev)

    def one():
        out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        opt.step(net.allreduce_gradients(out["grads"]))
        return out
    for _ in range(warmup):
        out = one()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = one()
    dist.barrier()
    torch.cuda.synchronize()
    t = torch.tensor([(time.perf_counter() - t0) / steps], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    return {"workload": f"FEARNet training step, data parallel over {world} rank(s): {batch} pairs per rank (global batch {world * batch}), "
                        "SyncBatchNorm, one all-reduce of the flat gradient buffer, Adam; fp32, random init, synthetic data",
            "value": world * batch / dt, "unit": "pairs/s (all ranks)", "ms_per_step": 1e3 * dt, "steps": steps, "ranks": world,
            "sync_bn": True, "loss": [float(out["loss_cls"]), float(out["loss_reg"])]}


def latency_batch1(weights, frames_cap: int = 120):
    """BASELINE configs[0] / SURVEY §8d config 1 at batch 1: `initialize` + `update` per frame through the drop-in tracker on
    the 480x256 demo-geometry clip (tests/clipgen.py: the init box of demo_video.py:45-46; assets/test.mp4 itself cannot be
    decoded on this box).  Host-crop path (what the reference config runs), device crop + device post-processing
    (fear_crop_normalize + fear_track + fear_decode), and the CPU-oracle tracker on the same frames."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from clipgen import DEMO_INIT_BBOX, demo_clip
    from feartracker_amd import DEFAULT_TRACKING_CONFIG, FEARNetHIP, FEARTracker
    from feartracker_amd import geometry as geo
    frames, _ = demo_clip(frames_cap)
    init = np.array(DEMO_INIT_BBOX)
    net = FEARNetHIP(weights, device=torch.cuda.current_device(), max_batch=1)

    def loop(trk, sync, split):
        t = dict(crop=0.0, pre_h2d=0.0, net=0.0, post=0.0, total=0.0)
        boxes = []
        for rep in range(2):                          # first pass = warm-up
            trk.initialize(frames[0], init.copy())
            cfg, st = trk.tracking_config, trk.tracking_state
            for f in frames[1:]:
                t0 = time.perf_counter()
                if split:
                    crop, box_in_crop, ctx = geo.get_extended_crop(f, st.bbox, cfg["instance_size"], cfg["search_context"],
                                                                   padding_value=st.mean_color)
                    st.mapping, st.prev_size = ctx, box_in_crop[2:]
                    t1 = time.perf_counter()
                    x = trk._preprocess_image(crop, trk._search_transform)
                    sync()
                    t2 = time.perf_counter()
                    out = trk.net.track(x, trk._template_features)
                    sync()
                    t3 = time.perf_counter()
                    pred, _ = trk._postprocess(out)
                    pred = geo.clamp_bbox(trk._rescale_bbox(pred, st.mapping), f.shape)
                    st.bbox = pred
                    st.paths.append(pred)
                    t4 = time.perf_counter()
                    if rep:
                        t["crop"] += t1 - t0; t["pre_h2d"] += t2 - t1; t["net"] += t3 - t2; t["post"] += t4 - t3
                else:
                    pred = trk.update(f)["bbox"]
                    sync()
                    t4 = time.perf_counter()
                if rep:
                    t["total"] += t4 - t0
                    boxes.append(np.array(pred))
        n = len(frames) - 1
        return {k: 1e3 * v / n for k, v in t.items() if v > 0}, np.stack(boxes)

    sync = torch.cuda.synchronize
    host_ms, host_boxes = loop(FEARTracker(net, cuda_id=torch.cuda.current_device(),
                                           **dict(DEFAULT_TRACKING_CONFIG, device_crop=False, device_postprocess=False)), sync, True)
    dev_ms, dev_boxes = loop(FEARTracker(net, cuda_id=torch.cuda.current_device(),
                                         **dict(DEFAULT_TRACKING_CONFIG, device_crop=True, device_postprocess=True)), sync, False)
    # a 1920x1080 leg: the same tracker on full-HD frames (the demo clip tiled 4 x 4.2 to 1080p, the init box moved with it):
    # the per-frame cost of a LARGE frame — host mean colour at initialize, context geometry, the upload of the context
    # rectangle only (hip_backend.crop_normalize), crop + net + decode on the device
    reps = (-(-1080 // frames.shape[1]), -(-1920 // frames.shape[2]))
    big = np.ascontiguousarray(np.tile(frames[:31], (1, reps[0], reps[1], 1))[:, :1080, :1920])
    big_init = init.copy()
    trk_hd = FEARTracker(net, cuda_id=torch.cuda.current_device(), **dict(DEFAULT_TRACKING_CONFIG, device_crop=True, device_postprocess=True))
    hd = {}
    for rep in range(2):
        trk_hd.initialize(big[0], big_init.copy())
        sync()
        t0 = time.perf_counter()
        ctx_px = 0
        for f in big[1:]:
            trk_hd.update(f)
            ctx_px += int(trk_hd.tracking_state.mapping[2]) * int(trk_hd.tracking_state.mapping[3])
        sync()
        hd = {"total": 1e3 * (time.perf_counter() - t0) / (len(big) - 1), "frames": len(big) - 1, "frame_shape": list(big[0].shape),
              "frame_bytes": int(big[0].nbytes), "mean_context_pixels": ctx_px // (len(big) - 1),
              "uploaded": "frame ∩ context rectangle per update (not the 6.2 MB frame)"}
    del big
    # the network alone: one search crop + resident template features per fear_track call, calls back to back on one stream
    xs = torch.randn(1, 3, 256, 256, device="cuda")
    zs = net.get_features(torch.randn(1, 3, 128, 128, device="cuda"))
    for _ in range(50):
        net.track_maps(xs, zs)
    sync()
    t0 = time.perf_counter()
    for _ in range(500):
        net.track_maps(xs, zs)
    sync()
    track_call_ms = 1e3 * (time.perf_counter() - t0) / 500
    from oracle.fear_oracle import OracleNet  # CPU baseline leg only
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ncpu = min(len(frames), 41)
    frames_all, frames = frames, frames[:ncpu]
    cpu_ms, cpu_boxes = loop(FEARTracker(OracleNet(weights), cuda_id="cpu", **DEFAULT_TRACKING_CONFIG), lambda: None, True)
    frames = frames_all
    return {"unit": "ms/frame", "frames": len(frames) - 1, "frame_shape": list(frames[0].shape), "clip": "tests/clipgen.demo_clip "
            "(480x256, init box [163,53,45,174]; assets/test.mp4 not decodable here: no H.264 decoder)",
            "host_crop_path": host_ms, "device_crop_and_postprocess": dev_ms, "device_path_1920x1080": hd,
            "track_call_batch1_ms": track_call_ms, "track_call_plan_ops": len(net.plan(256, True)),
            "device_boxes_identical_to_host_path": bool(np.array_equal(dev_boxes, host_boxes)),
            "cpu_oracle_tracker": dict(cpu_ms, frames=ncpu - 1, threads=torch.get_num_threads()),
            "boxes_identical_to_cpu_oracle": bool(np.array_equal(host_boxes[:ncpu - 1], cpu_boxes))}


def pmc_traffic(op_name: str, tag: str = ""):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of this same
    command (profiles/rNN_traffic.json via tools/pmc_to_traffic.py; op -> kernel symbol via rNN_per_op.csv).
    PMC counters cannot be collected from inside the timed run, so this is the offline measurement or null."""
    import csv
    import glob
    try:
        suf = f"_{tag}" if tag else ""
        pick = lambda pat: sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", pat))
                                  if tag or not any(t in os.path.basename(f) for t in ("_fear_m_", "_train_")))[-1]
        per_op = pick(f"r*{suf}_per_op.csv")
        traffic = pick(f"r*{suf}_traffic.json")
        # both files must come from the same profiling round: a traffic file older than the newest per-op table describes
        # kernels that may no longer exist (or their predecessors of the same name) — no number is better than a stale one
        rnd = lambda f: os.path.basename(f).split("_")[0]
        if rnd(per_op) != rnd(traffic):
            return None, None
        sym = None
        with open(per_op) as fh:
            for r in csv.DictReader(fh):
                if r["name"] == op_name:
                    sym = r["kernel"]
                    break
        t = json.load(open(traffic))
        return (t[sym]["traffic_bytes_per_launch"], os.path.relpath(traffic, ROOT)) if sym in t else (None, None)
    except Exception:
        return None, None


def train_profile():
    """The training step's committed profile (profiles/rNN_train_traffic.txt, written by tools/train_traffic.py from the kernel
    trace and the two PMC passes of tools/train_prof.py 128 ... block): per-step totals and the symbol with the largest share of
    the kernel time, under its real name, with its PMC bytes per launch.  None when there is no such file."""
    import glob
    import re
    try:
        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_train_traffic.txt")))[-1]
        txt = open(f).read()
        m = re.search(r"per step: ([0-9.]+) GB of PMC traffic.*?, ([0-9]+) launches, ([0-9.]+) ms of kernel time", txt)
        rows = re.findall(r"^\s*([0-9.]+)\s+(\S.*?)\s+([0-9]+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s*$", txt, re.M)
        if not m or not rows:
            return None
        ms, name, calls, avg_us, mb, tbs = rows[0]
        return {"file": os.path.relpath(f, ROOT), "pmc_gb_per_step": float(m.group(1)), "launches_per_step": int(m.group(2)),
                "kernel_ms_per_step": float(m.group(3)),
                "dominant": {"kernel": name.strip(), "ms_per_step": float(ms), "calls_per_step": int(calls), "avg_launch_us": float(avg_us),
                             "traffic_bytes_per_launch": float(mb) * 1e6, "achieved_gbs": float(tbs) * 1e3}}
    except Exception:      # noqa: BLE001
        return None


def sync_bn_one_rank_ms(dev, batch, steps, warmup, data):
    """The same training step as FEARNetTrainHIP(mode="block", sync_bn=True) in a torch.distributed group of the ONE rank a 1-GPU
    run has: every BatchNorm's sums go through the library's all-reduce hook and RCCL (the reference's multi-GPU backends train
    with sync_bn: True, config/backend/2gpu.yaml:5).  Best effort: None if no process group can be made here."""
    import socket
    import torch.distributed as dist
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    made = False
    try:
        if not dist.is_initialized():
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
            made = True
        net = FEARNetTrainHIP(random_init_state(3), device=dev.index, sync_bn=True)
        for _ in range(warmup):
            net.step(*data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            net.step(*data)
        torch.cuda.synchronize()
        return {"ms_per_step": 1e3 * (time.perf_counter() - t0) / steps, "trunk_implementation": net.mode, "two_streams": bool(net.two_streams),
                "ranks": dist.get_world_size()}
    except Exception as exc:      # noqa: BLE001
        return {"ms_per_step": None, "error": f"{type(exc).__name__}: {exc}"[:200]}
    finally:
        if made:
            try:
                dist.destroy_process_group()
            except Exception:      # noqa: BLE001
                pass


@contextlib.contextmanager
def _c_stdout_to_stderr():
    import ctypes
    libc = ctypes.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256, help="search crops per GPU per step")
    ap.add_argument("--max-batch", type=int, default=int(os.environ.get("FEAR_MAX_BATCH", "256")),
                    help="crops per internal engine pass (workspace / cache footprint)")
    ap.add_argument("--math", type=int, default=int(os.environ.get("FEAR_MATH", "0")), choices=[0, 1],
                    help="0: fp32 MFMA (exact fp32, default); 1: fp16 hi+lo split operands on the matrix pipe, fp32 accumulate")
    ap.add_argument("--dual-head", action="store_true", help="A/B: the head's two branches on two streams (FEAR_OPT_DUAL_HEAD)")
    ap.add_argument("--head-stagger", type=int, default=int(os.environ.get("FEAR_HEAD_STAGGER", "-1")),
                    help="A/B: microseconds the head's second branch is held back behind the first (two streams); -1 = the engine's default")
    ap.add_argument("--no-tile-v4", action="store_true", help="A/B: every tiled block on ir_tile_v2 (no phase-overlapped kernel)")
    ap.add_argument("--no-head-chain", action="store_true", help="A/B: the BoxTower as eight sep16 launches instead of one headchain launch")
    ap.add_argument("--no-e1-pair", action="store_true", help="A/B: the two 24-channel e1 blocks as one tile-kernel launch each instead of one e1pair launch")
    ap.add_argument("--chain32", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="A/B (FEAR_OPT_CHAIN32): the 32 x 32 stage as four tile launches (0), a chain launch of its own (1), one launch with "
                         "the stride-16 stage + neck (2, the engine's default); -1: leave the default")
    ap.add_argument("--no-chain", action="store_true", help="A/B: one fused kernel per stride-16 block instead of the chain kernel")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-math", action="store_true",
                    help="skip the supplementary run in the other arithmetic mode (profiling runs: keeps the trace to one plan)")
    ap.add_argument("--dump-ops", action="store_true", help="print the per-kernel time table to stderr")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 tracker latency object")
    ap.add_argument("--train-ddp", action="store_true", help="multi-GPU: also time the data-parallel training step (SyncBatchNorm, "
                    "gradient all-reduce, Adam) -> config5_train_step_data_parallel")
    ap.add_argument("--no-overlap", action="store_true", help="multi-GPU: blocking all-gather inside the step instead of the "
                    "double-buffered collective that overlaps the next batch")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the two-handles-on-two-streams supplementary number")
    ap.add_argument("--no-train", action="store_true", help="skip the BASELINE configs[4] object (head training step, first slice)")
    ap.add_argument("--no-fear-m", action="store_true", help="skip the BASELINE configs[3] object (synthetic FEAR-M, bf16, B=512)")
    ap.add_argument("--full", action="store_true", help="also every supplementary measurement: the per-kernel profile and roofline "
                    "(HIP events in the warm-up and timed steps), then CPU baseline, other math mode, two-stream numbers, configs[3] / "
                    "[4], batch-1 latency, ...; the --no-* flags above switch single legs off.  Off: set-up, warm-up, the timed steps "
                    "and the headline line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the maps of the last timed step as DIR/bbox.npy and DIR/cls.npy (fp32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: run N ranks (one per GPU) under torch.distributed.run on this node, as a child
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus} needs {args.gpus} GPUs on this node, {have} visible")
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        raise SystemExit(subprocess.run(cmd).returncode)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (no CPU fallback on the product path)"
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    # FEAR_BENCH_FORCE_DIST=1 takes the distributed code path (RCCL process group, barriers, all-gather) with a single rank
    # too: the only way to exercise it on a one-GPU box
    use_dist = world > 1 or os.environ.get("FEAR_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL prints a version banner through C stdio on STDOUT when the first communicator comes up; stdout must carry
        # exactly one JSON line, so fd 1 points at stderr while the communicator is created (and libc's buffer is flushed
        # there before fd 1 is restored)
        # RCCL's own account of the communicator (its INIT lines carry "rank r nranks N") goes to STDERR, next to ours below,
        # so that a driver log shows N ranks the day a multi-GPU node runs this
        # (RCCL logs to a per-process FILE: at INFO level it writes to stdout from its own threads at times of its choosing, and
        # stdout must carry exactly one JSON line; the lines that name the communicator are relayed to stderr below)
        rccl_log = f"/tmp/fear_bench_rccl.{os.getpid()}.log"
        os.environ.setdefault("NCCL_DEBUG", "INFO")
        os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT")
        os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
        with _c_stdout_to_stderr():
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            dist.barrier()
            torch.cuda.synchronize()
        print(f"[bench] rank {dist.get_rank()} of {dist.get_world_size()} (torch.distributed, backend {dist.get_backend()}) on "
              f"cuda:{local_rank} = {torch.cuda.get_device_name(local_rank)}", file=sys.stderr, flush=True)
        try:
            with open(os.environ["NCCL_DEBUG_FILE"]) as fh:
                for line in fh:
                    if "nranks" in line or "Init COMPLETE" in line or "RCCL version" in line:
                        print(f"[bench] RCCL: {line.strip()}", file=sys.stderr, flush=True)
        except OSError:
            pass

    from feartracker_amd import FEARNetHIP, DEFAULT_WEIGHTS
    from feartracker_amd.sharding import OverlappedGather, gather_packed

    B = args.batch
    net = FEARNetHIP(DEFAULT_WEIGHTS, device=local_rank, max_batch=args.max_batch)
    net.set_math(args.math)
    if args.no_chain:
        net.set_chain(False)
    if args.dual_head:
        net.set_dual_head(True)
    if args.head_stagger >= 0:
        net.set_head_stagger(args.head_stagger)
    if args.no_tile_v4:
        net.set_tile_v4(False)
    if args.no_head_chain:
        net.set_head_chain(False)
    if args.no_e1_pair:
        net.set_e1_pair(False)
    if args.chain32 >= 0:
        net.set_chain32(args.chain32)
    search_u8, tmpl_u8 = synth_batch(B, rank)
    search = norm_u8(search_u8.to(dev)).contiguous()
    tmpl_feats = net.get_features(norm_u8(tmpl_u8.to(dev)).contiguous())
    packed = torch.empty((B, 5, 16, 16), dtype=torch.float32, device=dev)
    bbox = torch.empty((B, 4, 16, 16), dtype=torch.float32, device=dev)
    cls = torch.empty((B, 1, 16, 16), dtype=torch.float32, device=dev)
    gathered = torch.empty((world * B, 5, 16, 16), dtype=torch.float32, device=dev) if use_dist else None
    # the all-gather of batch i travels over xGMI while batch i+1 computes (two send/receive slots); --no-overlap keeps the
    # blocking collective in the step for an A/B
    overlap = OverlappedGather(B, 16, device=dev) if use_dist and not args.no_overlap else None

    def step():
        if overlap is not None:
            # the engine writes (bbox | cls) straight into the packed send buffer: the step is its kernels + ONE collective
            net.track_packed(search, tmpl_feats, out=overlap.slot())
            overlap.launch()
        elif use_dist:
            net.track_packed(search, tmpl_feats, out=packed)
            gather_packed(packed, gathered)
        else:
            net.track_maps(search, tmpl_feats, out=(bbox, cls))

    def barrier():
        if overlap is not None:
            overlap.finish()               # every collective of the timed region has completed before the clock stops
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # warm-up; with --full (or --dump-ops) the first warm-up steps run with every kernel bracketed to find the dominant one
    n_prof = min(3, max(1, args.warmup)) if (args.full or args.dump_ops) else 0
    if n_prof:
        net.set_profile(True, op=-1)
        net.profile_reset()
        for _ in range(n_prof):
            step()
        torch.cuda.synchronize()
        plan = net.plan(256, True)
        prof = net.profile_read(256, True)
        net.set_profile(False)
        per_op = [(ms / max(cnt, 1), cnt) for ms, cnt in prof]
        launches_per_step = [cnt / n_prof for _, cnt in prof]
        op_time = [per_op[i][0] * launches_per_step[i] for i in range(len(plan))]
        # ops with the same name run the same kernel symbol on the same shape (what rocprofv3 --stats groups):
        # the dominant kernel is the name group with the largest share of the step
        group_time = {}
        for i, (nm, _, _) in enumerate(plan):
            group_time[nm] = group_time.get(nm, 0.0) + op_time[i]
        dom_name = max(group_time, key=group_time.get)
        dom_ops = [i for i, (nm, _, _) in enumerate(plan) if nm == dom_name]
        dom = dom_ops[0]
        if args.dump_ops and rank == 0:
            tot = sum(op_time)
            for i, (name, fl, by) in enumerate(plan):
                crops_per_launch = B / max(launches_per_step[i], 1)
                t = per_op[i][0]
                print(f"{i:3d} {name:28s} {op_time[i]:8.3f} ms/step {100 * op_time[i] / tot:5.1f}%  "
                      f"{fl * crops_per_launch / (t * 1e-3) / 1e12 if t else 0:7.2f} TF/s "
                      f"{by * crops_per_launch / (t * 1e-3) / 1e9 if t else 0:8.1f} GB/s", file=sys.stderr)
            print(f"sum of kernels {tot:.3f} ms/step", file=sys.stderr)
    for _ in range(max(0, args.warmup - n_prof)):
        step()

    # timed region; with --full only the dominant kernel is bracketed with HIP events (2 events per launch), a plain run
    # brackets nothing
    if args.full:
        net.profile_reset()
        net.set_profile(True, op=dom)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.full:
        net.set_profile(False)
        reads = net.profile_read(256, True)
        dom_ms = sum(reads[i][0] for i in dom_ops)
        dom_cnt = sum(reads[i][1] for i in dom_ops)

    # what the last timed step returned to its caller: the global batch's maps (the gathered packed maps with N > 1), written
    # out before any supplementary leg of --full reuses the buffers
    if args.dump_outputs and rank == 0:
        if use_dist:
            maps = overlap.finish() if overlap is not None else gathered
            dump_outputs(args.dump_outputs, {"bbox": maps[:, :4].cpu().numpy(), "cls": maps[:, 4:].cpu().numpy()})
        else:
            dump_outputs(args.dump_outputs, {"bbox": bbox.cpu().numpy(), "cls": cls.cpu().numpy()})

    gather_ms = None
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if use_dist and args.full:
        # the collective alone (outside the timed region): K all-gathers of the packed maps, barrier-bracketed
        barrier()
        tg = time.perf_counter()
        for _ in range(args.steps):
            gather_packed(packed, gathered)
        barrier()
        gather_ms = 1e3 * (time.perf_counter() - tg) / args.steps

    clocks = clocks_under_load(step) if (args.full and rank == 0 and not use_dist) else None

    # supplementary: the same K steps dealt alternately to TWO engine handles on two HIP streams (each step is still one whole
    # batch of B crops through one handle; consecutive independent batches overlap, so one batch's kernel tails are filled by
    # the other's kernels).  What a serving loop with two batches in flight gets; never `value`.
    elapsed_pipe = None
    if args.full and not args.no_pipelined and not use_dist:
        net_b = FEARNetHIP(DEFAULT_WEIGHTS, device=local_rank, max_batch=args.max_batch)
        net_b.set_math(args.math)
        bbox_b, cls_b = torch.empty_like(bbox), torch.empty_like(cls)
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        lanes = [(net, bbox, cls), (net_b, bbox_b, cls_b)]

        def pipelined(k):
            for i in range(k):
                nn, bb, cc = lanes[i & 1]
                with torch.cuda.stream(streams[i & 1]):
                    nn.track_maps(search, tmpl_feats, out=(bb, cc))
        torch.cuda.synchronize()
        pipelined(max(4, args.warmup // 2))
        torch.cuda.synchronize()
        tp = time.perf_counter()
        pipelined(args.steps)
        torch.cuda.synchronize()
        elapsed_pipe = time.perf_counter() - tp
        same = bool(torch.equal(bbox, bbox_b) and torch.equal(cls, cls_b))
        del net_b, lanes
        torch.cuda.empty_cache()

    # supplementary: the same K steps with FEAR_OPT_SPLIT_STREAMS (each call issued as two half-batches on two streams of the SAME
    # handle, joined before the call returns to its stream; bit-identical maps — tests/test_gpu_parity.py).  A serving option: `value`
    # stays the single-stream number so that every per-kernel figure of this line is a full-grid launch.
    elapsed_split = None
    if args.full and not args.no_pipelined and not use_dist:
        net.set_split_streams(True)
        for _ in range(max(4, args.warmup // 2)):
            net.track_maps(search, tmpl_feats, out=(bbox, cls))
        torch.cuda.synchronize()
        tp = time.perf_counter()
        for _ in range(args.steps):
            net.track_maps(search, tmpl_feats, out=(bbox, cls))
        torch.cuda.synchronize()
        elapsed_split = time.perf_counter() - tp
        net.set_split_streams(False)

    # the same K steps in the other arithmetic mode (supplementary number, same protocol)
    other = 1 - args.math
    elapsed_other = None
    if args.full and not args.no_other_math:
        net.set_math(other)
        for _ in range(max(3, args.warmup // 2)):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        elapsed_other = time.perf_counter() - t1
    if use_dist and elapsed_other is not None:
        t = torch.tensor([elapsed_other], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_other = float(t.item())
    net.set_math(args.math)
    if args.no_chain:
        net.set_chain(False)

    # configs[4] with its data parallelism — opt-in (--train-ddp): a rank that failed alone inside it would leave the others
    # waiting in a collective, and the default multi-GPU run must produce its line whatever happens to a side measurement
    ddp_train = None
    if use_dist and args.train_ddp:
        try:
            torch.cuda.empty_cache()
            ddp_train = config5_train_step_ddp(dev, world)
        except Exception as exc:      # noqa: BLE001 — reported in the JSON line instead
            ddp_train = {"error": f"{type(exc).__name__}: {exc}"}
        torch.cuda.empty_cache()

    if rank == 0:
        total_crops = world * B * args.steps
        value = total_crops / elapsed
        if args.full:
            name, fl, by = plan[dom]
            avg_ms = dom_ms / max(dom_cnt, 1)
            crops_per_launch = B * args.steps * len(dom_ops) / max(dom_cnt, 1)
            ai = fl / by
            ridge = PEAK_FP32_MFMA_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
            if ai >= ridge:
                achieved = fl * crops_per_launch / (avg_ms * 1e-3) / 1e12
                roof = {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": achieved / PEAK_FP32_MFMA_TFLOPS}
            else:
                achieved = by * crops_per_launch / (avg_ms * 1e-3) / 1e9
                roof = {"bound": "hbm", "achieved": achieved, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": achieved / PEAK_HBM_GBS}
            traffic, traffic_file = pmc_traffic(name)
            roof.update({"traffic": traffic, "traffic_source": (f"offline PMC: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                                                                f"command, committed as {traffic_file} (not measured in this run)")
                                                               if traffic is not None else None,
                         "kernel": name, "avg_launch_ms": avg_ms, "launches": dom_cnt,
                         "launches_per_step": len(dom_ops) * max(1, -(-B // args.max_batch)),
                         "share_of_step": group_time[dom_name] / max(sum(op_time), 1e-12),
                         "whole_path_tflops": value * FLOPS_PER_CROP / 1e12 / world,
                         "whole_path_frac_of_fp32_peak": value * FLOPS_PER_CROP / 1e12 / world / PEAK_FP32_MFMA_TFLOPS})
        out = {
            "metric": "search-region crops/sec (FEAR-XS 256x256)",
            "value": value,
            "unit": "crops/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"FEAR-XS track(): batch={B} synthetic 256x256 search / 128x128 template crops per GPU, fp32"
                                   + (f", sharded over {world} GPUs + 1 RCCL all-gather of (B,5,16,16) maps" if world > 1 else ""),
                       "batch_per_gpu": B, "global_batch": world * B, "weights": "FEAR-XS-NoEmbs (fp16 values upcast to fp32)",
                       "engine_pass": args.max_batch, "parallelism": f"dp{world}",
                       "math": ("fp32 MFMA (v_mfma_f32_16x16x4_f32), exact fp32" if args.math == 0 else
                                "pointwise convs of the fused 16x16 blocks: fp32 activations split into fp16 hi+lo, exact-fp16 "
                                "weights, v_mfma_f32_16x16x32_f16, fp32 accumulate; everything else fp32")},
        }
        if args.full:
            out["roofline"] = roof
        if elapsed_other is not None:
            out["other_math_mode"] = {
                "math": ("fp16 hi+lo split activations x exact-fp16 weights on the f16 matrix pipe, fp32 accumulate "
                         "(deviation from the fp32-MFMA path ~1e-6 rel, tests/test_gpu_parity.py)" if other == 1 else
                         "fp32 MFMA (exact fp32)"),
                "value": world * B * args.steps / elapsed_other, "unit": "crops/s",
                "ms_per_step": 1e3 * elapsed_other / args.steps}
        if clocks is not None:
            out["device_under_load"] = clocks
        if elapsed_pipe is not None:
            out["pipelined_two_streams"] = {
                "what": "the same K batches dealt alternately to two engine handles on two HIP streams (two independent batches in "
                        "flight); supplementary, never `value`",
                "value": B * args.steps / elapsed_pipe, "unit": "crops/s", "ms_per_step": 1e3 * elapsed_pipe / args.steps,
                "outputs_identical_between_handles": same}
        if elapsed_split is not None:
            out["split_streams_option"] = {
                "what": "FEAR_OPT_SPLIT_STREAMS = 1: every fear_track call as two half-batches on two streams of one handle "
                        "(bit-identical maps); supplementary, never `value`",
                "value": B * args.steps / elapsed_split, "unit": "crops/s", "ms_per_step": 1e3 * elapsed_split / args.steps}
        if ddp_train is not None:
            out["config5_train_step_data_parallel"] = ddp_train
        if use_dist:
            out["collective"] = {"backend": "nccl (RCCL)", "ranks": dist.get_world_size(), "op": "all_gather_into_tensor",
                                 "bytes_per_rank": B * 5 * 16 * 16 * 4, "overlapped_with_next_batch": overlap is not None}
            if gather_ms is not None:
                out["collective"]["ms_alone"] = gather_ms
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(search_u8, tmpl_u8, DEFAULT_WEIGHTS)
        # (configs[4] before configs[3]: measured order dependence — after the FEAR-M leg AND the two-handle / other-mode legs of this
        #  process the same training step runs 11 % slower (18.7 vs 16.7 ms; neither a cool-down pause nor the host explains it: host issue
        #  10 ms either way), after either of them alone it does not; FEAR-M's own number does not depend on the order)
        if args.full and not args.no_train and world == 1 and not use_dist:
            out["config5_train_step"] = config5_train_step(dev)
            torch.cuda.empty_cache()
        if args.full and not args.no_fear_m and world == 1 and not use_dist:
            del net, search, tmpl_feats
            torch.cuda.empty_cache()
            out["config4_fear_m_bf16"] = config4_fear_m(dev)
            net = search = tmpl_feats = None
        if args.full and not args.no_latency and world == 1 and not use_dist:
            del net, search, tmpl_feats
            torch.cuda.empty_cache()
            out["latency_batch1"] = latency_batch1(DEFAULT_WEIGHTS)
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
