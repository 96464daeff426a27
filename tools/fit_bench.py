"""Measures `fit` (feartracker_amd/fit.py) on the 256 synthetic 1280 x 720 files of tools/jpeg_decode_bench.py with 16 tracks of 16 frames
laid over them, at B = 128 and the default builder config, and writes profiles/fit_bench.json.  Needs the GPU.

    python tools/fit_bench.py [--dir DIR]       # DIR: the files of `jpeg_decode_bench.py --make`; without it they are written on the
                                                # device by JpegEncoder (the same bytes: quality 90, 4:2:0) and kept in memory

  fit_ms_per_step         one epoch of --steps steps inside `fit`, a host clock around the whole call (it ends in the epoch's read of
                          the losses, which waits for the device), divided by the steps: with prefetch=1 and with prefetch=0
  bare_ms_per_step        the yardstick: net.step + opt.step on ONE fixed pre-built batch, the same number of steps, one synchronise
  ratio_to_bare           each variant's median over the yardstick's
  loader_host_ms_per_batch    the loader alone (prefetch=0, nobody consumes): host time until a batch is handed out; it never waits
  loader_host_ms_per_batch_large_table    the same with a table of --large-rows rows (6667 tracks of 150 frames by default, a GOT-10k-sized
                          annotation file) laid over the same 256 files: what the sampler costs when the table is large
The variants alternate, --repeats rounds after one warm-up round; medians with minimum and maximum."""
import argparse
import glob
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TRACKS, B = 16, 128


def spread(values, digits=4):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def files(directory):
    import torch
    if directory:
        blobs = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(directory, "*.jpg")))]
        assert blobs, "no files in --dir"
        return blobs
    spec = importlib.util.spec_from_file_location("jpeg_decode_bench", os.path.join(ROOT, "tools", "jpeg_decode_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from feartracker_amd import JpegEncoder
    enc, blobs, group = JpegEncoder(device=0, quality=bench.QUALITY), [], []
    for img in bench.images():
        group.append(torch.from_numpy(img).cuda())
        if len(group) == 32:
            blobs += enc.encode(group).result()
            group = []
    assert not group and len(blobs) == bench.COUNT
    return blobs


def table_over(n, height, width, tracks=TRACKS, per=None):
    """`tracks` tracks of `per` (n / tracks when None) consecutive files each, wrapping round the n files: a box of 60..300 pixels a side
    that drifts by up to 12 pixels from frame to frame (a reflected random walk)."""
    from feartracker_amd.train_data.sampling import TrackTable
    rng = np.random.default_rng(41)
    per = n // tracks if per is None else per
    w, h = rng.integers(60, 300, (2, tracks, 1))

    def walk(limit):                         # positions in [0, limit], reflected at both ends
        p = rng.integers(0, limit + 1) + np.cumsum(rng.integers(-12, 13, (tracks, per)), axis=1)
        p = np.abs(p) % (2 * limit)
        return np.where(p > limit, 2 * limit - p, p)
    x, y = walk(width - w), walk(height - h)
    bbox = np.stack([x, y, np.broadcast_to(w, x.shape), np.broadcast_to(h, x.shape)], axis=-1).reshape(-1, 4)
    number = np.arange(tracks * per)
    return TrackTable.from_arrays([f"track{t:05d}" for t in number // per], number % per, [f"frame{k:03d}.jpg" for k in number % n], bbox,
                                  np.ones(number.size), np.zeros(number.size, bool), "synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--large-rows", type=int, default=1_000_050, help="rows of the large table (150 per track)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.json"))
    args = ap.parse_args()
    import torch
    from feartracker_amd import JpegStore
    from feartracker_amd.fit import fit
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_data.loader import PairLoader
    from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state

    blobs = files(args.dir)
    threads = 16
    store = JpegStore(device=0, threads=threads)
    ids = store.add(blobs)
    height, width = (int(v) for v in store.shape(ids[:1])[0])
    table = table_over(len(blobs), height, width)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    opt = AdamHIP(net, lr=1e-4)

    def loader(prefetch, seed, table=table, row_ids=ids):
        sampler = TrackSampler(table, 0, 8, B * args.steps, clip_range=True, seed=seed)
        return PairLoader(EpochPlan([sampler], B, seed=seed + 1), store, [row_ids], TrainPairBuilder(device=0, seed=seed + 2), prefetch=prefetch)
    loaders = {1: loader(1, 10), 0: loader(0, 10)}
    large = table_over(len(blobs), height, width, tracks=args.large_rows // 150, per=150)
    file_of = np.array([int(p[5:8]) for p in large.img_path.tolist()])
    loaders["large"] = loader(0, 10, large, ids[file_of])
    fixed = next(iter(loader(0, 20))).batch

    def inside_fit(prefetch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        history = fit(net, opt, loaders[prefetch], epochs=1)
        t = time.perf_counter() - t0
        assert np.isfinite(history[0]["train/loss"])
        return 1e3 * t / args.steps

    def bare():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            opt.step(net.step(*fixed[:5])["grads"])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    def loader_alone(which=0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = sum(1 for _ in loaders[which])
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        loaders[which].plan.end_epoch(0)
        return 1e3 * t / count

    variants = {"prefetch_1": lambda: inside_fit(1), "prefetch_0": lambda: inside_fit(0), "bare": bare, "loader": loader_alone,
                "loader_large": lambda: loader_alone("large")}
    times = {name: [] for name in variants}
    for round_ in range(args.repeats + 1):                                   # (round 0 warms every shape and is dropped)
        for name, fn in variants.items():
            v = fn()
            if round_:
                times[name].append(v)
    store.check()
    base = statistics.median(times["bare"])
    res = {"files": len(blobs), "width": width, "height": height, "batch": B, "steps_per_epoch": args.steps, "repeats": args.repeats,
           "tracks": TRACKS, "store_threads": threads, "large_table_rows": len(large),
           "fit_ms_per_step": {"prefetch_1": spread(times["prefetch_1"]), "prefetch_0": spread(times["prefetch_0"])},
           "bare_ms_per_step": spread(times["bare"]),
           "ratio_to_bare": {k: round(statistics.median(times[k]) / base, 4) for k in ("prefetch_1", "prefetch_0")},
           "loader_host_ms_per_batch": spread(times["loader"]), "loader_host_ms_per_batch_large_table": spread(times["loader_large"])}
    res["prefetch_1_faster"] = bool(max(times["prefetch_1"]) < min(times["prefetch_0"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
