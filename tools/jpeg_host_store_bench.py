"""Measures `JpegStore(residence="host")` against the store on the device, on the 256 synthetic 1280 x 720 files of
tools/jpeg_decode_bench.py, and writes profiles/jpeg_host_store_bench.json.  Needs the GPU.

    python tools/jpeg_host_store_bench.py [--dir DIR] [--parent TREE]

Three stores of the same files: `device`, `host` (the staged kernels) and `host_direct` (the bytes on the host, the direct kernels: the
ablation that shows what the staging buys).
  decode_ms, frames_per_s   `decode` of all files, `decode_rows` of a quarter of each frame's height, and `decode_windows` of the 128-pair
                            batch of tools/jpeg_windows_bench.py; a host clock around --calls calls and a synchronise
  huffman_ms                the same calls with the pixel stage's launches left out: the plan, the upload and the Huffman stage
  add_files_per_s           `add` of all files into a fresh store, by residence
  bytes_per_file            what a file holds of device memory (`nbytes`) and of pinned host memory (`host_nbytes`), by residence
  fit_ms_per_step           one epoch of --steps steps inside `fit` with `PairLoader(windows=True)`, prefetch=1, by residence; and
                            `consumed_frames_per_s`, the distinct frames a step reads over the device store's step time
  defaults_vs_parent        with --parent TREE (a built checkout of the parent commit): `decode` and the quarter-height `decode_rows` of a
                            store on the device in child processes that alternate between this tree and the parent's
The variants alternate in one process, --repeats rounds after one warm-up round; medians with minimum and maximum."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 128


def _tool(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                         # (fit_bench puts its own tree in front of sys.path)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for defaults_vs_parent")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the alternation with the parent")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured (the children of --parent use it)")
    ap.add_argument("--defaults-only", action="store_true", help="print the default paths' timings of --root as JSON and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_host_store_bench.json"))
    args = ap.parse_args()
    fit_bench = _tool(args.root, "fit_bench")
    spread = fit_bench.spread
    import torch
    from feartracker_amd import JpegStore, jpeg_store
    assert os.path.dirname(os.path.dirname(os.path.abspath(jpeg_store.__file__))) == os.path.abspath(args.root), "the package of another tree"

    blobs = fit_bench.files(args.dir)
    n = len(blobs)

    def timed(fn, calls=args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    def filled(**kw):
        store = JpegStore(device=0, threads=16, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = store.add(blobs)
        return store, ids, n / (time.perf_counter() - t0)

    device, ids, _ = filled()
    height, width = (int(v) for v in device.shape(ids[:1])[0])
    y0 = np.random.default_rng(11).integers(0, height - height // 4 + 1, n)
    quarter = np.stack([y0, y0 + height // 4], axis=1)
    variants = {"decode device": lambda: timed(lambda: device.decode(ids)),
                "rows device": lambda: timed(lambda: device.decode_rows(ids, quarter))}
    if args.defaults_only:
        times = {name: [] for name in variants}
        for round_ in range(args.repeats + 1):
            for name, fn in variants.items():
                v = fn()
                if round_:
                    times[name].append(v)
        device.check()
        print("DEFAULTS " + json.dumps({k: round(statistics.median(v), 4) for k, v in times.items()}))
        return

    from feartracker_amd.fit import fit
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_data.loader import PairLoader
    from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    stores = {"device": device, "host": filled(residence="host")[0], "host_direct": filled(residence="host")[0]}
    stores["host_direct"]._staged = False
    table = _tool(ROOT, "jpeg_windows_bench").table_over(n, height, width)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    opt = AdamHIP(net, lr=1e-4)

    def loader(store, seed, **kw):
        sampler = TrackSampler(table, 0, 8, B * args.steps, clip_range=True, seed=seed)
        return PairLoader(EpochPlan([sampler], B, seed=seed + 1), store, [ids], TrainPairBuilder(device=0, seed=seed + 2), **kw)

    first = loader(device, 30, prefetch=0)                               # one batch of 128 pairs, fixed: its files and rectangles
    first.plan.start_epoch()
    pairs, distinct = first._host(first.plan.batches[0])[:2]
    shapes = device.shape(distinct)
    wins = first.builder.frame_windows(pairs, first.builder.draw(pairs, shapes), shapes)
    pixels = jpeg_store._launch_pixels

    def without_pixels(fn):
        jpeg_store._launch_pixels = lambda *a, **k: None
        try:
            return timed(fn)
        finally:
            jpeg_store._launch_pixels = pixels

    def inside_fit(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        history = fit(net, opt, which, epochs=1)
        t = time.perf_counter() - t0
        assert np.isfinite(history[0]["train/loss"])
        return 1e3 * t / args.steps

    calls = {"decode": lambda s: s.decode(ids), "rows": lambda s: s.decode_rows(ids, quarter), "windows": lambda s: s.decode_windows(distinct, wins)}
    variants = {}
    for kind, call in calls.items():
        for name, store in stores.items():
            variants[f"{kind} {name}"] = lambda call=call, store=store: timed(lambda: call(store))
            variants[f"huffman {kind} {name}"] = lambda call=call, store=store: without_pixels(lambda: call(store))
    loaders = {name: loader(stores[name], 10, prefetch=1, windows=True) for name in ("device", "host")}
    for name, which in loaders.items():
        variants[f"fit {name}"] = lambda which=which: inside_fit(which)
    times = {name: [] for name in variants}
    for round_ in range(args.repeats + 1):                               # (round 0 warms every shape and is dropped)
        for name, fn in variants.items():
            v = fn()
            if round_:
                times[name].append(v)
    for store in stores.values():
        store.check()
    adds = {"device": [], "host": []}
    for _ in range(args.repeats):
        for name in adds:
            store, _, rate = filled(**({"residence": "host"} if name == "host" else {}))
            adds[name].append(rate)
            store.close()

    want = device.decode(ids)
    same = all(torch.equal(a, b) for name in ("host", "host_direct") for a, b in zip(stores[name].decode(ids), want))
    frames = {"decode": n, "rows": n, "windows": int(distinct.size)}
    res = {"files": n, "width": width, "height": height, "file_bytes": round(sum(map(len, blobs)) / n, 1), "pairs": B,
           "distinct_files": int(distinct.size), "repeats": args.repeats, "calls_per_window": args.calls, "steps_per_epoch": args.steps,
           "subsequence_bytes": device.subsequence_bytes, "rows_band": height // 4, "frames_equal": bool(same),
           "decode_ms": {k: {s: spread(times[f"{k} {s}"]) for s in stores} for k in calls},
           "frames_per_s": {k: {s: round(1e3 * frames[k] / statistics.median(times[f"{k} {s}"]), 1) for s in stores} for k in calls},
           "huffman_ms": {k: {s: spread(times[f"huffman {k} {s}"]) for s in stores} for k in calls},
           "add_files_per_s": {k: spread(v, 1) for k, v in adds.items()},
           "bytes_per_file": {s: {"device": round(stores[s].nbytes / n, 1), "host": round(stores[s].host_nbytes / n, 1),
                                  **{k: round(v / n, 1) for k, v in stores[s].resident.items() if k != "pixels"}} for s in ("device", "host")},
           "fit_ms_per_step": {s: spread(times[f"fit {s}"]) for s in loaders}}
    res["consumed_frames_per_s"] = round(1e3 * int(distinct.size) / res["fit_ms_per_step"]["device"]["median"], 1)
    if args.parent:                                                      # fresh child processes, alternating between the trees
        rounds = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for name, root in (("this", ROOT), ("parent", os.path.abspath(args.parent))):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "jpeg_host_store_bench.py"), "--defaults-only", "--root", root,
                       "--repeats", str(args.repeats), "--calls", str(args.calls)]
                if args.dir:
                    cmd += ["--dir", args.dir]
                out = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=300)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("DEFAULTS ")]
                assert out.returncode == 0 and line, out.stderr[-2000:]
                rounds[name].append(json.loads(line[-1][9:]))
        res["defaults_vs_parent"] = rounds
        # not slower: this tree's median over the rounds lies within the parent's own minimum-to-maximum range, or below it
        res["defaults_within_parent_range"] = {
            key: bool(statistics.median(r[key] for r in rounds["this"]) <= max(r[key] for r in rounds["parent"]))
            for key in ("decode device", "rows device")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
