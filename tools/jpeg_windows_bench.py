"""Measures `JpegStore.decode_windows` against `decode_rows` on the 256 synthetic 1280 x 720 files of tools/jpeg_decode_bench.py, for the
same 128 pairs of 40 to 300 pixel boxes, and writes profiles/jpeg_windows_bench.json.  Needs the GPU.

    python tools/jpeg_windows_bench.py [--dir DIR] [--parent TREE]

  decode_ms               one call over the batch's distinct files, a host clock around the call and a synchronise: `rows` and `windows`
  huffman_ms              the same call with the pixel stage's launch left out: the plan, the upload and the Huffman stage
  decode_build_ms         the call and `TrainPairBuilder.build(..., borders=)` behind it
  bytes_per_batch         the frames' bytes a batch allocates: full frames (`rows`) and compact tensors (`windows`)
  lanes_per_batch         the Huffman lanes in the grid of each form (the window form's lanes that return early are in its count)
  fit_ms_per_step         one epoch of --steps steps inside `fit` with `PairLoader()` and with `PairLoader(windows=True)`, prefetch=1
  defaults_vs_parent      with --parent TREE (a built checkout of the parent commit): `decode_rows` and `fit` with `PairLoader()` in
                          child processes that alternate between this tree and the parent's, every round's median listed
The variants alternate, --repeats rounds after one warm-up round; medians with minimum and maximum."""
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
B, TRACKS = 128, 16


def _fit_bench(root):
    spec = importlib.util.spec_from_file_location("fit_bench", os.path.join(root, "tools", "fit_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                         # (it puts its own tree in front of sys.path)
    return mod


def table_over(n, height, width):
    """fit_bench's table with boxes of 40 to 300 pixels a side: 16 tracks of n / 16 consecutive files, a reflected random walk."""
    from feartracker_amd.train_data.sampling import TrackTable
    rng = np.random.default_rng(43)
    per = n // TRACKS
    w, h = rng.integers(40, 301, (2, TRACKS, 1))

    def walk(limit):
        p = rng.integers(0, limit + 1) + np.cumsum(rng.integers(-12, 13, (TRACKS, per)), axis=1)
        p = np.abs(p) % (2 * limit)
        return np.where(p > limit, 2 * limit - p, p)
    x, y = walk(width - w), walk(height - h)
    bbox = np.stack([x, y, np.broadcast_to(w, x.shape), np.broadcast_to(h, x.shape)], axis=-1).reshape(-1, 4)
    number = np.arange(TRACKS * per)
    return TrackTable.from_arrays([f"track{t:05d}" for t in number // per], number % per, [f"frame{k:03d}.jpg" for k in number % n], bbox,
                                  np.ones(number.size), np.zeros(number.size, bool), "synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window of the decode variants")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for defaults_vs_parent")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of the alternation with the parent")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured (the children of --parent use it)")
    ap.add_argument("--defaults-only", action="store_true", help="print the default paths' timings of --root as JSON and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_windows_bench.json"))
    args = ap.parse_args()
    fit_bench = _fit_bench(args.root)
    spread = fit_bench.spread
    import torch
    from feartracker_amd import JpegStore, jpeg_store
    from feartracker_amd.fit import fit
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_data import TrainPairBuilder
    from feartracker_amd.train_data.loader import PairLoader
    from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    assert os.path.dirname(os.path.dirname(os.path.abspath(jpeg_store.__file__))) == os.path.abspath(args.root), "the package of another tree"

    blobs = fit_bench.files(args.dir)
    store = JpegStore(device=0, threads=16)
    ids = store.add(blobs)
    height, width = (int(v) for v in store.shape(ids[:1])[0])
    table = table_over(len(blobs), height, width)
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    opt = AdamHIP(net, lr=1e-4)

    def loader(seed, **kw):
        sampler = TrackSampler(table, 0, 8, B * args.steps, clip_range=True, seed=seed)
        return PairLoader(EpochPlan([sampler], B, seed=seed + 1), store, [ids], TrainPairBuilder(device=0, seed=seed + 2), **kw)

    # one batch of 128 pairs, fixed: its distinct files, its draws, the rows and the rectangles it reads
    first = loader(30, prefetch=0)
    first.plan.start_epoch()
    pairs, distinct = first._host(first.plan.batches[0])[:2]
    builder = first.builder
    shapes = store.shape(distinct)
    params = builder.draw(pairs, shapes)
    rows = builder.frame_rows(pairs, params, shapes)
    borders = store.borders(distinct)

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    def inside_fit(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        history = fit(net, opt, which, epochs=1)
        t = time.perf_counter() - t0
        assert np.isfinite(history[0]["train/loss"])
        return 1e3 * t / args.steps

    default_loader = loader(10, prefetch=1)
    variants = {"decode_rows": lambda: timed(lambda: store.decode_rows(distinct, rows), args.calls),
                "fit_default": lambda: inside_fit(default_loader)}
    if not args.defaults_only:
        wins = builder.frame_windows(pairs, params, shapes)
        windows_loader = loader(10, prefetch=1, windows=True)
        pixels = jpeg_store._launch_pixels

        def without_pixels(fn):
            jpeg_store._launch_pixels = lambda *a, **k: None
            try:
                return timed(fn, args.calls)
            finally:
                jpeg_store._launch_pixels = pixels
        variants.update({
            "decode_windows": lambda: timed(lambda: store.decode_windows(distinct, wins), args.calls),
            "huffman_rows": lambda: without_pixels(lambda: store.decode_rows(distinct, rows)),
            "huffman_windows": lambda: without_pixels(lambda: store.decode_windows(distinct, wins)),
            "build_rows": lambda: timed(lambda: builder.build(store.decode_rows(distinct, rows), pairs, params, borders=borders), args.calls),
            "build_windows": lambda: timed(lambda: builder.build(store.decode_windows(distinct, wins), pairs, params, borders=borders), args.calls),
            "fit_windows": lambda: inside_fit(windows_loader)})
    times = {name: [] for name in variants}
    for round_ in range(args.repeats + 1):                                   # (round 0 warms every shape and is dropped)
        for name, fn in variants.items():
            v = fn()
            if round_:
                times[name].append(v)
    store.check()
    if args.defaults_only:
        print("DEFAULTS " + json.dumps({k: round(statistics.median(v), 4) for k, v in times.items()}))
        return

    same = all(torch.equal(x, y) for x, y in zip(builder.build(store.decode_rows(distinct, rows), pairs, params, borders=borders),
                                                 builder.build(store.decode_windows(distinct, wins), pairs, params, borders=borders)))
    full, compact = store.decode_rows(distinct, rows), store.decode_windows(distinct, wins)
    plan_rows = jpeg_store.plan_decode_rows(store._columns, store._row_sub, distinct, rows, store.workspace_limit)
    plan_wins = jpeg_store.plan_decode_windows(store._columns, store._row_sub, distinct, wins, store.workspace_limit)
    res = {"files": len(blobs), "width": width, "height": height, "pairs": B, "distinct_files": int(distinct.size), "repeats": args.repeats,
           "calls_per_window": args.calls, "steps_per_epoch": args.steps, "box_side": [40, 300],
           "decode_ms": {"rows": spread(times["decode_rows"]), "windows": spread(times["decode_windows"])},
           "huffman_ms": {"rows": spread(times["huffman_rows"]), "windows": spread(times["huffman_windows"])},
           "decode_build_ms": {"rows": spread(times["build_rows"]), "windows": spread(times["build_windows"])},
           "bytes_per_batch": {"rows": int(sum(f.numel() for f in full)), "windows": int(compact.nbytes)},
           "coefficient_bytes_per_batch": {"rows": 2 * sum(p["values"] for p in plan_rows), "windows": 2 * sum(p["values"] for p in plan_wins)},
           "lanes_per_batch": {"rows": int(sum(int(p["sub_count"].sum()) for p in plan_rows)),
                               "windows": int(sum(int(p["sub_count"].sum()) for p in plan_wins))},
           "fit_ms_per_step": {"default": spread(times["fit_default"]), "windows": spread(times["fit_windows"])},
           "batches_equal": bool(same)}
    res["windows_faster"] = {key: bool(max(times[b]) < min(times[a])) for key, a, b in
                             (("decode", "decode_rows", "decode_windows"), ("decode_build", "build_rows", "build_windows"),
                              ("fit", "fit_default", "fit_windows"))}
    if args.parent:                                                          # fresh child processes, alternating between the trees
        rounds = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for name, root in (("this", ROOT), ("parent", os.path.abspath(args.parent))):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "jpeg_windows_bench.py"), "--defaults-only", "--root", root,
                       "--steps", str(args.steps), "--repeats", str(args.repeats), "--calls", str(args.calls)]
                if args.dir:
                    cmd += ["--dir", args.dir]
                env = dict(os.environ, PYTHONPATH=root)
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("DEFAULTS ")]
                assert out.returncode == 0 and line, out.stderr[-2000:]
                rounds[name].append(json.loads(line[-1][9:]))
        res["defaults_vs_parent"] = rounds
        # no slower than the parent: this tree's median over the rounds is at most the parent's slowest round
        res["defaults_within_parent_range"] = {
            key: bool(statistics.median(r[key] for r in rounds["this"]) <= max(r[key] for r in rounds["parent"]))
            for key in ("decode_rows", "fit_default")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
