"""Measures a decode scale per frame — `JpegStore` calls with a sequence of scales and `PairLoader(scale="auto")` — against scale 1, and
writes profiles/jpeg_mixed_bench.json.  Needs the GPU.

    python tools/jpeg_mixed_bench.py [--parent TREE]

The files: the 256 synthetic 1280 x 720 files of tools/jpeg_decode_bench.py, and 64 files of 1920 x 1080 from the same generator, so that
several scales occur: 16 tracks of boxes of 40 to 300 pixels over the first, 4 tracks of boxes of 300 to 900 pixels over the second, three
quarters of a batch of 128 pairs from the first table and a quarter from the second.

  scales                  the histogram of the scales `TrainPairBuilder.frame_scales` chooses for the fixed batch's distinct files
  windows_build_ms        `decode_windows` + `build(borders=)` of the fixed batch: at scale 1 and with `frame_scales`
  rows_build_ms           the same through `decode_rows`
  fit_ms_per_step         one epoch of --steps steps inside `fit`, `PairLoader(windows=True)` against `PairLoader(windows=True, scale="auto")`
  mixed_call_ms           `decode_windows` of the auto batch as ONE call with a scale per position (fear_jpeg_decode_mixed_u8: two pixel
                          launches) against the same positions as one uniform call per distinct scale
  crop_mean_abs_diff      how far the auto batch's crops are from the scale-1 batch's (normalised fp32 tensors): recorded, not judged
  defaults_vs_parent      with --parent TREE (a built checkout of the parent commit): `decode` at scale 1 and at scale 2 and `fit` with
                          `PairLoader()`, in fresh child processes that alternate between this tree and the parent's (and
                          which of the two runs first alternates from round to round)
The variants alternate, --repeats rounds after one warm-up round; medians with minimum and maximum.  A decode is timed by a host clock
around --calls calls and a synchronise."""
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
LARGE = (1080, 1920, 64)                                                      # height, width, count of the larger files


def _module(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                             # (it puts its own tree in front of sys.path)
    return mod


def larger_files(root):
    """LARGE[2] files of LARGE[1] x LARGE[0] from jpeg_decode_bench's generator, encoded on the device as fit_bench encodes the others."""
    import torch
    from feartracker_amd import JpegEncoder
    bench = _module(root, "jpeg_decode_bench")
    bench.H, bench.W, bench.COUNT = LARGE
    enc, blobs, group = JpegEncoder(device=0, quality=bench.QUALITY), [], []
    for img in bench.images():
        group.append(torch.from_numpy(img).cuda())
        if len(group) == 16:
            blobs += enc.encode(group).result()
            group = []
    assert not group and len(blobs) == LARGE[2]
    return blobs


def table_over(n, height, width, tracks, sides, seed):
    """`tracks` tracks of n / tracks consecutive files: a box of sides[0]..sides[1] pixels a side on a reflected random walk."""
    from feartracker_amd.train_data.sampling import TrackTable
    rng = np.random.default_rng(seed)
    per = n // tracks
    w, h = rng.integers(sides[0], sides[1] + 1, (2, tracks, 1))

    def walk(limit):
        p = rng.integers(0, limit + 1) + np.cumsum(rng.integers(-12, 13, (tracks, per)), axis=1)
        p = np.abs(p) % (2 * limit)
        return np.where(p > limit, 2 * limit - p, p)
    x, y = walk(width - w), walk(height - h)
    bbox = np.stack([x, y, np.broadcast_to(w, x.shape), np.broadcast_to(h, x.shape)], axis=-1).reshape(-1, 4)
    number = np.arange(tracks * per)
    return TrackTable.from_arrays([f"track{t:05d}" for t in number // per], number % per, [f"frame{k:03d}.jpg" for k in number], bbox,
                                  np.ones(number.size), np.zeros(number.size, bool), "synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window of the decode variants")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for defaults_vs_parent")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternation with the parent")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured (the children of --parent use it)")
    ap.add_argument("--defaults-only", action="store_true", help="print the default paths' timings of --root as JSON and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_mixed_bench.json"))
    args = ap.parse_args()
    fit_bench = _module(args.root, "fit_bench")
    spread = fit_bench.spread
    import torch
    from feartracker_amd import JpegStore, jpeg_store
    from feartracker_amd.fit import fit
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.train_data import TrainPairBuilder, scale_pairs
    from feartracker_amd.train_data.loader import PairLoader
    from feartracker_amd.train_data.sampling import EpochPlan, TrackSampler
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    assert os.path.dirname(os.path.dirname(os.path.abspath(jpeg_store.__file__))) == os.path.abspath(args.root), "the package of another tree"

    small, large = fit_bench.files(None), larger_files(args.root)
    store = JpegStore(device=0, threads=16)
    ids_small, ids_large = store.add(small), store.add(large)
    (h0, w0), (h1, w1) = store.shape(ids_small[:1])[0].tolist(), store.shape(ids_large[:1])[0].tolist()
    tables = [table_over(len(small), h0, w0, 16, (40, 300), 43), table_over(len(large), h1, w1, 4, (300, 900), 44)]
    net = FEARNetTrainHIP(random_init_state(0), device=0)
    opt = AdamHIP(net, lr=1e-4)

    def loader(seed, **kw):
        samplers = [TrackSampler(tables[0], 0, 8, B * args.steps * 3 // 4, clip_range=True, seed=seed),
                    TrackSampler(tables[1], 0, 8, B * args.steps // 4, clip_range=True, seed=seed + 5)]
        return PairLoader(EpochPlan(samplers, B, seed=seed + 1), store, [ids_small, ids_large], TrainPairBuilder(device=0, seed=seed + 2), **kw)

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

    # one batch of 128 pairs, fixed: its distinct files, its draws
    first = loader(30, prefetch=0)
    first.plan.start_epoch()
    pairs, distinct = first._host(first.plan.batches[0])[:2]
    builder = first.builder
    shapes = store.shape(distinct)
    params = builder.draw(pairs, shapes)
    borders = store.borders(distinct)

    default_loader = loader(10, prefetch=1)
    variants = {"decode_1": lambda: timed(lambda: store.decode(distinct), args.calls),
                "decode_2": lambda: timed(lambda: store.decode(distinct, scale=2), args.calls),
                "fit_default": lambda: inside_fit(default_loader)}
    if not args.defaults_only:
        import dataclasses
        scales = builder.frame_scales(pairs, params, shapes)
        small_pairs, small_shapes = scale_pairs(pairs, scales), store.shape(distinct, scales)
        small_params = dataclasses.replace(params, frame_shapes=tuple(map(tuple, small_shapes.tolist())))
        wins1, rows1 = builder.frame_windows(pairs, params, shapes), builder.frame_rows(pairs, params, shapes)
        wins, rows = builder.frame_windows(small_pairs, small_params, small_shapes), builder.frame_rows(small_pairs, small_params, small_shapes)
        distinct_scales = sorted(set(scales.tolist()))
        parts = [np.flatnonzero(scales == s) for s in distinct_scales]

        def split_call():
            for s, at in zip(distinct_scales, parts):
                store.decode_windows(distinct[at], wins[at], scale=s)
        windows_loader, auto_loader = loader(10, prefetch=1, windows=True), loader(10, prefetch=1, windows=True, scale="auto")
        variants.update({
            "windows_1": lambda: timed(lambda: builder.build(store.decode_windows(distinct, wins1), pairs, params, borders=borders), args.calls),
            "windows_auto": lambda: timed(lambda: builder.build(store.decode_windows(distinct, wins, scale=scales), small_pairs, small_params,
                                                                borders=borders), args.calls),
            "rows_1": lambda: timed(lambda: builder.build(store.decode_rows(distinct, rows1), pairs, params, borders=borders), args.calls),
            "rows_auto": lambda: timed(lambda: builder.build(store.decode_rows(distinct, rows, scale=scales), small_pairs, small_params,
                                                             borders=borders), args.calls),
            "fit_windows_1": lambda: inside_fit(windows_loader),
            "fit_windows_auto": lambda: inside_fit(auto_loader),
            "mixed_one_call": lambda: timed(lambda: store.decode_windows(distinct, wins, scale=scales), args.calls),
            "mixed_split_calls": lambda: timed(split_call, args.calls)})
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

    one = builder.build(store.decode_windows(distinct, wins1), pairs, params, borders=borders)
    auto = builder.build(store.decode_windows(distinct, wins, scale=scales), small_pairs, small_params, borders=borders)
    through_rows = builder.build(store.decode_rows(distinct, rows, scale=scales), small_pairs, small_params, borders=borders)
    plan1 = jpeg_store.plan_decode_windows(store._columns, store._row_sub, distinct, wins1, store.workspace_limit)
    plan = jpeg_store.plan_decode_windows(store._columns, store._row_sub, distinct, wins, store.workspace_limit, scale=scales)
    from feartracker_amd import train_abi                                    # the library calls of each form, by name
    launched, keep = [], train_abi.launch
    train_abi.launch = lambda lib, name, *a: launched.append(name) or keep(lib, name, *a)
    try:
        store.decode_windows(distinct, wins, scale=scales)
        mixed_launches = list(launched)
        del launched[:]
        split_call()
        split_launches = list(launched)
    finally:
        train_abi.launch = keep
    torch.cuda.synchronize()
    res = {"files": {"1280x720": len(small), "1920x1080": len(large)}, "pairs": B, "distinct_files": int(distinct.size),
           "repeats": args.repeats, "calls_per_window": args.calls, "steps_per_epoch": args.steps,
           "box_side": {"1280x720": [40, 300], "1920x1080": [300, 900]},
           "scales": {str(s): int((scales == s).sum()) for s in (1, 2, 4, 8)},
           "windows_build_ms": {"scale_1": spread(times["windows_1"]), "auto": spread(times["windows_auto"])},
           "rows_build_ms": {"scale_1": spread(times["rows_1"]), "auto": spread(times["rows_auto"])},
           "fit_ms_per_step": {"default": spread(times["fit_default"]), "windows_scale_1": spread(times["fit_windows_1"]),
                               "windows_auto": spread(times["fit_windows_auto"])},
           "mixed_call_ms": {"one_call": spread(times["mixed_one_call"]), "one_call_per_scale": spread(times["mixed_split_calls"])},
           "launches": {"one_call": mixed_launches, "one_call_per_scale": split_launches},
           "decode_ms": {"scale_1": spread(times["decode_1"]), "scale_2": spread(times["decode_2"])},
           "window_bytes_per_batch": {"scale_1": int(sum(int((p["high"] * p["wide"]).sum()) for p in plan1) * 3),
                                      "auto": int(sum(int((p["high"] * p["wide"]).sum()) for p in plan) * 3)},
           "crop_mean_abs_diff": {"template": float((one.template - auto.template).abs().mean()),
                                  "search": float((one.search - auto.search).abs().mean())},
           "rows_and_windows_equal_at_auto": bool(all(torch.equal(x, y) for x, y in zip(auto, through_rows)))}
    res["auto_faster"] = {key: bool(max(times[b]) < min(times[a])) for key, a, b in
                          (("windows_build", "windows_1", "windows_auto"), ("rows_build", "rows_1", "rows_auto"),
                           ("fit", "fit_windows_1", "fit_windows_auto"), ("one_call_against_split", "mixed_split_calls", "mixed_one_call"))}
    if args.parent:                                                          # fresh child processes, alternating between the trees
        rounds = {"this": [], "parent": []}
        trees = (("this", ROOT), ("parent", os.path.abspath(args.parent)))
        for k in range(args.rounds):
            for name, root in trees[::-1 if k % 2 else 1]:                   # (neither tree always runs first in its round)
                cmd = [sys.executable, os.path.join(ROOT, "tools", "jpeg_mixed_bench.py"), "--defaults-only", "--root", root,
                       "--steps", str(args.steps), "--repeats", str(args.repeats), "--calls", str(args.calls)]
                out = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("DEFAULTS ")]
                assert out.returncode == 0 and line, out.stderr[-2000:]
                rounds[name].append(json.loads(line[-1][9:]))
        keys = ("decode_1", "decode_2", "fit_default")
        res["defaults_vs_parent"] = dict(rounds, **{name: {key: spread([r[key] for r in rounds[which]]) for key in keys}
                                                    for name, which in (("this_spread", "this"), ("parent_spread", "parent"))})
        # no slower than the parent: this tree's median over the rounds lies within the parent's minimum to maximum, or below
        res["defaults_within_parent_range"] = {
            key: bool(res["defaults_vs_parent"]["this_spread"][key]["median"] <= res["defaults_vs_parent"]["parent_spread"][key]["max"])
            for key in keys}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
