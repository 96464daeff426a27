"""Measures reduced-size decoding from the resident store (JpegStore.decode(scale=), decode_rows(scale=); DESIGN.md section 14,
"Reduced-size decoding") on the 256 synthetic 1280 x 720 files of tools/jpeg_decode_bench.py and writes profiles/jpeg_scaled_bench.json.

    python tools/jpeg_decode_bench.py --make --dir DIR               # needs Pillow: writes the files (any machine)
    python tools/jpeg_scaled_bench.py --dir DIR [--parent-lib LIB]   # needs the GPU: measures
    python tools/jpeg_scaled_bench.py --dir DIR --kernels-only       # three decodes per scale and nothing else: the run for a kernel trace
    python tools/jpeg_scaled_bench.py --stats-from CSV               # folds the trace's kernel statistics into the json

One process, every shape warmed first, the variants ALTERNATING within each of the 5 rounds (a drift of the clocks falls on all of
them), medians with minimum and maximum, a host clock around work that ends in check(), which synchronises:
  decode_ms_per_call        store.decode of the 256 ids in a seeded permutation at scales 1, 2, 4 and 8
  decode_rows_ms_per_call   store.decode_rows at a quarter of the (scaled) height, seeded positions, at scales 1 and 2
  bytes_per_frame           what the pixel stage writes per frame: 3 H' W'
  against_parent            with --parent-lib, the parent commit's library: every path whose pixel kernels the two builds may compile
                            differently, through both builds alternating, the frames compared first — store.decode at scales 1, 2, 4
                            and 8, decode_rows with the rows on the device at a quarter of the height (where skipped workgroups matter)
                            and fear_jpeg_decode_u8 alone (timed inside store.decode, between two synchronisations around the call).  Per row
                            `not_slower_than_parents_slowest`: this build's median <= the parent's maximum in the same run, so the
                            margin is the parent's own spread; `within_parents_spread`: the median lies within its minimum..maximum
  pixel_kernels_us          with --stats-from: the two pixel kernels' time per launch at each scale, from a separate kernel trace of
                            --kernels-only (rocprofv3 --kernel-trace --stats, its kernel_trace csv)
The indexed Huffman stage decodes every coefficient at every scale and is not touched by this mode: it bounds the gain.
Before anything is timed the frames at every scale are compared with JpegDecoder's at that scale (`frames_equal_decoder`)."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_bench as db          # noqa: E402

OUT = os.path.join(ROOT, "profiles", "jpeg_scaled_bench.json")
SCALES = (1, 2, 4, 8)
KERNELS = ("jpeg_decode_blocks_kernel", "jpeg_decode_merge_kernel", "jpeg_scaled_blocks_kernel", "jpeg_scaled_merge_kernel",
           "jpeg_huffman_indexed_kernel")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def alternating(variants, repeats, clock=timed):
    """{name: [seconds] * repeats}: one warm-up of every variant, then `repeats` rounds in which each runs once, in order.  `clock(fn)`
    runs a variant and says how long it took: the whole of it by default."""
    for fn in variants.values():
        fn()
    times = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            times[name].append(clock(fn))
    return times


def parent_store(path, blobs):
    """A JpegStore whose every call goes to the library at `path`, bound with this build's prototypes of the symbols it has."""
    from feartracker_amd import JpegStore
    from feartracker_amd import train_abi as abi
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (args, res) in abi.TRAIN_SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
    store = JpegStore(device=0, threads=16)
    store._lib = store._host._lib = lib
    return store, store.add(blobs)


def pixel_stage_alone(store, ids):
    """Seconds of fear_jpeg_decode_u8 alone within store.decode(ids): the clock runs inside the call itself, from a device that has
    finished the Huffman stage to one that has finished the pixel stage, summed over the call's groups.  Nothing is launched a second
    time, so every buffer the call's addresses name is the live one of the decode that made it."""
    import torch
    from feartracker_amd import train_abi as abi
    took, real = [], abi.launch

    def spy(lib, name, *a):
        if name != "fear_jpeg_decode_u8":
            return real(lib, name, *a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = real(lib, name, *a)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
        return rc
    abi.launch = spy
    try:
        store.decode(ids, check=True)
    finally:
        abi.launch = real
    assert took, "store.decode launched no fear_jpeg_decode_u8"
    return sum(took)


def against_parent(path, blobs, store, ids, order, repeats):
    """The rows of `against_parent`, each {parent_ms_per_call, ms_per_call, frames_equal, the two verdicts}."""
    import torch
    theirs, their_ids = parent_store(path, blobs)
    their_order = their_ids[np.random.default_rng(5).permutation(their_ids.size)]
    high = db.H // 4
    y0 = np.random.default_rng(9).integers(0, db.H - high + 1, ids.size)
    windows = np.stack([y0, y0 + high], axis=1)
    on_device = torch.from_numpy(windows.astype(np.int32)).cuda()
    rows = {}
    for s in SCALES:
        rows[f"store.decode at scale {s}"] = (
            lambda s=s: theirs.decode(their_order, check=True, scale=s), lambda s=s: store.decode(order, check=True, scale=s),
            lambda s=s: zip(theirs.decode(their_ids[:16], check=True, scale=s), store.decode(ids[:16], check=True, scale=s)))
    rows["decode_rows, rows on the device, at 0.25 H"] = (
        lambda: theirs.decode_rows(their_order, on_device, check=True), lambda: store.decode_rows(order, on_device, check=True),
        lambda: ((a[lo:hi], b[lo:hi]) for a, b, (lo, hi) in zip(theirs.decode_rows(their_order, on_device, check=True),
                                                                 store.decode_rows(order, on_device, check=True), windows.tolist())))
    alone = "fear_jpeg_decode_u8 alone"
    rows[alone] = (lambda: pixel_stage_alone(theirs, their_order), lambda: pixel_stage_alone(store, order), rows["store.decode at scale 1"][2])
    out = {}
    for name, (parent_fn, this_fn, pairs) in rows.items():
        same = all(bool(torch.equal(a, b)) for a, b in pairs())
        times = alternating({"parent": parent_fn, "this": this_fn}, repeats, clock=(lambda fn: fn()) if name == alone else timed)
        parent, this = db.spread(times["parent"], 1e3), db.spread(times["this"], 1e3)
        out[name] = {"parent_ms_per_call": parent, "ms_per_call": this, "frames_equal": same,
                     "within_parents_spread": parent["min"] <= this["median"] <= parent["max"],
                     "not_slower_than_parents_slowest": this["median"] <= parent["max"]}
    theirs.close()
    return out


def stats_from(path):
    """The pixel kernels' times per scale from the kernel trace (csv, one row per dispatch) of a --kernels-only run, which decodes three
    times at each of the scales 1, 2, 4, 8 in that order, one group per call: the last three dispatches of the full-size pair are scale
    1's (`add` launches the pair too, earlier), the nine of the scaled pair are three per scale.  Median of the three, in microseconds;
    the indexed Huffman kernel's last twelve dispatches, the same work at every scale, next to them."""
    import statistics
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    cols = {c.lower(): c for c in rows[0]}
    name, start, end = cols["kernel_name"], cols["start_timestamp"], cols["end_timestamp"]
    rows.sort(key=lambda r: int(r[start]))
    took = {k: [(int(r[end]) - int(r[start])) / 1e3 for r in rows if k in r[name]] for k in KERNELS}
    out = {"1": {k: round(statistics.median(took[k][-3:]), 1) for k in KERNELS[:2]}}
    for i, s in enumerate(SCALES[1:]):
        assert all(len(took[k]) == 9 for k in KERNELS[2:4]), {k: len(v) for k, v in took.items()}
        out[str(s)] = {k: round(statistics.median(took[k][3 * i:3 * i + 3]), 1) for k in KERNELS[2:4]}
    out["every scale"] = {KERNELS[4]: round(statistics.median(took[KERNELS[4]][-12:]), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "jpeg_bench_frames"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library: the pixel paths through both builds in the same run")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats-from", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.stats_from:
        with open(args.out) as fh:
            res = json.load(fh)
        res["pixel_kernels_us"] = stats_from(args.stats_from)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res["pixel_kernels_us"]))
        return
    import torch
    from feartracker_amd import JpegDecoder, JpegStore, jpeg_scaled_shape
    paths = sorted(glob.glob(os.path.join(args.dir, "*.jpg")))
    assert len(paths) == db.COUNT, f"{len(paths)} files in {args.dir}: run tools/jpeg_decode_bench.py --make --dir {args.dir}"
    blobs = [open(p, "rb").read() for p in paths]
    store = JpegStore(device=0, threads=16)
    ids = store.add(blobs)
    order = ids[np.random.default_rng(5).permutation(ids.size)]
    if args.kernels_only:
        for s in SCALES:
            for _ in range(3):
                store.decode(order, check=True, scale=s)
        return
    res = {"files": db.COUNT, "size": [db.H, db.W], "sampling": "4:2:0", "quality": db.QUALITY, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "note": "the indexed Huffman stage is the same work at every scale and bounds the gain"}
    decoder = JpegDecoder(device=0, threads=16)
    equal = {}
    for s in SCALES:
        mine, theirs = store.decode(ids[:16], check=True, scale=s), decoder.decode(blobs[:16], scale=s)
        equal[str(s)] = all(bool(torch.equal(a, b)) for a, b in zip(mine, theirs))
    decoder.close()
    res["frames_equal_decoder"] = equal
    res["bytes_per_frame"] = {str(s): int(np.prod(jpeg_scaled_shape(db.H, db.W, s))) for s in SCALES}
    times = alternating({str(s): (lambda s=s: store.decode(order, check=True, scale=s)) for s in SCALES}, args.repeats)
    res["decode_ms_per_call"] = {k: db.spread(v, 1e3) for k, v in times.items()}
    rng = np.random.default_rng(9)
    rows = {}
    for s in (1, 2):
        high = jpeg_scaled_shape(db.H, db.W, s)[0]
        y0 = rng.integers(0, high - high // 4 + 1, ids.size)
        rows[s] = np.stack([y0, y0 + high // 4], axis=1)
    times = alternating({str(s): (lambda s=s: store.decode_rows(order, rows[s], check=True, scale=s)) for s in (1, 2)}, args.repeats)
    res["decode_rows_ms_per_call"] = {k: db.spread(v, 1e3) for k, v in times.items()}
    res["against_parent"] = against_parent(args.parent_lib, blobs, store, ids, order, args.repeats) if args.parent_lib else "not measured"
    res["pixel_kernels_us"] = "not measured"
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
