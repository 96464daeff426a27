"""Measures the JPEG frame decoder (jpeg_frames.JpegDecoder) on 256 synthetic 1280 x 720, quality 90, 4:2:0 files
and writes profiles/jpeg_decode_bench.json.

    python tools/jpeg_decode_bench.py --make --dir DIR      # needs Pillow: writes the files (any machine)
    python tools/jpeg_decode_bench.py --dir DIR             # needs the GPU: measures
    python tools/jpeg_decode_bench.py --dir DIR --entropy both      # the host and the device Huffman stage in the same run
    python tools/jpeg_decode_bench.py --dir DIR --rounds 4  # no GPU: synchronisation rounds of the first files, from the Python model

  entropy_ms_per_frame    fear_jpeg_parse + fear_jpeg_entropy_decode, one thread, mean over the files
  entropy_fps             the same on 1, 4, 8 and 16 threads (ctypes releases the GIL)
  device_ms               fear_jpeg_decode_u8 alone on the 256 frames, HIP events, coefficients already on the device
  decode_fps              JpegDecoder.decode end to end on 16 threads (files in memory -> frames on the device, one synchronise per batch)
  upload_bytes_per_frame  the packed coefficients and block_start, against 3 H W
  pillow_fps              where Pillow is importable: Image.open(...).convert("RGB") on the same thread counts plus the pinned,
                          non-blocking upload TrainPairBuilder gives host frames — the baseline to compare with
With --entropy device or both, under "device_entropy" (the host figures above stay the baseline: entropy="host" at 16 threads, unchanged):
  decode_fps              JpegDecoder(entropy="device").decode end to end, check() included, by subsequence_bytes 32, 64, 128, 256
  huffman_ms              fear_jpeg_huffman alone between HIP events, by subsequence_bytes; `subsequence_bytes` names the fastest
  device_ms_dense         fear_jpeg_decode_u8 alone on the dense coefficients (device_ms above is the packed input)
  upload_bytes_per_frame  the unstuffed bytes, seg_start and the scan record
  scan_prepare_ms_per_frame   fear_jpeg_parse + fear_jpeg_scan_prepare, one thread (entropy_ms_per_frame above is the host's Huffman stage)
  ratio_to_host           decode_fps at the fastest subsequence_bytes over the host mode's decode_fps
Every timing is the median of --repeats runs after one warm-up run; each entry carries the minimum and maximum of the runs as well.

    python tools/jpeg_decode_bench.py --dir DIR --store     # needs the GPU: the resident store, writes profiles/jpeg_store_bench.json

--store measures jpeg_store.JpegStore against JpegDecoder(entropy="device") on the same files in ONE run, every shape warmed first, medians
of 5 with minimum and maximum:
  decoder_fps             (a) JpegDecoder(entropy="device").decode end to end with check(), 16 threads: the baseline
  store_fps               (b) store.decode of the 256 ids in a seeded permutation with check(), a host clock around work that ends in a
                          synchronise; `faster_than_decoder` says whether its slowest run beats the baseline's fastest
  stage_ms                (c) fear_jpeg_huffman alone and fear_jpeg_huffman_indexed alone between HIP events at 64, 128 and 256 bytes
  host_ms_per_call, upload_bytes_per_image      (d) store.decode until it returns (it does not wait), and its one pinned transfer
  add_files_per_s         (e) JpegStore.add of the 256 files into a fresh store, 16 threads, verdicts awaited
  resident_bytes_per_file (f) by subsequence_bytes: bytes (with seg_start and sub_start), index, records
  training_step_fps       what the 128-pair step consumes, to read store_fps against
Before anything is timed the store's frames are compared with the decoder's at every subsequence length (`frames_equal_decoder`).

    python tools/jpeg_decode_bench.py --dir DIR --store --rows      # needs the GPU: bands of rows, writes profiles/jpeg_rows_bench.json

--store --rows measures JpegStore.decode_rows against JpegStore.decode on the same 256 files in ONE run, at band heights 1.0, 0.5 and 0.25
of H with seeded random positions (one window per file), every shape warmed first, medians of 5 with minimum and maximum:
  decode_ms_per_call       store.decode of the 256 ids in a seeded permutation with check(), a host clock around work that ends in a
                           synchronise
  decode_rows_ms_per_call  the same for store.decode_rows, by band height; `rows_decoded` is the mean number of pixel rows per frame the
                           pixel stage writes (the window's MCU rows and their halo)
  stage_ms                 fear_jpeg_huffman_indexed alone and fear_jpeg_huffman_indexed_rows alone by band height, between HIP events;
                           `lanes` the subsequences that get a lane
  conditions               full_band_within_spread: at 1.0 the slowest decode_rows run is no slower than the slowest decode run by more
                           than decode's own minimum-to-maximum spread; quarter_band_faster: at 0.25 the slowest decode_rows run is below
                           the fastest decode run
  borders_ms, host_ms_per_call      store.borders(ids) between HIP events; decode_rows at 0.25 until it returns (it does not wait)
Before anything is timed the rows asked for are compared with `decode`'s at every band height (`rows_equal_decode`).

    python tools/jpeg_decode_bench.py --dir DIR --store --rows-device   # needs the GPU: writes profiles/jpeg_rows_device_bench.json

--store --rows-device measures, in ONE run on the same 256 files and the same seeded windows as --rows, `decode` (the baseline),
`decode_rows` with the rows on the host (planned on the host) and `decode_rows` with the rows in a device tensor (planned on the device:
full grids, workgroups outside the band return early), medians of 5 with minimum and maximum:
  decode_ms_per_call, decode_rows_host_ms_per_call, decode_rows_device_ms_per_call      a host clock around work that ends in a synchronise
  stage_ms                 between HIP events: fear_jpeg_huffman_indexed and fear_jpeg_decode_u8 of `decode`, and by band height
                           fear_jpeg_huffman_indexed_rows_dev and fear_jpeg_decode_u8_rows_dev alone
  conditions               quarter_band_faster: at 0.25 the slowest device-planned run is below the fastest decode run;
                           full_band_excess_ms / full_band_ratio: at 1.0, the device-planned median over decode's (the idle exits and the
                           full workspace)
  host_ms_per_call         decode_rows with device rows at 0.25 until it returns (it does not wait)
Before anything is timed both forms' rows are compared with `decode`'s at every band height (`rows_equal_decode`)."""
import argparse
import glob
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, COUNT, QUALITY = 1280, 720, 256, 90
THREADS = (1, 4, 8, 16)
SWEEP = (32, 64, 128, 256)


def images():
    """The COUNT synthetic frames, uint8 (H, W, 3), in order."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(COUNT):
        # a smooth scene, a few hundred rectangles and mild noise: file sizes near a video frame's at this quality
        img = np.stack([(xx * (i % 7 + 1) // 5 + yy) % 256, (yy * 2 + 3 * i) % 256, (xx + 2 * yy) // 3 % 256], axis=-1).astype(np.int16)
        for _ in range(300):
            x0, y0 = rng.integers(0, W - 8), rng.integers(0, H - 8)
            img[y0:y0 + rng.integers(8, 160), x0:x0 + rng.integers(8, 160)] = rng.integers(0, 256, 3)
        img += rng.integers(-6, 7, img.shape, dtype=np.int16)
        yield np.clip(img, 0, 255).astype(np.uint8)


def make(directory):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i, img in enumerate(images()):
        Image.fromarray(img).save(os.path.join(directory, f"frame{i:03d}.jpg"), quality=QUALITY, subsampling=2)
    print("wrote", COUNT, "files to", directory)


def run_seconds(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def median_seconds(fn, repeats):
    return statistics.median(run_seconds(fn, repeats))


def spread(values, scale=1.0, digits=4):
    return {"median": round(statistics.median(values) * scale, digits), "min": round(min(values) * scale, digits),
            "max": round(max(values) * scale, digits)}


def event_ms(torch, call, repeats):
    """`call` between HIP events: the runs behind one warm-up run, in milliseconds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats + 1):
        e0.record()
        assert call() == 0
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times[1:]


def rounds(blobs, count):
    """The synchronisation rounds per sequence of the first `count` files at the sweep's subsequence lengths, from the Python model."""
    from feartracker_amd.jpeg_huffman import jpeg_entropy_parallel_host
    out = {}
    for sb in SWEEP:
        seen = []
        for b in blobs[:count]:
            _, _, status, r = jpeg_entropy_parallel_host(b, sb, 256)
            assert status == 0
            seen += r
        seen.sort()
        out[str(sb)] = {"sequences": len(seen), "median": seen[len(seen) // 2], "p90": seen[len(seen) * 9 // 10], "max": seen[-1]}
    return out


def device_entropy(torch, blobs, repeats, host_fps):
    """The figures of JpegDecoder(entropy="device") on the same files."""
    from feartracker_amd import JpegDecoder
    from feartracker_amd import train_abi as abi
    n, res = len(blobs), {"decode_fps": {}, "huffman_ms": {}}
    probe = JpegDecoder(device=0, threads=16, entropy="device")
    res["scan_prepare_ms_per_frame"] = round(1e3 * median_seconds(lambda: [probe.scan_prepare(b) for b in blobs], repeats) / n, 4)
    prepared = [probe.scan_prepare(b) for b in blobs]
    up = sum(p[1].nbytes + p[2].nbytes + abi.ctypes.sizeof(p[3]) for p in prepared) / n
    res["upload_bytes_per_frame"] = {"scan": round(up, 1), "decoded": 3 * H * W, "ratio": round(up / (3 * H * W), 4)}
    probe.close()
    for sb in SWEEP:
        dec = JpegDecoder(device=0, threads=16, entropy="device", subsequence_bytes=sb)

        def end_to_end():
            frames = dec.decode(blobs, check=True)
            torch.cuda.synchronize()
            return frames
        res["decode_fps"][str(sb)] = spread([n / t for t in run_seconds(end_to_end, repeats)], digits=1)
        captured, real = {}, abi.launch

        def spy(lib, name, *a):
            captured[name] = a
            return real(lib, name, *a)
        abi.launch = spy
        frames = dec.decode(blobs, check=True)
        abi.launch = real
        torch.cuda.synchronize()
        res["huffman_ms"][str(sb)] = spread(event_ms(torch, lambda: dec._lib.fear_jpeg_huffman(*captured["fear_jpeg_huffman"]), repeats))
        if sb == SWEEP[-1]:
            # the pixel stage on the dense coefficients the call above left (the buffers are alive in the allocator's cache)
            assert dec._lib.fear_jpeg_huffman(*captured["fear_jpeg_huffman"]) == 0
            res["device_ms_dense"] = spread(event_ms(torch, lambda: dec._lib.fear_jpeg_decode_u8(*captured["fear_jpeg_decode_u8"]), repeats))
        del frames
        dec.close()
    best = min(SWEEP, key=lambda sb: res["huffman_ms"][str(sb)]["median"])
    res["subsequence_bytes"] = best
    res["huffman_fps"] = round(n / (res["huffman_ms"][str(best)]["median"] * 1e-3), 1)
    res["ratio_to_host"] = round(res["decode_fps"][str(best)]["median"] / host_fps, 3)
    res["training_step_fps"] = 17600
    return res


def store_bench(torch, blobs, out):
    """JpegStore against JpegDecoder(entropy="device") in one run."""
    from feartracker_amd import JpegDecoder, JpegStore
    from feartracker_amd import train_abi as abi
    n, repeats, sweep = len(blobs), 5, (64, 128, 256)
    res = {"files": n, "width": W, "height": H, "quality": QUALITY, "file_bytes_per_frame": sum(map(len, blobs)) / n,
           "cpus_available": len(os.sched_getaffinity(0)), "repeats": repeats, "training_step_fps": 17600}
    perm = np.random.default_rng(17).permutation(n)
    decoders = {sb: JpegDecoder(device=0, threads=16, entropy="device", subsequence_bytes=sb) for sb in sweep}
    stores, ids = {}, {}
    for sb in sweep:
        stores[sb] = JpegStore(device=0, subsequence_bytes=sb, threads=16)
        ids[sb] = stores[sb].add(blobs)
    default = JpegStore(device=0, threads=16).subsequence_bytes
    res["subsequence_bytes"] = default
    dec, store = decoders[default], stores[default]

    def decoder_end_to_end():
        frames = dec.decode(blobs, check=True)
        torch.cuda.synchronize()
        return frames

    def store_end_to_end():
        frames = store.decode(ids[default][perm], check=True)
        torch.cuda.synchronize()
        return frames

    def captured_call(fn, name):
        captured, real = {}, abi.launch

        def spy(lib, called, *a):
            captured[called] = a
            return real(lib, called, *a)
        abi.launch = spy
        try:
            keep = fn()
        finally:
            abi.launch = real
        torch.cuda.synchronize()
        return keep, captured[name]

    for sb in sweep:                                                     # every shape warm before anything is timed
        decoders[sb].decode(blobs, check=True)
        stores[sb].decode(ids[sb][perm], check=True)
    torch.cuda.synchronize()
    for sb in sweep:                                                     # faster and different is not faster: the same frames, byte for byte
        same = all(torch.equal(x, y) for x, y in zip(decoders[sb].decode(blobs, check=True), stores[sb].decode(ids[sb], check=True)))
        assert same, f"the store's frames differ from the decoder's at {sb} bytes"
    res["frames_equal_decoder"] = True
    a = run_seconds(decoder_end_to_end, repeats)
    b = run_seconds(store_end_to_end, repeats)
    res["decoder_fps"] = spread([n / t for t in a], digits=1)
    res["store_fps"] = spread([n / t for t in b], digits=1)
    res["decoder_ms_per_call"], res["store_ms_per_call"] = spread(a, 1e3), spread(b, 1e3)
    res["faster_than_decoder"] = bool(max(b) < min(a))
    res["stage_ms"] = {}
    for sb in sweep:
        keep_a, plain = captured_call(lambda: decoders[sb].decode(blobs, check=True), "fear_jpeg_huffman")
        keep_b, indexed = captured_call(lambda: stores[sb].decode(ids[sb][perm], check=True), "fear_jpeg_huffman_indexed")
        # the replays read what the captured addresses point at: the decoder's ctypes records are in `plain` itself, the store keeps its
        # last call's host records (`_records`) until its next decode, and the device buffers are alive in the frames and the allocator's cache
        lib = dec._lib
        assert stores[sb]._records[0].ctypes.data == indexed[0].value
        one = event_ms(torch, lambda: lib.fear_jpeg_huffman(*plain), repeats)
        two = event_ms(torch, lambda: lib.fear_jpeg_huffman_indexed(*indexed), repeats)
        res["stage_ms"][str(sb)] = {"fear_jpeg_huffman": spread(one), "fear_jpeg_huffman_indexed": spread(two),
                                    "indexed_faster": bool(max(two) < min(one))}
        del keep_a, keep_b

    def host_only():
        t0 = time.perf_counter()
        frames = store.decode(ids[default][perm])
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        store.check()
        return t, frames
    host_only()
    res["host_ms_per_call"] = spread([host_only()[0] for _ in range(repeats)], 1e3)
    res["upload_bytes_per_image"] = round(store.last_upload_bytes / n, 1)

    def add_once():
        fresh = JpegStore(device=0, subsequence_bytes=default, threads=16)
        t0 = time.perf_counter()
        fresh.add(blobs)
        t = time.perf_counter() - t0
        fresh.close()
        return t
    add_once()
    res["add_files_per_s"] = spread([n / add_once() for _ in range(repeats)], digits=1)
    res["resident_bytes_per_file"] = {str(sb): dict({k: round(v / n, 1) for k, v in stores[sb].resident.items() if k != "pixels"},
                                                    total=round(stores[sb].nbytes / n, 1)) for sb in sweep}
    for sb in sweep:
        decoders[sb].close()
        stores[sb].close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def rows_bench(torch, blobs, out):
    """JpegStore.decode_rows against JpegStore.decode in one run."""
    from feartracker_amd import JpegStore
    from feartracker_amd import train_abi as abi
    n, repeats, fractions = len(blobs), 5, (1.0, 0.5, 0.25)
    res = {"files": n, "width": W, "height": H, "quality": QUALITY, "file_bytes_per_frame": sum(map(len, blobs)) / n,
           "cpus_available": len(os.sched_getaffinity(0)), "repeats": repeats}
    # (a workspace that holds the 256 frames' dense coefficients, 1.06 GB, in one group: the stage replays below replay the whole call)
    store = JpegStore(device=0, threads=16, workspace_limit=2 << 30)
    ids = store.add(blobs)[np.random.default_rng(17).permutation(n)]
    res["subsequence_bytes"], res["workspace_limit"] = store.subsequence_bytes, store.workspace_limit
    res["resident_bytes_per_file"] = dict({k: round(v / n, 1) for k, v in store.resident.items() if k != "pixels"}, total=round(store.nbytes / n, 1))
    rng = np.random.default_rng(29)
    heights = store.shape(ids)[:, 0].astype(np.int64)
    windows = {}
    for f in fractions:
        high = np.maximum((heights * f).astype(np.int64), 1)
        y0 = rng.integers(0, heights - high + 1)
        windows[f] = np.stack([y0, y0 + high], axis=1)

    def whole():
        frames = store.decode(ids, check=True)
        torch.cuda.synchronize()
        return frames

    def bands(f):
        frames = store.decode_rows(ids, windows[f], check=True)
        torch.cuda.synchronize()
        return frames

    def captured_call(fn, name):
        captured, real = {}, abi.launch

        def spy(lib, called, *a):
            captured[called] = a
            return real(lib, called, *a)
        abi.launch = spy
        try:
            keep = fn()
        finally:
            abi.launch = real
        torch.cuda.synchronize()
        return keep, captured[name], store._records

    full = whole()                                                       # every shape warm, and the same rows before anything is timed
    for f in fractions:
        for x, y, (a, b) in zip(bands(f), full, windows[f].tolist()):
            assert torch.equal(x[a:b], y[a:b]), f"decode_rows differs from decode at band height {f}"
    del full
    res["rows_equal_decode"] = True
    a = run_seconds(whole, repeats)
    res["decode_ms_per_call"] = spread(a, 1e3)
    res["decode_rows_ms_per_call"], res["stage_ms"], timed = {}, {}, {}
    for f in fractions:
        timed[f] = run_seconds(lambda: bands(f), repeats)
        plan = store._records[1]                                         # the call's FearJpegImage records: the bands' heights
        assert plan.size == n
        res["decode_rows_ms_per_call"][str(f)] = dict(spread(timed[f], 1e3), rows_asked=int(windows[f][0, 1] - windows[f][0, 0]),
                                                      rows_decoded=round(float(plan["height"].mean()), 1))
    lib = store._lib
    keep, indexed, records = captured_call(whole, "fear_jpeg_huffman_indexed")
    one = event_ms(torch, lambda: lib.fear_jpeg_huffman_indexed(*indexed), repeats)
    res["stage_ms"]["fear_jpeg_huffman_indexed"] = dict(spread(one), lanes=int(records[0]["n_sub"].sum()))
    del keep
    for f in fractions:
        keep, rows, records = captured_call(lambda: bands(f), "fear_jpeg_huffman_indexed_rows")
        two = event_ms(torch, lambda: lib.fear_jpeg_huffman_indexed_rows(*rows), repeats)
        res["stage_ms"][f"fear_jpeg_huffman_indexed_rows {f}"] = dict(spread(two), lanes=int(records[0]["sub_count"].sum()))
        del keep
    res["conditions"] = {
        "full_band_within_spread": bool(max(timed[1.0]) <= max(a) + (max(a) - min(a))),
        "quarter_band_faster": bool(max(timed[0.25]) < min(a)),
    }
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gathers = []
    for _ in range(repeats + 1):
        e0.record()
        store.borders(ids)
        e1.record()
        torch.cuda.synchronize()
        gathers.append(e0.elapsed_time(e1))
    res["borders_ms"] = spread(gathers[1:])

    def host_only():
        t0 = time.perf_counter()
        frames = store.decode_rows(ids, windows[0.25])
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        store.check()
        return t, frames
    host_only()
    res["host_ms_per_call"] = spread([host_only()[0] for _ in range(repeats)], 1e3)
    store.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def rows_device_bench(torch, blobs, out):
    """decode, host-planned decode_rows and device-planned decode_rows in one run."""
    from feartracker_amd import JpegStore
    from feartracker_amd import train_abi as abi
    n, repeats, fractions = len(blobs), 5, (1.0, 0.5, 0.25)
    res = {"files": n, "width": W, "height": H, "quality": QUALITY, "file_bytes_per_frame": sum(map(len, blobs)) / n,
           "cpus_available": len(os.sched_getaffinity(0)), "repeats": repeats}
    store = JpegStore(device=0, threads=16, workspace_limit=2 << 30)      # (one group, as --rows: the stage replays replay the whole call)
    ids = store.add(blobs)[np.random.default_rng(17).permutation(n)]
    res["subsequence_bytes"], res["workspace_limit"] = store.subsequence_bytes, store.workspace_limit
    rng = np.random.default_rng(29)                                       # the windows of --rows
    heights = store.shape(ids)[:, 0].astype(np.int64)
    windows, on_device = {}, {}
    for f in fractions:
        high = np.maximum((heights * f).astype(np.int64), 1)
        y0 = rng.integers(0, heights - high + 1)
        windows[f] = np.stack([y0, y0 + high], axis=1)
        on_device[f] = torch.from_numpy(windows[f].astype(np.int32)).cuda()

    def whole():
        frames = store.decode(ids, check=True)
        torch.cuda.synchronize()
        return frames

    def hosted(f):
        frames = store.decode_rows(ids, windows[f], check=True)
        torch.cuda.synchronize()
        return frames

    def device(f):
        frames = store.decode_rows(ids, on_device[f], check=True)
        torch.cuda.synchronize()
        return frames

    def captured_calls(fn):
        captured, real = {}, abi.launch

        def spy(lib, called, *a):
            captured[called] = a
            return real(lib, called, *a)
        abi.launch = spy
        try:
            keep = fn()
        finally:
            abi.launch = real
        torch.cuda.synchronize()
        return keep, captured, store._records

    full = whole()                                                       # every shape warm, and the same rows before anything is timed
    for f in fractions:
        for form in (hosted, device):
            for x, y, (a, b) in zip(form(f), full, windows[f].tolist()):
                assert torch.equal(x[a:b], y[a:b]), f"{form.__name__} decode_rows differs from decode at band height {f}"
    del full
    res["rows_equal_decode"] = True
    a = run_seconds(whole, repeats)
    res["decode_ms_per_call"] = spread(a, 1e3)
    res["decode_rows_host_ms_per_call"], res["decode_rows_device_ms_per_call"], timed = {}, {}, {}
    for f in fractions:
        rows_asked = int(windows[f][0, 1] - windows[f][0, 0])
        res["decode_rows_host_ms_per_call"][str(f)] = dict(spread(run_seconds(lambda: hosted(f), repeats), 1e3), rows_asked=rows_asked)
        timed[f] = run_seconds(lambda: device(f), repeats)
        res["decode_rows_device_ms_per_call"][str(f)] = dict(spread(timed[f], 1e3), rows_asked=rows_asked)
    lib, res["stage_ms"] = store._lib, {}
    keep, calls, records = captured_calls(whole)
    for name in ("fear_jpeg_huffman_indexed", "fear_jpeg_decode_u8"):
        res["stage_ms"][name] = spread(event_ms(torch, lambda: getattr(lib, name)(*calls[name]), repeats))
    del keep
    for f in fractions:
        keep, calls, records = captured_calls(lambda: device(f))        # (the rows are a slice of on_device[f]: alive)
        for name in ("fear_jpeg_huffman_indexed_rows_dev", "fear_jpeg_decode_u8_rows_dev"):
            res["stage_ms"][f"{name} {f}"] = spread(event_ms(torch, lambda: getattr(lib, name)(*calls[name]), repeats))
        del keep
    med = statistics.median
    res["conditions"] = {
        "quarter_band_faster": bool(max(timed[0.25]) < min(a)),
        "full_band_excess_ms": round(1e3 * (med(timed[1.0]) - med(a)), 4),
        "full_band_ratio": round(med(timed[1.0]) / med(a), 4),
    }

    def host_only():
        t0 = time.perf_counter()
        frames = store.decode_rows(ids, on_device[0.25])
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        store.check()
        return t, frames
    host_only()
    res["host_ms_per_call"] = spread([host_only()[0] for _ in range(repeats)], 1e3)
    store.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--make", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--entropy", choices=("host", "device", "both"), default="host")
    ap.add_argument("--rounds", type=int, default=0, help="no GPU: the model's synchronisation rounds on the first N files, merged into --out")
    ap.add_argument("--store", action="store_true", help="the resident store against the device decoder, to profiles/jpeg_store_bench.json")
    ap.add_argument("--rows", action="store_true", help="with --store: decode_rows against decode, to profiles/jpeg_rows_bench.json")
    ap.add_argument("--rows-device", action="store_true",
                    help="with --store: decode_rows with the rows on the device against the host-planned form and decode, to "
                         "profiles/jpeg_rows_device_bench.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "jpeg_decode_bench.json" if not args.store else ("jpeg_rows_device_bench.json" if args.rows_device else
                                                                "jpeg_rows_bench.json" if args.rows else "jpeg_store_bench.json")
        args.out = os.path.join(ROOT, "profiles", name)
    if args.make:
        return make(args.dir)
    blobs = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.dir, "*.jpg")))]
    assert blobs, "no files: run with --make first"
    if args.rounds:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res.setdefault("device_entropy", {})["rounds_per_sequence"] = dict(files=args.rounds, **rounds(blobs, args.rounds))
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res["device_entropy"]["rounds_per_sequence"]))
        return
    import torch
    if args.store and args.rows_device:
        return rows_device_bench(torch, blobs, args.out)
    if args.store and args.rows:
        return rows_bench(torch, blobs, args.out)
    if args.store:
        return store_bench(torch, blobs, args.out)
    from feartracker_amd import JpegDecoder
    n = len(blobs)
    dec = JpegDecoder(device=0, threads=16)
    res = {"files": n, "width": W, "height": H, "quality": QUALITY, "file_bytes_per_frame": sum(map(len, blobs)) / n,
           "cpus_available": len(os.sched_getaffinity(0)), "repeats": args.repeats}

    # the host stage
    res["entropy_ms_per_frame"] = round(1e3 * median_seconds(lambda: [dec.entropy_decode(b) for b in blobs], args.repeats) / n, 4)
    res["entropy_fps"] = {}
    for t in THREADS:
        with ThreadPoolExecutor(max_workers=t) as pool:
            res["entropy_fps"][str(t)] = round(n / median_seconds(lambda: list(pool.map(dec.entropy_decode, blobs)), args.repeats), 1)
    decoded = [dec.entropy_decode(b) for b in blobs]
    packed = sum(c.nbytes + s.nbytes for _, c, s in decoded) / n
    res["upload_bytes_per_frame"] = {"packed": round(packed, 1), "decoded": 3 * H * W, "ratio": round(packed / (3 * H * W), 4)}

    # end to end, and the device call alone (the decoder's own call, timed between HIP events around a second launch of it)
    def end_to_end():
        frames = dec.decode(blobs)
        torch.cuda.synchronize()
        return frames
    res["decode_fps"] = round(n / median_seconds(end_to_end, args.repeats), 1)
    from feartracker_amd import train_abi as abi
    captured = {}
    real = abi.launch

    def spy(lib, name, *a):
        captured["args"] = a
        return real(lib, name, *a)
    abi.launch = spy
    frames = dec.decode(blobs)
    abi.launch = real
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.repeats + 1):
        e0.record()
        assert dec._lib.fear_jpeg_decode_u8(*captured["args"]) == 0     # (the buffers are alive: `frames` and the allocator's cache)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    res["device_ms"] = round(statistics.median(times[1:]), 4)
    res["device_fps"] = round(n / (res["device_ms"] * 1e-3), 1)
    del frames

    # the baseline: Pillow on the host plus the upload of the decoded frames
    try:
        from PIL import Image
    except ImportError:
        res["pillow_fps"] = None
    else:
        def pillow(b):
            return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))

        def upload(frames):
            for f in frames:
                pinned = torch.empty(f.shape, dtype=torch.uint8, pin_memory=True)
                pinned.numpy()[...] = f
                pinned.to("cuda", non_blocking=True)
            torch.cuda.synchronize()
        res["pillow_fps"] = {}
        for t in THREADS:
            with ThreadPoolExecutor(max_workers=t) as pool:
                res["pillow_fps"][str(t)] = round(n / median_seconds(lambda: upload(list(pool.map(pillow, blobs))), args.repeats), 1)
    dec.close()
    if args.entropy != "host":
        kept = json.load(open(args.out)).get("device_entropy", {}).get("rounds_per_sequence") if os.path.exists(args.out) else None
        res["device_entropy"] = device_entropy(torch, blobs, args.repeats, res["decode_fps"])
        if kept:
            res["device_entropy"]["rounds_per_sequence"] = kept
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
