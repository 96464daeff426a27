#!/usr/bin/env python3
"""fear_hls_u8's kernel body on the host under Address- and UndefinedBehaviorSanitizer (tools/hls_kernel_host.cpp): the operator cases of
tests/test_hls_gpu.py, compared with `hls_u8_host` bit for bit.  Needs a C++ compiler with the sanitizer runtimes (CXX, default clang++
or g++) and no GPU.

Usage: python tools/hls_kernel_host_check.py [--lanes 64] [--keep DIR]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases():
    import test_hls_gpu as t
    from feartracker_amd.train_data import HLS_COPY, HLS_DTYPE, HLS_ISO, HLS_RAIN, HLS_SHADOW, shadow_segments
    for shape in t.SHAPES:
        for kind in (HLS_ISO, HLS_RAIN, HLS_SHADOW):
            ops, seg = t._records([kind] * 4, *shape, seed=shape[1] + kind)
            yield f"member {kind} {shape}", t._contents(*shape, seed=kind), ops, seg
        c = t._contents(*shape, seed=shape[0] + 1)
        ops, seg = t._records([HLS_RAIN, HLS_ISO, HLS_COPY, HLS_SHADOW, HLS_ISO], *shape, seed=shape[1] + 1)
        yield f"a record per crop {shape}", np.concatenate([c, c[:1][:, ::-1]]), ops, seg
        yield f"one crop {shape}", c[3:4], ops[3:4], seg
    ops, seg = t._records([HLS_SHADOW] * 8, 34, 70, seed=9)
    ops["kind"][:4] = [HLS_COPY, 4, -1, 1 << 20]
    ops["seg_count"][4], ops["seg_count"][5], ops["seg_offset"][6] = 0, -3, -1
    ops["kind"][7], ops["seg_count"][7] = HLS_RAIN, -1
    yield "copies", np.concatenate([t._contents(34, 70, seed=7), t._contents(34, 70, seed=8)]), ops, seg
    half = np.zeros((34, 70, 3), np.uint8)
    half[:, 35:] = 255
    ops, seg = t._records([HLS_ISO] * 3, 34, 70, seed=5)
    ops["intensity"] = [0.5, 0.5, 0.75]
    yield "lambda 0 and the cap", np.stack([t._contents(34, 70)[1], half, half]), ops, seg
    seg = np.concatenate([np.zeros((1, 4), np.int16), shadow_segments([np.array([[0, 0], [256, 0], [256, 256], [0, 256]])]),
                          np.array([[3, 0, 0, 0], [-300, -5, 600, 900], [32767, -32768, -32768, 32767], [9, 9, 9, 9]], np.int16)])
    ops = np.zeros(2, dtype=HLS_DTYPE)
    ops["kind"], ops["seg_offset"], ops["seg_count"] = HLS_SHADOW, [1, 6], [5, 4]
    yield "a polygon over the whole crop, edges far outside", t._contents(256, 256, seed=2)[:2], ops, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    from feartracker_amd.train_data import hls_u8_host, iso_exp_table, normal_quantiles
    q, e = normal_quantiles(), iso_exp_table()
    cxx = os.environ.get("CXX") or shutil.which("clang++") or shutil.which("g++")
    work = args.keep or tempfile.mkdtemp(prefix="hls_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "hls_kernel_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "hls_kernel_host.cpp")], check=True)
    failed = 0
    for name, crops, ops, seg in cases():
        n, h, w = crops.shape[:3]
        case, out = os.path.join(work, "case.bin"), os.path.join(work, "out.bin")
        with open(case, "wb") as fh:
            fh.write(np.array([n, h, w, len(seg)], dtype=np.int32).tobytes() + np.ascontiguousarray(crops).tobytes() + ops.tobytes() +
                     np.ascontiguousarray(seg, dtype=np.int16).tobytes() + q.tobytes() + e.tobytes())
        subprocess.run([exe, str(args.lanes), case, out], check=True)
        got = np.fromfile(out, dtype=np.uint8).reshape(crops.shape)
        diff = [i for i in range(n) if not np.array_equal(got[i], hls_u8_host(crops[i], ops[i], seg, q, e))]
        failed += bool(diff)
        print(f"{'FAIL' if diff else 'ok  '} {name}: {n} crops" + (f", crops {diff} differ" if diff else ""), flush=True)
    if not args.keep:
        shutil.rmtree(work)
    print("FAILED" if failed else "all cases equal hls_u8_host, no sanitizer report")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
