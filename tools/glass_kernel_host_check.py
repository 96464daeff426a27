#!/usr/bin/env python3
"""fear_glass_u8's kernel body on the host under Address- and UndefinedBehaviorSanitizer (tools/glass_kernel_host.cpp): the operator
cases of tests/test_glass_gpu.py, compared with `glass_u8_host` bit for bit.  Needs a C++ compiler with the sanitizer runtimes (CXX,
default clang++ or g++) and no GPU.

Usage: python tools/glass_kernel_host_check.py [--lanes 16] [--keep DIR]
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
    import test_glass_gpu as t
    from feartracker_amd.train_data import BLUR_BOX, BLUR_GAUSSIAN, BLUR_GLASS, BLUR_MOTION, BLUR_NONE
    for shape in t.SHAPES + [(8, 8), (256, 34), (34, 256)]:
        yield f"member {shape}", t._contents(*shape, seed=shape[0]), t._records([BLUR_GLASS] * 3, seed=shape[1])
        c = t._contents(*shape, seed=shape[0] + 1)
        ops = t._records([BLUR_GLASS, BLUR_NONE, BLUR_GAUSSIAN, 9, BLUR_GLASS], seed=shape[1] + 1)
        yield f"a record per crop {shape}", np.concatenate([c, c[:1][:, ::-1], c[:1]]), ops
        yield f"one crop {shape}", c[:1], ops[4:5]
    ops = t._records([BLUR_NONE, BLUR_BOX, BLUR_MOTION, -1, 6, 1 << 20], seed=9)
    yield "copies", np.concatenate([t._contents(34, 70, seed=7), t._contents(34, 70, seed=8)]), ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    from feartracker_amd.train_data import BLUR_GLASS, glass_u8_host
    cxx = os.environ.get("CXX") or shutil.which("clang++") or shutil.which("g++")
    work = args.keep or tempfile.mkdtemp(prefix="glass_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "glass_kernel_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-pthread", "-o", exe, os.path.join(ROOT, "tools", "glass_kernel_host.cpp")], check=True)
    failed = 0
    for name, crops, ops in cases():
        n, h, w = crops.shape[:3]
        case, out = os.path.join(work, "case.bin"), os.path.join(work, "out.bin")
        with open(case, "wb") as fh:
            fh.write(np.array([n, h, w], dtype=np.int32).tobytes() + np.ascontiguousarray(crops).tobytes() + ops.tobytes())
        subprocess.run([exe, str(args.lanes), case, out], check=True)
        got = np.fromfile(out, dtype=np.uint8).reshape(crops.shape)
        diff = [i for i in range(n) if not np.array_equal(got[i], glass_u8_host(crops[i], ops[i]) if ops["blur"][i] == BLUR_GLASS else crops[i])]
        failed += bool(diff)
        print(f"{'FAIL' if diff else 'ok  '} {name}: {n} crops" + (f", crops {diff} differ" if diff else ""), flush=True)
    if not args.keep:
        shutil.rmtree(work)
    print("FAILED" if failed else "all cases equal glass_u8_host, no sanitizer report")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
