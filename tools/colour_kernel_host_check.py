#!/usr/bin/env python3
"""fear_colour_u8's kernel body on the host under Address- and UndefinedBehaviorSanitizer (tools/colour_kernel_host.cpp): the operator
cases of tests/test_colour_gpu.py, compared with `colour_u8_host` bit for bit.  Needs a C++ compiler with the sanitizer runtimes
(CXX, default clang++ or g++) and no GPU.

Usage: python tools/colour_kernel_host_check.py [--lanes 1024] [--keep DIR]
"""
import argparse
import itertools
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
    import test_colour_gpu as t
    from feartracker_amd.train_data import COLOUR_EMBOSS, COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_JITTER, COLOUR_TONE_CURVE, colour_tables
    orders = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
    for shape in t.SHAPES:
        for kind in (COLOUR_EQUALIZE, COLOUR_HSV, COLOUR_EMBOSS):
            _, ops, aux = t._records([kind] * 4, seed=shape[1])
            yield f"member {kind} {shape}", t._contents(*shape, seed=kind), ops, aux
        params, _, _ = t._records([COLOUR_JITTER] * 24, seed=shape[0])
        params.colour_jitter_order = orders
        ops, aux = colour_tables(params)
        yield f"jitter orders {shape}", t._contents(*shape, seed=5)[np.arange(24) % 4], ops, aux
        c = t._contents(*shape, seed=shape[0] + 1)
        _, ops, aux = t._records([COLOUR_EMBOSS, COLOUR_JITTER, 0, COLOUR_EQUALIZE, COLOUR_HSV], seed=shape[1] + 1)
        yield f"a record per crop {shape}", np.concatenate([c, c[:1][:, ::-1]]), ops, aux
        yield f"one crop {shape}", c[3:4], ops[3:4], aux[3:4]
    _, ops, aux = t._records([COLOUR_JITTER] * 6)
    ops["kind"][:5] = [0, COLOUR_TONE_CURVE, 9, -1, 1 << 20]
    ops["order"][5] = [0, 1, 1, 3]
    yield "copies", np.concatenate([t._contents(34, 70, seed=7), t._contents(34, 70, seed=8)[:2]]), ops, aux


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    from feartracker_amd.train_data import colour_u8_host
    cxx = os.environ.get("CXX") or shutil.which("clang++") or shutil.which("g++")
    work = args.keep or tempfile.mkdtemp(prefix="colour_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "colour_kernel_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-pthread", "-o", exe, os.path.join(ROOT, "tools", "colour_kernel_host.cpp")], check=True)
    failed = 0
    for name, crops, ops, aux in cases():
        n, h, w = crops.shape[:3]
        case, out = os.path.join(work, "case.bin"), os.path.join(work, "out.bin")
        with open(case, "wb") as fh:
            fh.write(np.array([n, h, w], dtype=np.int32).tobytes() + np.ascontiguousarray(crops).tobytes() + ops.tobytes() +
                     np.ascontiguousarray(aux).tobytes())
        subprocess.run([exe, str(args.lanes), case, out], check=True)
        got = np.fromfile(out, dtype=np.uint8).reshape(crops.shape)
        diff = [i for i in range(n) if not np.array_equal(got[i], colour_u8_host(crops[i], ops[i], aux[i]))]
        failed += bool(diff)
        print(f"{'FAIL' if diff else 'ok  '} {name}: {n} crops" + (f", crops {diff} differ" if diff else ""))
    if not args.keep:
        shutil.rmtree(work)
    print("FAILED" if failed else "all cases equal colour_u8_host, no sanitizer report")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
