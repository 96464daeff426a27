"""Builds tools/jpeg_huff_build_host.cpp with the address and undefined-behaviour sanitizers, runs it on histograms chosen to reach
every branch of the table builder (feartracker_amd/csrc/fear_jpeg_huff_build.h) and compares its lines with
jpeg_encode.jpeg_optimal_table_host.  A tool run by hand; needs g++ and no GPU.

    python tools/jpeg_huff_build_check.py [--count 200]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feartracker_amd import jpeg_encode as E  # noqa: E402


def histograms(count):
    rng = np.random.default_rng(5)
    out = [np.zeros(256, dtype=np.uint32), np.ones(256, dtype=np.uint32), np.full(256, 0xFFFFFFFF, dtype=np.uint32)]
    one = np.zeros(256, dtype=np.uint32)
    one[255] = 1
    out.append(one)
    for symbols in (17, 20, 31, 32, 33, 40, 47, 200):                      # chains: depths at and around 16 and 32, and up to 47
        fib, a, b = np.zeros(256, dtype=np.uint32), 1, 2
        for s in range(symbols):
            fib[255 - s] = min(a, 0xFFFFFFFF)
            a, b = b, a + b
        out.append(fib)
    for _ in range(count):
        top = 1 << int(rng.integers(1, 33))
        out.append((rng.integers(0, top, 256, dtype=np.uint64) * (rng.random(256) < rng.random())).astype(np.uint32))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=200)
    args = ap.parse_args()
    hist = histograms(args.count)
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "jpeg_huff_build_host"), os.path.join(tmp, "hist.bin")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "jpeg_huff_build_host.cpp")], check=True)
        hist.astype("<u4").tofile(data)
        lines = subprocess.run([exe, data], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(hist)
    refused = limited = 0
    for k, line in enumerate(lines):
        index, ok, depth, n_values, counts, values, codes = (line.split(" ") + [""])[:7]
        assert int(index) == k
        try:
            want_counts, want_values, want_depth = E.jpeg_optimal_table_host(hist[k])
        except E.JpegHuffmanDepth:
            refused += 1
            assert (int(ok), int(n_values), counts, values) == (0, 0, "00" * 16, "") and int(depth) > 32 and set(codes) == {"0"}, k
            continue
        limited += want_depth > 16
        assert (int(ok), int(depth), int(n_values)) == (1, want_depth, len(want_values)), k
        assert bytes.fromhex(counts) == bytes(want_counts) and bytes.fromhex(values) == want_values, k
        table = E._codes(want_counts, want_values)
        for sym in range(256):
            code, length = table.get(sym, (0, 0))
            assert int(codes[6 * sym:6 * sym + 6], 16) == (length << 16 | code), (k, sym)
    print(f"{len(lines)} histograms equal jpeg_optimal_table_host under the sanitizers: {refused} refused, {limited} length-limited")


if __name__ == "__main__":
    main()
