"""Builds tools/jpeg_entropy_host.cpp with the address and undefined-behaviour sanitizers and runs it — a stand-alone host program, no
Python extension and no GPU — on the fixture's files (tests/golden/jpeg_decode.npz) and on the malformed set of
tests/test_jpeg_decode_host.py: every prefix and every flipped entropy byte of the 16 x 16 4:2:0 file, and the header faults.  Each line
of its output is compared with the Python decoder's verdict and packed stream; a file whose headers parse has a second line, fear_jpeg_scan_prepare's, compared with
jpeg_huffman.jpeg_scan_prepare_host, and where the scan is accepted a third, fear_jpeg_sub_start's at 4 and 128 bytes, compared with
jpeg_huffman.scan_sub_start.  Expect "0 sanitizer reports, 0 mismatches".

    python tools/jpeg_entropy_check.py [--dir SCRATCH] [--cxx g++]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import jpegdec                                                   # noqa: E402
import test_jpeg_decode_host as host_tests                       # noqa: E402
from feartracker_amd import jpeg_frames as jf                    # noqa: E402
from feartracker_amd import jpeg_huffman as jh                   # noqa: E402


def fnv(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def expected(name, data):
    """The program's line for one file, from the Python decoder."""
    try:
        hd, coef = jf.jpeg_coefficients_host(data)
    except jf.UnsupportedJPEG:
        try:
            jf.jpeg_info(data)
        except jf.UnsupportedJPEG:
            return f"{name} {jf.ERR_UNSUPPORTED}"
        return f"{name} 0 {jf.ERR_UNSUPPORTED}"
    except jf.MalformedJPEG:
        try:
            jf.jpeg_info(data)
        except jf.MalformedJPEG:
            return f"{name} {jf.ERR_FORMAT}"
        return f"{name} 0 {jf.ERR_FORMAT}"
    packed, start = [], [0]
    for plane in coef:
        for block in plane.reshape(-1, 64):
            nz = np.flatnonzero(block)
            count = max(1, int(nz[-1]) + 1) if nz.size else 1
            packed.append(block[:count])
            start.append(start[-1] + count)
    packed = np.concatenate(packed).astype("<i2")
    h = fnv(fnv(14695981039346656037, np.array(start, dtype="<u4").tobytes()), packed.tobytes())
    return f"{name} 0 0 {hd.width} {hd.height} {len(hd.ids)} {len(start) - 1} {packed.size} {h:016x}"


def expected_scan(name, data):
    """The program's second line for one file, or None where the headers do not parse."""
    try:
        hd = jf._parse(data)
    except (jf.MalformedJPEG, jf.UnsupportedJPEG):
        return None
    try:
        out, start = jh.jpeg_scan_prepare_host(data, hd)
    except jf.MalformedJPEG:
        return f"{name} scan {jf.ERR_FORMAT}"
    h = fnv(fnv(14695981039346656037, np.array(start, dtype="<u4").tobytes()), out)
    subs = [jh.scan_sub_start(start, b) for b in (4, 128)]
    third = f"{name} sub" + "".join(f" 0 {int(s[-1])} {fnv(14695981039346656037, s.astype('<u4').tobytes()):016x}" for s in subs)
    return f"{name} scan 0 {len(out)} {len(start) - 1} {h:016x}", third


def files():
    out = {f"case{i:02d}.jpg": data for i, (_, data, _) in enumerate(jpegdec.cases())}
    F = jpegdec.case("16x16_420")[1]
    for k in range(len(F)):
        out[f"prefix{k:04d}.jpg"] = F[:k]
    scan = F.index(b"\xff\xda")
    first = scan + 2 + struct.unpack(">H", F[scan + 2:scan + 4])[0]
    for k in range(first, len(F) - 2):
        bad = bytearray(F)
        bad[k] ^= 0xFF
        out[f"flip{k:04d}.jpg"] = bytes(bad)
    for i, (what, (data, _)) in enumerate(host_tests._header_faults().items()):
        out[f"fault{i:02d}.jpg"] = data
    import jpeghuff
    for i, (_, data, _) in enumerate(jpeghuff.entropy_cases()):
        out[f"entropy{i:02d}.jpg"] = data
    # restart files: every prefix, and every marker byte replaced
    R = jpegdec.case("15x50_420_random_q100_rst3")[1]
    for k in range(R.index(b"\xff\xda"), len(R)):
        out[f"rprefix{k:04d}.jpg"] = R[:k]
        if R[k] == 0xFF and 0xD0 <= R[k + 1] <= 0xD7:
            out[f"rmark{k:04d}.jpg"] = R[:k + 1] + bytes([0xD0 + (R[k + 1] + 1) % 8]) + R[k + 2:]
            out[f"rgone{k:04d}.jpg"] = R[:k] + R[k + 2:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="scratch directory (a temporary one by default)")
    ap.add_argument("--cxx", default="g++")
    args = ap.parse_args()
    scratch = args.dir or tempfile.mkdtemp(prefix="jpeg_entropy_")
    os.makedirs(scratch, exist_ok=True)
    exe = os.path.join(scratch, "jpeg_entropy_host")
    cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tools", "jpeg_entropy_host.cpp")]
    print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    made = files()
    for name, data in made.items():
        with open(os.path.join(scratch, name), "wb") as fh:
            fh.write(data)
    names = sorted(made)
    res = subprocess.run([exe] + [os.path.join(scratch, n) for n in names], capture_output=True, text=True)
    reports = res.stderr.count("ERROR: AddressSanitizer") + res.stderr.count("runtime error")
    lines = res.stdout.splitlines()
    wanted = []
    for name in names:
        scan = expected_scan(name, made[name])
        wanted += [(name, line) for line in ((scan,) if isinstance(scan, str) else scan or ())]
        wanted.append((name, expected(name, made[name])))
    mismatches = 0 if len(lines) == len(wanted) else 1
    for (name, want), line in zip(wanted, lines):
        if line != want:
            mismatches += 1
            print(f"MISMATCH {name}: program '{line}', Python '{want}'")
    if res.stderr:
        print(res.stderr[-4000:])
    print(f"{len(names)} files, exit status {res.returncode}: {reports} sanitizer reports, {mismatches} mismatches")
    return 0 if res.returncode == 0 and reports == 0 and mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
