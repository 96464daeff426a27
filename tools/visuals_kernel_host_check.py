#!/usr/bin/env python3
"""The kernel bodies of fear_draw_boxes_u8 and fear_miner_update on the host under Address- and UndefinedBehaviorSanitizer
(tools/visuals_kernel_host.cpp): the operator cases of tests/visualsgen.py, compared with `draw_boxes_host`, `render_sheet_host` and
`miner_decide_host` byte for byte.  Needs a C++ compiler with the sanitizer runtimes (CXX, default clang++ or g++) and no GPU.

Usage: python tools/visuals_kernel_host_check.py [--lanes 16] [--keep DIR]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    import visualsgen as vg
    from feartracker_amd import visuals as V
    from feartracker_amd.metrics import decode_host
    cxx = os.environ.get("CXX") or shutil.which("clang++") or shutil.which("g++")
    work = args.keep or tempfile.mkdtemp(prefix="visuals_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "visuals_kernel_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-pthread", "-o", exe, os.path.join(ROOT, "tools", "visuals_kernel_host.cpp")], check=True)
    case, out = os.path.join(work, "case.bin"), os.path.join(work, "out.bin")
    failed = 0

    def run(mode, lanes, blob):
        with open(case, "wb") as fh:
            fh.write(blob)
        subprocess.run([exe, mode, str(lanes), case, out], check=True)
        return np.fromfile(out, dtype=np.uint8)

    def report(name, ok):
        nonlocal failed
        failed += not ok
        print(f"{'ok  ' if ok else 'FAIL'} {name}", flush=True)

    for name, shapes, boxes, frame_of, cols, t in vg.draw_cases():
        frames = [vg.frame(h, w, i) for i, (h, w) in enumerate(shapes)]
        want = np.concatenate([f.reshape(-1) for f in V.draw_boxes_host([f.copy() for f in frames], boxes, frame_of, cols, t)])
        blob = (np.array([len(frames), len(boxes), t], np.int32).tobytes() + np.array(shapes, np.int32).tobytes() +
                b"".join(f.tobytes() for f in frames) + np.ascontiguousarray(boxes, np.int32).tobytes() +
                np.ascontiguousarray(frame_of, np.int32).tobytes() + np.ascontiguousarray(cols, np.uint8).tobytes())
        # the device's 256 lanes where the list of later boxes fills up (a chunk of candidates is one per lane)
        for lanes in [args.lanes] + ([256] if name in ("300 boxes t=5", "700 boxes t=5") else []):
            report(f"draw {name}, {lanes} lanes", np.array_equal(run("draw", lanes, blob), want))
    for B, n, seed in ((3, 2, 1), (2, 2, 2)):
        m = vg.miner_step(B, seed)
        with np.errstate(invalid="ignore", over="ignore"):
            pred = V.truncate_boxes_host(decode_host(m["cls"][:n], m["bbox"][:n]))
        want = V.render_sheet_host(m["template"], m["search"], pred, m["gt_box"], m["visible"], n)
        blob = (np.array([B, n], np.int32).tobytes() + m["template"].tobytes() + m["search"].tobytes() + pred.tobytes() +
                np.ascontiguousarray(m["gt_box"], np.int32).tobytes() + np.ascontiguousarray(m["visible"], np.int32).tobytes())
        report(f"render B={B} n={n}", np.array_equal(run("render", args.lanes, blob), want.reshape(-1)))
    nan = float("nan")
    for mode_max, delta, scores in ((0, 0.1, [1.0, 1.05, 0.5, 2.0, 0.4, 0.45]), (1, 0.1, [1.0, 1.05, 0.5, 2.0]), (0, 0.25, [1.0, 0.75, 1.25]),
                                    (0, 1e-4, [nan, 0.1, 5.0]), (1, 1e-4, [1.0, nan, 0.5]), (0, -1e30, [3.0, 1.0, 2.0])):
        blob = np.array([mode_max, len(scores)], np.int32).tobytes() + np.array([delta] + scores, np.float64).tobytes()
        got = run("decide", args.lanes, blob).view(V.MINER_STATE_DTYPE)
        state, ok = V.miner_state_host(), True
        for step, s in enumerate(scores):
            V.miner_decide_host(state, s, bool(mode_max), delta, step)
            ok = ok and got[step].tobytes() == state.tobytes()
        report(f"decide mode_max={mode_max} min_delta={delta} {scores}", ok)
    if not args.keep:
        shutil.rmtree(work)
    print("FAILED" if failed else "all cases equal the numpy forms, no sanitizer report")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
