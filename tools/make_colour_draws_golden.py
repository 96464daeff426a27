#!/usr/bin/env python3
"""Record `TrainPairBuilder.draw` of a fixed seed into tests/golden/train_pairs_draws.npz: every array of `TrainPairParams` with the
photometric stage off and on, default configuration otherwise.  The committed file was written by this script run on the commit BEFORE
`colour_members` existed (it touches nothing newer than `draw`), so tests/test_colour_host.py pins that the default members still
consume the generator and fill the record exactly as that commit did.

Usage: python tools/make_colour_draws_golden.py [--out tests/golden/train_pairs_draws.npz]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, PAIRS, SHAPES = 20240611, 16, ((48, 64), (256, 480))


def record(photometric: bool) -> dict:
    sys.path.insert(0, ROOT)
    from feartracker_amd.train_data import TrainPairBuilder
    builder = TrainPairBuilder(dict(photometric=photometric), device="cpu")
    pairs = np.zeros((PAIRS, 11))
    params = builder.draw(pairs, SHAPES, np.random.default_rng(SEED))
    prefix = "on_" if photometric else "off_"
    out = {}
    for name in ("context", "jitter", "tone", "colour", "alpha", "beta", "gamma", "shift"):
        out[prefix + name] = np.asarray(getattr(params, name))
    if photometric:
        for f in dataclasses.fields(params.photo):
            out[prefix + "photo_" + f.name] = np.asarray(getattr(params.photo, f.name))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_pairs_draws.npz"))
    args = ap.parse_args()
    arrays = {**record(False), **record(True)}
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
