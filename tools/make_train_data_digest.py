#!/usr/bin/env python3
"""Record the sha256 of `TrainPairBuilder.build_host`'s six arrays for four configurations into tests/golden/train_data_digests.json.
The committed file was written by this script run on the commit BEFORE `feartracker_amd/train_data.py` became a package (it uses
nothing but `TrainPairBuilder`, `COLOUR_MEMBERS` and `NOISE_MEMBERS`), so tests/test_train_data_layout.py pins that the host
restatement still computes, bit for bit, what that commit computed.  tests/test_train_data_layout.py loads this file for `CONFIGS`
and `scenario`, so the test and the record cannot drift apart.

Usage: python tools/make_train_data_digest.py [--out tests/golden/train_data_digests.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, B, SHAPES = 20241018, 8, ((40, 56), (97, 61))
CONFIGS = {
    "default": dict(),
    "photometric": dict(photometric=True),
    "colour_all": dict(colour_members="all"),
    "all": dict(photometric=True, noise_members="all", colour_members="all"),
}


def scenario(config: dict):
    """(builder, frames, pairs, params): two seeded frames, eight pairs — a box partly outside its frame, a search frame index outside
    the table, an absent target among them — and the draws of a fixed seed with every kind array overwritten so that every configured
    member, every blur and every tone occurs whatever the seed drew."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from feartracker_amd.train_data import COLOUR_MEMBERS, NOISE_MEMBERS, TrainPairBuilder
    rng = np.random.default_rng(SEED)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    pairs = np.zeros((B, 11))
    for k in range(B):
        for col, f in ((0, k % 2), (5, (k + 1) % 2)):
            h, w = SHAPES[f]
            bw, bh = rng.integers(4, w // 2), rng.integers(4, h // 2)
            pairs[k, col:col + 5] = [f, rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1), bw, bh]
        pairs[k, 10] = 1
    pairs[1, 1:5] = [-9, 30, 25, 20]               # a template box partly outside its frame
    pairs[2, 6:10] = [50, 85, 20, 30]              # a search box partly outside its frame
    pairs[3, 5] = 5                                # a search frame index outside the table
    pairs[4, 10] = 0                               # an absent target
    builder = TrainPairBuilder(config, device="cpu")
    params = builder.draw(pairs, [f.shape for f in frames], np.random.default_rng(SEED + 1))
    members = np.array([COLOUR_MEMBERS[m] for m in builder.colour_members], dtype=np.int32)
    params.colour = members[np.arange(B) % len(members)]
    params.tone = (np.arange(B) % 3).astype(np.int32)
    if params.photo is not None:
        crop = np.arange(2 * B).reshape(B, 2)
        noises = np.array([0] + [NOISE_MEMBERS[m] for m in builder.noise_members], dtype=np.int32)
        params.photo.blur = (crop % 5).astype(np.int32)
        params.photo.noise = noises[crop % len(noises)]
    return builder, frames, pairs, params


def digest(batch) -> str:
    h = hashlib.sha256()
    for a in batch:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_data_digests.json"))
    args = ap.parse_args()
    out = {}
    for name, config in CONFIGS.items():
        builder, frames, pairs, params = scenario(config)
        out[name] = digest(builder.build_host(frames, pairs, params))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(args.out, out)


if __name__ == "__main__":
    main()
