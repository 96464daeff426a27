"""Per-block taps of the trunk without a new ABI (test infrastructure).

`fear_features` runs the template-branch plan, whose neck is the exact fp32 `pw_mfma_kernel` in every arithmetic mode.  A model
made of the same stem and blocks 1..k followed by an IDENTITY neck (C x C, weights 1 / 0 and bias 0: exact in fp16, and
x * 1 + 0 * y summed in fp32 is x) therefore returns block k's output bit for bit as the engine computes it.  The writer below
keeps the source file's conv table and payload as they are (the identity neck's conv is appended), so every block of the
truncated model packs the very same fp16 weights.

Also: the edge-case crops the block tests feed in, and the split of a template-branch plan into the ops of each block.
"""
import struct

import numpy as np
import torch

HEADER = "<8s4IQ"
CONV = "<8I2Q24s"
BLOCK = "<2I3i3I"
K_STEM, K_IR, K_NECK = 0, 1, 2


def read_tables(path: str):
    with open(path, "rb") as fh:
        buf = fh.read()
    magic, version, n_convs, n_blocks, dtype, payload_bytes = struct.unpack_from(HEADER, buf, 0)
    assert magic == b"FEARW1\0\0" and dtype == 0, "fp16 FEARW1 files only"
    convs = [list(struct.unpack_from(CONV, buf, 64 + 72 * i)) for i in range(n_convs)]
    boff = 64 + 72 * n_convs
    blocks = [list(struct.unpack_from(BLOCK, buf, boff + 32 * i)) for i in range(n_blocks)]
    payload = buf[boff + 32 * n_blocks: boff + 32 * n_blocks + payload_bytes]
    return convs, blocks, payload


def trunk_length(path: str) -> int:
    """Number of trunk units in front of the neck: stem + IR blocks."""
    _, blocks, _ = read_tables(path)
    return next(i for i, b in enumerate(blocks) if b[0] == K_NECK)


def write_truncated(src: str, k: int, dst: str) -> int:
    """Write stem + blocks 1..k of `src` + an identity neck to `dst`.  Returns the neck's channel count (block k's output)."""
    convs, blocks, payload = read_tables(src)
    assert all(b[0] in (K_STEM, K_IR) for b in blocks[:k + 1]) and k >= 1
    last = blocks[k]
    c = convs[last[4]][0]                       # cout of block k's projection (conv[2])
    payload = bytearray(payload)
    while len(payload) % 16:
        payload += b"\0"
    w_off = len(payload)
    payload += np.eye(c, dtype="<f2").tobytes()
    b_off = len(payload)
    payload += np.zeros(c, dtype="<f2").tobytes()
    while len(payload) % 16:
        payload += b"\0"
    # cout, cin_g, groups, k, stride, pad, relu, has_bias, w_off, b_off, name
    convs = convs + [[c, c, 1, 1, 1, 0, 0, 1, w_off, b_off, b"identity_neck"]]
    blocks = blocks[:k + 1] + [[K_NECK, 0, len(convs) - 1, -1, -1, 0, 0, 0]]
    header = struct.pack(HEADER, b"FEARW1\0\0", 1, len(convs), len(blocks), 0, len(payload))
    header += b"\0" * (64 - len(header))
    with open(dst, "wb") as fh:
        fh.write(header)
        for e in convs:
            fh.write(struct.pack(CONV, *e))
        for b in blocks:
            fh.write(struct.pack(BLOCK, *b))
        fh.write(bytes(payload))
    return c


def block_ops(names_prev, names_k):
    """The ops of block k: the template plan of the model cut at k minus that of the model cut at k - 1 (both end with
    their identity neck, which is dropped).  The plan builder emits the blocks in order, so the shorter plan's trunk must be a
    prefix of the longer one's; asserted."""
    assert names_prev[-1].startswith("neck_") and names_k[-1].startswith("neck_"), (names_prev, names_k)
    prev, cur = names_prev[:-1], names_k[:-1]
    assert cur[:len(prev)] == prev, (prev, cur)
    return cur[len(prev):]


# ---------------------------------------------------------------------------------------------------------------- inputs
MEAN = np.array([0.485, 0.456, 0.406]) * 255.0
STD = np.array([0.229, 0.224, 0.225]) * 255.0


def normalise(u8: torch.Tensor) -> torch.Tensor:
    """(N, 3, H, W) uint8 -> the engine's normalised fp32 input (mean / std of base_tracker.py:70-81)."""
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    inv = 1.0 / torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    return (u8.float() - mean) * inv


def edge_crops(n: int, hw: int, seed: int = 0) -> torch.Tensor:
    """n normalised crops, by crop index i % 3: a random u8 image, a constant image (a different grey per crop), impulses on
    the 16- and 32-pixel tile seams (both pixels either side of every seam) and in the four corners on a mid-grey ground."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (n, 3, hw, hw), dtype=torch.uint8, generator=g)
    for i in range(n):
        if i % 3 == 1:
            u8[i] = int(torch.randint(0, 256, (1,), generator=g)) if i > 1 else 255
        elif i % 3 == 2:
            img = torch.full((3, hw, hw), 128, dtype=torch.uint8)
            seams = sorted({p for s in range(16, hw, 16) for p in (s - 1, s)})
            rows = torch.tensor(seams)
            for c in range(3):
                v = (0, 255, 64)[(c + i) % 3]
                img[c, rows[:, None], rows[None, :]] = v          # seam crossings
                img[c, rows, (i * 5) % hw] = v                    # a column of impulses across every horizontal seam
            for y, x in ((0, 0), (0, hw - 1), (hw - 1, 0), (hw - 1, hw - 1)):
                img[:, y, x] = torch.tensor([255, 0, 255], dtype=torch.uint8)
            u8[i] = img
    return normalise(u8)


def checked_crops(n: int):
    """Crops of a pass of n whose output is compared with the reference: the first three (one of each kind), the middle one
    and the last one."""
    return sorted({i for i in (0, 1, 2, n // 2, n - 1) if 0 <= i < n})
